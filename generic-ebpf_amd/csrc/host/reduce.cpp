// reduce.cpp — per-segment reductions over a list of a batch's packets (ebpf_gpu.h "Reducing a
// list per segment"): on the host (ebpf_batch_reduce, the statement of the semantics) and on the
// device (ebpf_batch_reduce_dev, reduce.hip).
#include "gather.h"
#include "list_args.h"
#include "reduce.h"

namespace {

int
reduce_args(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
	    uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
	    const uint64_t *seg_starts, uint64_t seg_cap, const struct ebpf_batch_sums *out)
{
	if (out == nullptr)
		return fail(EINVAL, "out is NULL");
	if (wants_values(*out)) {
		if (ret == nullptr)
			return fail(EINVAL, "ret is NULL where sum, min, max or bits is wanted");
		if (int err = check_field(val_shift, val_bits))
			return err;
	}
	if (out->bytes != nullptr && batch == nullptr)
		return fail(EINVAL, "batch is NULL where bytes is wanted");
	return check_list(batch, count, index, n, seg_starts, seg_cap);
}

inline bool
wants_nothing(const struct ebpf_batch_sums &o)
{
	return o.bytes == nullptr && !wants_values(o);
}

} // namespace

// A plain loop per segment: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_reduce(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
		  uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
		  const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		  const struct ebpf_batch_sums *out)
{
	int err = reduce_args(batch, ret, count, val_shift, val_bits, index, n, seg_starts, seg_cap, out);
	if (err)
		return err;
	const uint64_t R = seg_count(nseg, seg_cap);
	if (seg_cap == 0)
		return 0;
	if ((err = check_segments(seg_starts, R, seg_cap, n)))
		return err;
	const bit_field vf = field_of(val_shift, val_bits);
	for (uint64_t g = 0; g < R; g++) {
		uint64_t bytes = 0, sum = 0, mn = ~0ull, mx = 0, bits = 0;
		for (uint64_t j = seg_starts[g]; j < seg_starts[g + 1]; j++) {
			const uint32_t i = index[j];
			if (out->bytes != nullptr) {
				uint64_t s;
				bytes += packet_span(*batch, i, &s);
			}
			if (!wants_values(*out) || i >= count)
				continue;
			const uint64_t v = vf.of(ret[i]);
			sum += v;
			mn = std::min(mn, v);
			mx = std::max(mx, v);
			bits |= v;
		}
		if (out->bytes != nullptr)
			out->bytes[g] = bytes;
		if (out->sum != nullptr)
			out->sum[g] = sum;
		if (out->min != nullptr)
			out->min[g] = mn;
		if (out->max != nullptr)
			out->max[g] = mx;
		if (out->bits != nullptr)
			out->bits[g] = bits;
	}
	return 0;
}

EBPF_EXPORT int
ebpf_batch_reduce_dev(int device, const struct ebpf_pkt_batch *batch, const uint64_t *ret_dev,
		      uint64_t count, uint32_t val_shift, uint32_t val_bits, const uint32_t *index_dev,
		      uint64_t n, const uint64_t *seg_starts_dev, uint64_t seg_cap,
		      const uint64_t *nseg_dev, const struct ebpf_batch_sums *out, void *stream)
{
	int err = reduce_args(batch, ret_dev, count, val_shift, val_bits, index_dev, n, seg_starts_dev,
			      seg_cap, out);
	if (err || (err = check_device(device)))
		return err;
	if (seg_cap == 0 || wants_nothing(*out))
		return 0;
	if (count == 0) // no entry has a length or a value: every segment's results are an empty one's
		n = 0;
	return on_device(device, stream, n != 0 ? reduce_scratch_bytes(n) : 0, "reduce kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_reduce(batch, ret_dev, count, val_shift, val_bits, index_dev, n, seg_starts_dev,
				     seg_cap, nseg_dev, *out, reinterpret_cast<uint64_t *>(scratch), st);
	});
}
