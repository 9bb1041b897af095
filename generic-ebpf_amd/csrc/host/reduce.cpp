// reduce.cpp — per-segment reductions over a list of a batch's packets (ebpf_gpu.h "Reducing a
// list per segment"): on the host (ebpf_batch_reduce, the statement of the semantics) and on the
// device (ebpf_batch_reduce_dev, reduce.hip).
#include "gather.h"
#include "reduce.h"
#include "runtime.h"

namespace {

inline bool
wants_values(const struct ebpf_batch_sums &o)
{
	return o.sum != nullptr || o.min != nullptr || o.max != nullptr || o.bits != nullptr;
}

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
		if (val_bits < 1 || val_bits > 64 || val_shift > 64 - val_bits)
			return fail(EINVAL, "val_bits outside [1, 64], or val_shift + val_bits above 64");
	}
	if (out->bytes != nullptr && batch == nullptr)
		return fail(EINVAL, "batch is NULL where bytes is wanted");
	if (batch != nullptr) {
		// (EBPF_BATCH_HIST_OVERWRITE: as ebpf_batch_select_dev, no concern of the packets' places)
		int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
		if (err)
			return err;
		if (batch->count != count)
			return fail(EINVAL, "batch->count differs from count");
	}
	if (n != 0 && index == nullptr)
		return fail(EINVAL, "index is NULL with n > 0");
	if (seg_cap != 0 && seg_starts == nullptr)
		return fail(EINVAL, "seg_starts is NULL with seg_cap > 0");
	if (n > 0xffffffffull || count > 0xffffffffull || seg_cap > 0xffffffffull)
		return fail(E2BIG, "n, count or seg_cap above 2^32 - 1");
	return 0;
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
	const uint64_t R = nseg == nullptr ? seg_cap
			   : *nseg <= seg_cap ? *nseg
					      : (seg_cap != 0 ? seg_cap - 1 : 0);
	if (seg_cap == 0)
		return 0;
	for (uint64_t g = 0; g < R; g++)
		if (seg_starts[g] > seg_starts[g + 1])
			return fail(EINVAL, "seg_starts decreases");
	if (seg_starts[R] > n)
		return fail(EINVAL, "seg_starts ends past n");
	const uint64_t mask = val_bits >= 64 ? ~0ull : (1ull << val_bits) - 1;
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
			const uint64_t v = (ret[i] >> val_shift) & mask;
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
	device_guard dg;
	hipStream_t st = static_cast<hipStream_t>(stream);
	hipError_t e = hipSetDevice(device);
	if (e != hipSuccess)
		return hip_fail(e, "hipSetDevice");
	if (count == 0) // no entry has a length or a value: every segment's results are an empty one's
		n = 0;
	uint32_t *scratch = nullptr;
	// (the steering rows' buffer: calls on a stream run in order, so they share it)
	if (n != 0 && (err = steer_acquire(device, st, reduce_scratch_bytes(n), &scratch)))
		return fail(err, "reduce scratch");
	e = launch_reduce(batch, ret_dev, count, val_shift, val_bits, index_dev, n, seg_starts_dev,
			  seg_cap, nseg_dev, *out, reinterpret_cast<uint64_t *>(scratch), st);
	return e == hipSuccess ? 0 : hip_fail(e, "reduce kernels");
}
