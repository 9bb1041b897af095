// scan.cpp — running totals per segment over a list of a batch's packets (ebpf_gpu.h "Running
// totals per segment"): on the host (ebpf_batch_scan, the statement of the semantics) and on the
// device (ebpf_batch_scan_dev, scan.hip).
#include "gather.h"
#include "list_args.h"
#include "scan.h"

namespace {

inline bool
wants_lengths(const struct ebpf_batch_scans &o)
{
	return o.bytes_before != nullptr || o.over != nullptr;
}

inline bool
wants_nothing(const struct ebpf_batch_scans &o)
{
	return o.rank == nullptr && o.sum_before == nullptr && !wants_lengths(o);
}

int
scan_args(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
	  uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
	  const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *budgets,
	  const struct ebpf_batch_scans *out)
{
	if (out == nullptr)
		return fail(EINVAL, "out is NULL");
	if (out->sum_before != nullptr) {
		if (ret == nullptr)
			return fail(EINVAL, "ret is NULL where sum_before is wanted");
		if (int err = check_field(val_shift, val_bits))
			return err;
	}
	if (wants_lengths(*out) && batch == nullptr)
		return fail(EINVAL, "batch is NULL where bytes_before or over is wanted");
	if (out->over != nullptr && budgets == nullptr)
		return fail(EINVAL, "budgets is NULL where over is wanted");
	return check_list(batch, count, index, n, seg_starts, seg_cap);
}

} // namespace

// A plain loop per segment: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_scan(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
		uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
		const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		const uint64_t *budgets, const struct ebpf_batch_scans *out)
{
	int err = scan_args(batch, ret, count, val_shift, val_bits, index, n, seg_starts, seg_cap,
			    budgets, out);
	if (err)
		return err;
	const uint64_t R = seg_count(nseg, seg_cap);
	if ((err = check_segments(seg_starts, R, seg_cap, n)))
		return err;
	// the positions that no segment covers
	for (uint64_t j = 0; j < n; j++) {
		if (R != 0 && j >= seg_starts[0] && j < seg_starts[R])
			continue;
		if (out->rank != nullptr)
			out->rank[j] = 0;
		if (out->bytes_before != nullptr)
			out->bytes_before[j] = 0;
		if (out->sum_before != nullptr)
			out->sum_before[j] = 0;
		if (out->over != nullptr)
			out->over[j] = 0;
	}
	const bit_field vf = field_of(val_shift, val_bits);
	for (uint64_t g = 0; g < R; g++) {
		uint64_t bytes = 0, sum = 0;
		for (uint64_t j = seg_starts[g]; j < seg_starts[g + 1]; j++) {
			const uint32_t i = index[j];
			uint64_t len = 0;
			if (wants_lengths(*out)) {
				uint64_t s;
				len = packet_span(*batch, i, &s);
			}
			if (out->rank != nullptr)
				out->rank[j] = (uint32_t)(j - seg_starts[g]);
			if (out->bytes_before != nullptr)
				out->bytes_before[j] = bytes;
			if (out->sum_before != nullptr)
				out->sum_before[j] = sum;
			if (out->over != nullptr)
				out->over[j] = bytes + len > budgets[g];
			bytes += len;
			if (out->sum_before != nullptr && i < count)
				sum += vf.of(ret[i]);
		}
	}
	return 0;
}

EBPF_EXPORT int
ebpf_batch_scan_dev(int device, const struct ebpf_pkt_batch *batch, const uint64_t *ret_dev,
		    uint64_t count, uint32_t val_shift, uint32_t val_bits, const uint32_t *index_dev,
		    uint64_t n, const uint64_t *seg_starts_dev, uint64_t seg_cap,
		    const uint64_t *nseg_dev, const uint64_t *budgets_dev,
		    const struct ebpf_batch_scans *out, void *stream)
{
	int err = scan_args(batch, ret_dev, count, val_shift, val_bits, index_dev, n, seg_starts_dev,
			    seg_cap, budgets_dev, out);
	if (err || (err = check_device(device)))
		return err;
	if (n == 0 || wants_nothing(*out))
		return 0;
	// (rank alone, or a batch of no packets, keeps no rows)
	const bool rows = count != 0 && (wants_lengths(*out) || out->sum_before != nullptr);
	return on_device(device, stream, rows ? scan_scratch_bytes(n) : 0, "scan kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_scan(batch, ret_dev, count, val_shift, val_bits, index_dev, n, seg_starts_dev,
				   seg_cap, nseg_dev, budgets_dev, *out, reinterpret_cast<uint64_t *>(scratch), st);
	});
}
