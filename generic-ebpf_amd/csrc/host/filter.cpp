// filter.cpp — keeping part of a list (ebpf_gpu.h "Keeping part of a list"): on the host
// (ebpf_batch_filter, the statement of the semantics) and on the device (ebpf_batch_filter_dev,
// filter.hip).
#include "filter.h"
#include "list_args.h"

namespace {

int
filter_args(const struct ebpf_batch_test *test, uint64_t count, const uint32_t *index, uint64_t n,
	    const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
	    const struct ebpf_batch_parts *out, const uint64_t *info)
{
	if (test == nullptr || out == nullptr || info == nullptr)
		return fail(EINVAL, "test, out or info is NULL");
	if (test->ret != nullptr)
		if (int err = check_field(test->val_shift, test->val_bits))
			return err;
	if (n != 0 && index == nullptr)
		return fail(EINVAL, "index is NULL with n > 0");
	if (seg_starts == nullptr) {
		if (seg_cap != 0 || nseg != nullptr)
			return fail(EINVAL, "seg_starts is NULL with seg_cap > 0 or with nseg");
		if (out->kept_starts != nullptr || out->dropped_starts != nullptr)
			return fail(EINVAL, "a table is wanted of an unsegmented list");
	}
	return check_sizes(n, count, seg_cap);
}

} // namespace

// A plain loop over the positions that take part: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_filter(const struct ebpf_batch_test *test, uint64_t count, const uint32_t *index,
		  uint64_t n, const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		  const struct ebpf_batch_parts *out, uint64_t *info)
{
	int err = filter_args(test, count, index, n, seg_starts, seg_cap, nseg, out, info);
	if (err)
		return err;
	const uint64_t R = seg_count(nseg, seg_cap);
	if ((err = check_segments(seg_starts, R, seg_cap, n)))
		return err;
	// the positions that take part
	uint64_t first = 0, end = n;
	if (seg_starts != nullptr) {
		first = R != 0 ? seg_starts[0] : 0;
		end = R != 0 ? seg_starts[R] : 0;
	}
	const bit_field vf = field_of(test->val_shift, test->val_bits);
	uint64_t K = 0, D = 0, g = 0;
	for (uint64_t j = first; j < end; j++) {
		// the segments that begin here hold what was counted before this position
		for (; seg_starts != nullptr && g <= R && seg_starts[g] <= j; g++) {
			if (out->kept_starts != nullptr)
				out->kept_starts[g] = K;
			if (out->dropped_starts != nullptr)
				out->dropped_starts[g] = D;
		}
		const uint32_t i = index[j];
		bool pass = true;
		if (test->flags != nullptr)
			pass = pass && test->flags[j] == 0;
		if (test->rank != nullptr)
			pass = pass && test->rank[j] < test->rank_below;
		if (test->ret != nullptr) {
			if (i < count) {
				const uint64_t v = vf.of(test->ret[i]);
				pass = pass && test->val_lo <= v && v <= test->val_hi;
			} else {
				pass = false;
			}
		}
		if (pass) {
			if (out->kept != nullptr)
				out->kept[K] = i;
			K++;
		} else {
			if (out->dropped != nullptr)
				out->dropped[D] = i;
			D++;
		}
	}
	// (and those that begin where the last one ends, entry R among them)
	for (; seg_starts != nullptr && g <= R; g++) {
		if (out->kept_starts != nullptr)
			out->kept_starts[g] = K;
		if (out->dropped_starts != nullptr)
			out->dropped_starts[g] = D;
	}
	for (uint64_t j = K; j < n && out->kept != nullptr; j++)
		out->kept[j] = EBPF_NO_PACKET;
	for (uint64_t j = D; j < n && out->dropped != nullptr; j++)
		out->dropped[j] = EBPF_NO_PACKET;
	info[0] = K;
	info[1] = D;
	return 0;
}

EBPF_EXPORT int
ebpf_batch_filter_dev(int device, const struct ebpf_batch_test *test, uint64_t count,
		      const uint32_t *index_dev, uint64_t n, const uint64_t *seg_starts_dev,
		      uint64_t seg_cap, const uint64_t *nseg_dev, const struct ebpf_batch_parts *out,
		      uint64_t *info_dev, void *stream)
{
	int err = filter_args(test, count, index_dev, n, seg_starts_dev, seg_cap, nseg_dev, out,
			      info_dev);
	if (err || (err = check_device(device)))
		return err;
	return on_device(device, stream, filter_scratch_bytes(n), "filter kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		return launch_filter(*test, count, index_dev, n, seg_starts_dev, seg_cap, nseg_dev, *out,
				     info_dev, scratch, st);
	});
}
