// steer.cpp — the step after the verdict (ebpf_gpu.h "Steering a batch by verdict"): a batch's
// packets grouped by verdict class, on the host (ebpf_batch_steer) and on the device
// (ebpf_batch_steer_dev), and a packet list as an extents batch (ebpf_batch_select_dev).
#include "runtime.h"
#include "steer.h"

namespace {

int
steer_args(const uint64_t *ret, uint64_t count, const uint32_t *index, const uint64_t *starts)
{
	if (starts == nullptr || (count != 0 && (ret == nullptr || index == nullptr)))
		return fail(EINVAL, "ret, index or starts is NULL");
	if (count > 0xffffffffull)
		return fail(E2BIG, "count above 2^32 - 1: the packet index is 32 bits");
	return 0;
}

inline uint32_t
class_of(const uint64_t *ret, const uint8_t *faults, uint64_t i)
{
	if (faults && faults[i])
		return EBPF_HIST_BINS - 1;
	return ret[i] < 255 ? (uint32_t)ret[i] : 255u;
}

} // namespace

// A counting sort: the reference for the device kernels.
EBPF_EXPORT int
ebpf_batch_steer(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t *index,
		 uint64_t *starts)
{
	int err = steer_args(ret, count, index, starts);
	if (err)
		return err;
	uint64_t next[EBPF_HIST_BINS] = {0};
	for (uint64_t i = 0; i < count; i++)
		next[class_of(ret, faults, i)]++;
	uint64_t run = 0;
	for (uint32_t b = 0; b < EBPF_HIST_BINS; b++) {
		starts[b] = run;
		run += next[b];
		next[b] = starts[b];
	}
	starts[EBPF_HIST_BINS] = run;
	for (uint64_t i = 0; i < count; i++)
		index[next[class_of(ret, faults, i)]++] = (uint32_t)i;
	return 0;
}

EBPF_EXPORT int
ebpf_batch_steer_dev(int device, const uint64_t *ret_dev, const uint8_t *faults_dev, uint64_t count,
		     uint32_t *index_dev, uint64_t *starts_dev, void *stream)
{
	int err = steer_args(ret_dev, count, index_dev, starts_dev);
	if (err || (err = check_device(device)))
		return err;
	return on_device(device, stream, count != 0 ? steer_scratch_words(count) * sizeof(uint32_t) : 0,
			 count != 0 ? "steering kernels" : "hipMemsetAsync(starts)",
			 [&](hipStream_t st, uint32_t *scratch) {
		if (count == 0)
			return hipMemsetAsync(starts_dev, 0, EBPF_STEER_STARTS * sizeof(uint64_t), st);
		return launch_steer(ret_dev, faults_dev, count, index_dev, starts_dev, scratch, st);
	});
}

EBPF_EXPORT int
ebpf_batch_select_dev(int device, const struct ebpf_pkt_batch *batch, const uint32_t *index_dev,
		      uint64_t n, uint64_t *extents_dev, void *stream)
{
	// (the descriptor a batch was just run with may carry EBPF_BATCH_HIST_OVERWRITE: no concern
	// of the packets' places)
	int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
	if (err)
		return err;
	if (n != 0 && (index_dev == nullptr || extents_dev == nullptr))
		return fail(EINVAL, "index or extents is NULL");
	if ((err = check_device(device)))
		return err;
	if (n == 0)
		return 0;
	return on_device(device, stream, 0, "select kernel", [&](hipStream_t st, uint32_t *) {
		return launch_select(*batch, index_dev, n, extents_dev, st);
	});
}
