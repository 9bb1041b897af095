// scatter.cpp — a dense batch's packets written back into the batch, and a second stage's results
// written into the batch's ret / faults (ebpf_gpu.h "Scattering a dense batch back"): on the host
// (ebpf_batch_scatter, ebpf_batch_merge, the statement of the semantics) and on the device
// (ebpf_batch_scatter_dev, ebpf_batch_merge_dev, scatter.hip).
#include <string.h>

#include "gather.h"
#include "runtime.h"
#include "scatter.h"

namespace {

int
scatter_args(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n, uint32_t in_stride,
	     const void *in, uint64_t in_bytes, const uint64_t *in_offsets)
{
	// (EBPF_BATCH_HIST_OVERWRITE: as ebpf_batch_gather, no concern of the packets' places)
	int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
	if (err)
		return err;
	if (n != 0 && (index == nullptr || in == nullptr))
		return fail(EINVAL, "index or in is NULL");
	if (in_stride != 0 && in_offsets != nullptr)
		return fail(EINVAL, "the strided form takes no in_offsets");
	if (in_stride == 0 && in_offsets == nullptr)
		return fail(EINVAL, "the packed form needs in_offsets");
	if (n > 0xffffffffull)
		return fail(E2BIG, "n above 2^32 - 1");
	if (in_stride != 0 && n > in_bytes / in_stride)
		return fail(EINVAL, "n * in_stride exceeds in_bytes");
	return 0;
}

int
merge_args(const uint64_t *ret, const uint32_t *index, uint64_t n, const uint64_t *ret2)
{
	if (n != 0 && (ret == nullptr || ret2 == nullptr || index == nullptr))
		return fail(EINVAL, "ret, ret2 or index is NULL");
	if (n > 0xffffffffull)
		return fail(E2BIG, "n above 2^32 - 1");
	return 0;
}

} // namespace

EBPF_EXPORT int
ebpf_batch_scatter(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n,
		   uint32_t in_stride, const void *in, uint64_t in_bytes, const uint64_t *in_offsets)
{
	int err = scatter_args(batch, index, n, in_stride, in, in_bytes, in_offsets);
	if (err)
		return err;
	uint8_t *data = static_cast<uint8_t *>(const_cast<void *>(batch->data));
	const uint8_t *src = static_cast<const uint8_t *>(in);
	for (uint64_t j = 0; j < n; j++) {
		uint64_t s, at;
		const uint32_t len = packet_span(*batch, index[j], &s);
		uint64_t m; // the slot's length
		if (in_stride != 0) {
			at = j * in_stride;
			m = in_stride;
		} else {
			at = in_offsets[j];
			const uint64_t e = in_offsets[j + 1];
			m = (e < at || e - at > 0xffffffffull) ? 0 : e - at;
			m = std::min(m, at < in_bytes ? in_bytes - at : 0);
		}
		const uint64_t k = std::min<uint64_t>(len, m);
		if (k != 0)
			memcpy(data + s, src + at, k);
	}
	return 0;
}

EBPF_EXPORT int
ebpf_batch_scatter_dev(int device, const struct ebpf_pkt_batch *batch, const uint32_t *index_dev,
		       uint64_t n, uint32_t in_stride, const void *in_dev, uint64_t in_bytes,
		       const uint64_t *in_offsets_dev, void *stream)
{
	int err = scatter_args(batch, index_dev, n, in_stride, in_dev, in_bytes, in_offsets_dev);
	if (err || (err = check_device(device)))
		return err;
	if (n == 0 || batch->count == 0) // (an empty batch: every length is 0)
		return 0;
	return on_device(device, stream, 0, "scatter kernels", [&](hipStream_t st, uint32_t *) {
		return launch_scatter(*batch, index_dev, n, in_stride, in_dev, in_bytes, in_offsets_dev, st);
	});
}

EBPF_EXPORT int
ebpf_batch_merge(uint64_t *ret, uint8_t *faults, uint64_t count, const uint32_t *index, uint64_t n,
		 const uint64_t *ret2, const uint8_t *faults2)
{
	int err = merge_args(ret, index, n, ret2);
	if (err)
		return err;
	for (uint64_t j = 0; j < n; j++) {
		if (index[j] >= count)
			continue;
		ret[index[j]] = ret2[j];
		if (faults != nullptr)
			faults[index[j]] = faults2 != nullptr ? faults2[j] : 0;
	}
	return 0;
}

EBPF_EXPORT int
ebpf_batch_merge_dev(int device, uint64_t *ret_dev, uint8_t *faults_dev, uint64_t count,
		     const uint32_t *index_dev, uint64_t n, const uint64_t *ret2_dev,
		     const uint8_t *faults2_dev, void *stream)
{
	int err = merge_args(ret_dev, index_dev, n, ret2_dev);
	if (err || (err = check_device(device)))
		return err;
	if (n == 0 || count == 0)
		return 0;
	return on_device(device, stream, 0, "merge kernel", [&](hipStream_t st, uint32_t *) {
		return launch_merge(ret_dev, faults_dev, count, index_dev, n, ret2_dev, faults2_dev, st);
	});
}
