// gather.cpp — a list of a batch's packets copied into a dense batch (ebpf_gpu.h "Gathering
// packets into a dense batch"): on the host (ebpf_batch_gather, the statement of the semantics)
// and on the device (ebpf_batch_gather_dev, gather.hip).
#include <string.h>

#include "gather.h"
#include "runtime.h"

namespace {

int
gather_args(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n, uint32_t out_stride,
	    const void *out, uint64_t out_bytes, const uint64_t *out_offsets)
{
	// (EBPF_BATCH_HIST_OVERWRITE: as ebpf_batch_select_dev, no concern of the packets' places)
	int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
	if (err)
		return err;
	if (n != 0 && (index == nullptr || out == nullptr))
		return fail(EINVAL, "index or out is NULL");
	if (out_stride != 0 && out_offsets != nullptr)
		return fail(EINVAL, "the strided form takes no out_offsets");
	if (out_stride == 0 && out_offsets == nullptr)
		return fail(EINVAL, "the packed form needs out_offsets");
	if (n > 0xffffffffull)
		return fail(E2BIG, "n above 2^32 - 1");
	if (out_stride != 0 && n > out_bytes / out_stride)
		return fail(EINVAL, "n * out_stride exceeds out_bytes");
	return 0;
}

} // namespace

EBPF_EXPORT int
ebpf_batch_gather(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n,
		  uint32_t out_stride, void *out, uint64_t out_bytes, uint64_t *out_offsets)
{
	int err = gather_args(batch, index, n, out_stride, out, out_bytes, out_offsets);
	if (err)
		return err;
	const uint8_t *data = static_cast<const uint8_t *>(batch->data);
	uint8_t *o = static_cast<uint8_t *>(out);
	if (out_stride != 0) {
		for (uint64_t j = 0; j < n; j++) {
			uint64_t s;
			const uint32_t len = std::min(packet_span(*batch, index[j], &s), out_stride);
			uint8_t *slot = o + j * out_stride;
			if (len != 0)
				memcpy(slot, data + s, len);
			memset(slot + len, 0, out_stride - len);
		}
		return 0;
	}
	uint64_t at = 0;
	for (uint64_t j = 0; j < n; j++) {
		uint64_t s;
		const uint32_t len = packet_span(*batch, index[j], &s);
		out_offsets[j] = at;
		const uint64_t room = at < out_bytes ? out_bytes - at : 0;
		if (len != 0 && room != 0)
			memcpy(o + at, data + s, std::min<uint64_t>(len, room));
		at += len;
	}
	out_offsets[n] = at;
	return at <= out_bytes ? 0 : fail(ENOSPC, "out_bytes below the packets' total: out_offsets[n]");
}

EBPF_EXPORT int
ebpf_batch_gather_dev(int device, const struct ebpf_pkt_batch *batch, const uint32_t *index_dev,
		      uint64_t n, uint32_t out_stride, void *out_dev, uint64_t out_bytes,
		      uint64_t *out_offsets_dev, void *stream)
{
	int err = gather_args(batch, index_dev, n, out_stride, out_dev, out_bytes, out_offsets_dev);
	if (err || (err = check_device(device)))
		return err;
	if (n == 0 && out_stride != 0)
		return 0;
	const bool empty = n == 0 || batch->count == 0; // every length is 0: zero slots, or zero offsets
	return on_device(device, stream, empty ? 0 : gather_scratch_bytes(n, out_stride),
			 empty ? "hipMemsetAsync(gather)" : "gather kernels",
			 [&](hipStream_t st, uint32_t *scratch) {
		if (empty)
			return out_stride != 0
				   ? hipMemsetAsync(out_dev, 0, n * out_stride, st)
				   : hipMemsetAsync(out_offsets_dev, 0, (n + 1) * sizeof(uint64_t), st);
		return launch_gather(*batch, index_dev, n, out_stride, out_dev, out_bytes, out_offsets_dev,
				     reinterpret_cast<uint64_t *>(scratch), st);
	});
}
