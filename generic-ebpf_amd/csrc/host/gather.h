// gather.h — shared by the host runtime and gather.hip (ebpf_batch_gather_dev: a list of a batch's
// packets copied into a dense batch on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"

// Packet i's start and its length on the host (gather.cpp, scatter.cpp): the run functions' rule
// (0 for an end below the start or 2^32 bytes or more past it) and 0 for an index past the batch.
inline uint32_t
packet_span(const struct ebpf_pkt_batch &b, uint32_t i, uint64_t *start)
{
	uint64_t s = 0, e = 0;
	if (i < b.count) {
		if (b.offsets == nullptr) {
			s = (uint64_t)i * b.stride;
			e = s + b.stride;
		} else if (b.flags & EBPF_BATCH_EXTENTS) {
			s = b.offsets[2 * (uint64_t)i];
			e = b.offsets[2 * (uint64_t)i + 1];
		} else {
			s = b.offsets[i];
			e = b.offsets[(uint64_t)i + 1];
		}
	}
	*start = s;
	return (e < s || e - s > 0xffffffffull) ? 0u : (uint32_t)(e - s);
}

// List entries per tile of the packed form's length and offset passes: one workgroup of 256 sums,
// and later scans, GATHER_TILE consecutive entries.
constexpr uint32_t GATHER_TILE = 4096;
// Past this many tiles the scan of the tile sums takes two levels (segments of tiles, then the
// tiles of each).
constexpr uint32_t GATHER_SEGS = 256;

// The row path's condition: both sides fixed at one stride, a multiple of 16, on 16-byte bases.
bool gather_takes_rows(const struct ebpf_pkt_batch &b, uint32_t out_stride, const void *out);
// Scratch of one packed gather, in bytes: a u64 sum per tile and (two levels) per segment.  Any
// contents on entry.  0 for the strided form.
size_t gather_scratch_bytes(uint64_t n, uint32_t out_stride);
// The gather of ebpf_gpu.h "Gathering packets into a dense batch"; device pointers, n >= 1,
// n <= 0xffffffff, b.count >= 1, the strided form's n * out_stride <= out_bytes checked.
hipError_t launch_gather(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n,
			 uint32_t out_stride, void *out, uint64_t out_bytes, uint64_t *out_offsets,
			 uint64_t *scratch, hipStream_t stream);
