// gather.h — shared by the host runtime and gather.hip (ebpf_batch_gather_dev: a list of a batch's
// packets copied into a dense batch on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ebpf_pkt_batch;

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
