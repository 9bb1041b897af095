// scatter.h — shared by the host runtime and scatter.hip (ebpf_batch_scatter_dev: a dense batch's
// packets written back into the batch; ebpf_batch_merge_dev: a second stage's results written into
// the batch's ret / faults).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ebpf_pkt_batch;

// The row path's condition: both sides fixed at one stride, a multiple of 16, on 16-byte bases.
bool scatter_takes_rows(const struct ebpf_pkt_batch &b, uint32_t in_stride, const void *in);
// The scatter of ebpf_gpu.h "Scattering a dense batch back"; device pointers, n >= 1,
// n <= 0xffffffff, b.count >= 1, the strided form's n * in_stride <= in_bytes checked.
hipError_t launch_scatter(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n,
			  uint32_t in_stride, const void *in, uint64_t in_bytes,
			  const uint64_t *in_offsets, hipStream_t stream);
// The merge of the same section; device pointers, 1 <= n <= 0xffffffff, count >= 1; faults and
// faults2 may be NULL.
hipError_t launch_merge(uint64_t *ret, uint8_t *faults, uint64_t count, const uint32_t *index,
			uint64_t n, const uint64_t *ret2, const uint8_t *faults2, hipStream_t stream);
