// reduce.h — shared by the host runtime and reduce.hip (ebpf_batch_reduce_dev: per-segment sums of
// a list of a batch's packets on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"
#include "host/wants_values.h"

// A scratch row, in u64 words: bytes, sum, min, max, bits, and one word about the tile.
constexpr uint32_t REDUCE_ROW_WORDS = 6;
// Library scratch of one call, in bytes: two rows per tile of STEER_TILE list entries (what is
// open at the tile's two edges).  Any contents on entry.
size_t reduce_scratch_bytes(uint64_t n);
// The whole call (arguments checked, seg_cap >= 1, n, count and seg_cap <= 0xffffffff, at least
// one output wanted; n == 0 writes the identities alone, and a batch with count == 0 is passed
// as n == 0: none of its entries has a length or a value).  scratch is not used for n == 0.
// Nothing synchronises.
hipError_t launch_reduce(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
			 uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
			 const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
			 const struct ebpf_batch_sums &out, uint64_t *scratch, hipStream_t stream);
