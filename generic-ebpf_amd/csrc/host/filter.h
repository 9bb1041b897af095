// filter.h — shared by the host runtime and filter.hip (ebpf_batch_filter_dev: the entries of a
// list that pass a test, and those that do not, as lists with their segments, on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"

// Library scratch of one call, in u32 words:
//   0          K, the positions that pass (filter_carry writes it); 1 .. 3 unused
//   4 ..       a word per tile of STEER_TILE list positions: the tile's passing positions, then
//              (filter_carry) those of the tiles before it
//   then       128 words per tile: a bit per position, set iff it takes part and passes; a
//              thread's 16 consecutive positions are 16 bits
// A call over no position still has one tile.  Any contents on entry.
constexpr uint32_t FILTER_HEAD_WORDS = 4;
constexpr uint32_t FILTER_TILE_WORDS = 1 + 128;
size_t filter_scratch_bytes(uint64_t n);
// The whole call (arguments checked; n, count and seg_cap <= 0xffffffff).  seg_starts NULL: an
// unsegmented list, every position takes part (then neither table is given).  Nothing
// synchronises.
hipError_t launch_filter(const struct ebpf_batch_test &test, uint64_t count, const uint32_t *index,
			 uint64_t n, const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
			 const struct ebpf_batch_parts &out, uint64_t *info, uint32_t *scratch,
			 hipStream_t stream);
