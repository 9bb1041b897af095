// top.h — shared by the host runtime and top.hip (ebpf_batch_top_dev: the k best entries of a
// keyed sequence by a bit field of the value, a radix select on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"

// The tiles of one call: those of the cap entries, STEER_TILE each; a sequence of no entry still
// has one.  The select's histograms are a row a run of tiles: at most TOP_ROWS rows, every row the
// same number of consecutive tiles (one tile a row up to TOP_ROWS tiles).
// Library scratch of one call, in u32 words, any contents on entry:
//   0, 1       the prefix found so far, at last the cut T (a u64, in the order's own terms: the
//              field, complemented for EBPF_TOP_SMALLEST)
//   2          what is still wanted below the prefix, at last e = the entries equal to T to take
//   3          m = min(k, N)
//   4, 5       the entries above T and those equal to T (top_carry); 6 .. 15 unused
//   16 ..      EBPF_TOP_MAX candidates: their fields (u64 each), then their positions (u32 each)
//   then       256 words per row: the current digit's histogram
//   then       4 words per tile: the tile's entries above T and equal to T, then (top_carry) those
//              of the tiles before it
constexpr uint32_t TOP_HEAD_WORDS = 16;
constexpr uint32_t TOP_ROWS = 1024;
constexpr uint32_t TOP_TILE_WORDS = 4;
size_t top_scratch_bytes(uint64_t cap);
// The whole call (arguments checked; cap <= 0xffffffff, k <= EBPF_TOP_MAX).  Nothing synchronises.
hipError_t launch_top(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
		      uint32_t flags, uint32_t val_shift, uint32_t val_bits, uint64_t k,
		      const struct ebpf_batch_tops &out, uint64_t *info, uint32_t *scratch,
		      hipStream_t stream);
