// scan.h — shared by the host runtime and scan.hip (ebpf_batch_scan_dev: running totals per
// segment of a list of a batch's packets on the device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"

// A tile's scratch row, in u64 words (72 bytes per tile of STEER_TILE list entries):
//   0, 1  bytes and sum over the tile's leading positions, those before the first position at
//         which a segment begins (all of them if none does)
//   2     does a segment begin in the tile
//   3, 4  bytes and sum over the positions from the last such on
//   5     the number of leading positions that a segment covers (0: nothing to fix up)
//   6     that segment's budget
//   7, 8  bytes and sum that the segment accumulated in the tiles before (scan_carry writes them)
constexpr uint32_t SCAN_ROW_WORDS = 9;
// Library scratch of one call, in bytes: a row per tile.  Any contents on entry.
size_t scan_scratch_bytes(uint64_t n);
// The whole call (arguments checked, n >= 1, n, count and seg_cap <= 0xffffffff, at least one
// output wanted).  count == 0: no entry has a length or a value, batch and ret are not used and
// bytes_before, sum_before and over are all 0.  scratch is not used where neither lengths nor
// values are (rank alone, or count == 0).  Nothing synchronises.
hipError_t launch_scan(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
		       uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
		       const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		       const uint64_t *budgets, const struct ebpf_batch_scans &out, uint64_t *scratch,
		       hipStream_t stream);
