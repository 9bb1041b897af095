// rollup.h — shared by the host runtime and rollup.hip (ebpf_batch_rollup_dev: the runs of equal
// key prefix of a keyed sequence reduced, a segmented reduction whose segments the keys give).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"
#include "host/wants_values.h"

// The tiles of one call: those of the cap entries, STEER_TILE each; a sequence of no entry still
// has one.  Library scratch of one call, any contents on entry: a row of ROLLUP_ROW_WORDS u64 a
// tile,
//   0          the runs that begin in the tile (rollup_tiles)
//   1          the runs that begin in the tiles before it (rollup_carry)
//   2 .. 5     sum, min, max, bits over the tile's entries before the first that begins a run (all
//              of them if none does)
//   6          the position of the last entry of the tile that begins a run, or ROLLUP_NO_RUN
//   7 .. 10    sum, min, max, bits over the entries from that one on
//   11 .. 14   sum, min, max, bits of the run that is open where the tile begins, over the entries
//              before the tile (rollup_carry)
//   15         that run's first position (rollup_carry)
// 2 .. 5, 7 .. 10 and 11 .. 14 are written and read only when a value output is wanted.
constexpr uint32_t ROLLUP_ROW_WORDS = 16;
constexpr uint64_t ROLLUP_NO_RUN = ~0ull;
size_t rollup_scratch_bytes(uint64_t cap);
// The whole call (arguments checked; cap and out_cap <= 0xffffffff).  Nothing synchronises.
hipError_t launch_rollup(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
			 uint32_t flags, uint32_t key_shift, uint32_t val_shift, uint32_t val_bits,
			 uint64_t out_cap, const struct ebpf_batch_rolls &out, uint64_t *info,
			 uint64_t *scratch, hipStream_t stream);
