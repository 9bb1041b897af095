// table.h — shared by the host runtime and table.hip (ebpf_batch_lookup_dev and
// ebpf_batch_accumulate_dev: a sorted table of keys and values on the device, a batch's keys looked
// up in it and a batch's per-key sums merged into it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ebpf_gpu.h"

// The tiles of one accumulate call: those of the table's cap entries, then those of the batch's
// key_cap keys, STEER_TILE entries each; a sequence of no entry still has one tile.
// Library scratch of one call, in u32 words, any contents on entry:
//   0, 1       the kept entries of the table's side and of the batch's (table_carry writes them);
//              2 .. 7 unused
//   8 ..       128 words per tile: a bit per entry, set iff it is a kept candidate, in entry order
//              (64 words of 64 bits)
//   then       32 words per tile: per 64-bit word the set bits of the tile's words before it (u16)
//   then       2 words per tile: the tile's kept entries, then (table_carry) those of its side's
//              tiles before it; and, of a batch tile, the keys that the table does not hold
// The lookup needs none.
constexpr uint32_t TABLE_HEAD_WORDS = 8;
constexpr uint32_t TABLE_TILE_WORDS = 128 + 32 + 2;
size_t accumulate_scratch_bytes(uint64_t cap, uint64_t key_cap);
// The whole calls (arguments checked; caps and key_cap <= 0xffffffff; a NULL table is passed as
// one of cap 0).  Nothing synchronises.
hipError_t launch_lookup(const struct ebpf_key_table &table, const uint64_t *keys, uint64_t key_cap,
			 const uint64_t *nkeys, uint32_t mode, uint64_t missing, uint64_t limit,
			 uint64_t *vals_out, uint32_t *pos_out, hipStream_t stream);
hipError_t launch_accumulate(const struct ebpf_key_table &in, const uint64_t *keys,
			     const uint64_t *adds, uint64_t key_cap, const uint64_t *nkeys,
			     uint32_t op, uint64_t keep_lo, uint64_t keep_hi,
			     const struct ebpf_key_table &out, uint64_t *info, uint32_t *scratch,
			     hipStream_t stream);
