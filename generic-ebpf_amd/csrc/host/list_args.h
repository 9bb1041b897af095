// list_args.h — the argument rules that the list operations share on the host (reduce.cpp,
// scan.cpp, filter.cpp; group.cpp for its key; table.cpp, top.cpp and rollup.cpp for their
// entries): a bit field of ret, the 32-bit sizes, a batch and a list, a list's segment table and a
// keyed sequence's entries (ebpf_gpu.h).  The device states the two counts once more: seg_tile.h
// segments_of and entries_of.
#pragma once
#include <string>

#include "bit_field.h"
#include "runtime.h"

// name: "val" or "key"
inline int
check_field(uint32_t shift, uint32_t bits, const std::string &name = "val")
{
	if (!field_ok(shift, bits))
		return fail(EINVAL, name + "_bits outside [1, 64], or " + name + "_shift + " + name +
					"_bits above 64");
	return 0;
}

// a list position, a packet index and a segment number are 32 bits
inline int
check_sizes(uint64_t n, uint64_t count, uint64_t seg_cap)
{
	if (n > 0xffffffffull || count > 0xffffffffull || seg_cap > 0xffffffffull)
		return fail(E2BIG, "n, count or seg_cap above 2^32 - 1");
	return 0;
}

// What reduce and scan ask of the batch (needed for lengths alone), the list and the table.
inline int
check_list(const struct ebpf_pkt_batch *batch, uint64_t count, const uint32_t *index, uint64_t n,
	   const uint64_t *seg_starts, uint64_t seg_cap)
{
	if (batch != nullptr) {
		// (EBPF_BATCH_HIST_OVERWRITE: as ebpf_batch_select_dev, no concern of the packets' places)
		int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
		if (err)
			return err;
		if (batch->count != count)
			return fail(EINVAL, "batch->count differs from count");
	}
	if (n != 0 && index == nullptr)
		return fail(EINVAL, "index is NULL with n > 0");
	if (seg_cap != 0 && seg_starts == nullptr)
		return fail(EINVAL, "seg_starts is NULL with seg_cap > 0");
	return check_sizes(n, count, seg_cap);
}

// The number of segments of a list: a short table (*nseg > seg_cap) holds no end for its last group.
inline uint64_t
seg_count(const uint64_t *nseg, uint64_t seg_cap)
{
	return nseg == nullptr ? seg_cap : *nseg <= seg_cap ? *nseg : (seg_cap != 0 ? seg_cap - 1 : 0);
}

// The entries of a keyed sequence that take part: the rule above, or the table's, a short sequence
// (*n > cap) being its first cap entries.  (The device's statement: seg_tile.h entries_of.)
inline uint64_t
entry_count(const uint64_t *n, uint64_t cap, bool segments)
{
	return segments ? seg_count(n, cap) : n == nullptr ? cap : (*n < cap ? *n : cap);
}

inline int
check_segments(const uint64_t *seg_starts, uint64_t R, uint64_t seg_cap, uint64_t n)
{
	for (uint64_t g = 0; g < R; g++)
		if (seg_starts[g] > seg_starts[g + 1])
			return fail(EINVAL, "seg_starts decreases");
	if (seg_cap != 0 && seg_starts[R] > n)
		return fail(EINVAL, "seg_starts ends past n");
	return 0;
}
