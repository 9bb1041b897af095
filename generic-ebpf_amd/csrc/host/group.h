// group.h — shared by the host runtime and group.hip (ebpf_batch_group_dev: a batch's packets
// sorted by a key field of ret on the device, and the table of its groups).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// How a key of key_bits bits is sorted: `passes` radix passes, least significant digit first,
// every digit `digit_bits` wide but the last, which takes what is left; keys travel as words of
// `key_bytes` bytes.
struct group_plan {
	uint32_t passes, digit_bits, key_bytes;
};
group_plan group_plan_of(uint32_t key_bits);
// The caller's temporary storage (ebpf_batch_group_tmp_bytes): `keys` key buffers and, with more
// than one pass, a second index buffer, each of group_padded(count) entries.
inline uint64_t
group_padded(uint64_t count)
{
	return (count + 63) & ~63ull;
}
size_t group_tmp_bytes(uint64_t count, uint32_t key_bits);
// Library scratch of one call, in u32 words: the passes' starts, their tile rows
// (steer_scratch_words) and the group table's head counts, one per tile.  Any contents on entry.
size_t group_scratch_words(uint64_t count);
// The whole call (count >= 1, count <= 0xffffffff, arguments checked); nothing synchronises.
hipError_t launch_group(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t key_shift,
			uint32_t key_bits, uint32_t *index, uint64_t group_cap, uint64_t *group_keys,
			uint64_t *group_starts, uint64_t *info, void *tmp, uint32_t *scratch,
			hipStream_t stream);
