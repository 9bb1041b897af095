// bit_field.h — a bit field of a 64-bit verdict: the value of reduce, scan and filter and the key
// of group, on the host and on the device (constexpr: one definition compiles for both).
#pragma once
#include <stdint.h>

struct bit_field {
	uint32_t shift;
	uint64_t mask;
	constexpr uint64_t
	of(uint64_t v) const
	{
		return (v >> shift) & mask;
	}
};

// bits in [1, 64], and the field inside the 64
constexpr bool
field_ok(uint32_t shift, uint32_t bits)
{
	return bits >= 1 && bits <= 64 && shift <= 64 - bits;
}

constexpr bit_field
field_of(uint32_t shift, uint32_t bits)
{
	return {shift, bits >= 64 ? ~0ull : (1ull << bits) - 1};
}
