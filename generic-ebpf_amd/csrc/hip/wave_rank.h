// wave_rank.h — the tile shape and the wave-ranking helpers of the stable multisplits: steer.hip
// (a batch by verdict class) and group.hip (one radix pass by digit).  A class is a number below
// 2^CLASS_BITS; within a 64-packet chunk every lane learns which lanes hold its class from one
// ballot per bit in which the wave's classes differ at all, and its rank is the population of
// that mask below it.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host/steer.h"

namespace wave_rank {

constexpr uint32_t CLASS_BITS = 9;
constexpr uint32_t THREADS = 256;
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t WAVE_SPAN = STEER_TILE / WAVES; // packets of a tile that one wave owns
constexpr uint32_t CHUNKS = WAVE_SPAN / 64;
constexpr uint32_t NONE = ~0u;                     // the class of a lane past the batch's end
static_assert(STEER_TILE % THREADS == 0 && WAVE_SPAN % 64 == 0, "tile shape");

// ret and faults of packets first, first + step, ...  Every load is issued before the first is
// used — a packet past the end reads the last packet instead, so no load sits behind a branch —
// and the wave then waits for memory once, not once per packet.
template <bool FAULTS, uint32_t N>
__device__ __forceinline__ void
load_verdicts(const uint64_t *__restrict__ ret, const uint8_t *__restrict__ faults, uint64_t count,
	      uint64_t first, uint32_t step, uint64_t (&r)[N], uint32_t (&f)[N])
{
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		const uint64_t i = first + k * step;
		const uint64_t at = i < count ? i : count - 1;
		r[k] = ret[at];
		f[k] = FAULTS ? faults[at] : 0;
	}
}

__device__ __forceinline__ uint32_t
below(uint64_t mask)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// The bits of the class in which the wave's packets (N a lane) differ: a bit that some packet
// has set and some packet has clear.  Wave-uniform; 2 ballots a bit, once per tile.
template <uint32_t N>
__device__ __forceinline__ uint32_t
varying_bits(const uint32_t (&cls)[N])
{
	uint32_t some = 0, every = NONE;
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		some |= cls[k] == NONE ? 0u : cls[k];
		every &= cls[k]; // (NONE is all ones)
	}
	uint32_t vary = 0;
#pragma unroll
	for (uint32_t k = 0; k < CLASS_BITS; k++)
		if (__ballot((some >> k) & 1) != 0 && __ballot(!((every >> k) & 1)) != 0)
			vary |= 1u << k;
	return __builtin_amdgcn_readfirstlane(vary);
}

// The lanes of the wave whose class is this lane's (itself included); lanes of class NONE match
// nothing and nobody.  One ballot per bit of `vary`, the bits in which the wave's classes may
// differ: a lane keeps the ballot or its complement according to its own bit.
__device__ __forceinline__ uint64_t
match_class(uint32_t cls, uint32_t vary)
{
	const uint64_t all = __ballot(cls != NONE);
	uint64_t m = all;
#pragma unroll
	for (uint32_t k = 0; k < CLASS_BITS; k++) {
		if (!(vary & (1u << k))) // (a scalar test: skipping a bit costs no vector work)
			continue;
		const bool bit = (cls >> k) & 1;
		const uint64_t b = __ballot(bit);
		m &= bit ? b : ~b;
	}
	return cls != NONE ? m : 0;
}

} // namespace wave_rank
