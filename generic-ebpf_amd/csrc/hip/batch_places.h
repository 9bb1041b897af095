// batch_places.h — what gather.hip, scatter.hip, reduce.hip and scan.hip share: where a batch
// keeps its packets, the length rule, a workgroup's scan, the 16-byte load / store forms, and what
// the segmented kernels need of a list's segments (their number, the 64-way search, a tile's LDS
// slots, a thread's lengths and values).  Device code only; every file that includes it is compiled
// on its own, so everything here is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"

namespace {

constexpr uint32_t THREADS = 256;
constexpr uint32_t WAVES = THREADS / 64;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_any __attribute__((aligned(1))); // at any address: one unaligned 16-byte access

// where a batch keeps its packets (ebpf_pkt_batch without the data)
struct places {
	const uint64_t *offsets;
	uint64_t count;
	uint32_t stride;
	uint32_t extents;
};

// Packet i's start, and its length by the run functions' rule: 0 for an end below the start or
// 2^32 bytes or more past it, and for an index past the batch.
__device__ __forceinline__ void
span_of(const places &f, uint32_t i, uint64_t &start, uint32_t &len)
{
	uint64_t s = 0, e = 0;
	if (i < f.count) {
		if (f.offsets == nullptr) {
			s = (uint64_t)i * f.stride;
			e = s + f.stride;
		} else if (f.extents) {
			s = f.offsets[2 * (uint64_t)i];
			e = f.offsets[2 * (uint64_t)i + 1];
		} else {
			s = f.offsets[i];
			e = f.offsets[(uint64_t)i + 1];
		}
	}
	const uint64_t d = e - s;
	start = s;
	len = (e < s || (d >> 32) != 0) ? 0u : (uint32_t)d;
}

// The lengths of list entries first, first + THREADS, ... (0 past the list's end).  The index
// loads are issued together — an entry past the end re-reads the last one, so none sits behind a
// branch — and then the offsets loads, so that a lane waits for memory twice, not twice an entry.
template <uint32_t N>
__device__ __forceinline__ void
lens_of(const places &f, const uint32_t *__restrict__ index, uint64_t n, uint64_t first,
	uint32_t (&len)[N])
{
	uint32_t idx[N];
	uint64_t s[N], e[N];
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		const uint64_t j = first + k * THREADS;
		idx[k] = index[j < n ? j : n - 1];
	}
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		s[k] = e[k] = 0;
		if (first + k * THREADS >= n || idx[k] >= f.count)
			continue;
		if (f.offsets == nullptr) {
			e[k] = f.stride;
		} else if (f.extents) {
			s[k] = f.offsets[2 * (uint64_t)idx[k]];
			e[k] = f.offsets[2 * (uint64_t)idx[k] + 1];
		} else {
			s[k] = f.offsets[idx[k]];
			e[k] = f.offsets[(uint64_t)idx[k] + 1];
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		const uint64_t d = e[k] - s[k];
		len[k] = (e[k] < s[k] || (d >> 32) != 0) ? 0u : (uint32_t)d;
	}
}

// The sum of v over the threads before this one; total = over them all.  wsum: WAVES words of
// LDS, free again on return.
__device__ __forceinline__ uint64_t
block_scan(uint64_t v, uint64_t *wsum, uint64_t &total)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t inc = v; // inclusive scan over the wave
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint64_t up = __shfl_up((unsigned long long)inc, d);
		if (lane >= d)
			inc += up;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	uint64_t before = 0, all = 0;
#pragma unroll
	for (uint32_t q = 0; q < WAVES; q++) {
		const uint64_t s = wsum[q];
		before += q < w ? s : 0;
		all += s;
	}
	__syncthreads();
	total = all;
	return before + inc - v;
}

// The number of segments of a list (ebpf_gpu.h): a short table holds no end for its last group.
__device__ __forceinline__ uint64_t
segments_of(uint64_t cap, const uint64_t *__restrict__ nseg)
{
	if (nseg == nullptr)
		return cap;
	const uint64_t g = *nseg;
	return g <= cap ? g : (cap != 0 ? cap - 1 : 0);
}

// How many of S[0 .. m) are <= p, for a non-decreasing S: a wave's 64-way search, every lane the
// same answer.  For any other S it still ends, with an answer in [0, m], having read only S[0 .. m).
__device__ __forceinline__ uint64_t
upper(const uint64_t *__restrict__ S, uint64_t m, uint64_t p)
{
	const uint32_t lane = threadIdx.x & 63;
	uint64_t lo = 0, hi = m;
	while (lo < hi) {
		const uint64_t step = (hi - lo + 63) / 64;
		const uint64_t at = lo + lane * step;
		const bool le = at < hi && S[at] <= p;
		const uint64_t b = ~__ballot(le);
		const uint32_t c = b == 0 ? 64u : (uint32_t)__builtin_ctzll(b); // the probes <= p, from lo on
		if (c == 0)
			break;
		const uint64_t end = lo + c * step;
		lo += (c - 1) * step + 1;
		hi = end < hi ? end : hi;
	}
	return lo;
}

// Where position q of a tile sits in LDS: a thread's 16 positions are a row, and a word of
// padding a row keeps both the tile-order and the row-order accesses off one another's banks.
__device__ __forceinline__ uint32_t
slot(uint32_t q)
{
	return q + (q >> 4);
}

// A thread's N list entries idx[k]: their lengths (0 where !has[k]: past the list's end, or past
// the batch's) and their value fields of ret (ret has f.count >= 1 entries; an entry past the
// batch reads the last one, and its value is not used).  The ret loads are issued together, then
// the offsets loads, as lens_of's.
template <bool LENS, bool VALS, uint32_t N>
__device__ __forceinline__ void
fields_of(const places &f, const uint64_t *__restrict__ ret, uint32_t val_shift, uint64_t val_mask,
	  const uint32_t (&idx)[N], const bool (&has)[N], uint32_t (&len)[N], uint64_t (&val)[N])
{
	uint64_t s[N], e[N];
	if (VALS) {
#pragma unroll
		for (uint32_t k = 0; k < N; k++)
			val[k] = ret[idx[k] < f.count ? idx[k] : f.count - 1];
#pragma unroll
		for (uint32_t k = 0; k < N; k++)
			val[k] = (val[k] >> val_shift) & val_mask;
	}
	if (LENS) {
#pragma unroll
		for (uint32_t k = 0; k < N; k++) {
			s[k] = e[k] = 0;
			if (!has[k])
				continue;
			if (f.offsets == nullptr) {
				e[k] = f.stride;
			} else if (f.extents) {
				s[k] = f.offsets[2 * (uint64_t)idx[k]];
				e[k] = f.offsets[2 * (uint64_t)idx[k] + 1];
			} else {
				s[k] = f.offsets[idx[k]];
				e[k] = f.offsets[(uint64_t)idx[k] + 1];
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < N; k++) {
			const uint64_t d = e[k] - s[k];
			len[k] = (e[k] < s[k] || (d >> 32) != 0) ? 0u : (uint32_t)d;
		}
	}
}

// 16 bytes at a 16-byte-aligned address
template <bool NT>
__device__ __forceinline__ u32x4
load16(const uint8_t *p)
{
	const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
	return NT ? __builtin_nontemporal_load(q) : *q;
}

// 16 bytes at any address
template <bool NT>
__device__ __forceinline__ u32x4
load16_any(const uint8_t *p)
{
	const u32x4_any *q = reinterpret_cast<const u32x4_any *>(p);
	return NT ? __builtin_nontemporal_load(q) : *q;
}

template <bool NT>
__device__ __forceinline__ void
store16(uint8_t *p, u32x4 v)
{
	u32x4 *q = reinterpret_cast<u32x4 *>(p);
	if (NT)
		__builtin_nontemporal_store(v, q);
	else
		*q = v;
}

inline places
places_of(const struct ebpf_pkt_batch &b)
{
	return {b.offsets, b.count, b.stride, (b.flags & EBPF_BATCH_EXTENTS) ? 1u : 0u};
}

} // namespace
