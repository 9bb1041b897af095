// batch_places.h — what the list kernels share: where a batch keeps its packets and the length
// rule (gather.hip, scatter.hip, and through seg_tile.h reduce.hip and scan.hip), a workgroup's
// scan (those four and filter.hip), and the 16-byte load / store forms (gather.hip, scatter.hip,
// scan.hip, filter.hip).  What only the segmented kernels need is in seg_tile.h.  Device code only;
// every file that includes it is compiled on its own, so everything here is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

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

// The sum of v over the threads before this one, of a workgroup of NW waves; total = over them
// all.  wsum: NW words of LDS, free again on return.  T, uint32_t or uint64_t, is wsum's: v
// converts to it.
template <uint32_t NW = WAVES, typename T>
__device__ __forceinline__ T
block_scan(std::common_type_t<T> v, T *wsum, T &total)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	T inc = v; // inclusive scan over the wave
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const T up = __shfl_up(inc, d);
		if (lane >= d)
			inc += up;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	T before = 0, all = 0;
#pragma unroll
	for (uint32_t q = 0; q < NW; q++) {
		const T s = wsum[q];
		before += q < w ? s : 0;
		all += s;
	}
	__syncthreads();
	total = all;
	return before + inc - v;
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
