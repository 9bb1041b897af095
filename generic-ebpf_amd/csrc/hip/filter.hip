// filter.hip — keeping part of a list (ebpf_batch_filter_dev): the entries whose position passes
// a test (a flag, a rank, a bit field of the verdict) in list order, those that fail likewise, and
// for each of the two lists the table of the segments it inherits.  DESIGN.md §2 "Keeping part of
// a list".
//
// The positions that take part are one range [c0, c1) of the list (what the segments cover), so
// how many of them lie before a position is arithmetic; only the passing ones are counted.
//   filter_tiles  one workgroup per tile of STEER_TILE list positions, a thread 16 consecutive
//                 ones.  Flags and ranks are neighbouring bytes and words: 16-byte loads; for the
//                 value test the index loads, then the ret loads, are issued together.  A thread's
//                 16 decisions are 16 bits; the tile's 4,096 bits and their count go to scratch,
//                 so that no later pass looks at the tests again.
//   filter_carry  one workgroup: an exclusive scan over the tiles' counts, two levels (a thread
//                 walks a run of tiles).  It leaves K in scratch and writes info.
//   filter_place  one workgroup per tile: reads the tile's bits and index entries, ranks every
//                 position from the popcounts of the threads' bits and a workgroup scan, and
//                 compacts the tile in LDS, passing entries first, so that neighbouring lanes
//                 store neighbouring entries of kept and dropped.  Workgroup t also fills what of
//                 tile t lies in the lists' tails, [K, n) and [D, n), with EBPF_NO_PACKET.  The
//                 table entries whose start lies in the tile are found with two 64-way searches
//                 and get the tile's base plus the count before that position (a thread's count in
//                 LDS plus a popcount); those at the end of the range, entry R and the empty
//                 segments before it, are workgroup 0's, in a strided loop.
// Every output entry is written by one thread, no atomic decides anything and no workgroup waits
// for another: the output is a function of the input alone.  For a table that is not
// non-decreasing, or that ends past n, c0 <= c1 <= n still holds, every table entry written is
// one of [0 .. R], and the list entries written are those of a good table with that range.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/filter.h"

namespace {

constexpr uint32_t BITS_WORDS = TILE / 32;
static_assert(FILTER_TILE_WORDS == 1 + BITS_WORDS, "a count and a bit per position");

typedef struct ebpf_batch_test tests;
typedef struct ebpf_batch_parts parts;

// The positions that take part, [c0, c1) with c0 <= c1 <= n whatever the table holds.  S NULL: an
// unsegmented list, all of [0, n).
struct cover {
	uint64_t c0, c1, R;
};

__device__ __forceinline__ cover
cover_of(const uint64_t *__restrict__ S, uint64_t cap, const uint64_t *__restrict__ nseg, uint64_t n)
{
	if (S == nullptr)
		return {0, n, 0};
	const uint64_t R = segments_of(cap, nseg);
	if (R == 0)
		return {0, 0, 0};
	const uint64_t a = S[0], b = seg_end(S, R, n);
	return {a < b ? a : b, b, R};
}

__device__ __forceinline__ uint64_t
clamp(uint64_t p, uint64_t lo, uint64_t hi)
{
	return p < lo ? lo : (p < hi ? p : hi);
}

// Bit k is set iff position j0 + k lies in [c0, c1), for k < 16.
__device__ __forceinline__ uint32_t
part_bits(uint64_t j0, const cover &c)
{
	const uint32_t lo = (uint32_t)(clamp(c.c0, j0, j0 + PER_THREAD) - j0);
	const uint32_t hi = (uint32_t)(clamp(c.c1, j0, j0 + PER_THREAD) - j0);
	return hi > lo ? ((1u << hi) - 1) & ~((1u << lo) - 1) : 0u;
}

// A thread's 16 consecutive words p[j0 .. j0 + 16): four 16-byte loads where the list has them
// all, else one by one (0 at and past n).  p is 4-byte aligned.
__device__ __forceinline__ void
words_of(const uint32_t *__restrict__ p, uint64_t j0, uint64_t n, uint32_t (&v)[PER_THREAD])
{
	if (j0 + PER_THREAD <= n) {
		const uint8_t *b = reinterpret_cast<const uint8_t *>(p + j0);
#pragma unroll
		for (uint32_t c = 0; c < 4; c++) {
			const u32x4 w = load16_any<false>(b + 16 * c);
#pragma unroll
			for (uint32_t k = 0; k < 4; k++)
				v[4 * c + k] = w[k];
		}
		return;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		v[k] = j0 + k < n ? p[j0 + k] : 0;
}

// Bit k is set iff flags[j0 + k] != 0 (clear at and past n).  flags has any alignment.
__device__ __forceinline__ uint32_t
flag_bits(const uint8_t *__restrict__ flags, uint64_t j0, uint64_t n)
{
	uint32_t set = 0;
	if (j0 + PER_THREAD <= n) {
		const u32x4 w = load16_any<false>(flags + j0);
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			set |= ((w[k / 4] >> (8 * (k % 4)) & 0xff) != 0 ? 1u : 0u) << k;
		return set;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		set |= (j0 + k < n && flags[j0 + k] != 0 ? 1u : 0u) << k;
	return set;
}

// Which of the three tests are given.  scratch: filter.h.  One tile at least (n == 0: it holds no
// position, and nothing of the inputs is read).
template <bool FLAGS, bool RANK, bool VAL>
__global__ void __launch_bounds__(THREADS)
filter_tiles(tests t, uint64_t val_mask, uint64_t count, const uint32_t *__restrict__ index,
	     uint64_t n, const uint64_t *__restrict__ S, uint64_t cap,
	     const uint64_t *__restrict__ nseg, uint32_t *__restrict__ scratch, uint32_t ntiles)
{
	__shared__ uint64_t wsum[WAVES];
	const uint32_t tid = threadIdx.x;
	const cover c = cover_of(S, cap, nseg, n);
	const uint64_t first = (uint64_t)blockIdx.x * TILE, j0 = first + tid * PER_THREAD;
	uint32_t *counts = scratch + FILTER_HEAD_WORDS;
	uint16_t *bits = reinterpret_cast<uint16_t *>(counts + ntiles) + (size_t)blockIdx.x * THREADS;
	// (the same for every thread) nothing of the tile takes part: nothing is read
	const bool live = first < c.c1 && first + TILE > c.c0;
	uint32_t pass = live ? part_bits(j0, c) : 0;
	if (live && (FLAGS || RANK || VAL)) {
		// every load is issued before the first is used: flags, ranks, index, then ret
		uint32_t fset = 0, rk[PER_THREAD], idx[PER_THREAD];
		uint64_t v[PER_THREAD];
		if (FLAGS)
			fset = flag_bits(t.flags, j0, n);
		if (RANK)
			words_of(t.rank, j0, n, rk);
		if (VAL && count != 0) {
			words_of(index, j0, n, idx);
#pragma unroll
			for (uint32_t k = 0; k < PER_THREAD; k++)
				v[k] = t.ret[idx[k] < count ? idx[k] : count - 1];
		}
		if (FLAGS)
			pass &= ~fset;
		if (RANK) {
#pragma unroll
			for (uint32_t k = 0; k < PER_THREAD; k++)
				pass &= ~((rk[k] < t.rank_below ? 0u : 1u) << k);
		}
		if (VAL && count != 0) {
#pragma unroll
			for (uint32_t k = 0; k < PER_THREAD; k++) {
				const uint64_t f = bit_field{t.val_shift, val_mask}.of(v[k]);
				const bool ok = idx[k] < count && t.val_lo <= f && f <= t.val_hi;
				pass &= ~((ok ? 0u : 1u) << k);
			}
		}
		if (VAL && count == 0) // (no entry has a value)
			pass = 0;
	}
	bits[tid] = (uint16_t)pass;
	uint64_t total;
	block_scan(__builtin_popcount(pass), wsum, total);
	if (tid == 0)
		counts[blockIdx.x] = (uint32_t)total;
}

// One workgroup: tile_counts_scan leaves in every tile's word the passing positions of the tiles
// before.  K <= n < 2^32: 32-bit sums.
__global__ void __launch_bounds__(CARRY_THREADS)
filter_carry(uint32_t *__restrict__ scratch, uint32_t ntiles, uint64_t n,
	     const uint64_t *__restrict__ S, uint64_t cap, const uint64_t *__restrict__ nseg,
	     uint64_t *__restrict__ info)
{
	__shared__ uint32_t wsum[CARRY_THREADS / 64];
	uint32_t *counts = scratch + FILTER_HEAD_WORDS;
	const uint32_t all = tile_counts_scan(counts, counts, 1, ntiles, wsum);
	if (threadIdx.x == 0) {
		const cover c = cover_of(S, cap, nseg, n);
		scratch[0] = all;
		info[0] = all;
		info[1] = c.c1 - c.c0 - all;
	}
}

// LISTS: kept or dropped is wanted; TABLES: kept_starts or dropped_starts is.  One of them is.
template <bool LISTS, bool TABLES>
__global__ void __launch_bounds__(THREADS)
filter_place(const uint32_t *__restrict__ scratch, uint32_t ntiles,
	     const uint32_t *__restrict__ index, uint64_t n, const uint64_t *__restrict__ S,
	     uint64_t cap, const uint64_t *__restrict__ nseg, parts out)
{
	__shared__ uint32_t stage[LISTS ? TILE : 1]; // the tile's entries: the passing ones, then the others
	__shared__ uint32_t tex[THREADS];            // the passing positions of the threads before
	__shared__ uint16_t tbits[THREADS];
	__shared__ uint64_t wsum[WAVES];
	__shared__ uint64_t range[2];
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const cover c = cover_of(S, cap, nseg, n);
	const uint64_t first = (uint64_t)blockIdx.x * TILE, j0 = first + tid * PER_THREAD;
	const uint32_t *counts = scratch + FILTER_HEAD_WORDS;
	const uint16_t *bits = reinterpret_cast<const uint16_t *>(counts + ntiles) +
			       (size_t)blockIdx.x * THREADS;
	// the tile's positions that take part, [a, b), and how many take part before it
	const uint64_t a = clamp(first, c.c0, c.c1), b = clamp(first + TILE, c.c0, c.c1);
	const uint64_t K = scratch[0], D = c.c1 - c.c0 - K;
	const uint64_t kbase = counts[blockIdx.x], dbase = a - c.c0 - kbase;
	const uint32_t pass = bits[tid];
	uint64_t total;
	const uint32_t ex = (uint32_t)block_scan(__builtin_popcount(pass), wsum, total);
	const uint32_t P = (uint32_t)total, Dt = (uint32_t)(b - a) - P;
	if (LISTS) {
		uint32_t idx[PER_THREAD];
		words_of(index, j0, n, idx);
		const uint32_t drop = part_bits(j0, c) & ~pass;
		// (of the positions that take part before the thread's, ex pass)
		uint32_t r = ex, d = P + (uint32_t)(clamp(j0, a, b) - a) - ex;
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			if (pass >> k & 1)
				stage[r++] = idx[k];
			else if (drop >> k & 1)
				stage[d++] = idx[k];
		}
	}
	if (TABLES) {
		tex[tid] = ex;
		tbits[tid] = (uint16_t)pass;
	}
	__syncthreads();
	if (LISTS) {
		if (out.kept != nullptr)
			for (uint32_t q = tid; q < P; q += THREADS)
				out.kept[kbase + q] = stage[q];
		if (out.dropped != nullptr)
			for (uint32_t q = tid; q < Dt; q += THREADS)
				out.dropped[dbase + q] = stage[P + q];
		// the tails: what of this tile's positions lies at or past K, or D
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint64_t j = first + k * THREADS + tid;
			if (j >= n)
				continue;
			if (out.kept != nullptr && j >= K)
				out.kept[j] = EBPF_NO_PACKET;
			if (out.dropped != nullptr && j >= D)
				out.dropped[j] = EBPF_NO_PACKET;
		}
	}
	if (!TABLES)
		return;
	// Table entry g counts up to p = min(S[g], n).  Those with p in [a, b) are this tile's:
	// entries [lo, hi) of a non-decreasing table, lo the number of entries below a, hi the
	// number below b.  (a < b is the same for every thread.)
	if (a < b) {
		if (w < 2) {
			const uint64_t p = w == 0 ? a : b; // (b >= 1)
			const uint64_t u = p != 0 ? upper(S, c.R + 1, p - 1) : 0;
			if (lane == 0)
				range[w] = u;
		}
		__syncthreads();
		const uint64_t lo = range[0], hi = range[1];
		for (uint64_t g = lo + tid; g < hi; g += THREADS) {
			const uint64_t s = S[g];
			const uint64_t p = clamp(s < n ? s : n, c.c0, c.c1);
			if (p < a || p >= b)
				continue;
			const uint32_t q = (uint32_t)(p - first);
			const uint64_t k = kbase + tex[q >> 4] +
					   __builtin_popcount(tbits[q >> 4] & ((1u << (q & 15)) - 1));
			if (out.kept_starts != nullptr)
				out.kept_starts[g] = k;
			if (out.dropped_starts != nullptr)
				out.dropped_starts[g] = p - c.c0 - k;
		}
		__syncthreads(); // (range is read)
	}
	// Those whose p is the range's end, entry R and the empty segments before it (every entry
	// where nothing takes part): one workgroup's, at the cost of their number.
	if (blockIdx.x != 0)
		return;
	if (w == 0) {
		const uint64_t u = c.c1 != c.c0 ? upper(S, c.R + 1, c.c1 - 1) : 0;
		if (lane == 0)
			range[0] = u;
	}
	__syncthreads();
	for (uint64_t g = range[0] + tid; g <= c.R; g += THREADS) {
		if (out.kept_starts != nullptr)
			out.kept_starts[g] = K;
		if (out.dropped_starts != nullptr)
			out.dropped_starts[g] = D;
	}
}

} // namespace

size_t
filter_scratch_bytes(uint64_t n)
{
	return ((size_t)tiles_of(n) * FILTER_TILE_WORDS + FILTER_HEAD_WORDS) * sizeof(uint32_t);
}

hipError_t
launch_filter(const struct ebpf_batch_test &test, uint64_t count, const uint32_t *index, uint64_t n,
	      const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
	      const struct ebpf_batch_parts &out, uint64_t *info, uint32_t *scratch, hipStream_t stream)
{
	const uint32_t ntiles = tiles_of(n);
	const bool flags = test.flags != nullptr, rank = test.rank != nullptr, val = test.ret != nullptr;
	const uint64_t mask = field_of(test.val_shift, test.val_bits).mask;
	with_flags([&](auto F, auto R, auto V) {
		hipLaunchKernelGGL((filter_tiles<F, R, V>), dim3(ntiles), dim3(THREADS), 0, stream, test, mask,
				   count, index, n, seg_starts, seg_cap, nseg, scratch, ntiles);
	}, flags, rank, val);
	hipLaunchKernelGGL(filter_carry, dim3(1), dim3(CARRY_THREADS), 0, stream, scratch, ntiles, n,
			   seg_starts, seg_cap, nseg, info);
	const bool lists = out.kept != nullptr || out.dropped != nullptr;
	const bool tables = out.kept_starts != nullptr || out.dropped_starts != nullptr;
	with_flags([&](auto L, auto T) {
		if constexpr (L || T) // (no kernel for neither: nothing is placed)
			hipLaunchKernelGGL((filter_place<L, T>), dim3(ntiles), dim3(THREADS), 0, stream, scratch,
					   ntiles, index, n, seg_starts, seg_cap, nseg, out);
	}, lists, tables);
	return hipGetLastError();
}
