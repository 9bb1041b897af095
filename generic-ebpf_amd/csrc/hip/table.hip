// table.hip — a sorted table of keys and values on the device: a batch's keys looked up in it
// (ebpf_batch_lookup_dev) and a batch's per-key sums merged into it (ebpf_batch_accumulate_dev).
// DESIGN.md §2 "Carrying totals across batches".
//
// Both are merges of sorted sequences done by searching: an entry of one sequence finds its place
// in the other by a lower bound.  A workgroup has a tile of STEER_TILE entries, a thread 16 of
// them, THREADS apart, so that a wave loads and stores neighbouring entries and a wave's ballot
// over one of the 16 is 64 consecutive entries' bits.  The tile's smallest and largest key are
// searched first, by two waves with the 64-way search of seg_tile.h; a thread's 16 searches then
// run inside that range, level by level, all 16 loads of a level in flight together.  The number
// of levels depends on the range's length alone, so it is the same for every thread of the tile,
// and a search ends, inside its range, whatever the sequences hold.
//   table_lookup  one workgroup per tile of the batch's keys: position, value, budget.
//   table_tiles   one workgroup per tile of the table and per tile of the batch.  A table entry's
//                 value is joined with its partner's, if the batch has its key; a batch entry
//                 whose key the table has is represented by that table entry and not by itself.
//                 Whether an entry is a kept candidate is a bit; the tile's 4,096 bits, per 64-bit
//                 word the bits set before it, and the tile's count go to scratch.
//   table_carry   one workgroup: exclusive scans over the tiles' counts of either side, two levels
//                 (a thread walks a run of tiles).  It writes info and *out->n.
//   table_place   the same searches and values again (cheaper than keeping 12 bytes an entry in
//                 scratch).  A kept entry goes to the kept entries of its own side before it (the
//                 tile's base, the word's, a popcount of the ballot) plus the kept entries of the
//                 other side below its key: those before its lower bound there (that tile's base,
//                 that word's count, a popcount of that word).
// Every output entry is written by one thread, no atomic decides anything and no workgroup waits
// for another: the output is a function of the input alone.  For sequences that are not strictly
// ascending a lower bound is still a position in [0, the other's length], so every count read
// from scratch is one of a tile that exists, and a store is clamped to out->cap.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/table.h"

namespace {

constexpr uint32_t WORDS = TILE / 64; // a tile's 64-bit words of bits
static_assert(TILE == 1u << 12 && WORDS == PER_THREAD * WAVES, "a ballot a wave and round is a word");
static_assert(TABLE_TILE_WORDS == 2 * WORDS + WORDS / 2 + 2, "bits, u16 counts, two words a tile");

typedef struct ebpf_key_table table;

// a sorted sequence of keys: a table's valid entries, or the batch's keys
struct seq {
	const uint64_t *keys;
	uint64_t n;
};

struct search_lds {
	uint64_t wmin[WAVES], wmax[WAVES];
	uint32_t range[2];
};

// what an accumulate call merges into the table
struct merge_args {
	table in;
	const uint64_t *keys, *adds;
	uint64_t key_cap;
	const uint64_t *nkeys;
	uint32_t op;
	uint64_t keep_lo, keep_hi;
};

// the valid entries of a table (one without n has cap 0, table.cpp table_null: no entry)
__device__ __forceinline__ seq
seq_of(const table &t)
{
	if (t.n == nullptr)
		return {t.keys, 0};
	const uint64_t n = *t.n;
	return {t.keys, n < t.cap ? n : t.cap};
}

// Where the tile's keys can stand in s: [lo, hi], the lower bounds of the smallest and of the
// largest of them, lo <= hi <= s.n whatever s holds.  The tile has a key (the same for every
// thread).
__device__ __forceinline__ void
range_of(const seq &s, const uint64_t (&key)[PER_THREAD], uint32_t valid, search_lds &l,
	 uint32_t &lo, uint32_t &hi)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint64_t mn = ~0ull, mx = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (!(valid >> k & 1))
			continue;
		mn = key[k] < mn ? key[k] : mn;
		mx = key[k] > mx ? key[k] : mx;
	}
#pragma unroll
	for (uint32_t d = 32; d != 0; d >>= 1) {
		const uint64_t a = __shfl_xor(mn, d), b = __shfl_xor(mx, d);
		mn = a < mn ? a : mn;
		mx = b > mx ? b : mx;
	}
	if (lane == 0) {
		l.wmin[w] = mn;
		l.wmax[w] = mx;
	}
	__syncthreads();
	if (w < 2) { // (the 64-way search is a whole wave's)
#pragma unroll
		for (uint32_t q = 0; q < WAVES; q++) {
			mn = l.wmin[q] < mn ? l.wmin[q] : mn;
			mx = l.wmax[q] > mx ? l.wmax[q] : mx;
		}
		// the keys below p are those <= p - 1
		const uint64_t p = w == 0 ? mn : mx;
		const uint64_t below = p != 0 ? upper(s.keys, s.n, p - 1) : 0;
		if (lane == 0)
			l.range[w] = (uint32_t)below;
	}
	__syncthreads();
	lo = l.range[0];
	hi = l.range[1] > lo ? l.range[1] : lo;
}

// at[k] = lo + the number of S[lo .. hi) below key[k], for S ascending there.  The steps depend on
// hi - lo alone; every read is one of S[lo .. hi), and lo <= at[k] <= hi, for any S.
__device__ __forceinline__ void
lower_bounds(const uint64_t *__restrict__ S, uint32_t lo, uint32_t hi,
	     const uint64_t (&key)[PER_THREAD], uint32_t (&at)[PER_THREAD])
{
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		at[k] = lo;
	uint32_t len = hi - lo;
	while (len > 1) {
		const uint32_t half = len >> 1;
		uint64_t probe[PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			probe[k] = S[at[k] + (half - 1)];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			at[k] += probe[k] < key[k] ? half : 0;
		len -= half;
	}
	if (len == 1) {
		uint64_t probe[PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			probe[k] = S[at[k]];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			at[k] += probe[k] < key[k] ? 1 : 0;
	}
}

// Bit k is set iff the thread's entry k has a partner in s: s.keys[at[k]] is its key.
__device__ __forceinline__ uint32_t
partners_of(const seq &s, const uint64_t (&key)[PER_THREAD], const uint32_t (&at)[PER_THREAD],
	    uint32_t valid)
{
	uint64_t found[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		found[k] = at[k] < s.n ? s.keys[at[k]] : 0;
	uint32_t match = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		match |= (at[k] < s.n && found[k] == key[k] ? 1u : 0u) << k;
	return match & valid;
}

__device__ __forceinline__ uint64_t
combine(uint32_t op, uint64_t a, uint64_t b)
{
	switch (op) {
	case EBPF_ACC_ADD:
		return a + b;
	case EBPF_ACC_MIN:
		return a < b ? a : b;
	case EBPF_ACC_MAX:
		return a > b ? a : b;
	default:
		return a | b;
	}
}

template <bool VALS, bool POS, bool REMAINING>
__global__ void __launch_bounds__(THREADS)
table_lookup(table t, const uint64_t *__restrict__ keys, uint64_t key_cap,
	     const uint64_t *__restrict__ nkeys, uint64_t missing, uint64_t limit,
	     uint64_t *__restrict__ vals_out, uint32_t *__restrict__ pos_out)
{
	__shared__ search_lds l;
	const seq tab = seq_of(t), batch = {keys, segments_of(key_cap, nkeys)};
	const uint64_t first = (uint64_t)blockIdx.x * TILE;
	if (first >= batch.n)
		return;
	uint64_t key[PER_THREAD], v[PER_THREAD];
	uint32_t at[PER_THREAD], lo, hi;
	const uint32_t valid = strided_of(batch.keys, batch.n, first, key);
	range_of(tab, key, valid, l, lo, hi);
	lower_bounds(tab.keys, lo, hi, key, at);
	const uint32_t there = partners_of(tab, key, at, valid);
	if (VALS) {
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			v[k] = there >> k & 1 ? t.vals[at[k]] : missing;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (!(valid >> k & 1))
			continue;
		const uint64_t g = first + k * THREADS + threadIdx.x;
		if (POS)
			pos_out[g] = there >> k & 1 ? at[k] : EBPF_NO_ENTRY;
		if (VALS)
			vals_out[g] = REMAINING ? (v[k] < limit ? limit - v[k] : 0) : v[k];
	}
}

// One tile of the table (BATCH false) or of the batch's keys (BATCH true), which has an entry:
// per entry its key, its lower bound in the other sequence and its value as a candidate; bit k of
// keep is set iff entry k is a kept candidate, of only (the batch's side) iff the table has not
// its key.
template <bool BATCH>
__device__ __forceinline__ void
candidates(const merge_args &a, const seq &tab, const seq &batch, uint64_t first, search_lds &l,
	   uint64_t (&key)[PER_THREAD], uint64_t (&val)[PER_THREAD], uint32_t (&at)[PER_THREAD],
	   uint32_t &keep, uint32_t &only)
{
	const seq &self = BATCH ? batch : tab, &other = BATCH ? tab : batch;
	uint32_t lo, hi;
	const uint32_t valid = strided_of(self.keys, self.n, first, key);
	range_of(other, key, valid, l, lo, hi);
	lower_bounds(other.keys, lo, hi, key, at);
	const uint32_t match = partners_of(other, key, at, valid);
	const uint64_t *own = BATCH ? a.adds : a.in.vals;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		val[k] = valid >> k & 1 ? own[first + k * THREADS + threadIdx.x] : 0;
	if (!BATCH) {
		uint64_t add[PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			add[k] = match >> k & 1 ? a.adds[at[k]] : 0;
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			val[k] = match >> k & 1 ? combine(a.op, val[k], add[k]) : val[k];
	}
	only = BATCH ? valid & ~match : 0;
	keep = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		keep |= (a.keep_lo <= val[k] && val[k] <= a.keep_hi ? 1u : 0u) << k;
	keep &= BATCH ? only : valid;
}

// where a call's scratch keeps what (table.h); t: a tile of the call, the table's first
struct scratch_map {
	uint32_t *head;
	uint64_t *bits;   // WORDS a tile
	uint16_t *before; // WORDS a tile
	uint32_t *counts; // 2 a tile
};

__device__ __forceinline__ scratch_map
map_of(uint32_t *scratch, uint32_t ntiles)
{
	uint32_t *bits = scratch + TABLE_HEAD_WORDS, *before = bits + (size_t)ntiles * 2 * WORDS;
	return {scratch, reinterpret_cast<uint64_t *>(bits), reinterpret_cast<uint16_t *>(before),
		before + (size_t)ntiles * (WORDS / 2)};
}

__global__ void __launch_bounds__(THREADS)
table_tiles(merge_args a, uint32_t tab_tiles, uint32_t ntiles, uint32_t *__restrict__ scratch)
{
	__shared__ search_lds l;
	__shared__ uint32_t wpop[WORDS], wonly[WAVES];
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x;
	const seq tab = seq_of(a.in), batch = {a.keys, segments_of(a.key_cap, a.nkeys)};
	const bool side = t >= tab_tiles; // (the same for every thread, as is whether the tile has an entry)
	const uint64_t first = (uint64_t)(side ? t - tab_tiles : t) * TILE;
	const scratch_map m = map_of(scratch, ntiles);
	uint32_t keep = 0, only = 0;
	if (first < (side ? batch.n : tab.n)) {
		uint64_t key[PER_THREAD], val[PER_THREAD];
		uint32_t at[PER_THREAD];
		if (side)
			candidates<true>(a, tab, batch, first, l, key, val, at, keep, only);
		else
			candidates<false>(a, tab, batch, first, l, key, val, at, keep, only);
	}
	uint32_t lone = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t word = __ballot(keep >> k & 1);
		lone += __popcll(__ballot(only >> k & 1));
		if (lane == 0) {
			m.bits[word_of((size_t)t * WORDS, k, w)] = word;
			wpop[word_of(0u, k, w)] = __popcll(word);
		}
	}
	if (lane == 0)
		wonly[w] = lone;
	__syncthreads();
	if (w != 0)
		return;
	const uint32_t own = wpop[lane], inc = lanes_through(own, lane);
	m.before[(size_t)t * WORDS + lane] = (uint16_t)(inc - own);
	if (lane == 63) {
		uint32_t all = 0;
#pragma unroll
		for (uint32_t q = 0; q < WAVES; q++)
			all += wonly[q];
		m.counts[2 * (size_t)t] = inc;
		m.counts[2 * (size_t)t + 1] = all;
	}
}

// One workgroup: per side tile_counts_scan leaves in every tile's word the kept entries of its
// side's tiles before.  A side's sum is at most its cap < 2^32: 32-bit sums.
__global__ void __launch_bounds__(CARRY_THREADS)
table_carry(table in, table out, uint32_t tab_tiles, uint32_t ntiles,
	    uint32_t *__restrict__ scratch, uint64_t *__restrict__ info)
{
	__shared__ uint32_t wsum[CARRY_THREADS / 64];
	const scratch_map m = map_of(scratch, ntiles);
	uint32_t K[2];
	for (uint32_t side = 0; side < 2; side++) {
		uint32_t *counts = m.counts + (side ? 2 * (size_t)tab_tiles : 0);
		K[side] = tile_counts_scan(counts, counts, 2, side ? ntiles - tab_tiles : tab_tiles, wsum);
	}
	// the batch's keys that the table has not
	const uint32_t fresh = tile_counts_scan<uint32_t>(m.counts + 2 * (size_t)tab_tiles + 1, nullptr, 2,
							  ntiles - tab_tiles, wsum);
	if (threadIdx.x == 0) {
		const uint64_t M = (uint64_t)K[0] + K[1];
		m.head[0] = K[0];
		m.head[1] = K[1];
		info[0] = M;
		info[1] = K[1];
		info[2] = seq_of(in).n + fresh - M;
		if (out.n != nullptr)
			*out.n = M;
	}
}

__global__ void __launch_bounds__(THREADS)
table_place(merge_args a, table out, uint32_t tab_tiles, uint32_t ntiles,
	    uint32_t *__restrict__ scratch)
{
	__shared__ search_lds l;
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x;
	const seq tab = seq_of(a.in), batch = {a.keys, segments_of(a.key_cap, a.nkeys)};
	const bool side = t >= tab_tiles;
	const uint64_t first = (uint64_t)(side ? t - tab_tiles : t) * TILE;
	if (first >= (side ? batch.n : tab.n)) // (the same for every thread)
		return;
	const scratch_map m = map_of(scratch, ntiles);
	uint64_t key[PER_THREAD], val[PER_THREAD];
	uint32_t at[PER_THREAD], keep, only;
	if (side)
		candidates<true>(a, tab, batch, first, l, key, val, at, keep, only);
	else
		candidates<false>(a, tab, batch, first, l, key, val, at, keep, only);
	// the other side: its entries, its kept ones, its first tile
	const uint64_t n_other = side ? tab.n : batch.n;
	const uint64_t k_other = m.head[side ? 0 : 1];
	const size_t t_other = side ? 0 : tab_tiles;
	const uint64_t base = m.counts[2 * (size_t)t];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t word = __ballot(keep >> k & 1);
		if (!(keep >> k & 1))
			continue;
		uint64_t dest = base + m.before[word_of((size_t)t * WORDS, k, w)] +
				__popcll(word & ((1ull << lane) - 1));
		// at[k] <= n_other: a position of the other side, or its end
		const uint32_t j = at[k];
		if (j >= n_other) {
			dest += k_other;
		} else {
			const size_t wd = t_other * WORDS + (j >> 6);
			dest += (uint64_t)m.counts[2 * (t_other + (j >> 12))] + m.before[wd] +
				__popcll(m.bits[wd] & ((1ull << (j & 63)) - 1));
		}
		if (dest < out.cap) {
			out.keys[dest] = key[k];
			out.vals[dest] = val[k];
		}
	}
}

} // namespace

size_t
accumulate_scratch_bytes(uint64_t cap, uint64_t key_cap)
{
	return ((size_t)(tiles_of(cap) + tiles_of(key_cap)) * TABLE_TILE_WORDS + TABLE_HEAD_WORDS) *
	       sizeof(uint32_t);
}

hipError_t
launch_lookup(const struct ebpf_key_table &t, const uint64_t *keys, uint64_t key_cap,
	      const uint64_t *nkeys, uint32_t mode, uint64_t missing, uint64_t limit,
	      uint64_t *vals_out, uint32_t *pos_out, hipStream_t stream)
{
	with_flags([&](auto V, auto P, auto R) {
		if constexpr (V || P) // (no kernel for neither; the budget is a form of the value)
			hipLaunchKernelGGL((table_lookup<V, P, V && R>), dim3(tiles_of(key_cap)), dim3(THREADS),
					   0, stream, t, keys, key_cap, nkeys, missing, limit, vals_out,
					   pos_out);
	}, vals_out != nullptr, pos_out != nullptr, mode == EBPF_LOOKUP_REMAINING);
	return hipGetLastError();
}

hipError_t
launch_accumulate(const struct ebpf_key_table &in, const uint64_t *keys, const uint64_t *adds,
		  uint64_t key_cap, const uint64_t *nkeys, uint32_t op, uint64_t keep_lo,
		  uint64_t keep_hi, const struct ebpf_key_table &out, uint64_t *info, uint32_t *scratch,
		  hipStream_t stream)
{
	const uint32_t tab_tiles = tiles_of(in.cap), ntiles = tab_tiles + tiles_of(key_cap);
	const merge_args a = {in, keys, adds, key_cap, nkeys, op, keep_lo, keep_hi};
	hipLaunchKernelGGL(table_tiles, dim3(ntiles), dim3(THREADS), 0, stream, a, tab_tiles,
			   ntiles, scratch);
	hipLaunchKernelGGL(table_carry, dim3(1), dim3(CARRY_THREADS), 0, stream, in, out, tab_tiles,
			   ntiles, scratch, info);
	if (out.cap != 0) // (nothing is placed in a table of no entry)
		hipLaunchKernelGGL(table_place, dim3(ntiles), dim3(THREADS), 0, stream, a, out, tab_tiles,
				   ntiles, scratch);
	return hipGetLastError();
}
