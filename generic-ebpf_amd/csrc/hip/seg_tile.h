// seg_tile.h — what the segmented list kernels (reduce.hip, scan.hip, filter.hip) and the
// keyed-sequence kernels (table.hip, top.hip, rollup.hip) share: the tile shape and the tiles of a
// sequence, a list's segments (their number, bounds and end, the 64-way search) and a sequence's
// entries, a tile's LDS slots, a thread's lengths and values and its strided entries, a tile's
// ballot words and a wave's scan of their counts, the segmented scan over a workgroup's threads, a
// carry thread's run of tiles and the carry scan of the tiles' counts, the sum/min/max/OR record,
// and run-time flags as template arguments.  Device code but for tiles_of and with_flags; every
// file that includes it is compiled on its own: everything here is file-local.
#pragma once
#include <type_traits>

#include "bit_field.h"
#include "hip/batch_places.h"
#include "host/steer.h"

namespace {

constexpr uint32_t TILE = STEER_TILE;
constexpr uint32_t PER_THREAD = TILE / THREADS;
constexpr uint32_t CARRY_THREADS = 1024; // a carry kernel's one workgroup
constexpr uint32_t NOHEAD = ~0u;         // no segment begins here (a segment's number is below it)
static_assert(PER_THREAD == 16, "a thread's positions are one padded LDS row, and 16 bits");

// The tiles of n entries, at least one: a launcher's grid, and its scratch.
inline uint32_t
tiles_of(uint64_t n)
{
	const uint64_t t = (n + TILE - 1) / TILE;
	return t != 0 ? (uint32_t)t : 1;
}

// The number of segments of a list (ebpf_gpu.h): a short table holds no end for its last group.
// (host/list_args.h seg_count is the host's statement of the rule.)
__device__ __forceinline__ uint64_t
segments_of(uint64_t cap, const uint64_t *__restrict__ nseg)
{
	if (nseg == nullptr)
		return cap;
	const uint64_t g = *nseg;
	return g <= cap ? g : (cap != 0 ? cap - 1 : 0);
}

// The entries of a keyed sequence that take part (ebpf_gpu.h): the reduce's rule above, or the
// table's, a short sequence being its first cap entries.  (host/list_args.h entry_count.)
__device__ __forceinline__ uint64_t
entries_of(uint64_t cap, const uint64_t *__restrict__ n, uint32_t segments)
{
	if (segments)
		return segments_of(cap, n);
	if (n == nullptr)
		return cap;
	const uint64_t v = *n;
	return v < cap ? v : cap;
}

// Segment g's positions [a, b), clamped to the list.
__device__ __forceinline__ void
seg_bounds(const uint64_t *__restrict__ S, uint64_t g, uint64_t n, uint64_t &a, uint64_t &b)
{
	a = S[g];
	b = S[g + 1];
	a = a < n ? a : n;
	b = b < n ? b : n;
}

// Where the last of R segments ends, clamped to the list: no position at or past it is covered.
__device__ __forceinline__ uint64_t
seg_end(const uint64_t *__restrict__ S, uint64_t R, uint64_t n)
{
	const uint64_t end = R != 0 ? S[R] : 0;
	return end < n ? end : n;
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
fields_of(const places &f, const uint64_t *__restrict__ ret, bit_field vf, const uint32_t (&idx)[N],
	  const bool (&has)[N], uint32_t (&len)[N], uint64_t (&val)[N])
{
	uint64_t s[N], e[N];
	if (VALS) {
#pragma unroll
		for (uint32_t k = 0; k < N; k++)
			val[k] = ret[idx[k] < f.count ? idx[k] : f.count - 1];
#pragma unroll
		for (uint32_t k = 0; k < N; k++)
			val[k] = vf.of(val[k]);
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

// A thread's entries first + k * THREADS + tid of a[0 .. N), so that a wave loads neighbouring
// entries: bit k of the result is set iff the entry exists, and x[k] is 0 where it does not.
__device__ __forceinline__ uint32_t
strided_of(const uint64_t *__restrict__ a, uint64_t N, uint64_t first, uint64_t (&x)[PER_THREAD])
{
	uint32_t valid = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t e = first + k * THREADS + threadIdx.x;
		const bool has = e < N;
		x[k] = has ? a[e] : 0;
		valid |= (has ? 1u : 0u) << k;
	}
	return valid;
}

// A wave's ballot over bit k of such a thread's 16 is 64 consecutive entries' bits: where, of a
// tile's 64 words of bits that begin at index `base`, wave w's of round k is.
template <typename B>
__device__ __forceinline__ B
word_of(B base, uint32_t k, uint32_t w)
{
	return base + k * WAVES + w;
}

// One wave: the sum of own over the lanes up to and including this one.  A lane a word of a tile,
// own its set bits: less own, the set bits of the words before it.
__device__ __forceinline__ uint32_t
lanes_through(uint32_t own, uint32_t lane)
{
	uint32_t inc = own;
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t up = __shfl_up(inc, d);
		if (lane >= d)
			inc += up;
	}
	return inc;
}

// A segmented scan over the NW waves of a workgroup: the join of the runs of the threads before
// this one, in thread order.  P is a run of list entries reduced; JOIN(a, b) is run a, then run b
// (a segment that begins in b closes a), with `none` its identity; UP(p, d) is the p of the lane
// d below.  wtot: a P per wave, in LDS.
template <uint32_t NW, auto JOIN, auto UP, typename P>
__device__ __forceinline__ P
carry_in(const P &mine, const P &none, P *wtot)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	P inc = mine; // inclusive scan over the wave
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const P up = UP(inc, d);
		if (lane >= d)
			inc = JOIN(up, inc);
	}
	if (lane == 63)
		wtot[w] = inc;
	__syncthreads();
	P before = none;
	for (uint32_t q = 0; q < NW; q++) {
		const P s = wtot[q];
		if (q < w)
			before = JOIN(before, s);
	}
	const P prev = UP(inc, 1);
	return lane == 0 ? before : JOIN(before, prev);
}

// A carry kernel is one workgroup of CARRY_THREADS, two levels: thread s walks the tiles
// [t0, t1) = [s * seglen, (s + 1) * seglen) for what its run hands on, the threads scan that, and
// it walks them again with what the threads before it hand in.
struct tile_run {
	uint32_t t0, t1;
};

__device__ __forceinline__ tile_run
run_of(uint32_t ntiles)
{
	const uint32_t seglen = (ntiles + CARRY_THREADS - 1) / CARRY_THREADS;
	const uint32_t t0 = min(threadIdx.x * seglen, ntiles);
	return {t0, min(t0 + seglen, ntiles)};
}

// The carry kernel's exclusive scan of a count a tile, in[stride * t]: a thread sums its run of
// tiles, the threads scan that (wsum: CARRY_THREADS / 64 words of LDS), and it walks its run again
// to leave in out[stride * t] the counts of the tiles before t.  Returns the sum over all tiles.
// out may be in; out NULL: the sum alone.  Every thread of the workgroup calls it.
template <typename T>
__device__ __forceinline__ T
tile_counts_scan(const T *in, T *out, size_t stride, uint32_t ntiles, T *wsum)
{
	const auto [t0, t1] = run_of(ntiles);
	T mine = 0, all;
	for (uint32_t t = t0; t < t1; t++)
		mine += in[stride * t];
	T cur = block_scan<CARRY_THREADS / 64>(mine, wsum, all);
	if (out != nullptr) {
		for (uint32_t t = t0; t < t1; t++) {
			const T own = in[stride * t];
			out[stride * t] = cur;
			cur += own;
		}
	}
	return all;
}

// The sum, minimum, maximum and OR of some values: what reduce.hip keeps per run, four consecutive
// words of a scratch row.  (rollup.hip writes the four out: see its part.)
struct stats {
	uint64_t sum, mn, mx, bits;
};

constexpr stats NO_STATS = {0, ~0ull, 0, 0}; // of no value

__device__ __forceinline__ void
add(stats &a, const stats &b)
{
	a.sum += b.sum;
	a.mn = b.mn < a.mn ? b.mn : a.mn;
	a.mx = b.mx > a.mx ? b.mx : a.mx;
	a.bits |= b.bits;
}

__device__ __forceinline__ void
add_value(stats &a, uint64_t v)
{
	a.sum += v;
	a.mn = v < a.mn ? v : a.mn;
	a.mx = v > a.mx ? v : a.mx;
	a.bits |= v;
}

// the stats of the lane d below
__device__ __forceinline__ stats
up(const stats &s, uint32_t d)
{
	return {__shfl_up((unsigned long long)s.sum, d), __shfl_up((unsigned long long)s.mn, d),
		__shfl_up((unsigned long long)s.mx, d), __shfl_up((unsigned long long)s.bits, d)};
}

__device__ __forceinline__ void
store(uint64_t *__restrict__ w, const stats &s)
{
	w[0] = s.sum;
	w[1] = s.mn;
	w[2] = s.mx;
	w[3] = s.bits;
}

__device__ __forceinline__ stats
load(const uint64_t *__restrict__ w)
{
	return {w[0], w[1], w[2], w[3]};
}

// One statistic on its own (a file's further outputs are numbered from STATS on; one that is
// none of MIN, MAX and BITS folds as a sum).
enum { SUM, MIN, MAX, BITS, STATS };

template <int STAT>
__device__ __forceinline__ uint64_t
ident()
{
	return STAT == MIN ? ~0ull : 0;
}

template <int STAT>
__device__ __forceinline__ uint64_t
fold(uint64_t a, uint64_t b)
{
	return STAT == MIN ? (b < a ? b : a) : STAT == MAX ? (b > a ? b : a) : STAT == BITS ? a | b : a + b;
}

// Run-time booleans as template flags: f(std::bool_constant<b>{}, std::bool_constant<rest>{}...),
// so that a launcher names its argument list once.
template <typename F, typename... B>
inline void
with_flags(F f, bool b, B... rest)
{
	auto on = [&](auto c) {
		if constexpr (sizeof...(rest) == 0)
			f(c);
		else
			with_flags([&](auto... d) { f(c, d...); }, rest...);
	};
	b ? on(std::true_type{}) : on(std::false_type{});
}

} // namespace
