// seg_tile.h — what the segmented list kernels share (reduce.hip, scan.hip, filter.hip): the tile
// shape, a list's segments (their number, bounds and end, the 64-way search), a tile's LDS slots,
// a thread's lengths and values, the segmented scan over a workgroup's threads, a carry thread's
// run of tiles, and run-time flags as template arguments.  Device code but for with_flags; every
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
