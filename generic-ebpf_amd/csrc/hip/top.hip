// top.hip — the k best entries of a keyed sequence by a bit field of the value
// (ebpf_batch_top_dev): a most-significant-digit radix select, then a sort of what was selected.
// DESIGN.md §2 "The heaviest entries".
//
// The order's own terms: g(p) = f(p), or its complement inside the field for EBPF_TOP_SMALLEST, so
// that the best entry has the largest g and both orders are one code path.  A workgroup has a tile
// of STEER_TILE entries, a thread 16 of them, THREADS apart, so that a wave's ballot over one of
// the 16 is 64 consecutive entries' bits.
//   top_count  a pass per 8 bits of the field, from the top: a workgroup per run of tiles counts
//              the current digit of the entries whose higher digits are the prefix found so far,
//              in LDS, and writes a row of 256 counts.  A run past N writes a row of zeros.
//   top_pick   after each: one workgroup sums the rows, walks the bins from the top until the
//              running count reaches what is still wanted, extends the prefix by that bin and
//              lowers "wanted" by the entries above it.  The first fixes m = min(k, N).  After the
//              last the prefix is the cut T and "wanted" is e, the entries equal to T to take.
//   top_tiles  per tile the entries above T and those equal to T.
//   top_carry  one workgroup: exclusive scans of both over the tiles, two levels.
//   top_place  an entry above T goes to candidate slot (those above before it); an entry equal to
//              T whose rank r among the equal ones, by position, is below e goes to slot
//              (m - e) + r.  A tile that takes nothing returns before it loads.
//   top_order  one workgroup sorts the m candidates by (g descending, position ascending), a
//              bitonic network in LDS over the pair compared in one piece, gathers keys and vals
//              and writes the outputs and info.
// Every slot is written by one thread, no atomic touches global memory and no workgroup waits for
// another: the output is a function of the input alone.  Every load of keys and vals is of a
// position below N, and every store to an output of a rank below m.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/top.h"

namespace {

constexpr uint32_t BINS = 256;
constexpr uint32_t WORDS = TILE / 64; // a tile's ballots: one a wave and round
constexpr uint32_t NO_POS = ~0u;      // the position of a padding candidate: past every entry
static_assert(EBPF_TOP_MAX == TILE && WORDS == PER_THREAD * WAVES && WORDS == 64, "k is at most a tile");
constexpr uint32_t PICK_ROWS = CARRY_THREADS / 64; // the rows that top_pick reads at a time
static_assert(BINS == 4 * 64 && (TOP_HEAD_WORDS + 3 * EBPF_TOP_MAX) % 4 == 0, "a wave reads a row, 16 bytes a lane");

typedef struct ebpf_batch_tops tops;

// the sequence and the order of one call
struct top_args {
	const uint64_t *keys, *vals;
	uint64_t cap;
	const uint64_t *n;
	bit_field f;
	uint32_t segments, smallest;
};

// where a call's scratch keeps what (top.h)
struct scratch_map {
	uint32_t *head;
	uint64_t *cand_g;
	uint32_t *cand_pos;
	uint32_t *rows;
	uint32_t *counts; // 4 a tile
};

__device__ __forceinline__ scratch_map
map_of(uint32_t *scratch, uint32_t nrows)
{
	uint32_t *g = scratch + TOP_HEAD_WORDS, *pos = g + 2 * EBPF_TOP_MAX, *rows = pos + EBPF_TOP_MAX;
	return {scratch, reinterpret_cast<uint64_t *>(g), pos, rows, rows + (size_t)nrows * BINS};
}

__device__ __forceinline__ uint64_t
prefix_of(const uint32_t *head)
{
	return *reinterpret_cast<const uint64_t *>(head);
}

// A thread's entries first + k * THREADS + tid of the N (strided_of) in the order's terms: g[k] is
// 0 where the entry does not exist.
__device__ __forceinline__ uint32_t
load_tile(const top_args &a, uint64_t N, uint64_t first, uint64_t (&g)[PER_THREAD])
{
	const uint32_t valid = strided_of(a.vals, N, first, g);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t v = a.f.of(g[k]);
		g[k] = valid >> k & 1 ? (a.smallest ? a.f.mask - v : v) : 0;
	}
	return valid;
}

// Bits k of above and equal: the thread's entry k exists and lies above T, or is T.
__device__ __forceinline__ void
against_cut(const uint64_t (&g)[PER_THREAD], uint32_t valid, uint64_t T, uint32_t &above,
	    uint32_t &equal)
{
	above = equal = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		above |= (g[k] > T ? 1u : 0u) << k;
		equal |= (g[k] == T ? 1u : 0u) << k;
	}
	above &= valid;
	equal &= valid;
}

// One pass's histogram: digit (g >> shift) & 255 of the entries whose bits above it are the
// prefix's (all of them in the first pass, which does not read the head).  A wave whose matching
// entries of a round share a digit, as the high digits of most sequences do, counts them with one
// addition; otherwise a lane an entry adds to LDS.
__global__ void __launch_bounds__(THREADS)
top_count(top_args a, uint32_t shift, uint32_t first_pass, uint32_t per_row, uint32_t ntiles,
	  uint32_t nrows, uint32_t *__restrict__ scratch)
{
	__shared__ uint32_t hist[BINS];
	const scratch_map m = map_of(scratch, nrows);
	const uint32_t lane = threadIdx.x & 63, row = blockIdx.x;
	const uint64_t N = entries_of(a.cap, a.n, a.segments);
	const uint64_t prefix = first_pass ? 0 : prefix_of(m.head);
	const uint32_t hi = shift + 8; // (the bits from here up are the prefix's; 64: there are none)
	hist[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t t0 = row * per_row, t1 = min(t0 + per_row, ntiles);
	for (uint32_t t = t0; t < t1; t++) {
		const uint64_t first = (uint64_t)t * TILE;
		if (first >= N) // (the same for every thread; so are the tiles after it)
			break;
		uint64_t g[PER_THREAD];
		const uint32_t valid = load_tile(a, N, first, g);
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const bool in = (valid >> k & 1) && (hi >= 64 || (g[k] >> hi) == (prefix >> hi));
			const uint32_t digit = (uint32_t)(g[k] >> shift) & (BINS - 1);
			const uint64_t any = __ballot(in);
			if (any == 0)
				continue;
			const uint32_t d0 = __shfl(digit, (int)__builtin_ctzll(any));
			if (__ballot(in && digit == d0) == any) {
				if (lane == 0)
					atomicAdd(&hist[d0], (uint32_t)__popcll(any));
			} else if (in) {
				atomicAdd(&hist[digit], 1u);
			}
		}
	}
	__syncthreads();
	m.rows[(size_t)row * BINS + threadIdx.x] = hist[threadIdx.x];
}

// One workgroup: 16 rows at a time, a lane four bins of a row (16 bytes), summed per bin; then
// one wave walks the bins from the top, four a lane.  The sums are at most cap < 2^32.
__global__ void __launch_bounds__(CARRY_THREADS)
top_pick(top_args a, uint64_t k, uint32_t shift, uint32_t first_pass, uint32_t nrows,
	 uint32_t *__restrict__ scratch)
{
	__shared__ uint32_t part[PICK_ROWS][BINS + 4]; // (4 words of padding a row: the rows' banks apart)
	__shared__ uint32_t total[BINS];
	const scratch_map m = map_of(scratch, nrows);
	const u32x4 *rows = reinterpret_cast<const u32x4 *>(m.rows);
	const uint32_t col = threadIdx.x & 63, q = threadIdx.x >> 6;
	u32x4 sum = {0, 0, 0, 0};
#pragma unroll 4
	for (uint32_t r = q; r < nrows; r += PICK_ROWS)
		sum += rows[(size_t)r * (BINS / 4) + col];
#pragma unroll
	for (uint32_t i = 0; i < 4; i++)
		part[q][4 * col + i] = sum[i];
	__syncthreads();
	if (threadIdx.x < BINS) {
		uint32_t all = 0;
#pragma unroll
		for (uint32_t r = 0; r < PICK_ROWS; r++)
			all += part[r][threadIdx.x];
		total[threadIdx.x] = all;
	}
	__syncthreads();
	if (threadIdx.x >= 64)
		return;
	const uint32_t lane = threadIdx.x;
	uint64_t prefix = 0;
	uint32_t want;
	if (first_pass) {
		const uint64_t N = entries_of(a.cap, a.n, a.segments);
		want = (uint32_t)(k < N ? k : N); // m: k <= EBPF_TOP_MAX
		if (lane == 0)
			m.head[3] = want;
	} else {
		prefix = prefix_of(m.head);
		want = m.head[2];
	}
	// lane l has bins 255 - 4l down to 252 - 4l
	uint32_t c[4], own = 0;
#pragma unroll
	for (uint32_t i = 0; i < 4; i++) {
		const uint32_t bin = BINS - 1 - (4 * lane + i);
		c[i] = total[bin];
		own += c[i];
	}
	const uint32_t inc = lanes_through(own, lane);
	// the lane whose bins hold the want-th entry from the top (none for want == 0)
	uint32_t before = inc - own, digit = 0;
	const bool here = want != 0 && before < want && want <= inc;
	if (here) {
#pragma unroll
		for (uint32_t i = 0; i < 4; i++) {
			if (before + c[i] >= want) {
				digit = BINS - 1 - (4 * lane + i);
				break;
			}
			before += c[i];
		}
	}
	const uint64_t found = __ballot(here);
	if (found == 0) {
		if (lane == 0) {
			*reinterpret_cast<uint64_t *>(m.head) = prefix;
			m.head[2] = 0;
		}
		return;
	}
	if (lane == (uint32_t)__builtin_ctzll(found)) {
		*reinterpret_cast<uint64_t *>(m.head) = prefix | (uint64_t)digit << shift;
		m.head[2] = want - before;
	}
}

// The set bits of above and of equal summed over the workgroup: na and ne, in every thread.
__device__ __forceinline__ void
tile_counts(uint32_t above, uint32_t equal, uint32_t (*wsum)[2], uint32_t &na, uint32_t &ne)
{
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	uint32_t ca = __popc(above), ce = __popc(equal);
#pragma unroll
	for (uint32_t d = 32; d != 0; d >>= 1) {
		ca += __shfl_xor(ca, d);
		ce += __shfl_xor(ce, d);
	}
	if (lane == 0) {
		wsum[w][0] = ca;
		wsum[w][1] = ce;
	}
	__syncthreads();
	na = ne = 0;
#pragma unroll
	for (uint32_t q = 0; q < WAVES; q++) {
		na += wsum[q][0];
		ne += wsum[q][1];
	}
}

__global__ void __launch_bounds__(THREADS)
top_tiles(top_args a, uint32_t nrows, uint32_t *__restrict__ scratch)
{
	__shared__ uint32_t wsum[WAVES][2];
	const scratch_map m = map_of(scratch, nrows);
	const uint32_t t = blockIdx.x;
	const uint64_t N = entries_of(a.cap, a.n, a.segments), first = (uint64_t)t * TILE;
	uint32_t above = 0, equal = 0, na, ne;
	if (first < N) { // (the same for every thread)
		uint64_t g[PER_THREAD];
		const uint32_t valid = load_tile(a, N, first, g);
		against_cut(g, valid, prefix_of(m.head), above, equal);
	}
	tile_counts(above, equal, wsum, na, ne);
	if (threadIdx.x == 0) {
		m.counts[TOP_TILE_WORDS * (size_t)t] = na;
		m.counts[TOP_TILE_WORDS * (size_t)t + 1] = ne;
	}
}

// One workgroup: per kind tile_counts_scan leaves beside every tile's count the entries of that
// kind in the tiles before.  A sum is at most cap < 2^32.
__global__ void __launch_bounds__(CARRY_THREADS)
top_carry(uint32_t ntiles, uint32_t nrows, uint32_t *__restrict__ scratch)
{
	__shared__ uint32_t wsum[CARRY_THREADS / 64];
	const scratch_map m = map_of(scratch, nrows);
	for (uint32_t kind = 0; kind < 2; kind++) {
		uint32_t *counts = m.counts + kind;
		const uint32_t all = tile_counts_scan(counts, counts + 2, TOP_TILE_WORDS, ntiles, wsum);
		if (threadIdx.x == 0)
			m.head[4 + kind] = all;
	}
}

__global__ void __launch_bounds__(THREADS)
top_place(top_args a, uint32_t nrows, uint32_t *__restrict__ scratch)
{
	__shared__ uint32_t wpop[2][WORDS];
	const scratch_map m = map_of(scratch, nrows);
	const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x;
	const uint32_t *mine = m.counts + TOP_TILE_WORDS * (size_t)t;
	const uint32_t e = m.head[2], taken = m.head[3];
	const uint32_t base_a = mine[2], base_e = mine[3];
	// (the same for every thread) a tile past N has no count; most tiles of a long sequence hold
	// nothing above the cut and no equal entry of rank below e
	if (mine[0] == 0 && (mine[1] == 0 || base_e >= e))
		return;
	const uint64_t N = entries_of(a.cap, a.n, a.segments), first = (uint64_t)t * TILE;
	if (first >= N)
		return;
	uint64_t g[PER_THREAD];
	uint32_t above, equal;
	const uint32_t valid = load_tile(a, N, first, g);
	against_cut(g, valid, prefix_of(m.head), above, equal);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t wa = __ballot(above >> k & 1), we = __ballot(equal >> k & 1);
		if (lane == 0) {
			wpop[0][word_of(0u, k, w)] = __popcll(wa);
			wpop[1][word_of(0u, k, w)] = __popcll(we);
		}
	}
	__syncthreads();
	if (w < 2) { // the set bits of the tile's words before each, of either kind
		const uint32_t own = wpop[w][lane], inc = lanes_through(own, lane);
		wpop[w][lane] = inc - own;
	}
	__syncthreads();
	const uint32_t slots = taken < EBPF_TOP_MAX ? taken : EBPF_TOP_MAX;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t wa = __ballot(above >> k & 1), we = __ballot(equal >> k & 1);
		const uint64_t lower = (1ull << lane) - 1;
		uint32_t dest = NO_POS;
		if (above >> k & 1) {
			dest = base_a + wpop[0][word_of(0u, k, w)] + __popcll(wa & lower);
		} else if (equal >> k & 1) {
			const uint32_t r = base_e + wpop[1][word_of(0u, k, w)] + __popcll(we & lower);
			dest = r < e ? (taken - e) + r : NO_POS;
		}
		if (dest < slots) {
			m.cand_g[dest] = g[k];
			m.cand_pos[dest] = (uint32_t)(first + k * THREADS + threadIdx.x);
		}
	}
}

// a before b: the larger g, then the lower position
__device__ __forceinline__ bool
first_of(uint64_t ga, uint32_t pa, uint64_t gb, uint32_t pb)
{
	return ga > gb || (ga == gb && pa < pb);
}

template <bool KEYS, bool VALS, bool POS>
__global__ void __launch_bounds__(CARRY_THREADS)
top_order(top_args a, uint32_t nrows, uint32_t *__restrict__ scratch, tops out,
	  uint64_t *__restrict__ info)
{
	__shared__ uint64_t sg[EBPF_TOP_MAX];
	__shared__ uint32_t sp[EBPF_TOP_MAX];
	const scratch_map m = map_of(scratch, nrows);
	const uint64_t N = entries_of(a.cap, a.n, a.segments);
	const uint32_t taken = m.head[3] < EBPF_TOP_MAX ? m.head[3] : EBPF_TOP_MAX;
	uint32_t P = 1; // the network's size: a power of two, at least taken
	while (P < taken)
		P <<= 1;
	for (uint32_t j = threadIdx.x; j < P; j += CARRY_THREADS) {
		sg[j] = j < taken ? m.cand_g[j] : 0;
		sp[j] = j < taken ? m.cand_pos[j] : NO_POS; // (padding: after every entry)
	}
	__syncthreads();
	for (uint32_t size = 2; size <= P; size <<= 1) {
		for (uint32_t stride = size >> 1; stride != 0; stride >>= 1) {
			for (uint32_t i = threadIdx.x; i < P / 2; i += CARRY_THREADS) {
				const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
				const uint64_t ga = sg[lo], gb = sg[hi];
				const uint32_t pa = sp[lo], pb = sp[hi];
				const bool forward = (lo & size) == 0;
				if (first_of(gb, pb, ga, pa) == forward) {
					sg[lo] = gb;
					sp[lo] = pb;
					sg[hi] = ga;
					sp[hi] = pa;
				}
			}
			__syncthreads();
		}
	}
	for (uint32_t j = threadIdx.x; j < taken; j += CARRY_THREADS) {
		const uint32_t p = sp[j];
		const bool there = p < N;
		if (KEYS)
			out.keys[j] = there ? a.keys[p] : 0;
		if (VALS)
			out.vals[j] = there ? a.vals[p] : 0;
		if (POS)
			out.pos[j] = p;
	}
	if (threadIdx.x == 0) {
		const uint64_t T = prefix_of(m.head);
		info[0] = taken;
		info[1] = N;
		info[2] = taken == 0 ? 0 : (a.smallest ? a.f.mask - T : T);
		info[3] = taken == 0 ? 0 : m.head[5] - m.head[2];
	}
}

// the tiles of a row, and the rows
void
rows_of(uint32_t ntiles, uint32_t &per_row, uint32_t &nrows)
{
	per_row = (ntiles + TOP_ROWS - 1) / TOP_ROWS;
	nrows = (ntiles + per_row - 1) / per_row;
}

} // namespace

size_t
top_scratch_bytes(uint64_t cap)
{
	uint32_t per_row, nrows;
	const uint32_t ntiles = tiles_of(cap);
	rows_of(ntiles, per_row, nrows);
	return ((size_t)TOP_HEAD_WORDS + 3 * EBPF_TOP_MAX + (size_t)nrows * BINS +
		(size_t)ntiles * TOP_TILE_WORDS) * sizeof(uint32_t);
}

hipError_t
launch_top(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
	   uint32_t flags, uint32_t val_shift, uint32_t val_bits, uint64_t k, const tops &out,
	   uint64_t *info, uint32_t *scratch, hipStream_t stream)
{
	uint32_t per_row, nrows;
	const uint32_t ntiles = tiles_of(cap);
	rows_of(ntiles, per_row, nrows);
	const top_args a = {keys, vals, cap, n, field_of(val_shift, val_bits),
			    flags & EBPF_TOP_SEGMENTS ? 1u : 0u, flags & EBPF_TOP_SMALLEST ? 1u : 0u};
	const uint32_t passes = (val_bits + 7) / 8;
	for (uint32_t i = 0; i < passes; i++) {
		const uint32_t shift = 8 * (passes - 1 - i);
		hipLaunchKernelGGL(top_count, dim3(nrows), dim3(THREADS), 0, stream, a, shift,
				   i == 0 ? 1u : 0u, per_row, ntiles, nrows, scratch);
		hipLaunchKernelGGL(top_pick, dim3(1), dim3(CARRY_THREADS), 0, stream, a, k, shift,
				   i == 0 ? 1u : 0u, nrows, scratch);
	}
	hipLaunchKernelGGL(top_tiles, dim3(ntiles), dim3(THREADS), 0, stream, a, nrows, scratch);
	hipLaunchKernelGGL(top_carry, dim3(1), dim3(CARRY_THREADS), 0, stream, ntiles, nrows, scratch);
	hipLaunchKernelGGL(top_place, dim3(ntiles), dim3(THREADS), 0, stream, a, nrows, scratch);
	with_flags([&](auto K, auto V, auto P) {
		hipLaunchKernelGGL((top_order<K, V, P>), dim3(1), dim3(CARRY_THREADS), 0, stream, a,
				   nrows, scratch, out, info);
	}, out.keys != nullptr, out.vals != nullptr, out.pos != nullptr);
	return hipGetLastError();
}
