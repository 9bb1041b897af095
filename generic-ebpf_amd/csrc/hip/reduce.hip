// reduce.hip — per-segment reductions over a list of a batch's packets (ebpf_batch_reduce_dev):
// bytes, and the sum, minimum, maximum and OR of a bit field of ret.  DESIGN.md §2 "Reducing per
// group".
//
// A segmented reduction whose cost follows the list, not the shape of its segments:
//   reduce_tiles   one workgroup per tile of STEER_TILE list positions.  Two of its waves find the
//                  segments of the tile's first and last position (a 64-way search of seg_starts);
//                  the segments that begin in the tile mark their first position in LDS (empty
//                  ones mark nothing, so any number of them at one position costs their reads
//                  alone).  A thread owns 16 consecutive positions: it reduces them run by run,
//                  the runs that end in it are closed with what a segmented scan over the threads
//                  carries in, and a segment that begins and ends in the tile is written at once
//                  (a tile that closes many of them stages them in LDS and stores them in
//                  segment order: write_staged).
//                  What is open at the tile's edges goes to two scratch rows: the positions before
//                  the tile's first marked one, and those from its last marked one on.
//   reduce_carry   one workgroup: the same segmented scan over the tiles' rows, two levels (a
//                  thread walks a run of tiles).  Every tile edge is crossed by at most one
//                  segment; the tile in which such a segment ends writes it.
//   reduce_empty   a thread per segment: an empty segment's identities.
// Every output entry below R is written by exactly one thread of one kernel, no atomic decides
// anything and no workgroup waits for another: the output is a function of the input alone.
// Positions at or past seg_starts[R] add identities, positions before seg_starts[0] add to a run
// that nobody writes.  A table that is not non-decreasing, or that ends past n, gives unspecified
// sums, but every position is clamped to n, every segment number that is written is below R, and
// the marks stay inside the tile.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/reduce.h"

namespace {

constexpr uint32_t ROW = REDUCE_ROW_WORDS;
// A tile that closes this many segments or more writes them out through LDS, STAGE at a time.
constexpr uint32_t STAGE_MIN = 256;
constexpr uint32_t STAGE = TILE / 2;

typedef struct ebpf_batch_sums sums;

// A run of list entries reduced: of segment g if flag, else of the segment that was open before
// the run began.
struct part {
	uint64_t bytes;
	stats s;
	uint32_t g, flag;
};

__device__ __forceinline__ part
nothing()
{
	return {0, NO_STATS, 0, 0};
}

// a's entries, then b's, of one segment
template <bool LENS, bool VALS>
__device__ __forceinline__ void
add(part &a, const part &b)
{
	if (LENS)
		a.bytes += b.bytes;
	if (VALS)
		add(a.s, b.s);
}

// The segmented scan's operator: run a, then run b.  A segment that begins in b closes a.
template <bool LENS, bool VALS>
__device__ __forceinline__ part
join(const part &a, const part &b)
{
	if (b.flag)
		return b;
	part r = a;
	add<LENS, VALS>(r, b);
	return r;
}

template <bool LENS, bool VALS>
__device__ __forceinline__ part
lane_up(const part &p, uint32_t d)
{
	part r = p;
	r.g = __shfl_up(p.g, d);
	r.flag = __shfl_up(p.flag, d);
	if (LENS)
		r.bytes = __shfl_up((unsigned long long)p.bytes, d);
	if (VALS)
		r.s = up(p.s, d);
	return r;
}

template <bool LENS, bool VALS>
__device__ __forceinline__ void
store_row(uint64_t *__restrict__ row, const part &p)
{
	if (LENS)
		row[0] = p.bytes;
	if (VALS)
		store(row + 1, p.s);
}

template <bool LENS, bool VALS>
__device__ __forceinline__ part
load_row(const uint64_t *__restrict__ row)
{
	part p = nothing();
	if (LENS)
		p.bytes = row[0];
	if (VALS)
		p.s = load(row + 1);
	return p;
}

// segment g's results, if it is one of the R
template <bool LENS, bool VALS>
__device__ __forceinline__ void
write_out(const sums &out, uint64_t g, uint64_t R, const part &p)
{
	if (g >= R)
		return;
	if (LENS)
		out.bytes[g] = p.bytes;
	if (VALS) {
		if (out.sum != nullptr)
			out.sum[g] = p.s.sum;
		if (out.min != nullptr)
			out.min[g] = p.s.mn;
		if (out.max != nullptr)
			out.max[g] = p.s.mx;
		if (out.bits != nullptr)
			out.bits[g] = p.s.bits;
	}
}

// the one output beside the four statistics of seg_tile.h: a sum
enum { BYTES = STATS };

// One output of the segments that a tile closes, written in segment order: the tile's e-th
// marked position closes the segment that the one before it began, number sg[e - 1].  The thread
// walks its entries for this statistic alone, puts what it closes into sv (STAGE results at a
// time), and the workgroup then stores sv to neighbouring entries of dst from neighbouring lanes:
// a thread that closes 16 one-entry segments would otherwise store them one by one, 8 bytes a
// lane at a 128-byte stride.  hb: the marked positions before the thread's; closed: the segments
// the tile closes.  Every thread of the workgroup calls it.
template <int STAT>
__device__ __forceinline__ void
write_staged(uint64_t *__restrict__ dst, uint64_t R, const uint32_t (&seg)[PER_THREAD],
	     const uint32_t (&len)[PER_THREAD], const uint64_t (&val)[PER_THREAD],
	     const bool (&has)[PER_THREAD], uint64_t carried, uint32_t hb, uint32_t closed,
	     const uint32_t *sg, uint64_t *sv)
{
	if (dst == nullptr) // (the same for every thread)
		return;
	for (uint32_t base = 0; base < closed; base += STAGE) {
		uint64_t acc = carried;
		uint32_t e = hb;
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			if (seg[k] != NOHEAD) {
				// (unsigned: false for e - 1 below base as well)
				if (e != 0 && e - 1 - base < STAGE)
					sv[e - 1 - base] = acc;
				acc = ident<STAT>();
				e++;
			}
			acc = fold<STAT>(acc, STAT == BYTES ? len[k] : has[k] ? val[k] : ident<STAT>());
		}
		__syncthreads();
		const uint32_t m = closed - base < STAGE ? closed - base : STAGE;
		for (uint32_t r = threadIdx.x; r < m; r += THREADS) {
			const uint64_t g = sg[base + r];
			if (g < R)
				dst[g] = sv[r];
		}
		__syncthreads();
	}
}

// rows: per tile, {bytes, sum, min, max, bits, does a segment begin in the tile} over the
// positions before the first that begins one (all of them if none does), then {..., that
// segment} over the positions from the last such on.  count >= 1, n >= 1.  val_shift, val_mask:
// the value's bit_field.
template <bool LENS, bool VALS>
__global__ void __launch_bounds__(THREADS, 3) // (three waves a SIMD: the gathers want them)
reduce_tiles(places f, const uint64_t *__restrict__ ret, uint32_t val_shift, uint64_t val_mask,
	     const uint32_t *__restrict__ index, uint64_t n, const uint64_t *__restrict__ S,
	     uint64_t cap, const uint64_t *__restrict__ nseg, sums out, uint64_t *__restrict__ rows)
{
	__shared__ uint32_t sidx[TILE + TILE / 16]; // the tile's list entries
	// the segment that begins at a position, or NOHEAD; later STAGE results on their way out
	__shared__ __attribute__((aligned(8))) uint32_t sseg[TILE + TILE / 16];
	static_assert(STAGE * sizeof(uint64_t) <= sizeof(sseg), "the staged results fit");
	__shared__ part wtot[WAVES];
	__shared__ uint64_t wsum[WAVES];
	__shared__ uint64_t range[2];
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint64_t R = segments_of(cap, nseg);
	uint64_t *row = rows + (size_t)blockIdx.x * 2 * ROW;
	const uint64_t first = (uint64_t)blockIdx.x * TILE;
	const uint64_t end = seg_end(S, R, n); // the list ends where the last segment does
	if (first >= end) { // (the same for every thread)
		if (tid == 0) {
			store_row<LENS, VALS>(row, nothing());
			row[ROW - 1] = 0;
		}
		return;
	}
	const uint64_t last = (first + TILE < end ? first + TILE : end) - 1;
	uint32_t raw[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t j = first + k * THREADS + tid;
		raw[k] = index[j < end ? j : end - 1];
	}
	if (w < 2) {
		const uint64_t u = upper(S, R, w == 0 ? first : last);
		if (lane == 0)
			range[w] = u;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		sidx[slot(k * THREADS + tid)] = raw[k];
		sseg[slot(k * THREADS + tid)] = NOHEAD;
	}
	__syncthreads();
	// Segments [lo, hi) are those of the tile's positions: lo the one that holds `first` (0 if
	// none does yet), hi past the one that holds `last`.  One that is not empty marks its start.
	const uint64_t lo = range[0] != 0 ? range[0] - 1 : 0;
	const uint64_t hi = range[1] < R ? range[1] : R;
	for (uint64_t g = lo + tid; g < hi; g += THREADS) {
		uint64_t a, b;
		seg_bounds(S, g, n, a, b);
		if (a < b && a >= first && a - first < TILE)
			sseg[slot((uint32_t)(a - first))] = (uint32_t)g;
	}
	// The thread's 16 entries: the ret and offsets loads are issued together, as lens_of's.
	uint32_t idx[PER_THREAD], len[PER_THREAD] = {};
	uint64_t val[PER_THREAD] = {}; // the entry's value field
	bool has[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		idx[k] = sidx[slot(tid * PER_THREAD + k)];
		has[k] = first + tid * PER_THREAD + k < end && idx[k] < f.count;
	}
	fields_of<LENS, VALS>(f, ret, {val_shift, val_mask}, idx, has, len, val);
	__syncthreads();
	uint32_t seg[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		seg[k] = sseg[slot(tid * PER_THREAD + k)];
	// entry k as a part (identities for an entry with no value, and past the list's end)
	auto entry = [&](uint32_t k) {
		part p = nothing();
		if (LENS)
			p.bytes = len[k];
		if (VALS && has[k])
			p.s = {val[k], val[k], val[k], val[k]};
		return p;
	};
	// what leaves the thread on its right: its last run
	part mine = nothing();
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (seg[k] != NOHEAD) {
			mine = nothing();
			mine.flag = 1;
			mine.g = seg[k];
		}
		add<LENS, VALS>(mine, entry(k));
	}
	part cur = carry_in<WAVES, join<LENS, VALS>, lane_up<LENS, VALS>>(mine, nothing(), wtot);
	// The marked positions before this thread's, and the tile's.  All but the last close a
	// segment inside the tile; many of them go out through LDS (every thread decides alike).
	uint32_t marked = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		marked += seg[k] != NOHEAD;
	uint64_t all;
	const uint32_t hb = (uint32_t)block_scan(marked, wsum, all);
	const uint32_t closed = all != 0 ? (uint32_t)all - 1 : 0;
	const bool staged = closed >= STAGE_MIN;
	if (staged) {
		// (sidx and sseg are free: every thread has its entries and marks in registers)
		uint32_t *sg = sidx;
		uint64_t *sv = reinterpret_cast<uint64_t *>(sseg);
		uint32_t e = hb;
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			if (seg[k] != NOHEAD)
				sg[e++] = seg[k];
		if (LENS)
			write_staged<BYTES>(out.bytes, R, seg, len, val, has, cur.bytes, hb, closed, sg, sv);
		if (VALS) {
			write_staged<SUM>(out.sum, R, seg, len, val, has, cur.s.sum, hb, closed, sg, sv);
			write_staged<MIN>(out.min, R, seg, len, val, has, cur.s.mn, hb, closed, sg, sv);
			write_staged<MAX>(out.max, R, seg, len, val, has, cur.s.mx, hb, closed, sg, sv);
			write_staged<BITS>(out.bits, R, seg, len, val, has, cur.s.bits, hb, closed, sg, sv);
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (seg[k] != NOHEAD) {
			if (cur.flag) {
				if (!staged)
					write_out<LENS, VALS>(out, cur.g, R, cur);
			} else { // the tile's first: what came before it belongs to an earlier tile's segment
				store_row<LENS, VALS>(row, cur);
			}
			cur = nothing();
			cur.flag = 1;
			cur.g = seg[k];
		}
		add<LENS, VALS>(cur, entry(k));
	}
	if (tid == THREADS - 1) {
		row[ROW - 1] = cur.flag;
		if (cur.flag) {
			store_row<LENS, VALS>(row + ROW, cur);
			row[2 * ROW - 1] = cur.g;
		} else {
			store_row<LENS, VALS>(row, cur);
		}
	}
}

// What tile t hands to the tiles after it.
template <bool LENS, bool VALS>
__device__ __forceinline__ part
tile_tail(const uint64_t *__restrict__ rows, uint32_t t)
{
	const uint64_t *row = rows + (size_t)t * 2 * ROW;
	const bool begins = row[ROW - 1] != 0;
	part p = load_row<LENS, VALS>(begins ? row + ROW : row);
	p.flag = begins;
	p.g = begins ? (uint32_t)row[2 * ROW - 1] : 0;
	return p;
}

// One workgroup: a thread walks its run of tiles (run_of) twice, first for what the run hands
// on, then, with what the threads before it hand in, to close the segments that cross tile
// edges: each is written where the next segment begins, the last one by the last tile.
template <bool LENS, bool VALS>
__global__ void __launch_bounds__(CARRY_THREADS)
reduce_carry(const uint64_t *__restrict__ rows, uint32_t ntiles, uint64_t cap,
	     const uint64_t *__restrict__ nseg, sums out)
{
	__shared__ part wtot[CARRY_THREADS / 64];
	const uint64_t R = segments_of(cap, nseg);
	const auto [t0, t1] = run_of(ntiles);
	part mine = nothing();
	for (uint32_t t = t0; t < t1; t++)
		mine = join<LENS, VALS>(mine, tile_tail<LENS, VALS>(rows, t));
	part cur =
	    carry_in<CARRY_THREADS / 64, join<LENS, VALS>, lane_up<LENS, VALS>>(mine, nothing(), wtot);
	for (uint32_t t = t0; t < t1; t++) {
		const uint64_t *row = rows + (size_t)t * 2 * ROW;
		const part head = load_row<LENS, VALS>(row);
		add<LENS, VALS>(cur, head);
		if (row[ROW - 1] != 0) {
			if (cur.flag)
				write_out<LENS, VALS>(out, cur.g, R, cur);
			cur = tile_tail<LENS, VALS>(rows, t);
		}
	}
	if (t0 < t1 && t1 == ntiles && cur.flag)
		write_out<LENS, VALS>(out, cur.g, R, cur);
}

// A thread per segment: an empty one's results.  (n == 0: every segment is empty.)
__global__ void __launch_bounds__(THREADS)
reduce_empty(const uint64_t *__restrict__ S, uint64_t n, uint64_t cap,
	     const uint64_t *__restrict__ nseg, sums out)
{
	const uint64_t g = (uint64_t)blockIdx.x * THREADS + threadIdx.x;
	if (g >= segments_of(cap, nseg))
		return;
	uint64_t a, b;
	seg_bounds(S, g, n, a, b);
	if (a < b)
		return;
	if (out.bytes != nullptr)
		out.bytes[g] = 0;
	if (out.sum != nullptr)
		out.sum[g] = 0;
	if (out.min != nullptr)
		out.min[g] = ~0ull;
	if (out.max != nullptr)
		out.max[g] = 0;
	if (out.bits != nullptr)
		out.bits[g] = 0;
}

} // namespace

size_t
reduce_scratch_bytes(uint64_t n)
{
	return (size_t)((n + TILE - 1) / TILE) * 2 * ROW * sizeof(uint64_t);
}

hipError_t
launch_reduce(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
	      uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
	      const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
	      const struct ebpf_batch_sums &out, uint64_t *scratch, hipStream_t stream)
{
	const bool lens = out.bytes != nullptr, vals = wants_values(out);
	if (n != 0) {
		const places f = lens ? places_of(*batch) : places{nullptr, count, 0, 0};
		const bit_field vf = field_of(val_shift, val_bits);
		const uint32_t ntiles = (uint32_t)((n + TILE - 1) / TILE);
		with_flags([&](auto L, auto V) {
			if constexpr (L || V) { // (one output is wanted: no kernels for neither)
				hipLaunchKernelGGL((reduce_tiles<L, V>), dim3(ntiles), dim3(THREADS), 0, stream, f,
						   ret, vf.shift, vf.mask, index, n, seg_starts, seg_cap, nseg, out,
						   scratch);
				hipLaunchKernelGGL((reduce_carry<L, V>), dim3(1), dim3(CARRY_THREADS), 0, stream,
						   scratch, ntiles, seg_cap, nseg, out);
			}
		}, lens, vals);
	}
	const uint32_t blocks = (uint32_t)((seg_cap + THREADS - 1) / THREADS);
	hipLaunchKernelGGL(reduce_empty, dim3(blocks), dim3(THREADS), 0, stream, seg_starts, n, seg_cap,
			   nseg, out);
	return hipGetLastError();
}
