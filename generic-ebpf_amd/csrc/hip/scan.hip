// scan.hip — running totals per segment over a list of a batch's packets (ebpf_batch_scan_dev):
// per position its rank in its segment, the bytes and the sum of a bit field of ret of the
// segment's entries before it, and whether it passes the segment's byte budget.  DESIGN.md §2
// "Running totals per group".
//
// The reduce's structure (reduce.hip) with per-position outputs; the cost follows the list, not
// the shape of its segments:
//   scan_tiles   one workgroup per tile of STEER_TILE list positions.  Two of its waves find the
//                segments of the tile's first and last position (a 64-way search of seg_starts);
//                the segments that begin in the tile mark their first position in LDS, and then
//                leave their budget there (one fetch per segment and tile).  A thread owns 16
//                consecutive positions; a segmented scan over the threads carries in what the
//                open segment holds before them and where in the tile it began.  Every output is
//                turned through LDS, so that neighbouring lanes store neighbouring entries.  All of
//                [0, n) is written: 0 where no segment covers a position.  The tile's leading
//                positions, those before the first marked one, get their totals within the tile
//                alone; their rank needs no more than the start of the segment that holds the
//                tile's first position.  A scratch row keeps what the tile hands on.
//   scan_carry   one workgroup: a segmented scan over the tiles' rows, two levels (a thread walks
//                a run of tiles).  Every tile edge is crossed by at most one segment; a tile's row
//                gets what that segment accumulated in the tiles before.
//   scan_fix     one workgroup per tile but the first: adds that to the tile's leading positions
//                and decides `over` there again.  It reads and writes output entries alone; only
//                where `over` is wanted without `bytes_before` does it fetch the lengths again.
// Every output entry is written by one thread of scan_tiles and at most once more by one thread
// of scan_fix, no atomic decides anything and no workgroup waits for another: the output is a
// function of the input alone.  A table that is not non-decreasing, or that ends past n, gives
// unspecified results, but every position is clamped to n, every segment number is below R and
// the marks stay inside the tile.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/scan.h"

namespace {

constexpr uint32_t NOPOS = ~0u; // no segment has begun in the tile yet
constexpr uint32_t ROW = SCAN_ROW_WORDS;
constexpr uint32_t SLOTS = TILE + TILE / 16;

typedef struct ebpf_batch_scans scans;

// A run of list entries: of the segment that began at tile position pos, or (NOPOS) of the one
// that was open before the run began.
struct part {
	uint64_t bytes, sum;
	uint32_t pos;
};
constexpr part NOTHING = {0, 0, NOPOS};

// The segmented scan's operator: run a, then run b.  A segment that begins in b closes a.
template <bool LENS, bool VALS>
__device__ __forceinline__ part
join(const part &a, const part &b)
{
	if (b.pos != NOPOS)
		return b;
	part r = a;
	if (LENS)
		r.bytes += b.bytes;
	if (VALS)
		r.sum += b.sum;
	return r;
}

template <bool LENS, bool VALS>
__device__ __forceinline__ part
lane_up(const part &p, uint32_t d)
{
	part r = p;
	r.pos = __shfl_up(p.pos, d);
	if (LENS)
		r.bytes = __shfl_up((unsigned long long)p.bytes, d);
	if (VALS)
		r.sum = __shfl_up((unsigned long long)p.sum, d);
	return r;
}

// slot(k * THREADS + threadIdx.x), the thread's k-th position in tile order: a constant apart.
__device__ __forceinline__ uint32_t
tile_slot(uint32_t k)
{
	return slot(threadIdx.x) + k * (THREADS + THREADS / 16);
}

// A thread's 16 results, of consecutive positions, stored in tile order: through the padded rows
// in LDS, so that neighbouring lanes store neighbouring entries of dst (16 entries a lane would go
// out at a stride of 64 or 128 bytes).  Every thread of the workgroup calls it; stage is free again
// on return.
template <typename V>
__device__ __forceinline__ void
store_tile(V *__restrict__ dst, uint64_t first, uint64_t n, const V (&v)[PER_THREAD], V *stage)
{
	const uint32_t tid = threadIdx.x;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		stage[slot(tid * PER_THREAD + k)] = v[k];
	__syncthreads();
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t j = first + k * THREADS + tid;
		if (j < n)
			dst[j] = stage[tile_slot(k)];
	}
	__syncthreads();
}

// A thread's 16 flags: they are 16 neighbouring bytes, and neighbouring lanes' are neighbours.
__device__ __forceinline__ void
store_flags(uint8_t *__restrict__ dst, uint64_t first, uint64_t n, const uint8_t (&v)[PER_THREAD])
{
	const uint64_t j0 = first + threadIdx.x * PER_THREAD;
	uint8_t *p = dst + j0;
	if (j0 + PER_THREAD <= n && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
		u32x4 w;
#pragma unroll
		for (uint32_t c = 0; c < 4; c++)
			w[c] = v[4 * c] | (uint32_t)v[4 * c + 1] << 8 | (uint32_t)v[4 * c + 2] << 16 |
			       (uint32_t)v[4 * c + 3] << 24;
		store16<false>(p, w);
		return;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		if (j0 + k < n)
			p[k] = v[k];
}

// One output of a thread's 16 positions: 0 rank, 1 bytes_before, 2 sum_before, 3 over.  in: what
// the segment that is open at the thread's first position holds before it; marks: bit k is set if
// a segment begins at the thread's position k; covered: bit k is set if a segment covers it;
// lead: the tile's first position minus the start of the segment that holds it (for the leading
// positions' ranks).  An entry without a length or a value has 0 for it.
template <int OUT, typename V>
__device__ __forceinline__ void
walk(V (&v)[PER_THREAD], const part &in, uint32_t marks, uint32_t covered,
     const uint32_t (&len)[PER_THREAD], const uint64_t (&val)[PER_THREAD], uint32_t lead,
     uint64_t lead_budget, const uint64_t *sbud)
{
	const uint32_t q0 = threadIdx.x * PER_THREAD;
	uint64_t acc = OUT == 2 ? in.sum : in.bytes;
	uint32_t rank = in.pos != NOPOS ? q0 - in.pos : lead + q0;
	uint64_t budget = 0;
	if (OUT == 3)
		budget = in.pos != NOPOS ? sbud[slot(in.pos)] : lead_budget;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (marks >> k & 1) {
			acc = 0;
			rank = 0;
			if (OUT == 3)
				budget = sbud[slot(q0 + k)];
		}
		uint64_t r;
		if (OUT == 0)
			r = rank++;
		else if (OUT == 3)
			r = acc + len[k] > budget;
		else
			r = acc;
		v[k] = (covered >> k & 1) ? (V)r : (V)0;
		acc += OUT == 2 ? val[k] : len[k];
	}
}

// count == 0 (LENS and VALS both false): no entry has a length or a value
__device__ __forceinline__ void
zero_tile(const scans &out, uint64_t first, uint64_t n)
{
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t j = first + k * THREADS + threadIdx.x;
		if (j >= n)
			continue;
		if (out.bytes_before != nullptr)
			out.bytes_before[j] = 0;
		if (out.sum_before != nullptr)
			out.sum_before[j] = 0;
		if (out.over != nullptr)
			out.over[j] = 0;
	}
}

// LENS: bytes_before or over is wanted; VALS: sum_before is.  With neither, rank alone is
// computed, rows is not used, and the other outputs that are given are set to 0 (count == 0).
// n >= 1; count >= 1 where LENS or VALS.  val_shift, val_mask: the value's bit_field.
template <bool LENS, bool VALS>
__global__ void __launch_bounds__(THREADS, 3) // (three waves a SIMD: the gathers want them)
scan_tiles(places f, const uint64_t *__restrict__ ret, uint32_t val_shift, uint64_t val_mask,
	   const uint32_t *__restrict__ index, uint64_t n, const uint64_t *__restrict__ S,
	   uint64_t cap, const uint64_t *__restrict__ nseg, const uint64_t *__restrict__ budgets,
	   scans out, uint64_t *__restrict__ rows)
{
	// The tile's list entries, and the segment that begins at a position, or NOHEAD; once both
	// are in registers, the budget of the segment that begins at a position, and then the
	// results on their way out.
	__shared__ __attribute__((aligned(16))) uint64_t stage[SLOTS];
	uint32_t *sidx = reinterpret_cast<uint32_t *>(stage), *sseg = sidx + SLOTS;
	__shared__ part wtot[WAVES];
	__shared__ uint64_t range[2];
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint64_t R = segments_of(cap, nseg);
	uint64_t *row = rows + (size_t)blockIdx.x * ROW;
	const uint64_t first = (uint64_t)blockIdx.x * TILE;
	const uint64_t end = seg_end(S, R, n); // the segments end where the last one does
	if (first >= end) { // (the same for every thread) no segment covers any of the tile
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint64_t j = first + k * THREADS + tid;
			if (j < n && out.rank != nullptr)
				out.rank[j] = 0;
		}
		if (LENS || VALS) {
			if (tid == 0)
				row[0] = row[1] = row[2] = row[5] = 0;
		}
		zero_tile(out, first, n);
		return;
	}
	const uint64_t last = (first + TILE < end ? first + TILE : end) - 1;
	uint32_t raw[PER_THREAD];
	if (LENS || VALS) {
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint64_t j = first + k * THREADS + tid;
			raw[k] = index[j < end ? j : end - 1];
		}
	}
	if (w < 2) {
		const uint64_t u = upper(S, R, w == 0 ? first : last);
		if (lane == 0)
			range[w] = u;
	}
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (LENS || VALS)
			sidx[tile_slot(k)] = raw[k];
		sseg[tile_slot(k)] = NOHEAD;
	}
	__syncthreads();
	// Segments [lo, hi) are those of the tile's positions: lo the one that holds `first` (0 if
	// none does yet), hi past the one that holds `last`.  One that is not empty marks its start.
	const bool held = range[0] != 0;
	const uint64_t lo = held ? range[0] - 1 : 0;
	const uint64_t hi = range[1] < R ? range[1] : R;
	for (uint64_t g = lo + tid; g < hi; g += THREADS) {
		uint64_t a, b;
		seg_bounds(S, g, n, a, b);
		if (a < b && a >= first && a - first < TILE)
			sseg[slot((uint32_t)(a - first))] = (uint32_t)g;
	}
	// The thread's 16 entries: the ret and offsets loads are issued together, as lens_of's.
	uint32_t idx[PER_THREAD] = {}, len[PER_THREAD] = {};
	uint64_t val[PER_THREAD] = {}; // the entry's value field
	const uint32_t live = (uint32_t)(last - first) + 1; // the tile's positions before the end
	const uint32_t q0 = tid * PER_THREAD;                // and the thread's
	const uint32_t mine_live = live > q0 ? (live - q0 < PER_THREAD ? live - q0 : PER_THREAD) : 0;
	if (LENS || VALS) {
		bool has[PER_THREAD];
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			idx[k] = sidx[slot(tid * PER_THREAD + k)];
			has[k] = k < mine_live && idx[k] < f.count;
		}
		fields_of<LENS, VALS>(f, ret, {val_shift, val_mask}, idx, has, len, val);
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			val[k] = has[k] ? val[k] : 0; // (an entry past the batch has no value)
	}
	__syncthreads();
	uint32_t marks = 0; // bit k: a segment begins at the thread's position k
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		marks |= (sseg[slot(tid * PER_THREAD + k)] != NOHEAD ? 1u : 0u) << k;
	__syncthreads();
	// (sidx and sseg are free: every thread has its entries and marks in registers)
	if (LENS && out.over != nullptr) {
		for (uint64_t g = lo + tid; g < hi; g += THREADS) {
			uint64_t a, b;
			seg_bounds(S, g, n, a, b);
			if (a < b && a >= first && a - first < TILE)
				stage[slot((uint32_t)(a - first))] = budgets[g];
		}
	}
	// what the leading positions need of the segment that holds `first`
	uint32_t lead = 0;
	uint64_t lead_budget = 0;
	if (held) {
		const uint64_t s = S[lo];
		lead = (uint32_t)(first - (s < first ? s : first));
		if (LENS && out.over != nullptr)
			lead_budget = budgets[lo];
	}
	// What leaves the thread on its right, its last run, and what lies before its first marked
	// position (fpos; all of its positions if it has none).
	part mine = NOTHING, head = NOTHING;
	uint32_t fpos = NOPOS;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (marks >> k & 1) {
			if (fpos == NOPOS) {
				fpos = k;
				head = mine;
			}
			mine = {0, 0, k};
		}
		if (LENS)
			mine.bytes += len[k];
		if (VALS)
			mine.sum += val[k];
	}
	if (fpos != NOPOS) { // (counted within the thread so far)
		fpos += q0;
		mine.pos += q0;
	}
	// (and the budgets are in LDS)
	const part in = carry_in<WAVES, join<LENS, VALS>, lane_up<LENS, VALS>>(mine, NOTHING, wtot);
	// The positions that a segment covers: those before the end, from the first marked one on,
	// or all of them if a segment is open at the thread's first.
	uint32_t covered = marks;
	covered |= covered << 1;
	covered |= covered << 2;
	covered |= covered << 4;
	covered |= covered << 8;
	if (in.pos != NOPOS || held)
		covered = 0xffff;
	covered &= (1u << mine_live) - 1;
	if (LENS || VALS) {
		// The row: the thread that meets the tile's first marked position has the leading
		// positions' totals, the last thread what the tile hands on.
		if (in.pos == NOPOS && fpos != NOPOS) {
			const part lead_sums = join<LENS, VALS>(in, head);
			row[0] = lead_sums.bytes;
			row[1] = lead_sums.sum;
			row[5] = held ? fpos : 0;
			row[6] = lead_budget;
		}
		if (tid == THREADS - 1) {
			const part cur = join<LENS, VALS>(in, mine);
			row[2] = cur.pos != NOPOS;
			if (cur.pos != NOPOS) {
				row[3] = cur.bytes;
				row[4] = cur.sum;
			} else { // no segment begins in the tile: every position before the end leads
				row[0] = cur.bytes;
				row[1] = cur.sum;
				row[5] = held ? live : 0;
				row[6] = lead_budget;
			}
		}
	}
	// (the flags first: the budgets are in LDS; then the values, the lengths and the marks, each
	// needed no longer once its output is stored)
	if (LENS && out.over != nullptr) {
		uint8_t v[PER_THREAD];
		walk<3>(v, in, marks, covered, len, val, lead, lead_budget, stage);
		store_flags(out.over, first, n, v);
		__syncthreads(); // (the budgets are read)
	}
	if (VALS) {
		uint64_t v[PER_THREAD];
		walk<2>(v, in, marks, covered, len, val, lead, 0, stage);
		store_tile(out.sum_before, first, n, v, stage);
	}
	if (LENS && out.bytes_before != nullptr) {
		uint64_t v[PER_THREAD];
		walk<1>(v, in, marks, covered, len, val, lead, 0, stage);
		store_tile(out.bytes_before, first, n, v, stage);
	}
	if (out.rank != nullptr) {
		uint32_t v[PER_THREAD];
		walk<0>(v, in, marks, covered, len, val, lead, 0, stage);
		store_tile(out.rank, first, n, v, sidx);
	}
	if (!LENS && !VALS)
		zero_tile(out, first, n);
}

// What tile t hands to the tiles after it.
__device__ __forceinline__ part
tile_tail(const uint64_t *__restrict__ rows, uint32_t t)
{
	const uint64_t *row = rows + (size_t)t * ROW;
	const bool begins = row[2] != 0;
	return {begins ? row[3] : row[0], begins ? row[4] : row[1], begins ? 0u : NOPOS};
}

// One workgroup: a thread walks its run of tiles (run_of) twice, first for what the run hands
// on, then, with what the threads before it hand in, to leave in every tile's row what the
// segment that is open at the tile's first position accumulated before it.
__global__ void __launch_bounds__(CARRY_THREADS)
scan_carry(uint64_t *__restrict__ rows, uint32_t ntiles)
{
	__shared__ part wtot[CARRY_THREADS / 64];
	const auto [t0, t1] = run_of(ntiles);
	part mine = NOTHING;
	for (uint32_t t = t0; t < t1; t++)
		mine = join<true, true>(mine, tile_tail(rows, t));
	part cur = carry_in<CARRY_THREADS / 64, join<true, true>, lane_up<true, true>>(mine, NOTHING, wtot);
	for (uint32_t t = t0; t < t1; t++) {
		uint64_t *row = rows + (size_t)t * ROW;
		row[7] = cur.bytes;
		row[8] = cur.sum;
		cur = join<true, true>(cur, tile_tail(rows, t));
	}
}

// One workgroup per tile but the first: the tile's leading positions get what their segment
// accumulated in the tiles before.  Entry j's length is the next entry's bytes_before less its
// own (the row's total less its own for the last leading position) where bytes_before is
// written; where over is wanted alone, the lengths are fetched again (GATHER).
template <bool GATHER>
__global__ void __launch_bounds__(THREADS)
scan_fix(const uint64_t *__restrict__ rows, places f, const uint32_t *__restrict__ index, uint64_t n,
	 scans out)
{
	const uint32_t tid = threadIdx.x;
	const uint64_t *row = rows + (size_t)(blockIdx.x + 1) * ROW;
	const uint64_t first = (uint64_t)(blockIdx.x + 1) * TILE;
	uint64_t L = row[5];
	L = L < n - first ? L : n - first;
	const uint64_t base_bytes = row[7], base_sum = row[8], head_bytes = row[0], budget = row[6];
	if (L == 0 || (base_bytes == 0 && base_sum == 0)) // (the same for every thread)
		return;
	if (out.sum_before != nullptr && base_sum != 0) {
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint32_t q = k * THREADS + tid;
			if (q < L)
				out.sum_before[first + q] += base_sum;
		}
	}
	if (base_bytes == 0 || (out.bytes_before == nullptr && out.over == nullptr))
		return;
	if (GATHER) { // over alone: the running total inside the tile is kept nowhere
		__shared__ uint64_t wsum[WAVES];
		uint32_t len[PER_THREAD];
		lens_of(f, index, first + L, first + tid, len);
		uint64_t before = 0;
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint32_t q = k * THREADS + tid;
			uint64_t all;
			const uint64_t mine = q < L ? len[k] : 0;
			const uint64_t ex = before + block_scan(mine, wsum, all);
			if (q < L)
				out.over[first + q] = base_bytes + ex + mine > budget;
			before += all;
		}
		return;
	}
	uint64_t own[PER_THREAD], next[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint32_t q = k * THREADS + tid;
		own[k] = q < L ? out.bytes_before[first + q] : 0;
		next[k] = q + 1 < L ? out.bytes_before[first + q + 1] : head_bytes;
	}
	__syncthreads(); // (every leading entry is read before any is written)
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint32_t q = k * THREADS + tid;
		if (q >= L)
			continue;
		out.bytes_before[first + q] = own[k] + base_bytes;
		if (out.over != nullptr)
			out.over[first + q] = base_bytes + next[k] > budget;
	}
}

} // namespace

size_t
scan_scratch_bytes(uint64_t n)
{
	return (size_t)((n + TILE - 1) / TILE) * ROW * sizeof(uint64_t);
}

hipError_t
launch_scan(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
	    uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
	    const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg, const uint64_t *budgets,
	    const struct ebpf_batch_scans &out, uint64_t *scratch, hipStream_t stream)
{
	const bool lens = count != 0 && (out.bytes_before != nullptr || out.over != nullptr);
	const bool vals = count != 0 && out.sum_before != nullptr;
	const places f = lens ? places_of(*batch) : places{nullptr, count, 0, 0};
	const bit_field vf = field_of(val_shift, val_bits);
	const uint32_t ntiles = (uint32_t)((n + TILE - 1) / TILE);
	with_flags([&](auto L, auto V) {
		hipLaunchKernelGGL((scan_tiles<L, V>), dim3(ntiles), dim3(THREADS), 0, stream, f, ret, vf.shift,
				   vf.mask, index, n, seg_starts, seg_cap, nseg, budgets, out, scratch);
	}, lens, vals);
	if ((!lens && !vals) || ntiles < 2) // (the first tile's leading positions have nothing before them)
		return hipGetLastError();
	hipLaunchKernelGGL(scan_carry, dim3(1), dim3(CARRY_THREADS), 0, stream, scratch, ntiles);
	// (over without bytes_before: the lengths are fetched again)
	with_flags([&](auto G) {
		hipLaunchKernelGGL(scan_fix<G>, dim3(ntiles - 1), dim3(THREADS), 0, stream, scratch, f, index, n,
				   out);
	}, out.bytes_before == nullptr && out.over != nullptr);
	return hipGetLastError();
}
