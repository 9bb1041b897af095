// steer.hip — a batch's packets grouped by verdict class (ebpf_batch_steer_dev) and a packet
// list turned into an extents batch (ebpf_batch_select_dev).  DESIGN.md §2 "Steering by verdict".
//
// A multisplit over the histogram's EBPF_HIST_BINS classes in two sweeps over ret / faults:
//   steer_count    one workgroup per tile of STEER_TILE packets: the tile's class counts, one row
//                  of EBPF_HIST_BINS u32 per tile (rows[tile][class])
//   the tile scan  every class's tile counts become exclusive prefix sums: steer_col_scan, a
//                  workgroup per class over up to STEER_SEGS rows (a thread per row), leaves the
//                  class totals, whose prefix sums steer_starts writes to `starts`; past
//                  STEER_SEGS tiles the rows scanned are sums over segments of tiles
//                  (steer_seg_sum), and steer_scan_tiles then scans inside every segment
//   steer_scatter  re-reads the tile; wave w owns packets [w, w+1) * STEER_TILE/4 of it, so the
//                  waves' counts, prefix-summed in LDS on top of the tile's row, give every wave
//                  its first position per class; a wave then takes its 64-packet chunks in order.
// Within a 64-packet chunk every lane learns which lanes hold its class from one ballot per bit
// of the class in which the wave's classes differ at all (varying_bits, match_class: 2 bits for 4
// ports, all 9 for 257 classes); its rank is the population of that mask below it, and the mask's
// first lane counts, or advances the position, for them all.
// Every position is a sum of counts: atomics (LDS, integer) only ever count, so the output is a
// function of the input alone.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/wave_rank.h"
#include "host/steer.h"

namespace {

using namespace wave_rank;

constexpr uint32_t BINS = EBPF_HIST_BINS;
static_assert(BINS <= (1u << CLASS_BITS) && STEER_SEGS <= THREADS, "scan shape");

// The classes of packets first, first + step, ... (NONE past the batch's end); the loads as
// load_verdicts issues them.
template <bool FAULTS, uint32_t N>
__device__ __forceinline__ void
load_classes(const uint64_t *__restrict__ ret, const uint8_t *__restrict__ faults, uint64_t count,
	     uint64_t first, uint32_t step, uint32_t (&cls)[N])
{
	uint64_t r[N];
	uint32_t f[N];
	load_verdicts<FAULTS>(ret, faults, count, first, step, r, f);
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		const uint32_t c = f[k] ? BINS - 1 : (r[k] < 255 ? (uint32_t)r[k] : 255u);
		cls[k] = first + k * step < count ? c : NONE;
	}
}

template <bool FAULTS>
__global__ void __launch_bounds__(THREADS)
steer_count(const uint64_t *__restrict__ ret, const uint8_t *__restrict__ faults, uint64_t count,
	    uint32_t *__restrict__ rows)
{
	__shared__ uint32_t h[BINS];
	const uint32_t tid = threadIdx.x;
	for (uint32_t b = tid; b < BINS; b += THREADS)
		h[b] = 0;
	__syncthreads();
	const uint64_t first = (uint64_t)blockIdx.x * STEER_TILE;
	uint32_t cls[STEER_TILE / THREADS];
	load_classes<FAULTS>(ret, faults, count, first + tid, THREADS, cls);
	const uint32_t vary = varying_bits(cls);
#pragma unroll
	for (uint32_t k = 0; k < STEER_TILE / THREADS; k++) {
		const uint64_t m = match_class(cls[k], vary);
		if (m != 0 && below(m) == 0)
			atomicAdd(&h[cls[k]], (uint32_t)__popcll(m));
	}
	__syncthreads();
	uint32_t *row = rows + (size_t)blockIdx.x * BINS;
	for (uint32_t b = tid; b < BINS; b += THREADS)
		row[b] = h[b];
}

// seg[s][b] = the sum of rows[r][b] over segment s = rows [s*seglen, (s+1)*seglen)
__global__ void __launch_bounds__(THREADS)
steer_seg_sum(const uint32_t *__restrict__ rows, uint32_t nrows, uint32_t seglen,
	      uint32_t *__restrict__ seg)
{
	const uint32_t r0 = blockIdx.x * seglen;
	const uint32_t r1 = min(r0 + seglen, nrows);
	for (uint32_t b = threadIdx.x; b < BINS; b += THREADS) {
		uint32_t sum = 0;
#pragma unroll 16
		for (uint32_t r = r0; r < r1; r++)
			sum += rows[(size_t)r * BINS + b];
		seg[(size_t)blockIdx.x * BINS + b] = sum;
	}
}

// Workgroup b, thread r: rows[r][b] becomes the sum of rows[r'][b] over r' < r (nrows <= THREADS),
// tot[b] the sum of them all.
__global__ void __launch_bounds__(THREADS)
steer_col_scan(uint32_t *__restrict__ rows, uint32_t nrows, uint32_t *__restrict__ tot)
{
	__shared__ uint32_t wsum[WAVES];
	const uint32_t b = blockIdx.x, r = threadIdx.x, lane = r & 63, w = r >> 6;
	const uint32_t v = r < nrows ? rows[(size_t)r * BINS + b] : 0;
	uint32_t inc = v; // inclusive scan over the wave
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t up = __shfl_up(inc, d);
		if (lane >= d)
			inc += up;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	uint32_t before = 0;
	for (uint32_t q = 0; q < w; q++)
		before += wsum[q];
	if (r < nrows)
		rows[(size_t)r * BINS + b] = before + inc - v;
	if (r == THREADS - 1)
		tot[b] = before + inc;
}

// One workgroup: starts[b] = the sum of tot[b'] over b' < b, for b in [0, BINS].
__global__ void __launch_bounds__(THREADS)
steer_starts(const uint32_t *__restrict__ tot, uint64_t *__restrict__ starts)
{
	__shared__ uint32_t t[BINS + 1];
	const uint32_t tid = threadIdx.x;
	for (uint32_t b = tid; b < BINS; b += THREADS)
		t[b] = tot[b];
	__syncthreads();
	if (tid == 0) {
		uint32_t run = 0;
		for (uint32_t b = 0; b < BINS; b++) {
			const uint32_t v = t[b];
			t[b] = run;
			run += v;
		}
		t[BINS] = run;
	}
	__syncthreads();
	for (uint32_t b = tid; b <= BINS; b += THREADS)
		starts[b] = t[b];
}

// rows[r][b] of segment s becomes starts[b] + seg[s][b] + the sum of the segment's rows before r
__global__ void __launch_bounds__(THREADS)
steer_scan_tiles(uint32_t *__restrict__ rows, uint32_t nrows, uint32_t seglen,
		 const uint32_t *__restrict__ seg, const uint64_t *__restrict__ starts)
{
	const uint32_t r0 = blockIdx.x * seglen;
	const uint32_t r1 = min(r0 + seglen, nrows);
	for (uint32_t b = threadIdx.x; b < BINS; b += THREADS) {
		uint32_t run = (uint32_t)starts[b] + seg[(size_t)blockIdx.x * BINS + b];
#pragma unroll 16
		for (uint32_t r = r0; r < r1; r++) {
			const uint32_t v = rows[(size_t)r * BINS + b];
			rows[(size_t)r * BINS + b] = run;
			run += v;
		}
	}
}

// rows[tile][b] = the packets of class b in the tiles before this one, plus starts[b] already
// (rows_absolute: steer_scan_tiles added it) or not.
template <bool FAULTS>
__global__ void __launch_bounds__(THREADS)
steer_scatter(const uint64_t *__restrict__ ret, const uint8_t *__restrict__ faults, uint64_t count,
	      const uint32_t *__restrict__ rows, const uint64_t *__restrict__ starts,
	      uint32_t rows_absolute, uint32_t *__restrict__ index)
{
	// pos[w][b]: first the count of class b in wave w's packets, then the next position in
	// `index` for a packet of class b from wave w
	__shared__ uint32_t pos[WAVES][BINS];
	const uint32_t tid = threadIdx.x;
	const uint32_t w = tid >> 6, lane = tid & 63;
	for (uint32_t k = tid; k < WAVES * BINS; k += THREADS)
		(&pos[0][0])[k] = 0;
	__syncthreads();
	const uint64_t first = (uint64_t)blockIdx.x * STEER_TILE + w * WAVE_SPAN + lane;
	// per chunk: class | rank among the chunk's packets of the class << 9 | their number << 16
	uint32_t info[CHUNKS];
	load_classes<FAULTS>(ret, faults, count, first, 64, info);
	const uint32_t vary = varying_bits(info);
#pragma unroll
	for (uint32_t k = 0; k < CHUNKS; k++) {
		const uint32_t c = info[k];
		const uint64_t m = match_class(c, vary);
		if (m != 0) {
			const uint32_t rank = below(m), n = (uint32_t)__popcll(m);
			if (rank == 0)
				atomicAdd(&pos[w][c], n);
			info[k] = c | rank << CLASS_BITS | n << 16;
		}
	}
	__syncthreads();
	const uint32_t *row = rows + (size_t)blockIdx.x * BINS;
	for (uint32_t b = tid; b < BINS; b += THREADS) {
		uint32_t run = row[b] + (rows_absolute ? 0u : (uint32_t)starts[b]);
		for (uint32_t q = 0; q < WAVES; q++) {
			const uint32_t v = pos[q][b];
			pos[q][b] = run;
			run += v;
		}
	}
	__syncthreads();
	// (volatile: a lane reads the position another lane of its wave advanced a chunk earlier; a
	// wave's LDS operations complete in order)
	volatile uint32_t *next = pos[w];
#pragma unroll
	for (uint32_t k = 0; k < CHUNKS; k++) {
		if (info[k] == NONE)
			continue;
		const uint32_t c = info[k] & ((1u << CLASS_BITS) - 1);
		const uint32_t rank = (info[k] >> CLASS_BITS) & 63, n = info[k] >> 16;
		const uint32_t base = next[c];
		// (always true: the positions are sums of this input's own counts; kept so that an
		// input changed under the call cannot write outside)
		if (base + rank < count)
			index[base + rank] = (uint32_t)(first + k * 64);
		if (rank == 0)
			next[c] = base + n;
	}
}

__global__ void __launch_bounds__(THREADS)
steer_select(const uint64_t *__restrict__ offsets, uint64_t count, uint32_t stride, uint32_t extents,
	     const uint32_t *__restrict__ index, uint64_t n, uint64_t *__restrict__ out)
{
	for (uint64_t j = (uint64_t)blockIdx.x * THREADS + threadIdx.x; j < n;
	     j += (uint64_t)gridDim.x * THREADS) {
		const uint64_t i = index[j];
		uint64_t s = 0, e = 0;
		if (i < count) {
			if (offsets == nullptr) {
				s = i * stride;
				e = s + stride;
			} else if (extents) {
				s = offsets[2 * i];
				e = offsets[2 * i + 1];
			} else {
				s = offsets[i];
				e = offsets[i + 1];
			}
		}
		out[2 * j] = s;
		out[2 * j + 1] = e;
	}
}

inline uint32_t
tiles_of(uint64_t count)
{
	return (uint32_t)((count + STEER_TILE - 1) / STEER_TILE);
}

} // namespace

// tile rows | segment rows (two levels) | class totals
size_t
steer_scratch_words(uint64_t count)
{
	const uint32_t ntiles = tiles_of(count);
	return (size_t)(ntiles + (ntiles > STEER_SEGS ? STEER_SEGS : 0) + 1) * BINS;
}

bool
launch_tile_scan(uint32_t *scratch, uint32_t ntiles, uint64_t *starts, hipStream_t stream)
{
	const bool two = ntiles > STEER_SEGS;
	uint32_t *rows = scratch;
	uint32_t *seg = rows + (size_t)ntiles * BINS;
	uint32_t *tot = seg + (two ? (size_t)STEER_SEGS * BINS : 0);
	const uint32_t seglen = (ntiles + STEER_SEGS - 1) / STEER_SEGS;
	const uint32_t nseg = two ? (ntiles + seglen - 1) / seglen : 0;
	if (two)
		hipLaunchKernelGGL(steer_seg_sum, dim3(nseg), dim3(THREADS), 0, stream, rows, ntiles, seglen,
				   seg);
	hipLaunchKernelGGL(steer_col_scan, dim3(BINS), dim3(THREADS), 0, stream, two ? seg : rows,
			   two ? nseg : ntiles, tot);
	hipLaunchKernelGGL(steer_starts, dim3(1), dim3(THREADS), 0, stream, tot, starts);
	if (two)
		hipLaunchKernelGGL(steer_scan_tiles, dim3(nseg), dim3(THREADS), 0, stream, rows, ntiles,
				   seglen, seg, starts);
	return two;
}

hipError_t
launch_steer(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t *index,
	     uint64_t *starts, uint32_t *scratch, hipStream_t stream)
{
	const uint32_t ntiles = tiles_of(count);
	hipLaunchKernelGGL(faults ? steer_count<true> : steer_count<false>, dim3(ntiles), dim3(THREADS), 0,
			   stream, ret, faults, count, scratch);
	const bool two = launch_tile_scan(scratch, ntiles, starts, stream);
	hipLaunchKernelGGL(faults ? steer_scatter<true> : steer_scatter<false>, dim3(ntiles),
			   dim3(THREADS), 0, stream, ret, faults, count, scratch, starts, two ? 1u : 0u,
			   index);
	return hipGetLastError();
}

hipError_t
launch_select(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n, uint64_t *extents,
	      hipStream_t stream)
{
	const uint64_t blocks = (n + THREADS - 1) / THREADS;
	hipLaunchKernelGGL(steer_select, dim3((uint32_t)(blocks < (1u << 20) ? blocks : (1u << 20))),
			   dim3(THREADS), 0, stream, b.offsets, b.count, b.stride,
			   (b.flags & EBPF_BATCH_EXTENTS) ? 1u : 0u, index, n, extents);
	return hipGetLastError();
}
