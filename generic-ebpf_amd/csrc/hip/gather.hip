// gather.hip — a list of a batch's packets copied into a dense batch (ebpf_batch_gather_dev).
// DESIGN.md §2 "Gathering a class".
//
// Two paths:
//   gather_rows    both sides fixed at one stride, a multiple of 16, on 16-byte bases: stride/16
//                  lanes serve a packet, each with one 16-byte load and one 16-byte store, so a
//                  wave-instruction's stores are 1 KiB contiguous whatever the list holds
//   gather_copy    everything else, strided or packed: the copy is owned by the OUTPUT.  A
//                  workgroup takes COPY_TILE list entries, keeps their (source start, length,
//                  destination start) in LDS and walks the tile's destination range in 16-byte
//                  chunks aligned in memory; a lane finds its chunk's packet by a search over the
//                  destination starts.  A chunk inside one packet moves 16 bytes (the load at
//                  whatever alignment the source has, the store aligned); a chunk inside one slot's
//                  padding stores 16 zero bytes; a chunk with the end of one packet and the start
//                  of the next takes 16 bytes of each and shifts them together; a chunk that
//                  straddles anything else (short packets, padding, the tile's or the output's
//                  ends) goes byte by byte.  Every output byte has one writer, short packets cost
//                  no idle lanes and long ones need no per-packet loop.
// The packed form's destination starts are out_offsets, made first: gather_tile_sums (a u64 sum
// of lengths per GATHER_TILE entries), an exclusive scan of the tile sums (gather_scan_rows over
// up to GATHER_SEGS rows; past that many tiles the rows scanned are sums over segments of tiles,
// gather_seg_sum, and gather_scan_tiles then scans inside every segment), and
// gather_write_offsets, which scans each tile's lengths on top of its sum.
// Every position is a sum of lengths: no atomics, no waiting on another workgroup; the output is a
// function of the input alone.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/batch_places.h"
#include "host/gather.h"

// The choices measured in DESIGN.md §2 "Gathering a class", as -D switches for an A/B build
// (tools/gather_bench.py under EBPF_LIB): nontemporal loads / stores of the row path, nontemporal
// 16-byte moves of the general copy, 16-byte units a lane of gather_rows loads before its first
// store, 16-byte chunks a lane of gather_copy takes per trip.
#ifndef GATHER_NT_LOAD
#define GATHER_NT_LOAD 1
#endif
#ifndef GATHER_NT_STORE
#define GATHER_NT_STORE 1
#endif
#ifndef GATHER_COPY_NT
#define GATHER_COPY_NT 0
#endif
#ifndef GATHER_ROW_K
#define GATHER_ROW_K 4
#endif
#ifndef GATHER_COPY_K
#define GATHER_COPY_K 1
#endif

namespace {

constexpr uint32_t ROW_K = GATHER_ROW_K;
constexpr uint32_t COPY_K = GATHER_COPY_K;
constexpr uint32_t COPY_TILE = 256;   // list entries per workgroup of gather_copy
constexpr uint32_t ROUNDS = GATHER_TILE / THREADS;
static_assert(GATHER_TILE % THREADS == 0 && GATHER_SEGS <= THREADS, "scan shape");
static_assert((COPY_TILE & (COPY_TILE - 1)) == 0 && COPY_TILE <= THREADS, "copy tile shape");

// ---------------------------------------------------------------- row path

// Unit u = 16 bytes: part u % lanes of list entry u / lanes, at out + 16 u.  A lane takes ROW_K
// units a workgroup's width apart, and issues their index loads, then their packet loads, before
// its first store; a unit past the end reads the last one instead, so no load sits behind a branch.
template <bool POW2>
__global__ void __launch_bounds__(THREADS)
gather_rows(const uint8_t *__restrict__ data, uint64_t count, uint32_t stride, uint32_t lanes,
	    uint32_t shift, const uint32_t *__restrict__ index, uint64_t n, uint8_t *__restrict__ out)
{
	const uint64_t total = n * lanes;
	constexpr uint64_t SPAN = (uint64_t)THREADS * ROW_K;
	for (uint64_t base = blockIdx.x * SPAN + threadIdx.x; base < total + threadIdx.x;
	     base += gridDim.x * SPAN) {
		uint32_t idx[ROW_K], part[ROW_K];
		u32x4 v[ROW_K];
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			const uint64_t u = base + k * THREADS;
			const uint64_t at = u < total ? u : total - 1;
			const uint64_t j = POW2 ? at >> shift : at / lanes;
			part[k] = (uint32_t)(at - j * lanes);
			idx[k] = index[j];
		}
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			// (an index past the batch reads nothing and stores zeros)
			v[k] = (u32x4){0, 0, 0, 0};
			if (idx[k] < count)
				v[k] = load16<GATHER_NT_LOAD>(data + (uint64_t)idx[k] * stride + part[k] * 16u);
		}
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			const uint64_t u = base + k * THREADS;
			if (u < total)
				store16<GATHER_NT_STORE>(out + u * 16, v[k]);
		}
	}
}

// ---------------------------------------------------------------- packed form: out_offsets

__global__ void __launch_bounds__(THREADS)
gather_tile_sums(places f, const uint32_t *__restrict__ index, uint64_t n, uint64_t *__restrict__ sums)
{
	__shared__ uint64_t wsum[WAVES];
	const uint64_t first = (uint64_t)blockIdx.x * GATHER_TILE + threadIdx.x;
	uint32_t len[ROUNDS];
	lens_of(f, index, n, first, len);
	uint64_t sum = 0;
#pragma unroll
	for (uint32_t k = 0; k < ROUNDS; k++)
		sum += len[k];
	uint64_t total;
	block_scan(sum, wsum, total);
	if (threadIdx.x == 0)
		sums[blockIdx.x] = total;
}

// seg[s] = the sum of rows [s*seglen, (s+1)*seglen)
__global__ void __launch_bounds__(THREADS)
gather_seg_sum(const uint64_t *__restrict__ rows, uint32_t nrows, uint32_t seglen,
	       uint64_t *__restrict__ seg)
{
	__shared__ uint64_t wsum[WAVES];
	const uint32_t r0 = blockIdx.x * seglen;
	const uint32_t r1 = min(r0 + seglen, nrows);
	uint64_t sum = 0;
	for (uint32_t r = r0 + threadIdx.x; r < r1; r += THREADS)
		sum += rows[r];
	uint64_t total;
	block_scan(sum, wsum, total);
	if (threadIdx.x == 0)
		seg[blockIdx.x] = total;
}

// One workgroup: rows[r] becomes the sum of the rows before r (nrows <= THREADS).
__global__ void __launch_bounds__(THREADS)
gather_scan_rows(uint64_t *__restrict__ rows, uint32_t nrows)
{
	__shared__ uint64_t wsum[WAVES];
	const uint32_t r = threadIdx.x;
	uint64_t total;
	const uint64_t before = block_scan(r < nrows ? rows[r] : 0, wsum, total);
	if (r < nrows)
		rows[r] = before;
}

// rows[r] of segment s becomes seg[s] + the sum of the segment's rows before r
__global__ void __launch_bounds__(THREADS)
gather_scan_tiles(uint64_t *__restrict__ rows, uint32_t nrows, uint32_t seglen,
		  const uint64_t *__restrict__ seg)
{
	__shared__ uint64_t wsum[WAVES];
	const uint32_t r0 = blockIdx.x * seglen;
	const uint32_t r1 = min(r0 + seglen, nrows);
	uint64_t run = seg[blockIdx.x];
	for (uint32_t c = r0; c < r1; c += THREADS) {
		const uint32_t r = c + threadIdx.x;
		uint64_t total;
		const uint64_t before = block_scan(r < r1 ? rows[r] : 0, wsum, total);
		if (r < r1)
			rows[r] = run + before;
		run += total;
	}
}

// sums[tile] = the bytes of the entries before the tile
__global__ void __launch_bounds__(THREADS)
gather_write_offsets(places f, const uint32_t *__restrict__ index, uint64_t n,
		     const uint64_t *__restrict__ sums, uint64_t *__restrict__ out_offsets)
{
	__shared__ uint64_t wsum[WAVES];
	const uint64_t first = (uint64_t)blockIdx.x * GATHER_TILE + threadIdx.x;
	uint32_t len[ROUNDS];
	lens_of(f, index, n, first, len);
	uint64_t run = sums[blockIdx.x];
#pragma unroll
	for (uint32_t k = 0; k < ROUNDS; k++) {
		uint64_t total;
		const uint64_t before = block_scan(len[k], wsum, total);
		if (first + k * THREADS < n)
			out_offsets[first + k * THREADS] = run + before;
		run += total;
	}
	if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
		out_offsets[n] = run;
}

// ---------------------------------------------------------------- general path: the copy

// Entry e of the tile is list entry j0 + e: `len` bytes from data + src to out + dst, then zeros
// up to the next entry's dst (strided form: the slot's padding; packed: nothing).  Positions are
// kept shifted by a = out mod 16, so that position P lies at base + P with base 16-byte aligned
// and a chunk is 16 positions from a multiple of 16.  The tile owns positions [lo, hi): its
// entries' range, cut at `limit` (the strided form's n * out_stride, the packed form's out_bytes).
template <bool PACKED>
__global__ void __launch_bounds__(THREADS)
gather_copy(const uint8_t *__restrict__ data, places f, const uint32_t *__restrict__ index, uint64_t n,
	    uint32_t out_stride, uint8_t *__restrict__ out, uint64_t limit,
	    const uint64_t *__restrict__ out_offsets)
{
	__shared__ uint64_t s_src[COPY_TILE];
	__shared__ uint64_t s_dst[COPY_TILE + 1];
	__shared__ uint32_t s_len[COPY_TILE];
	const uint32_t tid = threadIdx.x;
	const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15);
	uint8_t *const base = out - a;
	const uint64_t j0 = (uint64_t)blockIdx.x * COPY_TILE;
	const uint32_t cnt = (uint32_t)min((uint64_t)COPY_TILE, n - j0);
	if (tid < cnt) {
		const uint64_t j = j0 + tid;
		uint64_t s;
		uint32_t len;
		span_of(f, index[j], s, len);
		s_src[tid] = s;
		s_len[tid] = PACKED ? len : min(len, out_stride);
		s_dst[tid] = (PACKED ? out_offsets[j] : j * out_stride) + a;
	}
	if (tid == 0)
		s_dst[cnt] = (PACKED ? out_offsets[j0 + cnt] : (j0 + cnt) * out_stride) + a;
	__syncthreads();
	const uint64_t lo = s_dst[0], hi = s_dst[cnt] - a <= limit ? s_dst[cnt] : limit + a;
	if (hi <= lo)
		return;
	// COPY_K chunks a lane and trip, a workgroup's width apart: their searches, then their loads,
	// then their stores, so that a lane has COPY_K loads in flight
	enum : uint32_t { NONE, MOVE, ZERO, PAIR, BYTES };
	const uint64_t c1 = (hi + 15) >> 4;
	for (uint64_t c = (lo >> 4) + tid; c < c1; c += THREADS * COPY_K) {
		uint64_t P[COPY_K];
		uint32_t e[COPY_K], kind[COPY_K], tail[COPY_K];
		u32x4 v[COPY_K], v2[COPY_K];
#pragma unroll
		for (uint32_t k = 0; k < COPY_K; k++) {
			P[k] = (c + k * THREADS) << 4;
			e[k] = 0;
		}
		// e = the last entry that starts at or before the chunk's first position of the tile
#pragma unroll
		for (uint32_t step = COPY_TILE / 2; step != 0; step >>= 1) {
#pragma unroll
			for (uint32_t k = 0; k < COPY_K; k++) {
				const uint32_t t = e[k] + step;
				if (t < cnt && s_dst[t] <= max(P[k], lo))
					e[k] = t;
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < COPY_K; k++) {
			const uint64_t off = P[k] - s_dst[e[k]]; // (meaningful when P >= lo)
			const uint32_t len = s_len[e[k]];
			const bool whole = P[k] >= lo && P[k] + 16 <= hi;
			kind[k] = P[k] >= hi ? NONE
				  : whole && off + 16 <= len ? MOVE
				  : !PACKED && whole && off >= len && P[k] + 16 <= s_dst[e[k] + 1] ? ZERO
												     : BYTES;
			// the end of one packet and the start of the next with no padding between, both
			// of 16 bytes or more: the first's last 16 bytes and the second's first 16 (two
			// loads inside the packets), shifted together
			if (kind[k] == BYTES && whole && off < len && len >= 16 && e[k] + 1 < cnt &&
			    s_dst[e[k]] + len == s_dst[e[k] + 1] && s_len[e[k] + 1] >= 16)
				kind[k] = PAIR;
			v[k] = v2[k] = (u32x4){0, 0, 0, 0};
			tail[k] = len - (uint32_t)off;
			if (kind[k] == MOVE)
				v[k] = load16_any<GATHER_COPY_NT>(data + s_src[e[k]] + off);
			if (kind[k] == PAIR) {
				v[k] = load16_any<GATHER_COPY_NT>(data + s_src[e[k]] + len - 16);
				v2[k] = load16_any<GATHER_COPY_NT>(data + s_src[e[k] + 1]);
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < COPY_K; k++) {
			if (kind[k] == PAIR) { // (tail in 1..15: the chunk is no MOVE and starts inside e)
				const unsigned __int128 first = __builtin_bit_cast(unsigned __int128, v[k]);
				const unsigned __int128 second = __builtin_bit_cast(unsigned __int128, v2[k]);
				v[k] = __builtin_bit_cast(u32x4, (first >> (8 * (16 - tail[k]))) |
								     (second << (8 * tail[k])));
			}
			if (kind[k] == MOVE || kind[k] == ZERO || kind[k] == PAIR)
				store16<GATHER_COPY_NT>(base + P[k], v[k]);
		}
		// a straddling chunk: its bytes' loads first, so that they are in flight together (one
		// after the other, a chunk is 16 trips to memory), then one store when the tile owns
		// the whole chunk, else a store a byte
#pragma unroll
		for (uint32_t k = 0; k < COPY_K; k++) {
			if (kind[k] != BYTES)
				continue;
			uint32_t at = e[k];
			uint32_t got[16];
#pragma unroll
			for (uint32_t b = 0; b < 16; b++) {
				const uint64_t Q = P[k] + b;
				got[b] = 0;
				if (Q < lo || Q >= hi)
					continue;
				while (at + 1 < cnt && s_dst[at + 1] <= Q)
					at++;
				const uint64_t o = Q - s_dst[at];
				if (o < s_len[at])
					got[b] = data[s_src[at] + o];
			}
			if (P[k] >= lo && P[k] + 16 <= hi) {
				u32x4 w;
#pragma unroll
				for (uint32_t i = 0; i < 4; i++)
					w[i] = got[4 * i] | got[4 * i + 1] << 8 | got[4 * i + 2] << 16 |
					       got[4 * i + 3] << 24;
				store16<false>(base + P[k], w);
			} else {
#pragma unroll
				for (uint32_t b = 0; b < 16; b++)
					if (P[k] + b >= lo && P[k] + b < hi)
						base[P[k] + b] = (uint8_t)got[b];
			}
		}
	}
}

inline uint32_t
tiles_of(uint64_t n)
{
	return (uint32_t)((n + GATHER_TILE - 1) / GATHER_TILE);
}

} // namespace

bool
gather_takes_rows(const struct ebpf_pkt_batch &b, uint32_t out_stride, const void *out)
{
	return b.offsets == nullptr && !(b.flags & EBPF_BATCH_EXTENTS) && out_stride != 0 &&
	       b.stride == out_stride && out_stride % 16 == 0 &&
	       (reinterpret_cast<uintptr_t>(b.data) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
}

// tile sums | segment sums (two levels)
size_t
gather_scratch_bytes(uint64_t n, uint32_t out_stride)
{
	if (out_stride != 0)
		return 0;
	const uint32_t ntiles = tiles_of(n);
	return (size_t)(ntiles + (ntiles > GATHER_SEGS ? GATHER_SEGS : 0)) * sizeof(uint64_t);
}

hipError_t
launch_gather(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n, uint32_t out_stride,
	      void *out, uint64_t out_bytes, uint64_t *out_offsets, uint64_t *scratch,
	      hipStream_t stream)
{
	const uint8_t *data = static_cast<const uint8_t *>(b.data);
	uint8_t *o = static_cast<uint8_t *>(out);
	if (gather_takes_rows(b, out_stride, out)) {
		const uint32_t lanes = out_stride / 16;
		const bool pow2 = (lanes & (lanes - 1)) == 0;
		const uint64_t blocks = (n * lanes + THREADS * ROW_K - 1) / (THREADS * ROW_K);
		hipLaunchKernelGGL(pow2 ? gather_rows<true> : gather_rows<false>,
				   dim3((uint32_t)(blocks < (1u << 24) ? blocks : (1u << 24))), dim3(THREADS),
				   0, stream, data, b.count, b.stride, lanes,
				   (uint32_t)__builtin_ctz(lanes), index, n, o);
		return hipGetLastError();
	}
	const places f = places_of(b);
	const uint32_t groups = (uint32_t)((n + COPY_TILE - 1) / COPY_TILE);
	if (out_stride != 0) {
		hipLaunchKernelGGL(gather_copy<false>, dim3(groups), dim3(THREADS), 0, stream, data, f, index,
				   n, out_stride, o, n * out_stride, (const uint64_t *)nullptr);
		return hipGetLastError();
	}
	const uint32_t ntiles = tiles_of(n);
	const bool two = ntiles > GATHER_SEGS;
	uint64_t *sums = scratch;
	uint64_t *seg = sums + ntiles;
	const uint32_t seglen = (ntiles + GATHER_SEGS - 1) / GATHER_SEGS;
	const uint32_t nseg = two ? (ntiles + seglen - 1) / seglen : 0;
	hipLaunchKernelGGL(gather_tile_sums, dim3(ntiles), dim3(THREADS), 0, stream, f, index, n, sums);
	if (two)
		hipLaunchKernelGGL(gather_seg_sum, dim3(nseg), dim3(THREADS), 0, stream, sums, ntiles, seglen,
				   seg);
	hipLaunchKernelGGL(gather_scan_rows, dim3(1), dim3(THREADS), 0, stream, two ? seg : sums,
			   two ? nseg : ntiles);
	if (two)
		hipLaunchKernelGGL(gather_scan_tiles, dim3(nseg), dim3(THREADS), 0, stream, sums, ntiles,
				   seglen, seg);
	hipLaunchKernelGGL(gather_write_offsets, dim3(ntiles), dim3(THREADS), 0, stream, f, index, n, sums,
			   out_offsets);
	hipLaunchKernelGGL(gather_copy<true>, dim3(groups), dim3(THREADS), 0, stream, data, f, index, n, 0u,
			   o, out_bytes, out_offsets);
	return hipGetLastError();
}
