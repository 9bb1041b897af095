// scatter.hip — a dense batch's packets written back into the batch (ebpf_batch_scatter_dev) and
// a second stage's results written into the batch's ret / faults (ebpf_batch_merge_dev).
// DESIGN.md §2 "Scattering a class back".
//
// Three kernels:
//   scatter_rows   gather_rows mirrored: both sides fixed at one stride, a multiple of 16, on
//                  16-byte bases: stride/16 lanes serve a packet, each with one 16-byte load (1 KiB
//                  contiguous per wave instruction) and one 16-byte store into the packet's row
//   scatter_copy   everything else, strided or packed: the copy is owned by the DESTINATION, per
//                  packet.  A workgroup takes COPY_TILE list entries, keeps their (dense start,
//                  length, destination start) in LDS, counts every packet's 16-byte chunks aligned
//                  in memory (the aligned interior, plus a head and a tail piece of 1..15 bytes),
//                  scans the counts over the tile and walks the tile's chunk list, a chunk a lane
//                  and trip; a lane finds its chunk's packet by a search over the scanned counts.
//                  An interior chunk moves 16 bytes (the load at whatever alignment the dense side
//                  has, the store aligned).  A head or tail piece goes byte by byte and never
//                  writes the chunk's other bytes: they belong to a neighbour that another lane
//                  may be writing, or that is not listed at all.  Every byte of a listed packet
//                  has one writer, short packets cost no idle lanes and long ones need no
//                  per-packet loop.
//   merge_rows     a thread per list entry: one 8-byte store into ret, one byte store into faults
// The access forms are those the gather and the general kernels already use: 16-byte loads at any
// alignment, naturally aligned 16-byte stores, byte stores.  No atomics, no waiting on another
// workgroup, no scratch: with distinct listings the result is a function of the input alone.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/batch_places.h"
#include "host/scatter.h"

// The choices measured in DESIGN.md §2 "Scattering a class back", as -D switches for an A/B build
// (tools/scatter_bench.py under EBPF_LIB): nontemporal loads / stores of the row path, nontemporal
// 16-byte moves of the general copy, 16-byte units a lane of scatter_rows loads before its first
// store, list entries a lane of merge_rows loads before its first store.
#ifndef SCATTER_NT_LOAD
#define SCATTER_NT_LOAD 1
#endif
#ifndef SCATTER_NT_STORE
#define SCATTER_NT_STORE 1
#endif
#ifndef SCATTER_COPY_NT
#define SCATTER_COPY_NT 1
#endif
#ifndef SCATTER_ROW_K
#define SCATTER_ROW_K 4
#endif
#ifndef MERGE_K
#define MERGE_K 4
#endif

namespace {

constexpr uint32_t ROW_K = SCATTER_ROW_K;
constexpr uint32_t MRG_K = MERGE_K;
constexpr uint32_t COPY_TILE = 256;   // list entries per workgroup of scatter_copy
static_assert((COPY_TILE & (COPY_TILE - 1)) == 0 && COPY_TILE == THREADS, "copy tile shape");

// ---------------------------------------------------------------- row path

// Unit u = 16 bytes: part u % lanes of list entry u / lanes, at in + 16 u.  A lane takes ROW_K
// units a workgroup's width apart, and issues their index loads, then their dense loads, before
// its first store; a unit past the end re-reads the last one instead, so no index load sits
// behind a branch.  The slot of an index past the batch is not read and nothing is stored for it.
template <bool POW2>
__global__ void __launch_bounds__(THREADS)
scatter_rows(uint8_t *__restrict__ data, uint64_t count, uint32_t stride, uint32_t lanes,
	     uint32_t shift, const uint32_t *__restrict__ index, uint64_t n,
	     const uint8_t *__restrict__ in)
{
	const uint64_t total = n * lanes;
	constexpr uint64_t SPAN = (uint64_t)THREADS * ROW_K;
	for (uint64_t base = blockIdx.x * SPAN + threadIdx.x; base < total + threadIdx.x;
	     base += gridDim.x * SPAN) {
		uint32_t idx[ROW_K], part[ROW_K];
		uint64_t at[ROW_K];
		u32x4 v[ROW_K];
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			const uint64_t u = base + k * THREADS;
			at[k] = u < total ? u : total - 1;
			const uint64_t j = POW2 ? at[k] >> shift : at[k] / lanes;
			part[k] = (uint32_t)(at[k] - j * lanes);
			idx[k] = index[j];
		}
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			v[k] = (u32x4){0, 0, 0, 0};
			if (idx[k] < count)
				v[k] = load16<SCATTER_NT_LOAD>(in + at[k] * 16);
		}
#pragma unroll
		for (uint32_t k = 0; k < ROW_K; k++) {
			if (base + k * THREADS < total && idx[k] < count)
				store16<SCATTER_NT_STORE>(data + (uint64_t)idx[k] * stride + part[k] * 16u,
							  v[k]);
		}
	}
}

// ---------------------------------------------------------------- general path

// Entry e of the tile is list entry j0 + e: its first k bytes go from in + src to data + dst.
// Destinations are kept shifted by a = data mod 16, so that position P lies at base + P with base
// 16-byte aligned and a chunk is 16 positions from a multiple of 16.
template <bool PACKED>
__global__ void __launch_bounds__(THREADS)
scatter_copy(uint8_t *__restrict__ data, places f, const uint32_t *__restrict__ index, uint64_t n,
	     uint32_t in_stride, const uint8_t *__restrict__ in, uint64_t in_bytes,
	     const uint64_t *__restrict__ in_offsets)
{
	__shared__ uint64_t s_src[COPY_TILE];
	__shared__ uint64_t s_dst[COPY_TILE];
	__shared__ uint64_t s_pre[COPY_TILE]; // the chunks of the tile's entries before this one
	__shared__ uint32_t s_k[COPY_TILE];
	__shared__ uint64_t wsum[WAVES];
	const uint32_t tid = threadIdx.x;
	const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(data) & 15);
	uint8_t *const base = data - a;
	const uint64_t j0 = (uint64_t)blockIdx.x * COPY_TILE;
	const uint32_t cnt = (uint32_t)min((uint64_t)COPY_TILE, n - j0);
	uint64_t chunks = 0;
	if (tid < cnt) {
		const uint64_t j = j0 + tid;
		uint64_t s, at, m;
		uint32_t len;
		span_of(f, index[j], s, len);
		if (PACKED) {
			// the slot as an offsets-form batch reads it, cut at in_bytes
			at = in_offsets[j];
			const uint64_t e = in_offsets[j + 1], d = e - at;
			m = (e < at || (d >> 32) != 0) ? 0 : d;
			m = min(m, at < in_bytes ? in_bytes - at : (uint64_t)0);
		} else {
			at = j * in_stride;
			m = in_stride;
		}
		const uint32_t k = (uint32_t)min((uint64_t)len, m);
		const uint64_t D = s + a;
		s_src[tid] = at;
		s_dst[tid] = D;
		s_k[tid] = k;
		chunks = k != 0 ? ((D + k + 15) >> 4) - (D >> 4) : 0;
	}
	uint64_t total;
	s_pre[tid] = block_scan(chunks, wsum, total);
	__syncthreads();
	for (uint64_t c = tid; c < total; c += THREADS) {
		// e = the last entry with no more than c chunks before it: the one chunk c is of (the
		// entries of no chunks before it share its count and come earlier)
		uint32_t e = 0;
#pragma unroll
		for (uint32_t step = COPY_TILE / 2; step != 0; step >>= 1) {
			const uint32_t t = e + step;
			if (t < cnt && s_pre[t] <= c)
				e = t;
		}
		const uint64_t D = s_dst[e];
		const uint64_t P = ((D >> 4) + (c - s_pre[e])) << 4;
		const uint64_t lo = max(P, D), hi = min(P + 16, D + s_k[e]);
		const uint8_t *from = in + s_src[e] + (lo - D);
		const uint32_t cut = (uint32_t)(hi - lo); // 16: an interior chunk; 1..15: a piece
		u32x4 v = (u32x4){0, 0, 0, 0};
		uint8_t got[16];
		if (cut == 16) {
			v = load16_any<SCATTER_COPY_NT>(from);
		} else {
			// a piece: its byte loads first, so that they are in flight together (a byte
			// past the piece re-reads the piece's last one: no load behind a branch)
#pragma unroll
			for (uint32_t b = 0; b < 15; b++)
				got[b] = from[min(b, cut - 1)];
		}
		if (cut == 16) {
			store16<SCATTER_COPY_NT>(base + P, v);
		} else {
#pragma unroll
			for (uint32_t b = 0; b < 15; b++)
				if (b < cut)
					base[lo + b] = got[b];
		}
	}
}

// ---------------------------------------------------------------- merge

// List entry j: ret[index[j]] = ret2[j], faults[index[j]] = faults2[j] (0 without faults2).  A
// lane takes MRG_K entries a workgroup's width apart and issues their loads before its first
// store; an entry past the end re-reads the last one and stores nothing.
__global__ void __launch_bounds__(THREADS)
merge_rows(uint64_t *__restrict__ ret, uint8_t *__restrict__ faults, uint64_t count,
	   const uint32_t *__restrict__ index, uint64_t n, const uint64_t *__restrict__ ret2,
	   const uint8_t *__restrict__ faults2)
{
	constexpr uint64_t SPAN = (uint64_t)THREADS * MRG_K;
	for (uint64_t base = blockIdx.x * SPAN + threadIdx.x; base < n + threadIdx.x;
	     base += gridDim.x * SPAN) {
		uint32_t idx[MRG_K];
		uint64_t r[MRG_K];
		uint8_t fl[MRG_K];
#pragma unroll
		for (uint32_t k = 0; k < MRG_K; k++) {
			const uint64_t j = base + k * THREADS;
			const uint64_t at = j < n ? j : n - 1;
			idx[k] = index[at];
			r[k] = ret2[at];
			fl[k] = faults2 != nullptr ? faults2[at] : (uint8_t)0;
		}
#pragma unroll
		for (uint32_t k = 0; k < MRG_K; k++) {
			if (base + k * THREADS >= n || idx[k] >= count)
				continue;
			ret[idx[k]] = r[k];
			if (faults != nullptr)
				faults[idx[k]] = fl[k];
		}
	}
}

inline uint32_t
grid_of(uint64_t units, uint32_t per_block)
{
	const uint64_t blocks = (units + per_block - 1) / per_block;
	return (uint32_t)(blocks < (1u << 24) ? blocks : (1u << 24));
}

} // namespace

bool
scatter_takes_rows(const struct ebpf_pkt_batch &b, uint32_t in_stride, const void *in)
{
	return b.offsets == nullptr && !(b.flags & EBPF_BATCH_EXTENTS) && in_stride != 0 &&
	       b.stride == in_stride && in_stride % 16 == 0 &&
	       (reinterpret_cast<uintptr_t>(b.data) | reinterpret_cast<uintptr_t>(in)) % 16 == 0;
}

hipError_t
launch_scatter(const struct ebpf_pkt_batch &b, const uint32_t *index, uint64_t n, uint32_t in_stride,
	       const void *in, uint64_t in_bytes, const uint64_t *in_offsets, hipStream_t stream)
{
	uint8_t *data = static_cast<uint8_t *>(const_cast<void *>(b.data));
	const uint8_t *src = static_cast<const uint8_t *>(in);
	if (scatter_takes_rows(b, in_stride, in)) {
		const uint32_t lanes = in_stride / 16;
		const bool pow2 = (lanes & (lanes - 1)) == 0;
		hipLaunchKernelGGL(pow2 ? scatter_rows<true> : scatter_rows<false>,
				   dim3(grid_of(n * lanes, THREADS * ROW_K)), dim3(THREADS), 0, stream, data,
				   b.count, b.stride, lanes, (uint32_t)__builtin_ctz(lanes), index, n, src);
		return hipGetLastError();
	}
	const places f = places_of(b);
	const uint32_t groups = (uint32_t)((n + COPY_TILE - 1) / COPY_TILE);
	if (in_stride != 0)
		hipLaunchKernelGGL(scatter_copy<false>, dim3(groups), dim3(THREADS), 0, stream, data, f, index,
				   n, in_stride, src, in_bytes, (const uint64_t *)nullptr);
	else
		hipLaunchKernelGGL(scatter_copy<true>, dim3(groups), dim3(THREADS), 0, stream, data, f, index,
				   n, 0u, src, in_bytes, in_offsets);
	return hipGetLastError();
}

hipError_t
launch_merge(uint64_t *ret, uint8_t *faults, uint64_t count, const uint32_t *index, uint64_t n,
	     const uint64_t *ret2, const uint8_t *faults2, hipStream_t stream)
{
	hipLaunchKernelGGL(merge_rows, dim3(grid_of(n, THREADS * MRG_K)), dim3(THREADS), 0, stream, ret,
			   faults, count, index, n, ret2, faults2);
	return hipGetLastError();
}
