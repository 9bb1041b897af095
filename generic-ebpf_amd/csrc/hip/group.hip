// group.hip — a batch's packets sorted by a key field of ret, stably, and the table of the groups
// of equal keys (ebpf_batch_group_dev).  DESIGN.md §2 "Grouping by key".
//
// A least-significant-digit radix sort.  One pass is steer.hip's stable multisplit with the class
// taken from one digit (at most 8 bits) of the key and a payload that moves: (key, packet index)
//   group_count    one workgroup per tile of STEER_TILE entries: the tile's class counts, a row of
//                  EBPF_HIST_BINS u32 per tile
//   the tile scan  steer.hip's own (launch_tile_scan)
//   group_scatter  re-reads the tile, ranks by ballots over the digit's varying bits (wave_rank.h),
//                  sorts the tile in LDS and writes keys and indices out run by run
// The first pass reads ret / faults in packet order; a later pass reads the pass before it.
// The fault flag does not travel.  The first pass puts faulted packets into class 256, so they
// land at [U, count) in packet order, where they belong; U = starts[256] stays in device memory.
// For a later pass an entry at a position >= U is faulted: class 256 again, and a stable
// multisplit leaves it where it is.  Unfaulted entries are never of class 256, so every pass's
// starts[256] is U.
// The group table is one sweep over the sorted keys of [0, U): a head is a position whose key
// differs from its predecessor's (position 0 is one).  group_heads counts them per tile,
// group_head_scan (one workgroup, two levels: a thread per segment of tiles) turns the counts into
// every tile's first group number and writes info and the closing start, group_table numbers the
// heads by ballots and writes the entries below group_cap.
// As in steer.hip no atomic decides a position: the output is a function of the input alone.
#include <hip/hip_runtime.h>

#include "bit_field.h"
#include "ebpf_gpu.h"
#include "hip/wave_rank.h"
#include "host/group.h"
#include "host/steer.h"

namespace {

using namespace wave_rank;

constexpr uint32_t BINS = EBPF_HIST_BINS;
constexpr uint32_t FAULTED = BINS - 1; // the class of a faulted entry
constexpr uint32_t STARTS_WORDS = 2 * (BINS + 1);
constexpr uint32_t PER_THREAD = STEER_TILE / THREADS;

// What a pass reads: ret / faults and the key field (first pass), or the pass before it.
template <typename K>
struct source {
	const uint64_t *ret;
	const uint8_t *faults;
	bit_field key;
	const K *keys;
	const uint32_t *index;
};

// Keys, packet indices and classes of entries first, first + step, ... (class NONE past the
// batch's end), every load issued before the first is used (load_verdicts).
template <typename K, bool FIRST, bool FAULTS, uint32_t N>
__device__ __forceinline__ void
load_entries(const source<K> &s, uint64_t count, uint64_t unfaulted, uint64_t first, uint32_t step,
	     uint32_t dshift, uint32_t dmask, K (&key)[N], uint32_t (&idx)[N], uint32_t (&cls)[N])
{
	uint32_t f[N];
	if (FIRST) {
		uint64_t r[N];
		load_verdicts<FAULTS>(s.ret, s.faults, count, first, step, r, f);
#pragma unroll
		for (uint32_t k = 0; k < N; k++) {
			key[k] = (K)s.key.of(r[k]);
			idx[k] = (uint32_t)(first + k * step);
		}
	} else {
#pragma unroll
		for (uint32_t k = 0; k < N; k++) {
			const uint64_t i = first + k * step;
			const uint64_t at = i < count ? i : count - 1;
			key[k] = s.keys[at];
			idx[k] = s.index[at];
			f[k] = i >= unfaulted;
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < N; k++) {
		const uint32_t c = f[k] ? FAULTED : (uint32_t)(key[k] >> dshift) & dmask;
		cls[k] = first + k * step < count ? c : NONE;
	}
}

template <typename K, bool FIRST, bool FAULTS>
__global__ void __launch_bounds__(THREADS)
group_count(source<K> s, uint64_t count, const uint64_t *__restrict__ starts, uint32_t dshift,
	    uint32_t dmask, uint32_t *__restrict__ rows)
{
	__shared__ uint32_t h[BINS];
	const uint32_t tid = threadIdx.x;
	for (uint32_t b = tid; b < BINS; b += THREADS)
		h[b] = 0;
	__syncthreads();
	const uint64_t unfaulted = FIRST ? 0 : starts[FAULTED];
	const uint64_t first = (uint64_t)blockIdx.x * STEER_TILE;
	K key[PER_THREAD];
	uint32_t idx[PER_THREAD], cls[PER_THREAD];
	load_entries<K, FIRST, FAULTS>(s, count, unfaulted, first + tid, THREADS, dshift, dmask, key, idx,
				       cls);
	const uint32_t vary = varying_bits(cls);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t m = match_class(cls[k], vary);
		if (m != 0 && below(m) == 0)
			atomicAdd(&h[cls[k]], (uint32_t)__popcll(m));
	}
	__syncthreads();
	uint32_t *row = rows + (size_t)blockIdx.x * BINS;
	for (uint32_t b = tid; b < BINS; b += THREADS)
		row[b] = h[b];
}

// rows / starts / rows_absolute as launch_tile_scan left them.  steer.hip's steer_scatter with a
// payload, and one step more: ranked as there, an entry first goes to its place in the tile's own
// sorted order in LDS (classes ascending, a class's entries in tile order); the tile is then read
// back in that order, so that neighbouring lanes write neighbouring global positions — a class's
// run of the tile at a time, not 64 lines a store.
template <typename K, bool FIRST, bool FAULTS>
__global__ void __launch_bounds__(THREADS)
group_scatter(source<K> s, uint64_t count, uint32_t dshift, uint32_t dmask,
	      const uint32_t *__restrict__ rows, const uint64_t *__restrict__ starts,
	      uint32_t rows_absolute, K *__restrict__ keys_out, uint32_t *__restrict__ index_out)
{
	// pos[w][b]: first the count of class b in wave w's entries, then the next place in the
	// tile's sorted order for an entry of class b from wave w
	__shared__ uint32_t pos[WAVES][BINS];
	__shared__ uint32_t lstart[BINS]; // the tile's entries of the classes below b
	__shared__ uint32_t gbase[BINS];  // place l of the tile, of class b, is position gbase[b] + l
	__shared__ uint32_t wsum[WAVES];
	__shared__ K skey[STEER_TILE];
	__shared__ uint32_t sidx[STEER_TILE];
	static_assert(BINS == THREADS + 1, "a thread per class, and the faulted class");
	const uint32_t tid = threadIdx.x;
	const uint32_t w = tid >> 6, lane = tid & 63;
	for (uint32_t k = tid; k < WAVES * BINS; k += THREADS)
		(&pos[0][0])[k] = 0;
	__syncthreads();
	// (every pass's starts[FAULTED] is U: this pass's own tile scan has rewritten it unchanged)
	const uint64_t unfaulted = FIRST ? 0 : starts[FAULTED];
	const uint64_t tile = (uint64_t)blockIdx.x * STEER_TILE;
	{
		K key[CHUNKS];
		uint32_t idx[CHUNKS];
		// per chunk: class | rank among the chunk's entries of the class << 9 | their number << 16
		uint32_t info[CHUNKS];
		load_entries<K, FIRST, FAULTS>(s, count, unfaulted, tile + w * WAVE_SPAN + lane, 64, dshift,
					       dmask, key, idx, info);
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
		// thread b: the tile's entries of class b, and an exclusive scan of them over the classes
		uint32_t mine = 0;
		for (uint32_t q = 0; q < WAVES; q++)
			mine += pos[q][tid];
		uint32_t inc = mine;
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
		lstart[tid] = before + inc - mine;
		if (tid == THREADS - 1)
			lstart[FAULTED] = before + inc;
		__syncthreads();
		const uint32_t *row = rows + (size_t)blockIdx.x * BINS;
		for (uint32_t b = tid; b < BINS; b += THREADS) {
			uint32_t run = lstart[b];
			gbase[b] = row[b] + (rows_absolute ? 0u : (uint32_t)starts[b]) - run;
			for (uint32_t q = 0; q < WAVES; q++) {
				const uint32_t v = pos[q][b];
				pos[q][b] = run;
				run += v;
			}
		}
		__syncthreads();
		// (volatile: a lane reads the place another lane of its wave advanced a chunk earlier; a
		// wave's LDS operations complete in order)
		volatile uint32_t *next = pos[w];
#pragma unroll
		for (uint32_t k = 0; k < CHUNKS; k++) {
			if (info[k] == NONE)
				continue;
			const uint32_t c = info[k] & ((1u << CLASS_BITS) - 1);
			const uint32_t rank = (info[k] >> CLASS_BITS) & 63, n = info[k] >> 16;
			const uint32_t base = next[c];
			// (always true: the places are sums of counts of these same registers)
			if (base + rank < STEER_TILE) {
				skey[base + rank] = key[k];
				sidx[base + rank] = idx[k];
			}
			if (rank == 0)
				next[c] = base + n;
		}
	}
	__syncthreads();
	const uint32_t filled = (uint32_t)(count - tile < STEER_TILE ? count - tile : STEER_TILE);
	const uint32_t lfaulted = lstart[FAULTED];
#pragma unroll 4
	for (uint32_t l = tid; l < filled; l += THREADS) {
		const K key = skey[l];
		const uint32_t c = l >= lfaulted ? FAULTED : (uint32_t)(key >> dshift) & dmask;
		const uint32_t at = gbase[c] + l;
		// (always true: the positions are sums of this input's own counts; kept so that an
		// input changed under the call cannot write outside)
		if (at < count) {
			keys_out[at] = key;
			index_out[at] = sidx[l];
		}
	}
}

// Is position p of the sorted keys the first of its group?
template <typename K>
__device__ __forceinline__ bool
is_head(const K *__restrict__ keys, uint64_t p, uint64_t unfaulted, K *key)
{
	if (p >= unfaulted)
		return false;
	*key = keys[p];
	return p == 0 || keys[p - 1] != *key;
}

// heads[tile] = the heads among the tile's positions
template <typename K>
__global__ void __launch_bounds__(THREADS)
group_heads(const K *__restrict__ keys, const uint64_t *__restrict__ starts,
	    uint32_t *__restrict__ heads)
{
	__shared__ uint32_t wsum[WAVES];
	const uint32_t tid = threadIdx.x;
	const uint64_t unfaulted = starts[FAULTED];
	const uint64_t first = (uint64_t)blockIdx.x * STEER_TILE + tid;
	uint32_t n = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		K key;
		n += (uint32_t)__popcll(__ballot(is_head(keys, first + k * THREADS, unfaulted, &key)));
	}
	if ((tid & 63) == 0)
		wsum[tid >> 6] = n;
	__syncthreads();
	if (tid == 0) {
		uint32_t sum = 0;
		for (uint32_t q = 0; q < WAVES; q++)
			sum += wsum[q];
		heads[blockIdx.x] = sum;
	}
}

// One workgroup: heads[t] becomes the sum of heads[t'] over t' < t, in two levels: thread s sums
// segment s = tiles [s*seglen, (s+1)*seglen), the sums are scanned across the workgroup, and the
// thread then scans inside its segment.  Then info = {G, U} and, if the table holds G groups, its
// closing start.
__global__ void __launch_bounds__(THREADS)
group_head_scan(uint32_t *__restrict__ heads, uint32_t ntiles, const uint64_t *__restrict__ starts,
		uint64_t group_cap, uint64_t *__restrict__ group_starts, uint64_t *__restrict__ info)
{
	__shared__ uint32_t wsum[WAVES];
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint32_t seglen = (ntiles + THREADS - 1) / THREADS;
	const uint32_t t0 = min(tid * seglen, ntiles), t1 = min(t0 + seglen, ntiles);
	uint32_t sum = 0;
#pragma unroll 16
	for (uint32_t t = t0; t < t1; t++)
		sum += heads[t];
	uint32_t inc = sum; // inclusive scan over the wave
#pragma unroll
	for (uint32_t d = 1; d < 64; d <<= 1) {
		const uint32_t up = __shfl_up(inc, d);
		if (lane >= d)
			inc += up;
	}
	if (lane == 63)
		wsum[w] = inc;
	__syncthreads();
	uint32_t before = 0, all = 0;
	for (uint32_t q = 0; q < WAVES; q++) {
		before += q < w ? wsum[q] : 0;
		all += wsum[q];
	}
	uint32_t run = before + inc - sum;
#pragma unroll 16
	for (uint32_t t = t0; t < t1; t++) {
		const uint32_t v = heads[t];
		heads[t] = run;
		run += v;
	}
	if (tid == 0) {
		const uint64_t unfaulted = starts[FAULTED];
		info[0] = all;
		info[1] = unfaulted;
		if (group_starts != nullptr && all <= group_cap)
			group_starts[all] = unfaulted;
	}
}

// heads[tile] = the groups that begin before the tile.  A head's number is that, plus the heads
// of the tile before it: positions go to threads in steps of THREADS, so in (step, wave, lane)
// order.
template <typename K>
__global__ void __launch_bounds__(THREADS)
group_table(const K *__restrict__ keys, const uint64_t *__restrict__ starts,
	    const uint32_t *__restrict__ heads, uint64_t group_cap, uint64_t *__restrict__ group_keys,
	    uint64_t *__restrict__ group_starts)
{
	__shared__ uint32_t cnt[PER_THREAD * WAVES]; // [step][wave], then their exclusive prefix sums
	static_assert(PER_THREAD * WAVES == 64, "one wave scans the counts");
	const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const uint64_t unfaulted = starts[FAULTED];
	const uint64_t first = (uint64_t)blockIdx.x * STEER_TILE + tid;
	K key[PER_THREAD];
	uint32_t mine = 0, rank[PER_THREAD];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const bool head = is_head(keys, first + k * THREADS, unfaulted, &key[k]);
		const uint64_t m = __ballot(head);
		rank[k] = below(m);
		mine |= head ? 1u << k : 0u;
		if (lane == 0)
			cnt[k * WAVES + w] = (uint32_t)__popcll(m);
	}
	__syncthreads();
	if (w == 0) {
		const uint32_t v = cnt[lane];
		uint32_t inc = v;
#pragma unroll
		for (uint32_t d = 1; d < 64; d <<= 1) {
			const uint32_t up = __shfl_up(inc, d);
			if (lane >= d)
				inc += up;
		}
		cnt[lane] = inc - v;
	}
	__syncthreads();
	const uint64_t base = heads[blockIdx.x];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (!(mine & (1u << k)))
			continue;
		const uint64_t g = base + cnt[k * WAVES + w] + rank[k];
		if (g < group_cap) {
			group_starts[g] = first + k * THREADS;
			if (group_keys != nullptr)
				group_keys[g] = key[k];
		}
	}
}

inline uint32_t
tiles_of(uint64_t count)
{
	return (uint32_t)((count + STEER_TILE - 1) / STEER_TILE);
}

template <typename K>
hipError_t
launch_typed(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t key_shift,
	     uint32_t key_bits, uint32_t *index, uint64_t group_cap, uint64_t *group_keys,
	     uint64_t *group_starts, uint64_t *info, void *tmp, uint32_t *scratch, hipStream_t stream)
{
	const group_plan plan = group_plan_of(key_bits);
	const uint32_t ntiles = tiles_of(count);
	const uint64_t padded = group_padded(count);
	K *keybuf[2] = {static_cast<K *>(tmp), static_cast<K *>(tmp) + padded};
	uint32_t *idxbuf[2] = {index, reinterpret_cast<uint32_t *>(static_cast<K *>(tmp) + 2 * padded)};
	uint64_t *starts = reinterpret_cast<uint64_t *>(scratch);
	uint32_t *rows = scratch + STARTS_WORDS;
	uint32_t *heads = rows + steer_scratch_words(count);
	source<K> s = {ret, faults, field_of(key_shift, key_bits), nullptr, nullptr};
	for (uint32_t p = 0; p < plan.passes; p++) {
		const uint32_t dshift = p * plan.digit_bits;
		const uint32_t dbits = p + 1 < plan.passes ? plan.digit_bits : key_bits - dshift;
		const uint32_t dmask = (1u << dbits) - 1;
		K *keys_out = keybuf[p & 1];
		uint32_t *index_out = idxbuf[(plan.passes - 1 - p) & 1]; // the last pass writes `index`
		if (p == 0 && faults)
			hipLaunchKernelGGL((group_count<K, true, true>), dim3(ntiles), dim3(THREADS), 0, stream,
					   s, count, starts, dshift, dmask, rows);
		else if (p == 0)
			hipLaunchKernelGGL((group_count<K, true, false>), dim3(ntiles), dim3(THREADS), 0, stream,
					   s, count, starts, dshift, dmask, rows);
		else
			hipLaunchKernelGGL((group_count<K, false, false>), dim3(ntiles), dim3(THREADS), 0, stream,
					   s, count, starts, dshift, dmask, rows);
		const uint32_t absolute = launch_tile_scan(rows, ntiles, starts, stream) ? 1u : 0u;
		if (p == 0 && faults)
			hipLaunchKernelGGL((group_scatter<K, true, true>), dim3(ntiles), dim3(THREADS), 0, stream,
					   s, count, dshift, dmask, rows, starts, absolute, keys_out, index_out);
		else if (p == 0)
			hipLaunchKernelGGL((group_scatter<K, true, false>), dim3(ntiles), dim3(THREADS), 0,
					   stream, s, count, dshift, dmask, rows, starts, absolute, keys_out,
					   index_out);
		else
			hipLaunchKernelGGL((group_scatter<K, false, false>), dim3(ntiles), dim3(THREADS), 0,
					   stream, s, count, dshift, dmask, rows, starts, absolute, keys_out,
					   index_out);
		s.keys = keys_out;
		s.index = index_out;
	}
	hipLaunchKernelGGL(group_heads<K>, dim3(ntiles), dim3(THREADS), 0, stream, s.keys, starts, heads);
	hipLaunchKernelGGL(group_head_scan, dim3(1), dim3(THREADS), 0, stream, heads, ntiles, starts,
			   group_cap, group_starts, info);
	if (group_cap != 0)
		hipLaunchKernelGGL(group_table<K>, dim3(ntiles), dim3(THREADS), 0, stream, s.keys, starts,
				   heads, group_cap, group_keys, group_starts);
	return hipGetLastError();
}

} // namespace

// starts | tile rows, segment rows, class totals | head counts
size_t
group_scratch_words(uint64_t count)
{
	return STARTS_WORDS + steer_scratch_words(count) + tiles_of(count);
}

hipError_t
launch_group(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t key_shift,
	     uint32_t key_bits, uint32_t *index, uint64_t group_cap, uint64_t *group_keys,
	     uint64_t *group_starts, uint64_t *info, void *tmp, uint32_t *scratch, hipStream_t stream)
{
	if (group_plan_of(key_bits).key_bytes == 4)
		return launch_typed<uint32_t>(ret, faults, count, key_shift, key_bits, index, group_cap,
					      group_keys, group_starts, info, tmp, scratch, stream);
	return launch_typed<uint64_t>(ret, faults, count, key_shift, key_bits, index, group_cap, group_keys,
				      group_starts, info, tmp, scratch, stream);
}
