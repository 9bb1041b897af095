// rollup.hip — the runs of equal key prefix of a keyed sequence reduced (ebpf_batch_rollup_dev):
// per run its prefix, its entries, the sum, minimum, maximum and OR of a bit field of its values,
// and where it begins.  DESIGN.md §2 "Rolling a table up".
//
// A segmented reduction whose segments the keys give: entry p begins a run iff p == 0 or its prefix
// keys[p] >> key_shift differs from its predecessor's, and run r's results go to entry r of the
// outputs.  A workgroup has a tile of STEER_TILE entries.  It loads them THREADS apart, so that a
// wave reads neighbouring entries, and passes them through LDS to the threads that own them: a
// thread 16 consecutive ones (and the one before them, to compare with; the tile's first entry
// looks at the entry before the tile).
//   rollup_tiles  per tile the runs that begin in it, and what is open at its two edges: the
//                 entries before the first that begins a run, and those from the last such on.
//   rollup_carry  one workgroup, two levels (a thread walks a run of tiles): an exclusive scan of
//                 the tiles' counts and a segmented scan of their edges, which leaves with every
//                 tile the run that is open where it begins.  A run that covers whole tiles is
//                 carried through them.  It writes info and starts[C].
//   rollup_place  the same loads and runs again (cheaper than keeping up to 56 bytes an entry in
//                 scratch).  An entry that begins a run is that run's key and start; it also closes
//                 the run before it, whose count and values the thread holds: its own entries, what
//                 a segmented scan over the threads carries in, and for the tile's first such entry
//                 what the carry left.  The last tile closes the last run.  Per output the results
//                 are put into LDS in run order and stored from neighbouring lanes to neighbouring
//                 entries, so that a tile of one-entry runs stores as a tile of one run loads.
// Every output entry is written by one thread, no atomic decides anything and no workgroup waits
// for another: the output is a function of the input alone, for keys in any order.  Every load is
// of a position below N and every store of an entry below out_cap; a run's number is below C by
// construction.  The cost follows cap, not the shape of the runs.
#include <hip/hip_runtime.h>

#include "ebpf_gpu.h"
#include "hip/seg_tile.h"
#include "host/rollup.h"

namespace {

constexpr uint32_t ROW = ROLLUP_ROW_WORDS;
constexpr uint32_t BUF = TILE + TILE / 16; // a tile in LDS: a padded row a thread (slot)
static_assert(BUF > TILE + 1, "the staged results of a tile fit: a run an entry, and the last one");

typedef struct ebpf_batch_rolls rolls;

// the sequence, the prefix and the field of one call
struct roll_args {
	const uint64_t *keys, *vals;
	uint64_t cap;
	const uint64_t *n;
	uint32_t segments, key_shift;
	bit_field f;
};

// A stretch of entries reduced: of the run that begins at `start` if flag, else of the run that
// was open before the stretch began.  (The four values are written out here and not seg_tile.h's
// stats record as reduce.hip has it: as a member it moved rollup_carry<true>'s registers, and a
// line of tools/rollup_bench.py left the parent's spread; profiles/keyed_refactor.)
struct part {
	uint64_t sum, mn, mx, bits;
	uint32_t start, flag;
};

__device__ __forceinline__ part
nothing()
{
	return {0, ~0ull, 0, 0, 0, 0};
}

__device__ __forceinline__ part
begins_at(uint64_t p)
{
	return {0, ~0ull, 0, 0, (uint32_t)p, 1};
}

// a's values, then b's, of one run
__device__ __forceinline__ void
add_stats(part &a, const part &b)
{
	a.sum += b.sum;
	a.mn = b.mn < a.mn ? b.mn : a.mn;
	a.mx = b.mx > a.mx ? b.mx : a.mx;
	a.bits |= b.bits;
}

// The segmented scan's operator: stretch a, then stretch b.  A run that begins in b closes a.
template <bool VALS>
__device__ __forceinline__ part
join(const part &a, const part &b)
{
	if (b.flag)
		return b;
	part r = a;
	if (VALS)
		add_stats(r, b);
	return r;
}

template <bool VALS>
__device__ __forceinline__ part
lane_up(const part &p, uint32_t d)
{
	part r = p;
	r.start = __shfl_up(p.start, d);
	r.flag = __shfl_up(p.flag, d);
	if (VALS) {
		r.sum = __shfl_up((unsigned long long)p.sum, d);
		r.mn = __shfl_up((unsigned long long)p.mn, d);
		r.mx = __shfl_up((unsigned long long)p.mx, d);
		r.bits = __shfl_up((unsigned long long)p.bits, d);
	}
	return r;
}

template <bool VALS>
__device__ __forceinline__ void
store_vals(uint64_t *__restrict__ w, const part &p)
{
	if (VALS) {
		w[0] = p.sum;
		w[1] = p.mn;
		w[2] = p.mx;
		w[3] = p.bits;
	}
}

template <bool VALS>
__device__ __forceinline__ part
load_vals(const uint64_t *__restrict__ w)
{
	part p = nothing();
	if (VALS) {
		p.sum = w[0];
		p.mn = w[1];
		p.mx = w[2];
		p.bits = w[3];
	}
	return p;
}

// A thread's 16 consecutive entries first + tid * 16 + k: their prefixes and value fields; bit k
// of has is set iff the entry exists (is below N), of heads iff it begins a run.
struct owned {
	uint64_t c[PER_THREAD], val[PER_THREAD];
	uint32_t has, heads;
};

// The tile's entries, loaded THREADS apart and handed through buf to their owners.  The tile has
// an entry (first < N); only positions below N are loaded.  Every thread of the workgroup calls
// it; buf is free again after the next barrier.
template <bool VALS>
__device__ __forceinline__ void
load_tile(const roll_args &a, uint64_t N, uint64_t first, uint64_t *buf, owned &r)
{
	const uint32_t tid = threadIdx.x;
	uint64_t x[PER_THREAD], y[PER_THREAD];
	strided_of(a.keys, N, first, x);
	if (VALS)
		strided_of(a.vals, N, first, y);
	// the entry before the thread's: before the tile (thread 0), or its neighbour's last
	uint64_t prev = 0;
	if (tid == 0 && first != 0)
		prev = a.keys[first - 1];
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++)
		buf[slot(k * THREADS + tid)] = x[k];
	__syncthreads();
	if (tid != 0)
		prev = buf[slot(tid * PER_THREAD - 1)];
	prev >>= a.key_shift;
	r.has = r.heads = 0;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t p = first + tid * PER_THREAD + k;
		r.c[k] = buf[slot(tid * PER_THREAD + k)] >> a.key_shift;
		const bool has = p < N;
		const bool head = has && (p == 0 || r.c[k] != prev);
		prev = r.c[k];
		r.has |= (has ? 1u : 0u) << k;
		r.heads |= (head ? 1u : 0u) << k;
	}
	if (VALS) {
		__syncthreads();
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++)
			buf[slot(k * THREADS + tid)] = y[k];
		__syncthreads();
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint64_t v = a.f.of(buf[slot(tid * PER_THREAD + k)]);
			r.val[k] = r.has >> k & 1 ? v : 0;
		}
	}
}

// entry k of the thread joins the stretch (an entry past N adds nothing)
template <bool VALS>
__device__ __forceinline__ void
add_entry(part &a, const owned &r, uint32_t k)
{
	if (VALS && (r.has >> k & 1)) {
		const uint64_t v = r.val[k];
		a.sum += v;
		a.mn = v < a.mn ? v : a.mn;
		a.mx = v > a.mx ? v : a.mx;
		a.bits |= v;
	}
}

// what leaves the thread on its right: its last run, or all its entries if none begins in it
template <bool VALS>
__device__ __forceinline__ part
last_run(const owned &r, uint64_t first)
{
	part mine = nothing();
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (r.heads >> k & 1)
			mine = begins_at(first + threadIdx.x * PER_THREAD + k);
		add_entry<VALS>(mine, r, k);
	}
	return mine;
}

template <bool VALS>
__global__ void __launch_bounds__(THREADS)
rollup_tiles(roll_args a, uint64_t *__restrict__ scratch)
{
	__shared__ uint64_t buf[BUF];
	__shared__ part wtot[WAVES];
	__shared__ uint64_t wsum[WAVES];
	const uint32_t tid = threadIdx.x;
	uint64_t *row = scratch + (size_t)blockIdx.x * ROW;
	const uint64_t N = entries_of(a.cap, a.n, a.segments), first = (uint64_t)blockIdx.x * TILE;
	if (first >= N) { // (the same for every thread)
		if (tid == 0) {
			row[0] = 0;
			store_vals<VALS>(row + 2, nothing());
			row[6] = ROLLUP_NO_RUN;
		}
		return;
	}
	owned r;
	load_tile<VALS>(a, N, first, buf, r);
	part cur = carry_in<WAVES, join<VALS>, lane_up<VALS>>(last_run<VALS>(r, first), nothing(), wtot);
	uint64_t all;
	block_scan(__popc(r.heads), wsum, all);
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		if (r.heads >> k & 1) {
			if (!cur.flag) // the tile's first: what came before it belongs to an earlier tile's run
				store_vals<VALS>(row + 2, cur);
			cur = begins_at(first + tid * PER_THREAD + k);
		}
		add_entry<VALS>(cur, r, k);
	}
	if (tid == THREADS - 1) {
		row[0] = all;
		if (cur.flag) {
			row[6] = cur.start;
			store_vals<VALS>(row + 7, cur);
		} else {
			row[6] = ROLLUP_NO_RUN;
			store_vals<VALS>(row + 2, cur);
		}
	}
}

// What a tile hands to the tiles after it.
template <bool VALS>
__device__ __forceinline__ part
tile_tail(const uint64_t *__restrict__ row)
{
	// (both loaded, then one chosen: no load waits for another; a tile in which no run begins
	// has nothing in 7 .. 10, and what is read there is not used)
	const uint64_t at = row[6];
	const part head = load_vals<VALS>(row + 2), tail = load_vals<VALS>(row + 7);
	const bool begins = at != ROLLUP_NO_RUN;
	part p = begins ? tail : head;
	p.flag = begins ? 1u : 0u;
	p.start = begins ? (uint32_t)at : 0u;
	return p;
}

// One workgroup: a thread walks its run of tiles (run_of) twice, first for its run's count and
// for what the run hands on, then, with what the threads before it hand in, to leave with every
// tile the runs before it and the run that is open where it begins.  C <= cap < 2^32.
template <bool VALS>
__global__ void __launch_bounds__(CARRY_THREADS)
rollup_carry(roll_args a, uint32_t ntiles, uint64_t out_cap, uint64_t *__restrict__ starts,
	     uint64_t *__restrict__ info, uint64_t *__restrict__ scratch)
{
	__shared__ part wtot[CARRY_THREADS / 64];
	__shared__ uint64_t wsum[CARRY_THREADS / 64];
	const auto [t0, t1] = run_of(ntiles);
	uint64_t mine = 0, C;
	part last = nothing();
	for (uint32_t t = t0; t < t1; t++) {
		const uint64_t *row = scratch + (size_t)t * ROW;
		mine += row[0];
		last = join<VALS>(last, tile_tail<VALS>(row));
	}
	uint64_t before = block_scan<CARRY_THREADS / 64>(mine, wsum, C);
	part cur = carry_in<CARRY_THREADS / 64, join<VALS>, lane_up<VALS>>(last, nothing(), wtot);
	for (uint32_t t = t0; t < t1; t++) {
		uint64_t *row = scratch + (size_t)t * ROW;
		row[1] = before;
		before += row[0];
		store_vals<VALS>(row + 11, cur);
		row[15] = cur.start;
		cur = join<VALS>(cur, tile_tail<VALS>(row));
	}
	if (threadIdx.x == 0) {
		const uint64_t N = entries_of(a.cap, a.n, a.segments);
		info[0] = C;
		info[1] = N;
		if (starts != nullptr && C <= out_cap)
			starts[C] = N;
	}
}

// a tile of the placing kernel, the same for every thread but for hb
struct placing {
	uint64_t first, N, base, out_cap; // base: the runs that begin before the tile
	uint32_t hb, slots;               // the entries that begin a run before the thread's, and the tile's
	bool last;                        // the tile holds entry N - 1
};

// One output: the four statistics (seg_tile.h) and the count are of the run that an entry which
// begins a run closes, keys and starts are that entry's own.
enum { COUNT = STATS, KEYS, STARTS };

// One output of the tile, written in run order through sv: the tile's e-th entry that begins a
// run is run base + e, and closes run base + e - 1 (none for the sequence's first entry); the last
// tile's last thread closes the last run, C - 1 = base + slots - 1.  in: the run that is open where
// the thread's entries begin, over the entries before them.  Every thread of the workgroup calls
// it; sv has slots + 1 entries.
template <int STAT>
__device__ __forceinline__ void
stage(uint64_t *__restrict__ dst, const placing &t, const owned &r, const part &in, uint64_t *sv)
{
	if (dst == nullptr) // (the same for every thread)
		return;
	constexpr bool closes = STAT <= COUNT;
	const uint32_t tid = threadIdx.x;
	uint64_t acc = STAT == SUM ? in.sum : STAT == MIN ? in.mn : STAT == MAX ? in.mx : in.bits;
	uint64_t start = in.start;
	uint32_t e = t.hb;
#pragma unroll
	for (uint32_t k = 0; k < PER_THREAD; k++) {
		const uint64_t p = t.first + tid * PER_THREAD + k;
		if (r.heads >> k & 1) {
			sv[e++] = STAT == KEYS ? r.c[k] : STAT == STARTS ? p : STAT == COUNT ? p - start : acc;
			acc = ident<STAT>();
			start = p;
		}
		if (STAT < STATS)
			acc = fold<STAT>(acc, r.has >> k & 1 ? r.val[k] : ident<STAT>());
	}
	if (closes && t.last && tid == THREADS - 1)
		sv[e] = STAT == COUNT ? t.N - start : acc; // (e == slots here)
	__syncthreads();
	const uint32_t m = t.slots + (closes && t.last ? 1u : 0u);
	for (uint32_t i = tid; i < m; i += THREADS) {
		const uint64_t g = t.base + i; // the run that begins here; the one closed is before it
		if (closes ? (g != 0 && g - 1 < t.out_cap) : g < t.out_cap)
			dst[closes ? g - 1 : g] = sv[i];
	}
	__syncthreads();
}

template <bool VALS>
__global__ void __launch_bounds__(THREADS)
rollup_place(roll_args a, uint64_t out_cap, rolls out, const uint64_t *__restrict__ scratch)
{
	__shared__ uint64_t buf[BUF];
	__shared__ part wtot[WAVES];
	__shared__ uint64_t wsum[WAVES];
	const uint64_t *row = scratch + (size_t)blockIdx.x * ROW;
	const uint64_t N = entries_of(a.cap, a.n, a.segments), first = (uint64_t)blockIdx.x * TILE;
	if (first >= N) // (the same for every thread)
		return;
	owned r;
	load_tile<VALS>(a, N, first, buf, r);
	const part cur =
	    carry_in<WAVES, join<VALS>, lane_up<VALS>>(last_run<VALS>(r, first), nothing(), wtot);
	uint64_t all;
	const uint32_t hb = (uint32_t)block_scan(__popc(r.heads), wsum, all);
	// the run that is open where the thread's entries begin: one of the tile's, or the carry's
	part in = cur;
	if (!cur.flag) {
		in = load_vals<VALS>(row + 11);
		in.start = (uint32_t)row[15];
		if (VALS)
			add_stats(in, cur);
	}
	const placing t = {first, N, row[1], out_cap, hb, (uint32_t)all, N - first <= TILE};
	// (buf is free: every thread has its entries in registers, and barriers lie between)
	stage<KEYS>(out.keys, t, r, in, buf);
	stage<STARTS>(out.starts, t, r, in, buf);
	stage<COUNT>(out.count, t, r, in, buf);
	if (VALS) {
		stage<SUM>(out.sum, t, r, in, buf);
		stage<MIN>(out.min, t, r, in, buf);
		stage<MAX>(out.max, t, r, in, buf);
		stage<BITS>(out.bits, t, r, in, buf);
	}
}

} // namespace

size_t
rollup_scratch_bytes(uint64_t cap)
{
	return (size_t)tiles_of(cap) * ROW * sizeof(uint64_t);
}

hipError_t
launch_rollup(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
	      uint32_t flags, uint32_t key_shift, uint32_t val_shift, uint32_t val_bits,
	      uint64_t out_cap, const rolls &out, uint64_t *info, uint64_t *scratch, hipStream_t stream)
{
	const uint32_t ntiles = tiles_of(cap);
	const bool values = wants_values(out);
	const bool wanted = values || out.keys != nullptr || out.count != nullptr || out.starts != nullptr;
	const roll_args a = {keys, values ? vals : nullptr, cap, n, flags & EBPF_ROLLUP_SEGMENTS ? 1u : 0u,
			     key_shift, values ? field_of(val_shift, val_bits) : field_of(0, 64)};
	with_flags([&](auto V) {
		hipLaunchKernelGGL((rollup_tiles<V>), dim3(ntiles), dim3(THREADS), 0, stream, a, scratch);
		hipLaunchKernelGGL((rollup_carry<V>), dim3(1), dim3(CARRY_THREADS), 0, stream, a, ntiles,
				   out_cap, out.starts, info, scratch);
		if (wanted && out_cap != 0) // (nothing is placed in outputs of no entry)
			hipLaunchKernelGGL((rollup_place<V>), dim3(ntiles), dim3(THREADS), 0, stream, a,
					   out_cap, out, scratch);
	}, values);
	return hipGetLastError();
}
