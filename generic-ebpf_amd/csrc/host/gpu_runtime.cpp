// gpu_runtime.cpp — the GPU backend behind ebpf_gpu.h.
//
// Replaces the caller-side packet loop around ebpf_prog_run (hot loop #1) with
// device launches.  Per (program, device) it keeps the translated program (translate.cpp) and
// a table of the array maps the program references; per (map, device) a mirror of the map's
// storage that is refreshed before a launch whenever the host copy changed (host writes bump
// ebpf_map::version).  Launches are asynchronous on the caller's stream; nothing here ever
// executes eBPF on the CPU — without a GPU the entry points return ENODEV.
//
// This file: a program's device state and one launch.  The mirrors are map_mirror.cpp, the
// per-stream scratch stream_scratch.cpp, a batch's map writes map_write_log.cpp, the batch entry
// points batch.cpp (runtime.h).
#include <chrono>

#include "runtime.h"

namespace {

// Small array maps are copied into LDS by the assembly kernels at kernel start (value loads
// through a lookup result then read LDS).  Budget: kMapLdsBudget bytes per program.
uint32_t
plan_map_lds(const struct ebpf_map *em, uint32_t *used)
{
	if (em->is_hashtable())
		return ~0u;
	const uint64_t bytes = (uint64_t)em->value_size * em->max_entries;
	if (bytes == 0 || bytes % 4 != 0 || *used + bytes > kMapLdsBudget)
		return ~0u;
	const uint32_t off = kMapLdsBase + *used;
	*used += (uint32_t)((bytes + 15) & ~15ull);
	return off;
}

// The dp_map record of one map (dev_base filled in by the caller).
dp_map
map_record(const struct ebpf_map *em, uint32_t *lds_used)
{
	const map_device_layout l = map_device_layout_of(em);
	dp_map m;
	memset(&m, 0, sizeof(m));
	m.handle = (uint64_t)(uintptr_t)em;
	m.value_size = em->value_size;
	m.max_entries = l.slots;
	m.lds_off = plan_map_lds(em, lds_used);
	m.flags = l.flags;
	return m;
}

thread_local std::string t_err;
thread_local int t_dev = 0;
thread_local hipEvent_t t_time_ev[2] = {nullptr, nullptr}; // ebpf_gpu_time_next_launch
std::atomic<int> g_variant{0};

} // namespace

int
fail(int err, const std::string &msg)
{
	t_err = msg;
	return err;
}

int
hip_fail(hipError_t e, const char *what)
{
	return fail(e == hipErrorOutOfMemory ? ENOMEM : EIO,
		    std::string(what) + ": " + hipGetErrorString(e));
}

int
device_count()
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int
check_device(int device)
{
	if (device < 0 || device >= device_count())
		return fail(ENODEV, "no such GPU device");
	return 0;
}

static int
ensure_translated(struct ebpf_prog *ep)
{
	if (ep->xlated)
		return ep->xlated->error;
	auto x = std::make_unique<dprog_host>();
	const auto t0 = std::chrono::steady_clock::now();
	int err = translate_program(ep, *x);
	x->translate_ms =
	    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (err && x->error == 0)
		x->error = err;
	if (!x->error) {
		x->asm_needs_general = asm_program_needs_general(*x);
		x->asm_stores_last = x->asm_needs_general && asm_program_stores_last(*x);
		x->asm_gstage = asm_program_gstage(*x);
		x->asm_pktv = asm_program_hdrlds(*x);
		x->asm_hdrlds = x->asm_pktv && getenv("EBPF_NOHDRLDS") == nullptr;
		x->asm_keep = x->asm_pktv && getenv("EBPF_NOKEEP") == nullptr;
	}
	ep->xlated = std::move(x);
	if (ep->xlated->error)
		return fail(ep->xlated->error, ep->xlated->error_msg);
	return 0;
}

int
prepare(struct ebpf_prog *ep, int device, dprog_device **out)
{
	if (device < 0 || device >= device_count())
		return fail(ENODEV, "no such GPU device");
	std::lock_guard<std::mutex> g(ep->dlock);
	int err = ensure_translated(ep);
	if (err)
		return err;
	if ((int)ep->dev.size() <= device)
		ep->dev.resize(device + 1);
	auto &dp = ep->dev[device];
	if (dp) {
		*out = dp.get();
		return 0;
	}
	hipError_t e = hipSetDevice(device);
	if (e != hipSuccess)
		return hip_fail(e, "hipSetDevice");
	auto nd = std::make_unique<dprog_device>();
	nd->device = device;
	const std::vector<dp_entry> &entries = ep->xlated->entries;
	e = hipMalloc(&nd->d_entries, entries.size() * sizeof(dp_entry));
	if (e != hipSuccess)
		return hip_fail(e, "hipMalloc(program)");
	e = hipMemcpy(nd->d_entries, entries.data(), entries.size() * sizeof(dp_entry),
		      hipMemcpyHostToDevice);
	if (e != hipSuccess)
		return hip_fail(e, "hipMemcpy(program)");
	nd->nentries = (uint32_t)entries.size();
	for (struct ebpf_map *em : ep->xlated->maps) {
		void *mdev = nullptr;
		err = ensure_map_mirror(em, device, &mdev);
		if (err)
			return err;
		dp_map m = map_record(em, &nd->map_lds_bytes);
		m.dev_base = (uint64_t)(uintptr_t)mdev;
		nd->table.push_back(m);
	}
	// arrays changed only by counter updates: device atomics into their delta areas
	for (size_t k = 0; k < ep->xlated->atomic_maps.size(); k++) {
		dp_map &m = nd->table[ep->xlated->atomic_maps[k]];
		m.flags |= DP_MAP_ATOMIC | (ep->xlated->atomic_width[k] == 8 ? DP_MAP_ATOMIC64 : 0u);
		// an LDS-resident map: its workgroup-local sums too (DP_MAP_LDSDELTA), if they fit
		const uint32_t bytes = m.value_size * m.max_entries;
		const uint32_t at = (nd->map_lds_bytes + 7) & ~7u;
		if (m.lds_off != ~0u && at + bytes <= kMapLdsBudget && kMapLdsBase + at < 0x10000u) {
			m.flags |= DP_MAP_LDSDELTA | (kMapLdsBase + at);
			nd->map_lds_bytes = at + ((bytes + 15) & ~15u);
		}
	}
	if (!nd->table.empty()) {
		e = hipMalloc(&nd->d_maps, nd->table.size() * sizeof(dp_map));
		if (e != hipSuccess)
			return hip_fail(e, "hipMalloc(map table)");
		e = hipMemcpy(nd->d_maps, nd->table.data(), nd->table.size() * sizeof(dp_map),
			      hipMemcpyHostToDevice);
		if (e != hipSuccess)
			return hip_fail(e, "hipMemcpy(map table)");
	}
	nd->nmaps = (uint32_t)nd->table.size();
	if (prog_writes_maps(*ep->xlated)) {
		// map writes: the apply step's view of the table (map_writes.h), winner words for every
		// byte of every map whose records land on the device, the log record size
		// (update records: {u64 packet, u32 map << 20, u32 key, value}; hashtable update records
		// {u64 packet, u32 map << 20, u32 op, key, value}, the key and the value each padded to
		// 8 bytes; value-store records DP_REC_VALUE_BYTES)
		const dprog_host &xl = *ep->xlated;
		std::vector<upd_map> um(nd->table.size());
		uint32_t rmax = 8;
		for (size_t t = 0; t < nd->table.size(); t++) {
			um[t].dev_base = nd->table[t].dev_base;
			um[t].value_size = nd->table[t].value_size;
			um[t].max_entries = nd->table[t].max_entries;
			um[t].win_off = nd->win_words;
			um[t].cls = UPD_NONE;
			um[t].gran = nd->table[t].value_size;
			if (in_list(xl.upd_maps, t)) {
				um[t].cls = UPD_DEVICE;
				// byte winners only where a store into a value may land; a map written only by
				// map_update_elem (whole values) needs one word per key
				if (in_list(xl.vstore_maps, t))
					um[t].gran = 1;
				nd->win_words += (uint64_t)nd->table[t].value_size * nd->table[t].max_entries /
						 um[t].gran;
				rmax = std::max(rmax, (nd->table[t].value_size + 7) & ~7u);
			}
			if (in_list(xl.hupd_maps, t)) {
				um[t].cls = UPD_HOST;
				if (nd->table[t].flags & DP_MAP_HASH)
					rmax = std::max(rmax, dp_hash_key_bytes(dp_hash_key_size(nd->table[t].flags)) +
								  ((nd->table[t].value_size + 7) & ~7u));
				else
					rmax = std::max(rmax, (nd->table[t].value_size + 7) & ~7u);
			}
			for (size_t k = 0; k < xl.atomic_maps.size(); k++)
				if (xl.atomic_maps[k] == t) {
					um[t].cls = UPD_ATOMIC;
					um[t].width = xl.atomic_width[k];
				}
		}
		if (xl.vstore_sites)
			rmax = std::max(rmax, DP_REC_VALUE_BYTES - 16);
		nd->upd_stride = 16 + rmax;
		nd->upd_host = um;
		if ((e = hipMalloc(&nd->d_upd, um.size() * sizeof(upd_map))) != hipSuccess ||
		    (e = hipMemcpy(nd->d_upd, um.data(), um.size() * sizeof(upd_map),
				   hipMemcpyHostToDevice)) != hipSuccess)
			return hip_fail(e, "map-write table");
	}
	dp = std::move(nd);
	*out = dp.get();
	return 0;
}

// Compiled program for `mode`, built on first use.  Returns 0 with dp->jit_fn[mode] set, or
// the build error (E2BIG: too large for the code area — the caller runs the interpreter).
static int
jit_entries(struct ebpf_prog *ep, dprog_device *dp, int mode)
{
	std::lock_guard<std::mutex> g(ep->dlock);
	if (dp->jit_fn[mode])
		return 0;
	if (dp->jit_err[mode])
		return dp->jit_err[mode];
	std::string msg;
	const auto t0 = std::chrono::steady_clock::now();
	int err = asm_jit_build(dp->device, *ep->xlated, mode, dp->table, &dp->jit_mod[mode],
				&dp->jit_fn[mode], mode == 1 ? &dp->jit_fn_wide : nullptr,
				&dp->jit_stride[mode], &msg);
	dp->build_ms[mode] =
	    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (err) {
		dp->jit_err[mode] = err;
		return fail(err, msg);
	}
	return 0;
}

// Lowered assembly entries for `mode`, built on first use.
static int
asm_entries(struct ebpf_prog *ep, dprog_device *dp, int mode)
{
	std::lock_guard<std::mutex> g(ep->dlock);
	if (dp->d_asm[mode])
		return 0;
	if (dp->asm_err[mode])
		return dp->asm_err[mode];
	std::string msg;
	const auto t0 = std::chrono::steady_clock::now();
	int err = asm_build_entries(dp->device, *ep->xlated, mode, dp->table, &dp->d_asm[mode],
				    &dp->asm_stride[mode], &msg);
	dp->build_ms[mode] =
	    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	if (err) {
		dp->asm_err[mode] = err;
		return fail(err, msg);
	}
	return 0;
}

int
launch(struct ebpf_prog *ep, dprog_device *dp, const dp_launch &L0, hipStream_t stream,
       hipEvent_t ev_start, hipEvent_t ev_stop, bool hist_overwrite, upd_plan *plan)
{
	// What runs the batch, decided here once and before anything is built (g_variant: 0 = the
	// compiled program, 1 = the portable HIP interpreter, 2 = the assembly interpreter; an error
	// if a code object cannot be loaded — never a silent fallback)
	enum { COMPILED, ASM_INTERP, HIP_INTERP } path = HIP_INTERP;
	const int variant = g_variant.load();
	// the staged kernel reads its packets with LDS-DMA, 16 bytes a lane: only a 16-byte-aligned
	// base takes it (ebpf_gpu.h ebpf_prog_run_batch_dev); any other runs the general kernel
	const bool aligned = (reinterpret_cast<uintptr_t>(L0.data) & 15) == 0;
	// a program whose stores may touch the packet reads it from memory (the general kernel), unless
	// no packet read can follow such a store (asm_program_stores_last): a storing second stage
	// over a gathered batch
	const bool staged_ok = !ep->xlated->asm_needs_general || ep->xlated->asm_stores_last;
	const int mode = (L0.offsets == nullptr && L0.stride == 64 && aligned && staged_ok) ? 1 : 0;
	int err;
	// an overlay larger than the lanes keep on chip: the portable interpreter, spilled
	const bool spill = ep->xlated->vstore_overlay && ep->xlated->ovl_entries > DP_OVL_MAX;
	if (!spill && variant != 1) {
		// variant 0: the compiled program; a program too large for the code area runs on the
		// assembly interpreter instead (still the device path).  Programs with loops compile
		// too: the code generator keeps facts and liveness only across single-predecessor
		// edges, and a loop head (an entry point, >= 2 predecessors) starts from nothing known
		path = ASM_INTERP;
		if (variant == 0) {
			if ((err = jit_entries(ep, dp, mode)) == 0)
				path = COMPILED;
			else if (err != E2BIG)
				return err;
		}
		if (path == ASM_INTERP && (err = asm_entries(ep, dp, mode)))
			return err;
		// the assembly kernels keep 256 lanes' stack slices in LDS: a program whose slice (stack
		// depth, loop count, value-store overlay) leaves them no room runs on the portable HIP
		// interpreter instead (its stack is per-thread memory)
		if (!asm_lds_fits(mode, dp->map_lds_bytes,
				  path == COMPILED ? dp->jit_stride[mode] : dp->asm_stride[mode]))
			path = HIP_INTERP;
	}
	dp_launch L = L0;
	L.maps = dp->d_maps;
	L.nmaps = dp->nmaps;
	L.nentries = dp->nentries;
	L.start = ep->xlated->start;
	L.vflags = (ep->xlated->vstore_overlay ? DP_VF_OVERLAY : 0u) |
		   (ep->xlated->vstore_sites ? DP_VF_VSTORE : 0u) |
		   (std::min<uint32_t>(ep->xlated->ovl_entries, DP_VF_ENTRIES_MAX) << DP_VF_ENTRIES_SHIFT) |
		   (L0.vflags & DP_VF_EXTENTS) |
		   (ep->xlated->write_cap ? DP_VF_WCAP : 0u);
	launch_order order(ep->xlated->maps);
	if ((err = sync_map_mirrors(ep, dp->device, stream)))
		return err;
	hipError_t e;
	upd_plan own;
	if (prog_writes_maps(*ep->xlated)) {
		if (plan == nullptr && (err = upd_plan_for(ep, dp, L0.count, stream, &own)))
			return err; // (this launch is the whole batch: its own log, applied below)
		upd_plan &P = plan ? *plan : own;
		if (ep->xlated->vstore_sites) // (the slot -> key map of the tables this launch reads)
			for (uint16_t t : ep->xlated->hupd_maps) {
				struct ebpf_map *em = ep->xlated->maps[t];
				if (!em->is_hashtable())
					continue;
				std::lock_guard<std::mutex> g(em->mirror_lock);
				if (P.tables.size() <= t)
					P.tables.resize(t + 1);
				P.tables[t] = em->mirrors[dp->device].image;
			}
		L.upd_log = P.log;
		L.upd_cap = P.cap;
		L.upd_stride = dp->upd_stride;
		L.pkt_base = P.pkt_base;
		L.upd_faulted = P.faulted;
	}
	if (path != HIP_INTERP) {
		void *fn = nullptr;
		if (path == COMPILED) {
			L.prog = nullptr;
			L.stack_stride = dp->jit_stride[mode];
			fn = dp->jit_fn[mode];
		} else {
			L.prog = dp->d_asm[mode];
			L.stack_stride = dp->asm_stride[mode];
		}
		dp->last_exec = fn ? EBPF_EXEC_COMPILED : EBPF_EXEC_INTERPRETER;
		dp->last_layout = mode;
		// the staged kernels' keep mode (compiled and interpreted programs): a program that
		// loads its packet at run-time offsets reads them from the wave's LDS packet buffer
		// (gen_handlers.py h_ldx_pktv), so the next group's DMA waits for the group's end
		if (mode == 1 && ep->xlated->asm_keep)
			L.vflags |= DP_VF_KEEP;
		// general kernels: header staging, and the headers kept in LDS too (DP_PKTLDS_HDRKEEP;
		// when the 16 KB of packet buffers cost no resident workgroup: the VGPRs allow 6 per CU)
		const bool hdrlds = ep->xlated->asm_hdrlds && asm_hdrlds_fits(dp->map_lds_bytes, L.stack_stride);
		L.lds_pkt_base = mode != 0 ? 0 : hdrlds ? (DP_PKTLDS_HDRSTAGE | DP_PKTLDS_HDRKEEP)
						 : ep->xlated->asm_gstage ? DP_PKTLDS_HDRSTAGE : 0;
		unsigned long long *user_hist = L.hist;
		if (L.hist) {
			void *part = nullptr;
			if ((err = rows_acquire(dp->device, stream, &part)))
				return fail(err, "no verdict-partial buffer");
			// faults (bin 256) count into replica 0 of the partials; the kernel's last
			// workgroup moves everything into the caller's histogram (user_hist)
			L.hist_rows = static_cast<uint32_t *>(part);
			L.hist = static_cast<unsigned long long *>(part);
		}
		// workgroups per CU on the staged kernels (asm_runtime.cpp, occupancy): compiled programs
		// that only stream packets run 4 (and are the ones write phasing serves); one that probes
		// hashtables runs 5 (C4H 1.49 -> 1.46 ms against 6, 1.53 at 4, profiles/r05/c4h_occ/).
		// The interpreter (fn == NULL) is bound by its scalar dispatch and wants every wave: C4
		// 1.86 -> 1.42 ms at 6 instead of 4 (profiles/r02/v2occ).  A compiled program with loops
		// runs 5, as a probing one does (C3L 0.2238 -> 0.2160 ms against 6, 0.241 at 4, three
		// runs each, profiles/r06/c3l_occ/; round 4's code had gained from 4 to 6)
		bool hash = false;
		for (const dp_map &m : dp->table)
			hash = hash || (m.flags & DP_MAP_HASH) != 0;
		uint32_t wg_cap = 0;
		if (mode == 1 && fn)
			wg_cap = (hash || ep->xlated->has_loops) ? kProbeWorkgroups : kStreamWorkgroups;
		e = launch_interp_asm(L, stream, dp->device, mode, dp->map_lds_bytes, fn,
				      fn ? dp->jit_fn_wide : nullptr, wg_cap, ev_start, ev_stop, user_hist,
				      hist_overwrite);
	} else {
		L.prog = dp->d_entries;
		dp->last_exec = EBPF_EXEC_HIP;
		dp->last_layout = 0;
		if (hist_overwrite && L.hist &&
		    (e = hipMemsetAsync(L.hist, 0, EBPF_HIST_BINS * sizeof(uint64_t), stream)) !=
			hipSuccess)
			return hip_fail(e, "hipMemsetAsync(hist)");
		if (spill) { // (chunks whose overlays fit 1 GiB)
			const uint64_t per = 16ull * ep->xlated->ovl_entries;
			uint64_t chunk = std::max<uint64_t>(256, ((1ull << 30) / per) & ~255ull);
			chunk = std::min<uint64_t>(chunk, std::max<uint64_t>(L.count, 1));
			uint8_t *buf = nullptr;
			if ((err = ovl_acquire(dp->device, stream, chunk * per, &buf)))
				return fail(err, "spilled overlay");
			L.ovl_cap = ep->xlated->ovl_entries;
			L.ovl_chunk = (uint32_t)chunk;
			L.ovl_spill = buf;
		}
		if (ev_start)
			hipEventRecord(ev_start, stream);
		e = launch_interp_v0(L, stream); // (one kernel per chunk: the histogram is added in-kernel)
		if (ev_stop)
			hipEventRecord(ev_stop, stream);
	}
	if (e != hipSuccess)
		return hip_fail(e, "kernel launch");
	if (prog_writes_maps(*ep->xlated) && plan == nullptr)
		return upd_finish(ep, dp, own, stream);
	return 0;
}

int
validate_batch(const struct ebpf_pkt_batch *b, uint32_t allowed_flags)
{
	if (b == nullptr || (b->data == nullptr && b->count != 0))
		return fail(EINVAL, "batch or batch->data is NULL");
	if (b->flags & ~(allowed_flags | EBPF_BATCH_EXTENTS))
		return fail(EINVAL, "batch->flags: unknown bits");
	if ((b->flags & EBPF_BATCH_EXTENTS) && b->offsets == nullptr && b->count != 0)
		return fail(EINVAL, "extents batch without offsets");
	if (b->offsets == nullptr && b->stride == 0 && b->count != 0)
		return fail(EINVAL, "fixed-stride batch with stride 0");
	return 0;
}

int
prog_ensure_translated(struct ebpf_prog *ep)
{
	std::lock_guard<std::mutex> g(ep->dlock);
	return ensure_translated(ep);
}

void
set_last_error(const std::string &msg)
{
	t_err = msg;
}

device_guard::device_guard()
{
	if (hipGetDevice(&prev) != hipSuccess)
		prev = -1;
}

device_guard::~device_guard()
{
	int now = -1;
	if (prev >= 0 && (hipGetDevice(&now) != hipSuccess || now != prev))
		hipSetDevice(prev);
}

void
prog_release_device_state(struct ebpf_prog *ep)
{
	device_guard dg;
	for (auto &dp : ep->dev) {
		if (!dp)
			continue;
		if (hipSetDevice(dp->device) == hipSuccess) {
			if (dp->d_entries)
				hipFree(dp->d_entries);
			if (dp->d_maps)
				hipFree(dp->d_maps);
			if (dp->d_upd)
				hipFree(dp->d_upd);
			for (auto *a : dp->d_asm)
				if (a)
					hipFree(a);
			for (auto *m : dp->jit_mod)
				asm_jit_release(m);
		}
	}
	ep->dev.clear();
}

EBPF_EXPORT int
ebpf_gpu_device_count(void)
{
	return device_count();
}

EBPF_EXPORT int
ebpf_dev_init(int ndev)
{
	const int n = device_count();
	if (n <= 0)
		return fail(ENODEV, "no GPU visible");
	if (ndev <= 0)
		ndev = n;
	if (ndev > n)
		return fail(ENODEV, "ebpf_dev_init: more devices asked for than visible");
	device_guard dg;
	for (int d = 0; d < ndev; d++)
		if (!asm_available(d))
			return fail(EIO, "device " + std::to_string(d) + ": the kernels' code object did not load");
	return 0;
}

EBPF_EXPORT int
ebpf_gpu_set_device(int device)
{
	if (device < 0 || device >= device_count())
		return fail(ENODEV, "no such GPU device");
	t_dev = device;
	return 0;
}

int
current_device()
{
	return t_dev;
}

EBPF_EXPORT int
ebpf_gpu_time_next_launch(void *start_event, void *stop_event)
{
	if ((start_event == nullptr) != (stop_event == nullptr))
		return fail(EINVAL, "start_event and stop_event must both be set or both be NULL");
	t_time_ev[0] = static_cast<hipEvent_t>(start_event);
	t_time_ev[1] = static_cast<hipEvent_t>(stop_event);
	return 0;
}

void
take_time_events(hipEvent_t *start, hipEvent_t *stop)
{
	*start = t_time_ev[0];
	*stop = t_time_ev[1];
	t_time_ev[0] = t_time_ev[1] = nullptr;
}

EBPF_EXPORT int
ebpf_gpu_set_variant(int variant)
{
	if (variant < 0 || variant > 2)
		return fail(EINVAL, "variant must be 0 (compiled), 1 (portable HIP) or 2 (interpreter)");
	g_variant.store(variant);
	return 0;
}

EBPF_EXPORT const char *
ebpf_gpu_last_error(void)
{
	return t_err.c_str();
}

EBPF_EXPORT int
ebpf_prog_prepare_device(struct ebpf_prog *ep, int device)
{
	if (ep == nullptr)
		return fail(EINVAL, "prog is NULL");
	device_guard dg;
	dprog_device *dp;
	return prepare(ep, device, &dp);
}

EBPF_EXPORT int
ebpf_prog_set_semantics(struct ebpf_prog *ep, int semantics)
{
	if (ep == nullptr || (semantics != EBPF_SEM_REFERENCE && semantics != EBPF_SEM_STANDARD))
		return fail(EINVAL, "bad argument");
	std::lock_guard<std::mutex> g(ep->dlock);
	if (ep->xlated && ep->semantics.load() != semantics)
		return fail(EBUSY, "the program was already translated with other semantics");
	ep->semantics.store(semantics);
	return 0;
}

EBPF_EXPORT int
ebpf_prog_device_info(struct ebpf_prog *ep, struct ebpf_dprog_info *info)
{
	if (ep == nullptr || info == nullptr)
		return fail(EINVAL, "NULL argument");
	std::lock_guard<std::mutex> g(ep->dlock);
	int err = ensure_translated(ep);
	if (err)
		return err;
	info->nslots = ep->prog_len / 8;
	info->nentries = (uint32_t)ep->xlated->entries.size();
	info->nmaps = (uint32_t)ep->xlated->maps.size();
	info->max_stack = ep->xlated->max_stack;
	return 0;
}

EBPF_EXPORT int
ebpf_prog_device_exec(struct ebpf_prog *ep, int device, struct ebpf_dexec_info *info)
{
	if (ep == nullptr || info == nullptr)
		return fail(EINVAL, "NULL argument");
	std::lock_guard<std::mutex> g(ep->dlock);
	memset(info, 0, sizeof(*info));
	info->exec = -1;
	info->layout = -1;
	if (ep->xlated)
		info->translate_ms = ep->xlated->translate_ms;
	if (device < 0 || device >= (int)ep->dev.size() || !ep->dev[device])
		return 0;
	const dprog_device &dp = *ep->dev[device];
	info->exec = dp.last_exec;
	info->layout = dp.last_layout;
	if (dp.last_layout >= 0 && dp.last_exec != EBPF_EXEC_HIP)
		info->build_ms = dp.build_ms[dp.last_layout];
	return 0;
}

EBPF_EXPORT int
ebpf_prog_device_code(struct ebpf_prog *ep, int layout, void *buf, size_t *len)
{
	if (ep == nullptr || len == nullptr || layout < 0 || layout > 1)
		return fail(EINVAL, "bad argument");
	std::lock_guard<std::mutex> g(ep->dlock);
	int err = ensure_translated(ep);
	if (err)
		return err;
	// host-side map table: device bases are unknown without a device (0 here; the real table
	// differs only in those immediates)
	std::vector<dp_map> table;
	uint32_t used = 0;
	for (struct ebpf_map *em : ep->xlated->maps)
		table.push_back(map_record(em, &used));
	std::vector<unsigned char> img, code;
	uint32_t stride = 0;
	std::string msg;
	err = asm_jit_emit(*ep->xlated, layout, table, &img, &code, &stride, &msg);
	if (err)
		return fail(err, msg);
	const size_t cap = *len;
	*len = code.size();
	if (buf == nullptr || cap < code.size())
		return buf == nullptr ? 0 : fail(ENOSPC, "buffer too small");
	memcpy(buf, code.data(), code.size());
	return 0;
}

