// batch.cpp — the batch entry points of ebpf_gpu.h: device-resident batches, host-buffer batches
// (chunked through a pool of staging sets), and their multi-device forms.
#include <chrono>
#include <thread>

#include "hist_ops.h"
#include "runtime.h"

namespace {

// Staging buffers of the host-buffer entry points: per device, a pool of sets (two streams, two
// chunk buffers, a histogram), one set per call in flight on that device, reused across calls.
struct staging {
	int device = -1;
	hipStream_t stream[2] = {nullptr, nullptr};
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	hipEvent_t ev_plan = nullptr; // map-writing programs: the log's set-up on stream 0 (stream 1 waits)
	void *d_data[2] = {nullptr, nullptr};
	size_t data_cap[2] = {0, 0};
	void *d_small[2] = {nullptr, nullptr}; // ret | faults | offsets, per chunk
	size_t small_cap[2] = {0, 0};
	unsigned long long *d_hist = nullptr;
};
std::mutex g_stage_lock;
std::vector<std::vector<staging *>> g_stage_free; // per device

int
staging_acquire(int device, staging **out)
{
	{
		std::lock_guard<std::mutex> g(g_stage_lock);
		if ((int)g_stage_free.size() <= device)
			g_stage_free.resize(device + 1);
		if (!g_stage_free[device].empty()) {
			*out = g_stage_free[device].back();
			g_stage_free[device].pop_back();
			return 0;
		}
	}
	auto S = std::make_unique<staging>();
	S->device = device;
	hipError_t e = hipSetDevice(device);
	for (int i = 0; i < 2 && e == hipSuccess; i++)
		e = hipStreamCreateWithFlags(&S->stream[i], hipStreamNonBlocking);
	for (int i = 0; i < 4 && e == hipSuccess; i++)
		e = hipEventCreate(&S->ev[i]);
	if (e == hipSuccess)
		e = hipEventCreateWithFlags(&S->ev_plan, hipEventDisableTiming);
	if (e == hipSuccess)
		e = hipMalloc(&S->d_hist, EBPF_HIST_BINS * sizeof(unsigned long long));
	if (e != hipSuccess)
		return hip_fail(e, "staging set-up"); // (a set that failed half way is not pooled)
	*out = S.release();
	return 0;
}

void
staging_release(staging *S)
{
	std::lock_guard<std::mutex> g(g_stage_lock);
	g_stage_free[S->device].push_back(S);
}

int
stage_alloc(void **p, size_t *cap, size_t need)
{
	if (*cap >= need)
		return 0;
	if (*p)
		hipFree(*p);
	*p = nullptr;
	*cap = 0;
	hipError_t e = hipMalloc(p, need);
	if (e != hipSuccess)
		return hip_fail(e, "hipMalloc(staging)");
	*cap = need;
	return 0;
}

// One device-resident batch (ebpf_prog_run_batch_dev); with `keep` (a shard of a multi-device
// batch of a map-writing program) its writes stay in their log, described by *keep (keep->cap
// stays 0 for a program without writes), for the host-side merge instead of being applied on
// the device.
int
batch_dev(struct ebpf_prog *ep, int device, const struct ebpf_pkt_batch *batch, uint64_t *ret_dev,
	  uint8_t *faults_dev, uint64_t *hist_dev, void *stream, upd_plan *keep)
{
	// the measurement hook is consumed by this call, whatever it returns
	hipEvent_t ev_start, ev_stop;
	take_time_events(&ev_start, &ev_stop);
	if (ep == nullptr || ret_dev == nullptr)
		return fail(EINVAL, "prog or ret is NULL");
	int err = validate_batch(batch, EBPF_BATCH_HIST_OVERWRITE);
	if (err)
		return err;
	const bool overwrite = (batch->flags & EBPF_BATCH_HIST_OVERWRITE) != 0;
	device_guard dg;
	dprog_device *dp;
	err = prepare(ep, device, &dp);
	if (err)
		return err;
	if (batch->count == 0) {
		if (ev_start) { // no kernel: an empty interval
			hipEventRecord(ev_start, static_cast<hipStream_t>(stream));
			hipEventRecord(ev_stop, static_cast<hipStream_t>(stream));
		}
		if (overwrite && hist_dev) {
			hipError_t e = hipMemsetAsync(hist_dev, 0, EBPF_HIST_BINS * sizeof(uint64_t),
						      static_cast<hipStream_t>(stream));
			if (e != hipSuccess)
				return hip_fail(e, "hipMemsetAsync(hist)");
		}
		return 0;
	}
	hipError_t e = hipSetDevice(device);
	if (e != hipSuccess)
		return hip_fail(e, "hipSetDevice");
	dp_launch L;
	memset(&L, 0, sizeof(L));
	L.data = (uint8_t *)batch->data;
	L.offsets = batch->offsets;
	L.off_base = 0;
	L.vflags = (batch->flags & EBPF_BATCH_EXTENTS) ? DP_VF_EXTENTS : 0;
	L.ret = ret_dev;
	L.faults = faults_dev;
	L.hist = reinterpret_cast<unsigned long long *>(hist_dev);
	L.count = batch->count;
	L.stride = batch->stride;
	hipStream_t st = static_cast<hipStream_t>(stream);
	if (keep && prog_writes_maps(*ep->xlated)) {
		if ((err = sync_map_mirrors(ep, device, st)) ||
		    (err = upd_plan_for(ep, dp, batch->count, st, keep)))
			return err;
		return launch(ep, dp, L, st, ev_start, ev_stop, overwrite, keep);
	}
	return launch(ep, dp, L, st, ev_start, ev_stop, overwrite);
}

} // namespace

EBPF_EXPORT int
ebpf_prog_run_batch_dev(struct ebpf_prog *ep, int device, const struct ebpf_pkt_batch *batch,
			uint64_t *ret_dev, uint8_t *faults_dev, uint64_t *hist_dev, void *stream)
{
	return batch_dev(ep, device, batch, ret_dev, faults_dev, hist_dev, stream, nullptr);
}

namespace {

// Packets [lo, hi) of a host-buffer batch on `device` with staging set S: chunked,
// double-buffered H2D -> kernel -> D2H on S's two streams.  Results go to ret[lo..hi) (and
// faults[lo..hi)); the shard's verdict histogram is left in S.d_hist (zeroed first) and the
// interpreter kernels' device time is added to *kernel_ms.  Synchronous.
int
run_host_shard(struct ebpf_prog *ep, dprog_device *dp, staging &S,
	       const struct ebpf_pkt_batch *batch, uint64_t lo, uint64_t hi, uint64_t *ret,
	       uint8_t *faults, double *kernel_ms, host_log *log_out = nullptr)
{
	hipError_t e = hipSetDevice(S.device);
	if (e != hipSuccess)
		return hip_fail(e, "hipSetDevice");
	const bool copy_back = ep->xlated->writes_memory;
	// Chunked, double-buffered: chunk k's H2D overlaps chunk k-1's kernel and D2H.
	const uint64_t chunk = batch->offsets ? (1ull << 20) : (1ull << 22);
	const bool ext = (batch->flags & EBPF_BATCH_EXTENTS) != 0;
	if ((e = hipMemsetAsync(S.d_hist, 0, EBPF_HIST_BINS * sizeof(unsigned long long),
				S.stream[0])) != hipSuccess ||
	    (e = hipStreamSynchronize(S.stream[0])) != hipSuccess)
		return hip_fail(e, "hipMemsetAsync(hist)");
	int err;
	// a map-writing program: one log for the whole shard, applied after its last chunk (every
	// chunk reads the maps as they were when the batch started)
	upd_plan plan;
	if (prog_writes_maps(*ep->xlated)) {
		// the log is set up on stream 0; the odd chunks run on stream 1 and log into it too
		if ((err = upd_plan_for(ep, dp, hi - lo, S.stream[0], &plan)))
			return err;
		if ((e = hipEventRecord(S.ev_plan, S.stream[0])) != hipSuccess ||
		    (e = hipStreamWaitEvent(S.stream[1], S.ev_plan, 0)) != hipSuccess)
			return hip_fail(e, "map-write log set-up");
	}
	bool timed[2] = {false, false};
	// on any error: drain both streams (buffers stay valid for the copies in flight)
	auto drain = [&](int rc) {
		hipStreamSynchronize(S.stream[0]);
		hipStreamSynchronize(S.stream[1]);
		return rc;
	};
	auto collect = [&](int b) -> hipError_t {
		if (!timed[b])
			return hipSuccess;
		float ms = 0;
		hipError_t te = hipEventElapsedTime(&ms, S.ev[2 * b], S.ev[2 * b + 1]);
		*kernel_ms += ms;
		timed[b] = false;
		return te;
	};
	for (uint64_t c0 = lo, k = 0; c0 < hi; c0 += chunk, k++) {
		const int b = (int)(k & 1);
		hipStream_t st = S.stream[b];
		const uint64_t cn = (hi - c0 < chunk) ? hi - c0 : chunk;
		uint64_t byte0, byte1;
		if (ext) { // the bytes the chunk's packets span (in any order, gaps included)
			byte0 = UINT64_MAX;
			byte1 = 0;
			for (uint64_t i = c0; i < c0 + cn; i++) {
				byte0 = std::min(byte0, batch->offsets[2 * i]);
				byte1 = std::max(byte1, batch->offsets[2 * i + 1]);
			}
			if (byte1 < byte0)
				byte0 = byte1;
		} else if (batch->offsets) {
			byte0 = batch->offsets[c0];
			byte1 = batch->offsets[c0 + cn];
		} else {
			byte0 = c0 * batch->stride;
			byte1 = (c0 + cn) * batch->stride;
		}
		// buffers of chunk k-2 are free again
		if ((e = hipStreamSynchronize(st)) != hipSuccess || (e = collect(b)) != hipSuccess)
			return drain(hip_fail(e, "batch chunk"));
		if ((err = stage_alloc(&S.d_data[b], &S.data_cap[b], byte1 - byte0 + 16)))
			return drain(err);
		const uint64_t noffs = ext ? 2 * cn : cn + 1;
		const size_t small = cn * 9 + (batch->offsets ? noffs * 8 : 0) + 64;
		if ((err = stage_alloc(&S.d_small[b], &S.small_cap[b], small)))
			return drain(err);
		uint8_t *sm = static_cast<uint8_t *>(S.d_small[b]);
		uint64_t *d_ret = reinterpret_cast<uint64_t *>(sm);
		uint64_t *d_offs = batch->offsets ? reinterpret_cast<uint64_t *>(sm + cn * 8) : nullptr;
		uint8_t *d_faults = sm + cn * 8 + (batch->offsets ? noffs * 8 : 0);
		const uint8_t *src = static_cast<const uint8_t *>(batch->data) + byte0;
		if ((e = hipMemcpyAsync(S.d_data[b], src, byte1 - byte0, hipMemcpyHostToDevice, st)) !=
		    hipSuccess)
			return drain(hip_fail(e, "hipMemcpyAsync(packets H2D)"));
		if (d_offs && (e = hipMemcpyAsync(d_offs, batch->offsets + (ext ? 2 * c0 : c0), noffs * 8,
						  hipMemcpyHostToDevice, st)) != hipSuccess)
			return drain(hip_fail(e, "hipMemcpyAsync(offsets H2D)"));
		dp_launch L;
		memset(&L, 0, sizeof(L));
		L.data = static_cast<uint8_t *>(S.d_data[b]);
		L.offsets = d_offs;
		L.off_base = byte0;
		L.vflags = ext ? DP_VF_EXTENTS : 0;
		L.ret = d_ret;
		L.faults = d_faults;
		L.hist = S.d_hist;
		L.count = cn;
		L.stride = batch->stride;
		if ((e = hipEventRecord(S.ev[2 * b], st)) != hipSuccess)
			return drain(hip_fail(e, "hipEventRecord"));
		plan.pkt_base = c0 - lo; // (the shard's own packet index: its bitmap starts at lo)
		if ((err = launch(ep, dp, L, st, nullptr, nullptr, false, &plan)))
			return drain(err);
		if ((e = hipEventRecord(S.ev[2 * b + 1], st)) != hipSuccess)
			return drain(hip_fail(e, "hipEventRecord"));
		timed[b] = true;
		if ((e = hipMemcpyAsync(ret + c0, d_ret, cn * 8, hipMemcpyDeviceToHost, st)) != hipSuccess)
			return drain(hip_fail(e, "hipMemcpyAsync(results D2H)"));
		if (faults && (e = hipMemcpyAsync(faults + c0, d_faults, cn, hipMemcpyDeviceToHost, st)) !=
				  hipSuccess)
			return drain(hip_fail(e, "hipMemcpyAsync(faults D2H)"));
		if (copy_back && (e = hipMemcpyAsync(const_cast<uint8_t *>(src), S.d_data[b],
						     byte1 - byte0, hipMemcpyDeviceToHost, st)) !=
				     hipSuccess)
			return drain(hip_fail(e, "hipMemcpyAsync(packets D2H)"));
	}
	for (int i = 0; i < 2; i++) {
		if ((e = hipStreamSynchronize(S.stream[i])) != hipSuccess || (e = collect(i)) != hipSuccess)
			return drain(hip_fail(e, "batch"));
	}
	if (prog_writes_maps(*ep->xlated) && hi > lo) {
		if (log_out) { // (several shards: the caller merges the logs; no offer kernel runs)
			if ((err = upd_fetch(dp, plan, S.stream[0], lo, log_out)) == 0)
				upd_settled(plan.owner);
			return err;
		}
		if ((err = upd_finish(ep, dp, plan, S.stream[0])))
			return drain(err);
		if ((e = hipStreamSynchronize(S.stream[0])) != hipSuccess)
			return hip_fail(e, "map writes");
	}
	return 0;
}

int
fill_stats(struct ebpf_batch_stats *stats, uint64_t n, const unsigned long long *h, double kernel_ms,
	   std::chrono::steady_clock::time_point t0)
{
	stats->packets = n;
	stats->faulted = h[256];
	for (int i = 0; i < EBPF_HIST_BINS; i++)
		stats->hist[i] = h[i];
	stats->kernel_ms = kernel_ms;
	stats->total_ms =
	    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
	return 0;
}

int
check_devices(int ndev, const int *devices, bool distinct)
{
	if (ndev < 1 || devices == nullptr)
		return fail(EINVAL, "ndev < 1 or devices is NULL");
	const int have = device_count();
	for (int d = 0; d < ndev; d++) {
		if (devices[d] < 0 || devices[d] >= have)
			return fail(ENODEV, "no such GPU device");
		for (int d2 = 0; distinct && d2 < d; d2++)
			if (devices[d2] == devices[d])
				return fail(EINVAL, "a device appears twice in the list");
	}
	return 0;
}

std::mutex g_multi_lock; // ebpf_prog_run_batch_multi_dev's enqueue (its scratch is per stream)

} // namespace

EBPF_EXPORT int
ebpf_prog_run_batch(struct ebpf_prog *ep, const struct ebpf_pkt_batch *batch, uint64_t *ret,
		    uint8_t *faults, struct ebpf_batch_stats *stats)
{
	if (ep == nullptr || ret == nullptr)
		return fail(EINVAL, "prog or ret is NULL");
	int err = validate_batch(batch);
	if (err)
		return err;
	auto t0 = std::chrono::steady_clock::now();
	const int device = current_device();
	device_guard dg;
	dprog_device *dp;
	if ((err = prepare(ep, device, &dp)))
		return err;
	staging *S;
	if ((err = staging_acquire(device, &S)))
		return err;
	double kernel_ms = 0;
	err = run_host_shard(ep, dp, *S, batch, 0, batch->count, ret, faults, &kernel_ms);
	unsigned long long h[EBPF_HIST_BINS];
	hipError_t e;
	if (!err && stats &&
	    (e = hipMemcpy(h, S->d_hist, sizeof(h), hipMemcpyDeviceToHost)) != hipSuccess)
		err = hip_fail(e, "hipMemcpy(hist)");
	staging_release(S);
	if (!err && stats)
		fill_stats(stats, batch->count, h, kernel_ms, t0);
	return err;
}

EBPF_EXPORT int
ebpf_prog_run_batch_multi(struct ebpf_prog *ep, int ndev, const int *devices,
			  const struct ebpf_pkt_batch *batch, uint64_t *ret, uint8_t *faults,
			  struct ebpf_batch_stats *stats)
{
	if (ep == nullptr || ret == nullptr)
		return fail(EINVAL, "prog or ret is NULL");
	int err = validate_batch(batch);
	if (err || (err = check_devices(ndev, devices, false)))
		return err;
	auto t0 = std::chrono::steady_clock::now();
	device_guard dg;
	// a map-writing program: each shard's writes stay in its log, merged and applied on the host
	// in global packet order after every shard is done
	const bool merge = ndev > 1 && prog_ensure_translated(ep) == 0 && prog_writes_maps(*ep->xlated);
	std::vector<host_log> logs(merge ? ndev : 0);
	std::vector<dprog_device *> dps(ndev);
	std::vector<staging *> S(ndev, nullptr);
	for (int d = 0; d < ndev && !err; d++)
		if (!(err = prepare(ep, devices[d], &dps[d])))
			err = staging_acquire(devices[d], &S[d]);
	std::vector<int> rc(ndev, 0);
	std::vector<std::string> msg(ndev);
	std::vector<double> kms(ndev, 0.0);
	std::vector<unsigned long long> h((size_t)ndev * EBPF_HIST_BINS, 0);
	if (!err) {
		// one host thread per shard: contiguous shards [d*n/N, (d+1)*n/N) (shard.shard_bounds)
		std::vector<std::thread> th;
		const uint64_t n = batch->count, base = n / ndev, extra = n % ndev;
		for (int d = 0; d < ndev; d++) {
			const uint64_t lo = d * base + std::min<uint64_t>(d, extra);
			const uint64_t hi = lo + base + ((uint64_t)d < extra ? 1 : 0);
			th.emplace_back([&, d, lo, hi] {
				rc[d] = run_host_shard(ep, dps[d], *S[d], batch, lo, hi, ret, faults, &kms[d],
						       merge ? &logs[d] : nullptr);
				hipError_t e;
				if (!rc[d] && (e = hipMemcpy(&h[(size_t)d * EBPF_HIST_BINS], S[d]->d_hist,
							     EBPF_HIST_BINS * 8, hipMemcpyDeviceToHost)) !=
						  hipSuccess)
					rc[d] = hip_fail(e, "hipMemcpy(hist)");
				msg[d] = ebpf_gpu_last_error();
			});
		}
		for (auto &t : th)
			t.join();
		for (int d = 0; d < ndev && !err; d++)
			if ((err = rc[d]))
				fail(err, msg[d]);
	}
	for (staging *s : S)
		if (s)
			staging_release(s);
	if (!err && merge && !(err = delta_merge_host(ep, ndev, devices)))
		err = upd_apply_host(ep, logs, true);
	if (err || !stats)
		return err;
	// the results came back over PCIe anyway: the per-shard histograms are summed here
	unsigned long long sum[EBPF_HIST_BINS] = {0};
	double kmax = 0;
	for (int d = 0; d < ndev; d++) {
		for (int i = 0; i < EBPF_HIST_BINS; i++)
			sum[i] += h[(size_t)d * EBPF_HIST_BINS + i];
		kmax = std::max(kmax, kms[d]);
	}
	return fill_stats(stats, batch->count, sum, kmax, t0);
}

EBPF_EXPORT int
ebpf_prog_run_batch_multi_dev(struct ebpf_prog *ep, int ndev, const int *devices,
			      const struct ebpf_pkt_batch *shards, uint64_t *const *ret_dev,
			      uint8_t *const *faults_dev, uint64_t *const *hist_dev,
			      void *const *streams)
{
	if (ep == nullptr || shards == nullptr || ret_dev == nullptr)
		return fail(EINVAL, "prog, shards or ret_dev is NULL");
	int err = check_devices(ndev, devices, false);
	if (err)
		return err;
	for (int d = 0; d < ndev; d++)
		if ((err = validate_batch(&shards[d], EBPF_BATCH_HIST_OVERWRITE)))
			return err;
	device_guard dg;
	std::vector<hipStream_t> st(ndev);
	for (int d = 0; d < ndev; d++)
		st[d] = streams ? static_cast<hipStream_t>(streams[d]) : nullptr;
	// A map-writing program on several shards: the batch is the shards in list order; each
	// shard's writes stay in its log, copied to the host after its launch (synchronous), and
	// the merged logs are applied there in global packet order when every shard is done.
	const bool merge = ndev > 1 && prog_ensure_translated(ep) == 0 && prog_writes_maps(*ep->xlated);
	std::vector<host_log> logs(merge ? ndev : 0);
	auto run_shard = [&](int d, const struct ebpf_pkt_batch *b, uint64_t *hist) -> int {
		if (!merge)
			return batch_dev(ep, devices[d], b, ret_dev[d], faults_dev ? faults_dev[d] : nullptr,
					 hist, st[d], nullptr);
		uint64_t first = 0;
		for (int q = 0; q < d; q++)
			first += shards[q].count;
		upd_plan plan;
		int rc = batch_dev(ep, devices[d], b, ret_dev[d], faults_dev ? faults_dev[d] : nullptr, hist,
				   st[d], &plan);
		if (rc == 0 && plan.log) {
			device_guard g2;
			hipSetDevice(devices[d]);
			rc = upd_fetch(ep->dev[devices[d]].get(), plan, st[d], first, &logs[d]);
			if (rc == 0) // (merged on the host: no offer kernel runs)
				upd_settled(plan.owner);
		}
		return rc;
	};
	if (hist_dev == nullptr) { // no collective: independent launches
		for (int d = 0; d < ndev; d++)
			if ((err = run_shard(d, &shards[d], nullptr)))
				return err;
		if (!merge)
			return 0;
		return (err = delta_merge_host(ep, ndev, devices)) ? err : upd_apply_host(ep, logs, true);
	}
	// The histogram: every shard's launch SETS its row of the scratch of its device's leading
	// stream (the first shard on that device); the rows of one device are summed into row 0,
	// row 0 is summed across devices (RCCL), and only then stored into (EBPF_BATCH_HIST_OVERWRITE)
	// or added to each caller histogram.  The caller's buffers never take part in the collective.
	std::lock_guard<std::mutex> serial(g_multi_lock); // (one call's enqueue at a time: the scratch)
	struct group {
		int device;
		std::vector<int> shard; // shard[0] leads
		unsigned long long *mh = nullptr;
		hipEvent_t *ev = nullptr;
	};
	std::vector<group> G;
	for (int d = 0; d < ndev; d++) {
		auto it = std::find_if(G.begin(), G.end(), [&](const group &g) { return g.device == devices[d]; });
		if (it == G.end()) {
			G.push_back(group{devices[d], {}});
			it = G.end() - 1;
		}
		it->shard.push_back(d);
	}
	hipError_t e;
	for (group &g : G) {
		const hipStream_t lead = st[g.shard[0]];
		if ((e = hipSetDevice(g.device)) != hipSuccess)
			return hip_fail(e, "hipSetDevice");
		// events: [0] fork (lead -> the others), [1 + j] join of shard j, [1 + k] the result
		const size_t k = g.shard.size();
		if ((err = multi_acquire(g.device, lead, (uint32_t)k, k + 2, &g.mh, &g.ev)))
			return fail(err, "multi-device histogram scratch");
		if (k > 1 && (e = hipEventRecord(g.ev[0], lead)) != hipSuccess)
			return hip_fail(e, "hipEventRecord");
		for (size_t j = 0; j < k; j++) {
			const int d = g.shard[j];
			if (j > 0 && st[d] != lead && (e = hipStreamWaitEvent(st[d], g.ev[0], 0)) != hipSuccess)
				return hip_fail(e, "hipStreamWaitEvent");
			struct ebpf_pkt_batch b = shards[d];
			b.flags |= EBPF_BATCH_HIST_OVERWRITE;
			if ((err = run_shard(d, &b, reinterpret_cast<uint64_t *>(g.mh + j * EBPF_HIST_BINS))))
				return err;
			if (j > 0 && st[d] != lead &&
			    ((e = hipEventRecord(g.ev[1 + j], st[d])) != hipSuccess ||
			     (e = hipStreamWaitEvent(lead, g.ev[1 + j], 0)) != hipSuccess))
				return hip_fail(e, "shard join");
		}
		if ((e = hipSetDevice(g.device)) != hipSuccess ||
		    (e = launch_hist_sum_rows(g.mh, (uint32_t)k, lead)) != hipSuccess)
			return hip_fail(e, "histogram rows");
	}
	const char *force = getenv("EBPF_FORCE_RCCL"); // (tests: the collective on one GPU)
	if (G.size() > 1 || (force && *force == '1')) {
		std::vector<int> dv;
		std::vector<uint64_t *> hv;
		std::vector<hipStream_t> sv;
		for (const group &g : G) {
			dv.push_back(g.device);
			hv.push_back(reinterpret_cast<uint64_t *>(g.mh));
			sv.push_back(st[g.shard[0]]);
		}
		std::string msg;
		if ((err = rccl_hist_allreduce((int)G.size(), dv.data(), hv.data(), sv.data(), &msg)))
			return fail(err, msg);
	}
	for (group &g : G) {
		const hipStream_t lead = st[g.shard[0]];
		const size_t k = g.shard.size();
		if ((e = hipSetDevice(g.device)) != hipSuccess)
			return hip_fail(e, "hipSetDevice");
		for (size_t j = 0; j < k; j++) {
			const int d = g.shard[j];
			const bool ow = (shards[d].flags & EBPF_BATCH_HIST_OVERWRITE) != 0;
			if ((e = launch_hist_store(reinterpret_cast<unsigned long long *>(hist_dev[d]), g.mh, ow,
						   lead)) != hipSuccess)
				return hip_fail(e, "histogram store");
		}
		// the other shards' streams see their histogram (and the scratch is free) after this
		if (k > 1 && (e = hipEventRecord(g.ev[1 + k], lead)) != hipSuccess)
			return hip_fail(e, "hipEventRecord");
		for (size_t j = 1; j < k; j++) {
			const int d = g.shard[j];
			if (st[d] != lead && (e = hipStreamWaitEvent(st[d], g.ev[1 + k], 0)) != hipSuccess)
				return hip_fail(e, "hipStreamWaitEvent");
		}
	}
	if (!merge)
		return 0;
	return (err = delta_merge_host(ep, ndev, devices)) ? err : upd_apply_host(ep, logs, true);
}
