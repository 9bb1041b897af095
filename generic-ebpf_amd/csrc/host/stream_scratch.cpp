// stream_scratch.cpp — scratch buffers kept per stream and device: the assembly kernels' verdict
// partials, a map-writing batch's log and winner words, the spilled overlay, the multi-device
// histogram rows, the tile rows of a steering call.
#include <dlfcn.h>

#include <functional>
#include <thread>

#include "runtime.h"

// Verdict-partial buffers of the assembly kernels (dprog.h DP_HIST_*), one per STREAM and
// device: launches on one stream run in order and each kernel leaves its buffer zero, so a
// stream reuses its own buffer with no event and no wait.  Streams are told apart by
// hipStreamGetId where the HIP runtime has it (ROCm >= 7.1: a stream handle can be recycled
// while work from its previous life is still in flight, an id is never reused), else by handle.
// At most kRowsMax streams per device own a buffer; past that the least recently used stream's
// buffer moves to the new stream, which first waits (on the GPU) for everything the old stream
// has submitted — or, if that stream no longer exists, the device drains.
struct rows_slot {
	void *p = nullptr;
	unsigned long long sid = 0; // owning stream's id
	hipStream_t stream = nullptr;
	uint64_t last = 0;          // order of the last use
	// map-writing programs (map_writes.hip): the stream's write log and winner words, grown on
	// demand (the kernels leave the log's counter and every winner word zero)
	void *log = nullptr;
	size_t log_bytes = 0;
	void *win = nullptr;
	size_t win_bytes = 0;
	// a batch's log was handed out and its apply step has not been enqueued since: its offer
	// kernel may have left winner words set, so the next batch clears them first
	bool win_pending = false;
	// the portable interpreter's spilled overlays (dp_launch.ovl_spill), grown on demand
	void *ovl = nullptr;
	size_t ovl_bytes = 0;
	// ebpf_batch_steer_dev's tile and segment rows (steer.hip), grown on demand (any contents:
	// the count kernel writes every row the later kernels read)
	void *steer = nullptr;
	size_t steer_bytes = 0;
	// ebpf_prog_run_batch_multi_dev, when this stream leads its device: one histogram row per
	// shard on the device (any contents: every launch overwrites its row), and fork/join events
	void *mh = nullptr;
	size_t mh_bytes = 0;
	std::vector<hipEvent_t> ev;
	bool per_thread = false; // hipStreamPerThread: `stream` names a different stream per thread
};

namespace {

std::mutex g_rows_lock;
std::vector<std::vector<rows_slot>> g_rows; // per device (capacity kRowsMax: slots never move)
uint64_t g_rows_tick = 0;
constexpr size_t kRowsMax = 64;

// The stream's slot (under g_rows_lock), created or taken over as described above.
int
slot_for(int device, hipStream_t stream, rows_slot **out)
{
	// (resolved at run time: torch bundles a HIP runtime older than the one this is built on)
	using get_id_fn = hipError_t (*)(hipStream_t, unsigned long long *);
	static const get_id_fn get_id =
	    reinterpret_cast<get_id_fn>(dlsym(RTLD_DEFAULT, "hipStreamGetId"));
	unsigned long long sid = (unsigned long long)(uintptr_t)stream;
	// hipStreamPerThread is one handle for one stream PER THREAD: two threads launching on it
	// run unordered, so each thread's stream gets its own slot (keyed by the thread)
	const bool per_thread = stream == hipStreamPerThread;
	if (per_thread)
		sid = (1ull << 63) | (unsigned long long)std::hash<std::thread::id>()(std::this_thread::get_id());
	else if (get_id && get_id(stream, &sid) != hipSuccess)
		return EIO;
	if ((int)g_rows.size() <= device)
		g_rows.resize(device + 1);
	std::vector<rows_slot> &pool = g_rows[device];
	rows_slot *lru = nullptr;
	for (rows_slot &r : pool) {
		if (r.sid == sid) {
			r.stream = stream;
			r.last = ++g_rows_tick;
			*out = &r;
			return 0;
		}
		if (!lru || r.last < lru->last)
			lru = &r;
	}
	if (pool.size() < kRowsMax) {
		pool.reserve(kRowsMax);
		rows_slot r;
		if (hipMalloc(&r.p, DP_HIST_PARTIAL_BYTES) != hipSuccess)
			return ENOMEM;
		if (hipMemsetAsync(r.p, 0, DP_HIST_PARTIAL_BYTES, stream) != hipSuccess) {
			hipFree(r.p);
			return ENOMEM;
		}
		r.sid = sid;
		r.stream = stream;
		r.per_thread = per_thread;
		r.last = ++g_rows_tick;
		pool.push_back(r);
		*out = &pool.back();
		return 0;
	}
	hipError_t e;
	if (lru->per_thread) {
		// (the handle names the calling thread's stream, not the owner's: drain the device)
		e = hipDeviceSynchronize();
	} else {
		hipEvent_t ev;
		if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
			return ENOMEM;
		e = hipEventRecord(ev, lru->stream);
		e = (e == hipSuccess) ? hipStreamWaitEvent(stream, ev, 0) : hipDeviceSynchronize();
		hipEventDestroy(ev);
	}
	if (e != hipSuccess)
		return EIO;
	lru->sid = sid;
	lru->stream = stream;
	lru->per_thread = per_thread;
	lru->last = ++g_rows_tick;
	*out = lru;
	return 0;
}

// Grow a slot's buffer to `need` bytes.  Runs under g_rows_lock, so it waits for nothing: the new
// buffer is installed, zeroed where `zero` says so by a memset enqueued on `stream` (the stream
// that acquired the slot: the launches that use the buffer run on it, or on a stream that waits
// for it), and the old buffer comes back in *old.  The caller frees that one once the lock is
// released (`retired`): hipFree waits for the device, and so for the old buffer's users.
int
grow(void **p, size_t *have, size_t need, bool zero, hipStream_t stream, void **old)
{
	if (*have >= need)
		return 0;
	void *q = nullptr;
	if (hipMalloc(&q, need) != hipSuccess)
		return ENOMEM;
	if (zero && hipMemsetAsync(q, 0, need, stream) != hipSuccess) {
		*old = q;
		return ENOMEM;
	}
	*old = *p;
	*p = q;
	*have = need;
	return 0;
}

// The buffers an acquire call replaced, freed when its scope ends.  Declared BEFORE the lock
// guard: the lock is released first.
struct retired {
	void *p[2] = {nullptr, nullptr};
	~retired()
	{
		for (void *q : p)
			if (q)
				hipFree(q);
	}
};

} // namespace

int
rows_acquire(int device, hipStream_t stream, void **out)
{
	std::lock_guard<std::mutex> g(g_rows_lock);
	rows_slot *r;
	int err = slot_for(device, stream, &r);
	if (!err)
		*out = r->p;
	return err;
}

// The stream's spilled-overlay buffer of at least `bytes` (any contents: a lane reads only the
// entries it wrote itself)
int
ovl_acquire(int device, hipStream_t stream, size_t bytes, uint8_t **out)
{
	retired old;
	std::lock_guard<std::mutex> g(g_rows_lock);
	rows_slot *r;
	int err = slot_for(device, stream, &r);
	if (!err)
		err = grow(&r->ovl, &r->ovl_bytes, bytes, false, stream, &old.p[0]);
	if (!err)
		*out = static_cast<uint8_t *>(r->ovl);
	return err;
}

// The stream's steering rows of at least `bytes` (any contents)
int
steer_acquire(int device, hipStream_t stream, size_t bytes, uint32_t **out)
{
	retired old;
	std::lock_guard<std::mutex> g(g_rows_lock);
	rows_slot *r;
	int err = slot_for(device, stream, &r);
	if (!err)
		err = grow(&r->steer, &r->steer_bytes, bytes, false, stream, &old.p[0]);
	if (!err)
		*out = static_cast<uint32_t *>(r->steer);
	return err;
}

// The stream's map-write log (>= log_bytes) and winner words (>= win_bytes).
int
upd_acquire(int device, hipStream_t stream, size_t log_bytes, size_t win_bytes, uint8_t **log,
	    unsigned long long **win, upd_owner *owner)
{
	retired old;
	std::lock_guard<std::mutex> g(g_rows_lock);
	rows_slot *r;
	int err = slot_for(device, stream, &r);
	if (!err)
		err = grow(&r->log, &r->log_bytes, log_bytes, true, stream, &old.p[0]);
	if (!err)
		err = grow(&r->win, &r->win_bytes, win_bytes, true, stream, &old.p[1]);
	if (err)
		return err;
	if (r->win_pending) { // (the previous batch on this stream stopped before its apply step)
		if (hipMemsetAsync(r->win, 0, r->win_bytes, stream) != hipSuccess)
			return EIO;
	}
	r->win_pending = true;
	*log = static_cast<uint8_t *>(r->log);
	*win = static_cast<unsigned long long *>(r->win);
	owner->slot = r;
	owner->sid = r->sid;
	return 0;
}

// The batch's apply step is enqueued: the winner words will be zero again after it (unless the
// slot went to another stream meanwhile: that stream's flag is its own)
void
upd_settled(const upd_owner &o)
{
	std::lock_guard<std::mutex> g(g_rows_lock);
	if (o.slot && o.slot->sid == o.sid)
		o.slot->win_pending = false;
}

// The leading stream's multi-device scratch: `rows` histogram rows and `nev` events.
int
multi_acquire(int device, hipStream_t stream, uint32_t rows, size_t nev, unsigned long long **mh,
	      hipEvent_t **ev)
{
	retired old;
	std::lock_guard<std::mutex> g(g_rows_lock);
	rows_slot *r;
	int err = slot_for(device, stream, &r);
	if (!err)
		err = grow(&r->mh, &r->mh_bytes, (size_t)rows * EBPF_HIST_BINS * 8, false, stream, &old.p[0]);
	while (!err && r->ev.size() < nev) {
		hipEvent_t e;
		if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
			return ENOMEM;
		r->ev.push_back(e);
	}
	if (err)
		return err;
	*mh = static_cast<unsigned long long *>(r->mh);
	*ev = r->ev.data();
	return 0;
}
