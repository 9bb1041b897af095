// map_mirror.cpp — the device mirrors of the maps (internal.h map_mirror): their upload before a
// launch, the cross-stream order of their users, and the way back of a device batch's writes.
#include "runtime.h"

int
ensure_map_mirror(struct ebpf_map *em, int device, void **dev)
{
	std::lock_guard<std::mutex> g(em->mirror_lock);
	if ((int)em->mirrors.size() <= device)
		em->mirrors.resize(device + 1);
	map_mirror &m = em->mirrors[device];
	if (m.dev == nullptr) {
		// an array: its values padded to 64 bytes, then the delta area of counter updates
		// (dprog.h dp_delta_off), both zero until the first upload
		const size_t bytes = em->is_hashtable() ? map_device_layout_of(em).bytes
							: 2 * dp_delta_off(em->value_size, em->max_entries);
		hipError_t e = hipMalloc(&m.dev, bytes);
		if (e == hipSuccess && !em->is_hashtable())
			e = hipMemset(m.dev, 0, bytes);
		if (e == hipSuccess) // (done before any stream uses it: hipMemset may return early)
			e = hipDeviceSynchronize();
		if (e != hipSuccess)
			return hip_fail(e, "hipMalloc(map mirror)");
		m.version = ~0ull;
	}
	*dev = m.dev;
	return 0;
}

// Cross-stream order of one mirror's users (internal.h map_mirror; callers hold mirror_lock).
// Nothing is enqueued while every user of the mirror is on one stream.
static bool
has_stream(const std::vector<void *> &v, hipStream_t s)
{
	return std::find(v.begin(), v.end(), static_cast<void *>(s)) != v.end();
}

// A launch on `s` is about to read the mirror: after the last write made on another stream.
static void
mirror_read(map_mirror &m, hipStream_t s)
{
	if (m.wr_ev && !has_stream(m.synced, s)) {
		hipStreamWaitEvent(s, static_cast<hipEvent_t>(m.wr_ev), 0);
		m.synced.push_back(s);
	}
	if (!has_stream(m.readers, s))
		m.readers.push_back(s);
}

// A write of the mirror is about to be enqueued on `w`: after every launch that read it on
// another stream since the last write (an event recorded on that stream now covers all of
// them), and after the last write itself.
void
mirror_write_begin(map_mirror &m, hipStream_t w)
{
	for (void *r : m.readers) {
		if (r == static_cast<void *>(w))
			continue;
		hipEvent_t ev;
		if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
			hipStreamSynchronize(static_cast<hipStream_t>(r)); // (no event: wait on the host)
			continue;
		}
		hipEventRecord(ev, static_cast<hipStream_t>(r));
		hipStreamWaitEvent(w, ev, 0);
		hipEventDestroy(ev); // (released once it completes)
	}
	if (m.wr_ev && !has_stream(m.synced, w))
		hipStreamWaitEvent(w, static_cast<hipEvent_t>(m.wr_ev), 0);
}

// ... and it is enqueued: later users on other streams wait for it.
static void
mirror_write_end(map_mirror &m, hipStream_t w)
{
	if (m.wr_ev == nullptr) {
		hipEvent_t ev;
		if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
			hipStreamSynchronize(w);
			m.synced.clear();
			m.readers.clear();
			return;
		}
		m.wr_ev = ev;
	}
	hipEventRecord(static_cast<hipEvent_t>(m.wr_ev), w);
	m.synced.assign(1, static_cast<void *>(w));
	m.readers.clear();
}

int
sync_map_mirrors(struct ebpf_prog *ep, int device, hipStream_t stream)
{
	const uint16_t cpu = map_current_cpu();
	for (struct ebpf_map *em : ep->xlated->maps) {
		const uint16_t c = em->percpu ? cpu : 0;
		// a batch wrote the map on another device, or on this one for another CPU's copy of a
		// percpu map (which is about to be replaced by this CPU's): its writes reach the host
		// copy first
		const int dd = em->dev_dirty.load(std::memory_order_acquire);
		if (dd >= 0) {
			bool pull = dd != device;
			if (!pull) {
				std::lock_guard<std::mutex> g(em->mirror_lock);
				pull = em->mirrors[device].cpu != c;
			}
			if (pull && map_pull_device_writes(em) != 0)
				return fail(EIO, "copying a device batch's map writes back failed");
		}
		std::lock_guard<std::mutex> g(em->mirror_lock);
		map_mirror &m = em->mirrors[device];
		uint64_t v = em->version.load();
		if (m.version != v || m.cpu != c) {
			hipError_t e;
			mirror_write_begin(m, stream);
			if (em->is_hashtable()) {
				// a fresh snapshot of the table; the staging copy must outlive the transfer
				auto img = std::make_shared<std::vector<uint8_t>>();
				map_device_image(em, *img, c);
				m.image = img;
				e = hipMemcpyAsync(m.dev, img->data(), img->size(), hipMemcpyHostToDevice, stream);
				if (e == hipSuccess)
					e = hipStreamSynchronize(stream);
			} else {
				// from a snapshot: the upload may wait on the stream for other streams'
				// readers (mirror_write_begin) while the host writes the map again.  The
				// previous upload from the snapshot has finished once the last write has
				// (every write of the mirror is ordered after the one before it).
				if (m.wr_ev)
					hipEventSynchronize(static_cast<hipEvent_t>(m.wr_ev));
				const size_t bytes = (size_t)em->value_size * em->max_entries;
				const uint8_t *src = map_array_image(em, c);
				auto img = std::make_shared<std::vector<uint8_t>>(src, src + bytes);
				m.image = img;
				e = hipMemcpyAsync(m.dev, img->data(), bytes, hipMemcpyHostToDevice, stream);
			}
			if (e != hipSuccess)
				return hip_fail(e, "hipMemcpyAsync(map mirror)");
			mirror_write_end(m, stream);
			m.version = v;
			m.cpu = c;
		}
		mirror_read(m, stream); // (the launch that follows reads it)
	}
	return 0;
}

void
map_release_device_state(struct ebpf_map *em)
{
	device_guard dg;
	if (em->wb_event) {
		hipEventSynchronize(static_cast<hipEvent_t>(em->wb_event));
		hipEventDestroy(static_cast<hipEvent_t>(em->wb_event));
		em->wb_event = nullptr;
	}
	for (size_t d = 0; d < em->mirrors.size(); d++) {
		if (hipSetDevice((int)d) != hipSuccess)
			continue;
		if (em->mirrors[d].wr_ev)
			hipEventDestroy(static_cast<hipEvent_t>(em->mirrors[d].wr_ev));
		if (em->mirrors[d].dev)
			hipFree(em->mirrors[d].dev);
	}
	em->mirrors.clear();
}

// The device's mirror now holds the batch's writes: it is the newest copy.  The version moves on
// so that other devices re-upload (after pulling these writes, sync_map_mirrors) while this
// device keeps its mirror.
void
map_mark_device_write(struct ebpf_map *em, int device, void *stream)
{
	std::lock_guard<std::mutex> g(em->mirror_lock);
	if (em->wb_event == nullptr) {
		hipEvent_t ev;
		if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
			return;
		em->wb_event = ev;
	} else if (em->dev_dirty.load() == device) {
		// another stream may have written the mirror and not finished: the event recorded below
		// must cover that apply too (the pull waits for every writer, not only the last)
		hipStreamWaitEvent(static_cast<hipStream_t>(stream), static_cast<hipEvent_t>(em->wb_event), 0);
	}
	hipEventRecord(static_cast<hipEvent_t>(em->wb_event), static_cast<hipStream_t>(stream));
	const uint64_t v = em->version.fetch_add(1) + 1;
	if ((int)em->mirrors.size() > device) {
		em->mirrors[device].version = v;
		mirror_write_end(em->mirrors[device], static_cast<hipStream_t>(stream));
	}
	em->dev_dirty.store(device, std::memory_order_release);
}

int
map_pull_device_writes(struct ebpf_map *em)
{
	if (em->dev_dirty.load(std::memory_order_acquire) < 0)
		return 0;
	std::lock_guard<std::mutex> g(em->mirror_lock);
	const int d = em->dev_dirty.load(std::memory_order_acquire);
	if (d < 0 || d >= (int)em->mirrors.size())
		return 0;
	const map_mirror &m = em->mirrors[d];
	hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(em->wb_event));
	// array / percpu array: the mirror is the (submitting CPU's) value array
	uint8_t *dst = const_cast<uint8_t *>(map_array_image(em, em->percpu ? m.cpu : 0));
	if (e == hipSuccess && dst && m.dev)
		e = hipMemcpy(dst, m.dev, (size_t)em->value_size * em->max_entries, hipMemcpyDeviceToHost);
	if (e != hipSuccess) {
		set_last_error(std::string("map write-back: ") + hipGetErrorString(e));
		return EIO; // (still dirty: a later call tries again)
	}
	em->dev_dirty.store(-1, std::memory_order_release);
	return 0;
}
