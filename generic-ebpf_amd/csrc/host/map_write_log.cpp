// map_write_log.cpp — the map writes of a batch (map_writes.h, map_writes.hip): the log its
// launches fill, its apply step on the device, and its replay and merge on the host.
#include "runtime.h"

// Log capacity for `count` packets of a map-writing program (records, and bytes: the records,
// then the faulted-packet bitmap at *bitmap_off, *bitmap_bytes long).
static int
upd_size(const struct ebpf_prog *ep, const dprog_device *dp, uint64_t count, uint32_t *cap,
	 size_t *bytes, size_t *bitmap_off, size_t *bitmap_bytes)
{
	const uint64_t rec = count * ep->xlated->max_updates;
	if (rec > UINT32_MAX)
		return fail(E2BIG, "map-writing program: more than 2^32 writes in one batch");
	*cap = (uint32_t)rec;
	*bitmap_off = (64 + rec * dp->upd_stride + 255) & ~(size_t)255;
	*bitmap_bytes = ((count + 31) / 32) * 4;
	*bytes = *bitmap_off + *bitmap_bytes;
	return 0;
}

// The log (and its bitmap) for `count` packets on `stream`.
int
upd_plan_for(struct ebpf_prog *ep, dprog_device *dp, uint64_t count, hipStream_t stream, upd_plan *P)
{
	size_t bytes = 0, boff = 0, bbytes = 0;
	int err = upd_size(ep, dp, count, &P->cap, &bytes, &boff, &bbytes);
	if (!err)
		err = upd_acquire(dp->device, stream, bytes, dp->win_words * 8, &P->log, &P->win,
				  &P->owner);
	if (err)
		return fail(err, "map-write log");
	P->faulted = reinterpret_cast<uint32_t *>(P->log + boff);
	P->faulted_bytes = bbytes;
	// (the buffer is reused at other sizes: whatever lies where the bitmap now starts is stale).
	// The log's counter is zero after every apply step; it is zeroed here too, so that a batch
	// whose launch failed before its apply leaves nothing behind.  The winner words are zeroed
	// when allocated and only the apply step writes them (its first kernel offers, its second
	// re-arms every word that received an offer); a batch that stopped before its apply step was
	// enqueued leaves the stream's flag set, and upd_acquire clears them then
	hipError_t e = hipMemsetAsync(P->faulted, 0, bbytes, stream);
	if (e == hipSuccess)
		e = hipMemsetAsync(P->log, 0, 4, stream);
	return e == hipSuccess ? 0 : hip_fail(e, "hipMemsetAsync(map-write log)");
}

// After the batch: the logged writes land in the mirrors (packet order), and the written maps
// remember that this device's mirror is newer than their host copy.
static int
upd_apply(struct ebpf_prog *ep, dprog_device *dp, const upd_plan &P, hipStream_t stream)
{
	std::vector<uint16_t> dev = ep->xlated->upd_maps;
	dev.insert(dev.end(), ep->xlated->atomic_maps.begin(), ep->xlated->atomic_maps.end());
	for (uint16_t t : dev) { // (the writes land after other streams' readers)
		struct ebpf_map *em = ep->xlated->maps[t];
		std::lock_guard<std::mutex> g(em->mirror_lock);
		mirror_write_begin(em->mirrors[dp->device], stream);
	}
	hipError_t e = launch_map_writes(P.log, P.cap, dp->upd_stride,
					 static_cast<const upd_map *>(dp->d_upd), dp->upd_host.data(),
					 (uint32_t)dp->upd_host.size(), P.win, P.faulted, stream);
	if (e != hipSuccess)
		return hip_fail(e, "map writes");
	upd_settled(P.owner);
	for (uint16_t t : dev)
		map_mark_device_write(ep->xlated->maps[t], dp->device, static_cast<void *>(stream));
	return 0;
}

// Copy the plan's log (its records and faulted-packet bitmap) to the host.  Synchronous.
int
upd_fetch(const dprog_device *dp, const upd_plan &P, hipStream_t stream, uint64_t first, host_log *out)
{
	hipError_t e = hipStreamSynchronize(stream);
	uint32_t n = 0;
	if (e == hipSuccess && P.cap)
		e = hipMemcpy(&n, P.log, 4, hipMemcpyDeviceToHost);
	out->count = std::min(n, P.cap);
	out->stride = dp->upd_stride;
	out->first = first;
	out->device = dp->device;
	out->tables = P.tables;
	out->rec.resize((size_t)out->count * out->stride);
	out->faulted.resize(P.faulted_bytes / 4);
	if (e == hipSuccess && out->count)
		e = hipMemcpy(out->rec.data(), P.log + 64, out->rec.size(), hipMemcpyDeviceToHost);
	if (e == hipSuccess && P.faulted_bytes)
		e = hipMemcpy(out->faulted.data(), P.faulted, P.faulted_bytes, hipMemcpyDeviceToHost);
	// (the log's counter is re-armed by the apply step, or by the next batch's upd_plan_for)
	return e == hipSuccess ? 0 : hip_fail(e, "map-write log copy");
}

// A counter update, a store, or an update / delete call, applied to the host copy of a map.
static void
apply_value(uint8_t *at, uint32_t size, bool add, const uint8_t *data)
{
	if (!add) {
		memcpy(at, data, size);
		return;
	}
	uint64_t v = 0, d = 0;
	memcpy(&v, at, size);
	memcpy(&d, data, size);
	v += d;
	memcpy(at, &v, size);
}

// The logs of a batch applied on the host, every record of a packet that did not fault (a
// counter update's record even then: ebpf_gpu.h) in (global packet, call) order:
//   - records of hupd_maps (hashtables; arrays mixing counter updates and stores), always:
//     hashtable update / delete calls replayed through the map's own update / delete (the
//     program side of ebpf_map_hashtable.c:346-431 / :475-502, percpu: the submitting CPU's
//     value), a replayed call that fails against the table as it then is (EEXIST, ENOENT, EBUSY)
//     leaving it unchanged; stores and counter updates into a hashtable value applied to the
//     element with the slot's key (the device table's image) if it still exists; array stores
//     and counter updates applied to the host copy;
//   - records of upd_maps (`arrays`: a batch whose shards ran on several devices) too, so the
//     last write of a byte wins — the device apply step's rule (map_writes.hip); every device
//     mirror of the maps changed here is then stale.
int
upd_apply_host(struct ebpf_prog *ep, const std::vector<host_log> &logs, bool arrays)
{
	const dprog_host &xl = *ep->xlated;
	struct ref {
		uint64_t order;
		const uint8_t *r;
		const host_log *h;
	};
	std::vector<ref> all;
	for (const host_log &h : logs)
		for (uint32_t i = 0; i < h.count; i++) {
			const uint8_t *r = h.rec.data() + (size_t)i * h.stride;
			uint64_t pkt;
			uint32_t em;
			memcpy(&pkt, r, 8);
			memcpy(&em, r + 8, 4);
			if ((em >> 20) >= xl.maps.size())
				return fail(EIO, "map-write log: a record names no map of the program");
			const bool add = (em & DP_REC_VALUE) && (em & DP_REC_ADD);
			if (!add && pkt / 32 < h.faulted.size() && ((h.faulted[pkt / 32] >> (pkt % 32)) & 1))
				continue; // the packet faulted: none of its writes land (counter updates do)
			if (in_list(xl.hupd_maps, em >> 20) || (arrays && in_list(xl.upd_maps, em >> 20)))
				all.push_back(ref{h.first + pkt, r, &h});
		}
	// Within a packet the records are already in call order: a lane takes its log slots one call
	// after the other and every log is gathered in slot order.  (The entry index is no order: a
	// run-time-map compare chain's copies, and merge points under standard semantics, are
	// numbered after entries that a path reaches later.)  So sort by packet only, stably.
	std::stable_sort(all.begin(), all.end(), [](const ref &a, const ref &b) { return a.order < b.order; });
	const uint16_t cpu = map_current_cpu();
	std::vector<uint16_t> host_arrays; // the array maps whose host copy changes here
	for (size_t t = 0; t < xl.maps.size(); t++)
		if (!xl.maps[t]->is_hashtable() &&
		    (in_list(xl.hupd_maps, t) || (arrays && in_list(xl.upd_maps, t))))
			host_arrays.push_back((uint16_t)t);
	for (uint16_t t : host_arrays)
		if (map_pull_device_writes(xl.maps[t]) != 0)
			return fail(EIO, "copying a device batch's map writes back failed");
	for (const ref &x : all) {
		uint32_t em, word;
		memcpy(&em, x.r + 8, 4);
		memcpy(&word, x.r + 12, 4);
		struct ebpf_map *m = xl.maps[em >> 20];
		if (em & DP_REC_VALUE) {
			const uint32_t size = em & 0xf;
			const bool add = (em & DP_REC_ADD) != 0;
			if (m->is_hashtable()) {
				// the slot's key in the table the batch's launch read (upd_plan.tables), not in
				// whatever a later upload left in the mirror
				uint32_t slot;
				memcpy(&slot, x.r + 24, 4);
				const map_device_layout l = map_device_layout_of(m);
				const uint16_t t = (uint16_t)(em >> 20);
				if (t >= x.h->tables.size() || !x.h->tables[t] || slot >= l.slots)
					continue;
				const std::vector<uint8_t> &img = *x.h->tables[t];
				const size_t so = (size_t)slot << dp_hash_stride_log2(l.flags);
				if (so + 8 + m->key_size > img.size())
					continue;
				uint8_t *v = static_cast<uint8_t *>(
				    m->emt->ops.lookup_elem(m, const_cast<uint8_t *>(img.data() + so + 8)));
				if (v != nullptr && word + size <= m->value_size) // (deleted before: nothing)
					apply_value(v + word, size, add, x.r + 16);
				continue;
			}
			if ((uint64_t)word + size > (uint64_t)m->value_size * m->max_entries)
				continue;
			uint8_t *img = const_cast<uint8_t *>(map_array_image(m, m->percpu ? cpu : 0));
			apply_value(img + word, size, add, x.r + 16);
			continue;
		}
		if (m->is_hashtable()) {
			void *key = const_cast<uint8_t *>(x.r + 16);
			void *value = const_cast<uint8_t *>(x.r + 16 + dp_hash_key_bytes(m->key_size));
			if ((word & 0xff) == 1)
				m->emt->ops.delete_elem(m, key);
			else
				m->emt->ops.update_elem(m, key, value, (word >> 8) & 0xff);
			continue;
		}
		if (word >= m->max_entries)
			continue; // (never: the routine checked it)
		uint8_t *img = const_cast<uint8_t *>(map_array_image(m, m->percpu ? cpu : 0));
		memcpy(img + (size_t)m->value_size * word, x.r + 16, m->value_size);
	}
	for (uint16_t t : host_arrays)
		xl.maps[t]->version.fetch_add(1);
	return 0;
}

// A batch sharded over several devices: the counter updates of its UPD_ATOMIC maps, summed in
// each device's delta area (one area per device, however many shards ran there), go into the
// host copy — after every shard is done — and the areas are zeroed.  The device mirrors are then
// stale.
int
delta_merge_host(struct ebpf_prog *ep, int ndev, const int *devices)
{
	const dprog_host &xl = *ep->xlated;
	if (xl.atomic_maps.empty())
		return 0;
	const uint16_t cpu = map_current_cpu();
	for (size_t k = 0; k < xl.atomic_maps.size(); k++) {
		struct ebpf_map *m = xl.maps[xl.atomic_maps[k]];
		if (map_pull_device_writes(m) != 0)
			return fail(EIO, "copying a device batch's map writes back failed");
		const uint32_t w = xl.atomic_width[k];
		const size_t bytes = (size_t)m->value_size * m->max_entries;
		uint8_t *img = const_cast<uint8_t *>(map_array_image(m, m->percpu ? cpu : 0));
		std::vector<uint8_t> d(bytes);
		for (int q = 0; q < ndev; q++) {
			bool seen = false;
			for (int q2 = 0; q2 < q; q2++)
				seen = seen || devices[q2] == devices[q];
			if (seen)
				continue;
			void *mdev = nullptr;
			{
				std::lock_guard<std::mutex> g(m->mirror_lock);
				if (devices[q] < (int)m->mirrors.size())
					mdev = m->mirrors[devices[q]].dev;
			}
			if (mdev == nullptr)
				continue;
			device_guard g2;
			hipError_t e = hipSetDevice(devices[q]);
			uint8_t *da = static_cast<uint8_t *>(mdev) + dp_delta_off(m->value_size, m->max_entries);
			if (e == hipSuccess)
				e = hipMemcpy(d.data(), da, bytes, hipMemcpyDeviceToHost);
			if (e == hipSuccess)
				e = hipMemset(da, 0, bytes);
			if (e == hipSuccess) // (done before the next launch's atomics: hipMemset may return early)
				e = hipDeviceSynchronize();
			if (e != hipSuccess)
				return hip_fail(e, "counter updates copy");
			for (size_t o = 0; o < bytes; o += w)
				apply_value(img + o, w, true, d.data() + o);
		}
		m->version.fetch_add(1);
	}
	return 0;
}

// The end of a map-writing batch on one device: records of upd_maps and the counter updates of
// atomic_maps applied on the device (upd_apply), records of hupd_maps copied to the host and
// replayed there (synchronous).
int
upd_finish(struct ebpf_prog *ep, dprog_device *dp, const upd_plan &P, hipStream_t stream)
{
	const bool host = !ep->xlated->hupd_maps.empty();
	std::vector<host_log> logs(host ? 1 : 0);
	int err;
	if (host && (err = upd_fetch(dp, P, stream, 0, &logs[0])))
		return err;
	if (!ep->xlated->upd_maps.empty() || !ep->xlated->atomic_maps.empty()) {
		if ((err = upd_apply(ep, dp, P, stream)))
			return err;
	} else {
		upd_settled(P.owner); // (no offer kernel ran: the winner words are untouched)
	}
	return host ? upd_apply_host(ep, logs, false) : 0;
}
