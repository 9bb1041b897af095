// runtime.h — what the files of the GPU backend share.  The error and device helpers serve all
// of them; the stream scratch, the map mirrors and the write log serve the program launches
// (gpu_runtime.cpp, batch.cpp, pcap.cpp, rccl_sum.cpp, asm_runtime.cpp, asm_jit.cpp);
// steer_acquire, validate_batch, check_device and on_device serve the list operations (steer.cpp,
// group.cpp, gather.cpp, scatter.cpp, reduce.cpp, scan.cpp, filter.cpp), whose launchers are
// declared in each operation's own header.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "internal.h"

// gpu_runtime.cpp: the calling thread's last error (ebpf_gpu_last_error), and the device list
int fail(int err, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
int device_count();
// ENODEV for a device index that names no GPU
int check_device(int device);
// the events of ebpf_gpu_time_next_launch, consumed by the call
void take_time_events(hipEvent_t *start, hipEvent_t *stop);

inline bool
in_list(const std::vector<uint16_t> &v, size_t t)
{
	return std::find(v.begin(), v.end(), (uint16_t)t) != v.end();
}

// stream_scratch.cpp: per-stream scratch buffers
struct rows_slot;
// A batch's hold on its stream slot's winner words (upd_acquire -> upd_settled)
struct upd_owner {
	rows_slot *slot = nullptr;
	unsigned long long sid = 0;
};
int rows_acquire(int device, hipStream_t stream, void **out);
int ovl_acquire(int device, hipStream_t stream, size_t bytes, uint8_t **out);
int steer_acquire(int device, hipStream_t stream, size_t bytes, uint32_t **out);
int upd_acquire(int device, hipStream_t stream, size_t log_bytes, size_t win_bytes, uint8_t **log,
		unsigned long long **win, upd_owner *owner);
void upd_settled(const upd_owner &o);
int multi_acquire(int device, hipStream_t stream, uint32_t rows, size_t nev, unsigned long long **mh,
		  hipEvent_t **ev);

// map_mirror.cpp (and internal.h: map_mark_device_write, map_pull_device_writes)
int ensure_map_mirror(struct ebpf_map *em, int device, void **dev);
void mirror_write_begin(map_mirror &m, hipStream_t w);
int sync_map_mirrors(struct ebpf_prog *ep, int device, hipStream_t stream);

// The maps' order locks, taken in address order for the span of one launch (internal.h
// ebpf_map.order_lock).
struct launch_order {
	std::vector<std::unique_lock<std::mutex>> held;
	explicit launch_order(const std::vector<struct ebpf_map *> &maps)
	{
		std::vector<struct ebpf_map *> v(maps);
		std::sort(v.begin(), v.end());
		for (struct ebpf_map *m : v)
			held.emplace_back(m->order_lock);
	}
};

// map_write_log.cpp
// A device batch's map writes (map_writes.hip): the log its launches share, and where in the
// batch a launch starts.  The caller that passes a plan applies the log itself after the last
// launch (the host-buffer path: every chunk of one batch reads the maps as they were at its start).
struct upd_plan {
	uint8_t *log = nullptr;
	unsigned long long *win = nullptr;
	uint32_t cap = 0;
	uint64_t pkt_base = 0;
	uint32_t *faulted = nullptr; // one bit per packet of the batch (after the records)
	size_t faulted_bytes = 0;
	upd_owner owner;             // the stream slot whose winner words it uses (upd_acquire)
	// per table map, the device table its launches read (hashtables whose values the batch
	// stores into: a record names a slot, and this is the slot's key whatever is uploaded later)
	std::vector<std::shared_ptr<const std::vector<uint8_t>>> tables;
};
// A shard's write log brought to the host (a batch whose shards ran on several devices: the
// logs are merged there, in global packet order).  Records as on the device (map_writes.h);
// `first` = the global index of the shard's packet 0.
struct host_log {
	std::vector<uint8_t> rec;
	uint32_t count = 0;
	uint32_t stride = 0;
	std::vector<uint32_t> faulted;
	uint64_t first = 0;
	int device = -1;
	std::vector<std::shared_ptr<const std::vector<uint8_t>>> tables; // upd_plan.tables
};
int upd_plan_for(struct ebpf_prog *ep, dprog_device *dp, uint64_t count, hipStream_t stream, upd_plan *P);
int upd_fetch(const dprog_device *dp, const upd_plan &P, hipStream_t stream, uint64_t first, host_log *out);
int upd_apply_host(struct ebpf_prog *ep, const std::vector<host_log> &logs, bool arrays);
int delta_merge_host(struct ebpf_prog *ep, int ndev, const int *devices);
int upd_finish(struct ebpf_prog *ep, dprog_device *dp, const upd_plan &P, hipStream_t stream);

// gpu_runtime.cpp: a program's device state, and one launch
int prepare(struct ebpf_prog *ep, int device, dprog_device **out);
int launch(struct ebpf_prog *ep, dprog_device *dp, const dp_launch &L0, hipStream_t stream,
	   hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr, bool hist_overwrite = false,
	   upd_plan *plan = nullptr);
int validate_batch(const struct ebpf_pkt_batch *b, uint32_t allowed_flags = 0);

// A list operation's call on a device, once its arguments are checked and there is work: holds
// the caller's current device, selects `device`, takes scratch_bytes of the stream's steering
// scratch (none for 0; calls on a stream run in order, so they share the buffer), runs
// launch(stream, scratch) and maps its error.  what: the launch, for the messages.
template <typename F>
int
on_device(int device, void *stream, size_t scratch_bytes, const char *what, F launch)
{
	device_guard dg;
	hipStream_t st = static_cast<hipStream_t>(stream);
	hipError_t e = hipSetDevice(device);
	if (e != hipSuccess)
		return hip_fail(e, "hipSetDevice");
	uint32_t *scratch = nullptr;
	if (int err = scratch_bytes != 0 ? steer_acquire(device, st, scratch_bytes, &scratch) : 0)
		return fail(err, std::string("scratch of the ") + what);
	e = launch(st, scratch);
	return e == hipSuccess ? 0 : hip_fail(e, what);
}

hipError_t launch_interp_v0(const dp_launch &L, hipStream_t stream); // interp_v0.hip
// asm_runtime.cpp
hipError_t launch_interp_asm(const dp_launch &L, hipStream_t stream, int device, int mode,
			     uint32_t map_lds_bytes, void *fn, void *fn_wide, uint32_t stream_cap,
			     hipEvent_t ev_start, hipEvent_t ev_stop, unsigned long long *user_hist,
			     bool hist_overwrite);
int asm_available(int device);
bool asm_lds_fits(int mode, uint32_t map_lds_bytes, uint32_t stack_stride);
bool asm_program_needs_general(const dprog_host &xl);
bool asm_program_stores_last(const dprog_host &xl);
bool asm_program_gstage(const dprog_host &xl);
bool asm_program_hdrlds(const dprog_host &xl);
bool asm_hdrlds_fits(uint32_t map_lds_bytes, uint32_t stack_stride);
int asm_build_entries(int device, const dprog_host &xl, int mode, const std::vector<dp_map> &table,
		      dp_entry **d_out, uint32_t *stack_stride, std::string *err);
// asm_jit.cpp
int asm_jit_build(int device, const dprog_host &xl, int mode, const std::vector<dp_map> &table,
		  void **mod_out, void **fn_out, void **fn_wide_out, uint32_t *stack_stride, std::string *err);
void asm_jit_release(void *mod);
int asm_jit_emit(const dprog_host &xl, int mode, const std::vector<dp_map> &table,
		 std::vector<unsigned char> *img_out, std::vector<unsigned char> *code,
		 uint32_t *stack_stride, std::string *err);
// rccl_sum.cpp
int rccl_hist_allreduce(int ndev, const int *devices, uint64_t *const *hist, hipStream_t *streams,
			std::string *msg);
