/*
 * ebpf_gpu.h — batch execution of one loaded eBPF program over many packets on MI355X.
 *
 * This is the engine's C-ABI extension to the reference API (sys/sys/ebpf.h).  The reference
 * has no batch entry point: callers loop over packets and call ebpf_prog_run(ctx, ep) once per
 * packet (sys/dev/ebpf/ebpf_interpreter.c:23; hot loop #1 in SURVEY.md §3(C)).  Each function
 * below replaces that caller loop:
 *
 *   ebpf_prog_run_batch      ↔ for (i..n) ret[i] = ebpf_prog_run(pkt_i, ep);   host buffers
 *   ebpf_prog_run_batch_dev  ↔ the same loop over device-resident packets (the measured path)
 *
 * Per packet the result is bit-identical to ebpf_prog_run on the same bytes (reference
 * semantics, including its quirks: cumulative pc stepping, MOV64 = add, NEG, logical ARSH —
 * ebpf_interpreter.c:39,89-91,110-115,182-184,197-208).  Where the reference has no defined
 * behaviour (it crashes, aborts, hangs or reads stray memory) the device stops that packet
 * and records an ebpf_fault code instead; ret[i] is then 0.
 *
 * Plain pointers and sizes only; no torch or HIP types in any signature (a HIP stream is
 * passed as void*).
 */
#ifndef EBPF_AMD_EBPF_GPU_H
#define EBPF_AMD_EBPF_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct ebpf_prog;
struct ebpf_map;

/* Map writes in a device batch.  The reference runs packets one at a time, so a program's
 * map_update_elem (ebpf_map.c:101-108 -> ebpf_map_array.c:185-211) is seen by the next packet.
 * A device batch runs its packets at once; its defined semantics are those of the caller's
 * loop with the writes held back until the loop ends:
 *   - every packet reads the maps as they were when the batch started (its own writes too);
 *   - map_update_elem returns the reference's code: EINVAL for a NULL key or value or flags >
 *     EBPF_EXIST, EEXIST for EBPF_NOEXIST (an array's keys all exist), EINVAL for a key >=
 *     max_entries, else 0;
 *   - after the batch the writes land in packet order, a packet's own in call order: the last
 *     write of a key wins; a packet that faults (any code, even after its writes) leaves no
 *     write behind;
 *   - map_delete_elem on an array map returns EINVAL (ebpf_map_array.c:246-250);
 *   - on a hashtable map, map_update_elem returns the reference's code against the batch-start
 *     table: EINVAL as above, EEXIST (EBPF_NOEXIST, the key present) / ENOENT (EBPF_EXIST, the
 *     key absent) (ebpf_map_hashtable.c:87-100), EBUSY for a new key when the table was full
 *     (:371-377), else 0; map_delete_elem returns 0 (:475-502; EINVAL for a NULL key).  The key
 *     is read (region-checked) before the flags are judged, the value only by a call returning
 *     0.  The calls that returned 0 are replayed on the host table after the batch, in the same
 *     packet / call order, through the map's own update / delete (percpu: the submitting CPU's
 *     value): the table is the one the reference would hold after those calls in that order; a
 *     replayed call that fails against the table as it then is (EEXIST, ENOENT, EBUSY) leaves it
 *     unchanged.  A batch with hashtable writes synchronises with the host before it returns;
 *   - the map may be known only at run time (r1 computed or loaded): the helper then checks r1
 *     against the maps of the program; r1 NULL (or a NULL key / value, or flags > EBPF_EXIST)
 *     is EINVAL as in ebpf_map.c:101-108 / :130-136, a pointer that is no map of them faults
 *     EBPF_FAULT_BAD_MAP (the reference dereferences it);
 *   - a loop-free program makes every write its path reaches, however many, as the reference
 *     does (the log is sized by the program's longest path).  A program with loops (standard
 *     semantics: a backward jump reachable from slot 0 on the slot graph — not JA -1, which
 *     spins into EBPF_FAULT_LOOP, nor a jump before slot 0, EBPF_FAULT_SLOT; decided from the
 *     bytecode) has no per-path bound, so there a packet may make 16 logged
 *     writes: map_update_elem calls that return 0, every hashtable map_delete_elem (whether the
 *     key exists is known only at the replay), stores into map values, and counter updates
 *     into a hashtable's values (records replayed after the batch); counter updates into an
 *     array aligned to their width (below) are not counted (device atomics).  The 17th faults
 *     the packet with EBPF_FAULT_WRITES (a fault: its writes do not land, its counter updates
 *     do);
 *   - a writing program sharded over several devices (ebpf_prog_run_batch_multi*): the batch is
 *     the shards in order, every shard reads the batch-start maps, and the shards' writes are
 *     merged on the host in that global packet order after the last shard — the same result as
 *     one batch on one device (ebpf_prog_run_batch_multi_dev then synchronises its streams).
 * The written values live in the device's mirror of the map until the host API touches the map
 * (lookup / update / delete / get_next_key, or a helper call from ebpf_prog_run), which copies
 * them back first.  ebpf_prog_run itself keeps the reference's immediate writes.
 *
 * Stores into map values.  The reference hands the program a pointer into the map's storage
 * (array_map_lookup_elem, ebpf_map_array.c:115-124; a hashtable element's value,
 * ebpf_map_hashtable.c:285-301) and ST / STX write through it in place
 * (ebpf_interpreter.c:343-366).  In a device batch:
 *   - a packet's loads (LDX, and the load of a counter update or XADD below) see its own
 *     earlier stores into map values; other packets of the batch see the batch-start maps.
 *     Helper calls read keys and values as the batch started.  (A loop-free path may store and
 *     read back up to 2,048 times; past 16 such stores the batch runs on the portable
 *     interpreter, the packets' views in device memory.  Loops: below);
 *   - after the batch the stores land in packet order, a packet's own in program order, byte by
 *     byte: the last store of each byte wins (together with map_update_elem's whole values);
 *   - counter updates land as additions: three consecutive instructions (JA aside)
 *     LDX{W,DW} X = [P + off] (X != P); ADD or SUB to X of an immediate or of a register other
 *     than X (64-bit; 32-bit too for W; under the reference's semantics MOV64, which adds);
 *     STX [P + off] = X of the same width — and, under standard semantics, XADD
 *     (BPF_STX | BPF_XADD, W / DW; imm 0, or 1 = BPF_FETCH: src receives the old value) — add
 *     (stored - loaded) mod 2^width when the address is aligned to the width within the map's
 *     values (arrays: from the first value; hashtables: from the value's start), else land as
 *     plain stores.  Additions commute, so a map that only counter updates touch in a batch ends
 *     as the reference's sequential run leaves it (per-packet counters, byte counts);
 *   - a packet that faults leaves no write behind except its counter updates, which are atomic
 *     operations: they take effect when executed;
 *   - EBPF_FAULT_MAP_WRITE is left for a store into a map value the translation did not provide
 *     for (a packet-relative pointer that lands in a map);
 *   - in a program with loops (standard semantics) a counter update must go to a hashtable
 *     (a logged write, counted as above) or to an array that only aligned counter updates of
 *     one width change (the batch functions return EOPNOTSUPP for an array that mixes them with
 *     other writes).  The packet may read its counters back through an XADD with BPF_FETCH or
 *     through the idiom's register (live after the STX: the program "reads its counters back",
 *     decided from its bytecode on the slot graph — a reachable such XADD or idiom, a CALL
 *     reading its helper's arguments (lookup, delete r1-r2; update r1-r4), EXIT r0); it then
 *     sees the batch-start value plus its own additions,
 *     kept in 32 8-byte words of map values per packet: a store, counter update or XADD that
 *     needs a word beyond them faults EBPF_FAULT_WRITES before it happens (a word already held
 *     is free: one counter updated on every trip takes one).  The map still lands as additions.
 *     A read-back of another form (a later plain load of a counter's word) returns EOPNOTSUPP
 *     when the program also updates array counters (device atomics, not counted, so nothing
 *     else bounds that view); with hashtable counters alone it is allowed.  Plain stores,
 *     hashtable counter updates and map_update_elem / map_delete_elem in loops are limited
 *     only by the 16 logged writes per packet.
 * How it runs: arrays changed only by aligned counter updates of one width take device atomics
 * into a delta area next to their mirror (added into the values after the batch); other arrays'
 * stores land on the device (per-byte winners); hashtables, and arrays that mix counter updates
 * with stores, replay the batch's records on the host in order. */

/* Per-packet fault codes (0 = the program reached EXIT). */
enum ebpf_fault {
	EBPF_FAULT_NONE = 0,
	EBPF_FAULT_BAD_OPCODE = 1,   /* opcode outside the dispatch table (ebpf_interpreter.c:367-369: abort) */
	EBPF_FAULT_DIV_ZERO = 2,     /* DIV/MOD by 0 (reference: SIGFPE) */
	EBPF_FAULT_MEM = 3,          /* load/store outside this packet, its stack or a map value */
	EBPF_FAULT_SLOT = 4,         /* stepping left the program (reference reads past the buffer) */
	EBPF_FAULT_HELPER = 5,       /* CALL id outside [0,64) or an unset helper slot (:283) */
	EBPF_FAULT_HELPER_UNSUPPORTED = 6, /* helper with no device implementation */
	EBPF_FAULT_BAD_REG = 7,      /* dst/src register nibble >= 11 (reference overflows reg[]) */
	EBPF_FAULT_LOOP = 8,         /* a jump that re-enters its own state: the reference never returns;
	                                standard semantics: the loop budget is spent (see below) */
	EBPF_FAULT_MAP_WRITE = 9,    /* store into a map value through a pointer the translation did
	                                not see reach a map ("Stores into map values" above) */
	EBPF_FAULT_BAD_MAP = 10,     /* map helper called with r1 not a map of this program's env */
	EBPF_FAULT_WRITES = 11,      /* the packet's 17th logged map write in a device batch ("Map
	                                writes in a device batch" above) */
	EBPF_FAULT_MAX
};

/* Batch descriptor.  Fixed-stride mode (offsets == NULL): packet i occupies
 * [data + i*stride, data + (i+1)*stride).  Offsets mode: packet i occupies
 * [data + offsets[i], data + offsets[i+1]) — offsets has count+1 entries.  Extents mode
 * (flags & EBPF_BATCH_EXTENTS): packet i occupies [data + offsets[2i], data + offsets[2i+1]) —
 * offsets has 2*count entries, start <= end, packets in any order, with gaps between them or
 * overlapping (a capture's records in place: ebpf_pcap_extents).  A program that stores into
 * overlapping packets leaves their common bytes unspecified.  Offsets are 64-bit and may lie
 * 4 GiB or more from data; a packet is shorter than 4 GiB: in both offsets modes an end below
 * its start, or 2^32 bytes or more past it, gives a packet of length 0 (every load from it
 * faults EBPF_FAULT_MEM). */
struct ebpf_pkt_batch {
	const void *data;
	const uint64_t *offsets;
	uint64_t count;
	uint32_t stride;
	uint32_t flags; /* EBPF_BATCH_* */
};

/* ebpf_prog_run_batch_dev: hist_dev receives this batch's counts instead of having them added,
 * so the caller need not zero it before each launch. */
#define EBPF_BATCH_HIST_OVERWRITE 0x1u
/* Every batch entry point: offsets holds (start, end) pairs (extents mode above). */
#define EBPF_BATCH_EXTENTS 0x2u

/* Verdict histogram: bin min(r0, 255) for packets that reached EXIT, bin 256 = faulted. */
#define EBPF_HIST_BINS 257

/* Per-call summary for the host-buffer entry point. */
struct ebpf_batch_stats {
	uint64_t packets;
	uint64_t faulted;
	uint64_t hist[EBPF_HIST_BINS];
	double kernel_ms;     /* device time of the interpreter launches */
	double total_ms;      /* wall time including H2D/D2H */
};

/* A packet capture as a batch (the path starts in host memory: a NIC ring or a pcap buffer).
 * `capture` holds a classic libpcap file (magic 0xa1b2c3d4 / 0xa1b23c4d, either byte order):
 * packet i of the batch is record i's captured bytes, in offsets form, ready for
 * ebpf_prog_run_batch.  The library allocates batch->data and batch->offsets (pinned host memory
 * when `pinned` and a GPU is present, else pageable); release both with ebpf_pcap_batch_free.
 * The capture buffer stays the caller's and is not referenced afterwards.
 * A record whose captured length exceeds the header's snaplen becomes its first snaplen bytes
 * (libpcap's reader does the same), counted in info->truncated.
 * Returns 0, EINVAL (not a classic pcap capture, or a record header or record that runs past
 * the end of `capture`; ebpf_gpu_last_error says which), ENOMEM.  Host only: no GPU needed. */
struct ebpf_pcap_info {
	uint32_t linktype;     /* the capture's link-layer type (1 = Ethernet) */
	uint32_t snaplen;
	uint32_t nanosecond;   /* 1: nanosecond timestamps (magic 0xa1b23c4d) */
	uint32_t byte_swapped; /* 1: written in the other byte order */
	uint64_t truncated;    /* records whose captured length is below the original length */
	uint64_t bytes;        /* captured bytes of all records (batch->offsets[count]) */
};
int ebpf_pcap_batch(const void *capture, size_t len, int pinned, struct ebpf_pkt_batch *batch,
		    struct ebpf_pcap_info *info);
/* The same capture as an extents-mode batch over the capture itself: batch->data = capture (no
 * copy; it must stay valid while the batch is used), batch->offsets = the library's (start, end)
 * pair of every record's captured bytes (snaplen-truncated as above), flags =
 * EBPF_BATCH_EXTENTS.  Only the offsets are allocated (pinned on request); release them with
 * ebpf_pcap_batch_free, which leaves an extents batch's data alone.  Same errors. */
int ebpf_pcap_extents(const void *capture, size_t len, int pinned, struct ebpf_pkt_batch *batch,
		      struct ebpf_pcap_info *info);
void ebpf_pcap_batch_free(struct ebpf_pkt_batch *batch);

/* Number of visible GPUs (0 on a host without one). Never fails. */
int ebpf_gpu_device_count(void);

/* Initialise the device backend on GPUs 0..ndev-1 (ndev <= 0: every visible GPU): load the
 * kernels' code object on each, which the first batch on a device would otherwise do.  Optional.
 * Returns 0, ENODEV (no GPU, or ndev above the visible count), EIO (a code object did not
 * load on a device; ebpf_gpu_last_error says which).  (ebpf_dev_init) */
int ebpf_dev_init(int ndev);

/* Translate + upload the program (and its maps) to `device`.  Called implicitly by the run
 * functions; explicit calls move the one-time cost out of a timed region.
 * Returns 0, ENODEV (no GPU / no device code object), E2BIG (program state graph too large),
 * ENOMEM. */
int ebpf_prog_prepare_device(struct ebpf_prog *ep, int device);

/* Host buffers in, host buffers out; runs on the current device (ebpf_gpu_set_device).
 * ret: count u64 (required).  faults: count u8 (optional).  stats: optional.
 * Returns 0 or an errno; packet faults are NOT call errors. */
int ebpf_prog_run_batch(struct ebpf_prog *ep, const struct ebpf_pkt_batch *batch,
			uint64_t *ret, uint8_t *faults, struct ebpf_batch_stats *stats);

/* ebpf_prog_run_batch without blocking the caller: the job is queued for the worker pool of the
 * calling thread's current device (two persistent threads per device, a FIFO of at most 64
 * queued jobs) and the call returns at once, so a NIC-ring or capture consumer can fill its next
 * segment meanwhile; ebpf_batch_wait blocks until ret/faults hold the results, returns the
 * batch's error code (ebpf_prog_run_batch's) and releases the job (wait once per job).  The
 * program, the batch's buffers, ret and faults must stay valid until the wait; several jobs may
 * be in flight.
 * Returns 0, EINVAL (NULL argument), ENODEV (no GPU), ENOMEM, EAGAIN (the device's queue is
 * full — wait for an earlier job — or no worker thread could be started). */
struct ebpf_batch_job;
int ebpf_prog_run_batch_async(struct ebpf_prog *ep, const struct ebpf_pkt_batch *batch,
			      uint64_t *ret, uint8_t *faults, struct ebpf_batch_job **job);
int ebpf_batch_wait(struct ebpf_batch_job *job, struct ebpf_batch_stats *stats);

/* Device-resident batch: every pointer (batch->data, batch->offsets, ret_dev, faults_dev,
 * hist_dev) is device memory on `device`.  Enqueued on `stream` (hipStream_t, NULL = default
 * stream) and returns without synchronising.  faults_dev / hist_dev may be NULL; hist_dev is
 * EBPF_HIST_BINS u64 counters that the kernel ADDS to (zero it yourself), or, with
 * EBPF_BATCH_HIST_OVERWRITE in batch->flags, sets to this batch's counts.
 * batch->data may have any alignment.  The staged kernel for fixed 64-byte packets reads them
 * 16 bytes a lane, so it runs only when data is 16-byte aligned; a 64-byte-stride batch on any
 * other base runs on the general kernel (ebpf_dexec_info.layout 0; same results).  ret_dev and
 * batch->offsets must be 8-byte aligned, as their types say. */
int ebpf_prog_run_batch_dev(struct ebpf_prog *ep, int device, const struct ebpf_pkt_batch *batch,
			    uint64_t *ret_dev, uint8_t *faults_dev, uint64_t *hist_dev,
			    void *stream);

/* One batch sharded over several GPUs of this process (packets are independent,
 * maps are read-only during a batch, so the batch splits into contiguous shards
 * [d*n/N, (d+1)*n/N) with no data exchange; bytecode and map mirrors are replicated per device).
 *
 * ebpf_prog_run_batch_multi: host buffers, as ebpf_prog_run_batch; one host thread per device
 *   runs its shard's chunked H2D -> kernel -> D2H pipeline.  `devices` may repeat a device (two
 *   shards then share it).  stats->hist is the sum of the shards' histograms, stats->kernel_ms
 *   the slowest shard's device time.
 * ebpf_prog_run_batch_multi_dev: device-resident, asynchronous: shards[d], ret_dev[d],
 *   faults_dev[d] (optional), hist_dev[d] (optional) live on devices[d] and each launch is
 *   enqueued on streams[d] (NULL array = default streams).  `devices` may repeat a device.  With
 *   hist_dev, the batch's histogram — the SUM over all shards — is added to each hist_dev[d], or
 *   stored into it when shards[d].flags has EBPF_BATCH_HIST_OVERWRITE, as ebpf_prog_run_batch_dev
 *   does for one shard.  The sum is formed in library-owned scratch (the shards of one device
 *   summed on the first one's stream, then one RCCL all-reduce (uint64, sum) over the distinct
 *   devices: the path's only collective); streams[d] sees hist_dev[d] complete in stream order.
 *   Returns ENOSYS if several distinct devices are given and RCCL (librccl.so.1) cannot be
 *   loaded.
 * Neither changes the calling thread's current HIP device (no entry point of this header does).
 * Both return 0 or an errno (ENODEV: a device index out of range; EINVAL: bad arguments). */
int ebpf_prog_run_batch_multi(struct ebpf_prog *ep, int ndev, const int *devices,
			      const struct ebpf_pkt_batch *batch, uint64_t *ret, uint8_t *faults,
			      struct ebpf_batch_stats *stats);
int ebpf_prog_run_batch_multi_dev(struct ebpf_prog *ep, int ndev, const int *devices,
				  const struct ebpf_pkt_batch *shards, uint64_t *const *ret_dev,
				  uint8_t *const *faults_dev, uint64_t *const *hist_dev,
				  void *const *streams);

/* Steering a batch by verdict: the step after ret[] for a caller that acts on verdicts (a switch
 * whose verdict is the destination port, a classifier, a drop / pass filter).  The histogram
 * says how many packets went to each class; these functions say which, without per-packet data
 * crossing to the host:
 *
 *   ebpf_prog_run_batch_dev(ep, dev, &batch, ret, faults, hist, s);
 *   ebpf_batch_steer_dev(dev, ret, faults, batch.count, index, starts, s);
 *   (read starts — 258 words — or a class's two entries)
 *   ebpf_batch_select_dev(dev, &batch, index + starts[b], starts[b+1] - starts[b], extents, s);
 *   sub = {batch.data, extents, starts[b+1] - starts[b], 0, EBPF_BATCH_EXTENTS};
 *   ebpf_prog_run_batch_dev(ep2, dev, &sub, ret2, faults2, hist2, s);
 *
 * Classes are the histogram's bins: packet i is of class 256 if faults is given and faults[i]
 * != 0, else of class min(ret[i], 255).  A faulted packet's ret is 0, so without faults
 * (NULL) faulted packets fall into class 0 together with the packets that returned 0.
 * The result is a stable partition: index[starts[b] .. starts[b+1]) holds the packets of class b
 * in ascending order; starts has EBPF_STEER_STARTS entries, starts[0] = 0 and
 * starts[EBPF_HIST_BINS] = count, so starts[b+1] - starts[b] is bin b of the histogram.  It is
 * a function of ret / faults alone: two calls on the same input give the same bytes.
 *
 * ebpf_batch_steer: host buffers, a plain counting sort; no GPU needed (the results of
 *   ebpf_prog_run_batch, and the statement of what the device function computes).
 * ebpf_batch_steer_dev: every pointer is device memory on `device`; enqueued on `stream`
 *   (hipStream_t, NULL = default stream), returns without synchronising; after the program's
 *   launch on the same stream it reads what that launch wrote.  Temporary storage is the
 *   library's, per stream, grown on demand (1 KiB per 4,096 packets).  ret_dev and starts_dev
 *   must be 8-byte aligned, index_dev 4-byte aligned, as their types say.
 * Both return 0; EINVAL for a NULL starts, or a NULL ret or index with count > 0 (count == 0:
 * starts becomes all zeros); E2BIG for count > 0xffffffff (the packet index is 32 bits).  The
 * device function then returns ENODEV (no GPU, or no such device), ENOMEM (no scratch) or EIO.
 *
 * ebpf_batch_select_dev: a list of n packets of `batch` (any list: a class of a steered batch,
 *   several classes, a list of the caller's own) as an extents batch over the same data.  For
 *   j < n, extents_dev[2j], extents_dev[2j+1] = (start, end) of packet index_dev[j] relative to
 *   batch->data, whatever form `batch` has: i * stride and (i + 1) * stride, offsets[i] and
 *   offsets[i+1], or the pair offsets[2i], offsets[2i+1] as it stands.  An index >= batch->count
 *   gives (0, 0), a packet of length 0.  {batch->data, extents_dev, n, 0, EBPF_BATCH_EXTENTS} is
 *   then a batch for any entry point that takes device pointers; no packet byte is moved.  An
 *   extents batch runs on the general kernels even when `batch` was a 16-byte-aligned
 *   64-byte-stride batch that took the staged kernel.  batch->offsets, index_dev and extents_dev
 *   are device memory on `device`; batch->data is not read.  Asynchronous on `stream` as above.
 *   Returns 0; EINVAL (a batch that the run functions would refuse, or a NULL index or extents
 *   with n > 0); ENODEV; EIO.
 * None of the three changes the calling thread's current HIP device. */
#define EBPF_STEER_STARTS (EBPF_HIST_BINS + 1)
int ebpf_batch_steer(const uint64_t *ret, const uint8_t *faults, uint64_t count, uint32_t *index,
		     uint64_t *starts);
int ebpf_batch_steer_dev(int device, const uint64_t *ret_dev, const uint8_t *faults_dev,
			 uint64_t count, uint32_t *index_dev, uint64_t *starts_dev, void *stream);
int ebpf_batch_select_dev(int device, const struct ebpf_pkt_batch *batch, const uint32_t *index_dev,
			  uint64_t n, uint64_t *extents_dev, void *stream);

/* Grouping a batch by key: steering for a verdict with more values than the histogram has bins (a
 * load balancer's backend id, an RSS queue number, a flow hash whose packets a stateful second
 * stage wants side by side in arrival order, an action packed beside a target).  The packets are
 * sorted, stably, by a bit field of ret, and a table says where every group of equal keys begins:
 *
 *   ebpf_prog_run_batch_dev(ep, dev, &batch, ret, faults, hist, s);
 *   ebpf_batch_group_dev(dev, ret, faults, batch.count, 0, 32, index, cap, keys, starts, info,
 *                        tmp, ebpf_batch_group_tmp_bytes(batch.count, 32), s);
 *   ebpf_batch_gather_dev(dev, &batch, index, batch.count, 64, out, ...);   (flows side by side)
 *
 * Key: the key of packet i is (ret[i] >> key_shift) & (2^key_bits - 1), with 1 <= key_bits <= 64
 *   and key_shift + key_bits <= 64.  Bits of ret outside the field take no part, neither in the
 *   order nor in deciding where a group ends.  Keys compare as unsigned numbers.
 * Faulted packets: packet i is faulted iff faults is given and faults[i] != 0; its ret is then
 *   not looked at, even where it is not 0.  With faults NULL no packet is faulted.
 * Order: let U be the number of unfaulted packets.  index[0 .. U) holds them in ascending key
 *   order, packets of equal key in ascending packet order (a stable sort: a flow's packets keep
 *   their arrival order); index[U .. count) holds the faulted packets in ascending packet order.
 *   index has count entries and is always written in full.
 * Groups: a group is a maximal run of equal keys within index[0 .. U); let G be their number.
 *   info has 2 entries, always written: info[0] = G, info[1] = U.  group_starts has group_cap + 1
 *   entries and group_keys has group_cap.  For g < min(G, group_cap), group_keys[g] is the key of
 *   group g (the field's value, shifted down) and group_starts[g] its first position in index; if
 *   G <= group_cap then group_starts[G] = U as well, so group g is index[group_starts[g] ..
 *   group_starts[g + 1]).  No other entry is written: none at or past min(G, group_cap) of
 *   group_keys, none past min(G, group_cap) of group_starts, and group_starts[G] only when G <=
 *   group_cap.  The table is complete iff info[0] <= group_cap (snprintf's rule, as the packed
 *   gather's).  group_keys may be NULL: keys are then not written.  group_cap == 0 with
 *   group_keys NULL only sorts and counts; group_starts then still has its one entry, written
 *   (with U) iff G == 0, unless it is NULL too.
 * The output is a function of the inputs alone: two calls on the same input give the same bytes.
 * A group's list, or the whole index, is "any list" for ebpf_batch_select_dev,
 * ebpf_batch_gather_dev, ebpf_batch_scatter_dev and ebpf_batch_merge_dev.
 *
 * ebpf_batch_group: host buffers, a plain stable sort; no GPU needed (the statement of what the
 *   device function computes).  Returns ENOSPC when G > group_cap, with index, info and every
 *   table entry that fits written.
 * ebpf_batch_group_dev: every pointer is device memory on `device`; enqueued on `stream`
 *   (hipStream_t, NULL = default stream), returns without synchronising and never waits for the
 *   device, so a short table returns 0 and the caller compares info_dev[0] with its cap after the
 *   stream.  A radix sort over digits of at most 8 bits, least significant first: ceil(key_bits /
 *   8) passes, each moving every packet's key and index once.  tmp_dev is the caller's: at least
 *   ebpf_batch_group_tmp_bytes(count, key_bits) bytes, 8-byte aligned, any contents on entry and
 *   on return; it must outlive the call's work on the stream and may then be reused or freed.
 *   Neither tmp_dev nor index_dev may overlap ret_dev, faults_dev, each other or the tables.  The
 *   small per-tile tables (about 1 KiB per 4,096 packets) are the library's, per stream, shared
 *   with ebpf_batch_steer_dev.  ret_dev, group_keys_dev, group_starts_dev and info_dev must be
 *   8-byte aligned, index_dev 4-byte aligned, as their types say.
 * ebpf_batch_group_tmp_bytes: host only, no GPU needed, a pure function:
 *     n = count rounded up to a multiple of 64;  w = 4 if key_bits <= 32, else 8 (bytes a key)
 *     n * w               if key_bits <= 8  (one pass: the sorted keys)
 *     n * (2 * w + 4)     otherwise         (two key buffers and a second index buffer)
 *   so at most 2 * (8 + 4) bytes a packet plus 2 * (8 + 4) * 63; 0 for count == 0, and 0 for
 *   arguments the other two functions refuse (key_bits outside [1, 64], count > 0xffffffff).
 * Both return 0; EINVAL for key_bits outside [1, 64] or key_shift + key_bits > 64, a NULL info,
 * a NULL ret or index with count > 0, a NULL group_starts with group_cap > 0; then E2BIG for
 * count > 0xffffffff (the packet index is 32 bits).  count == 0 succeeds: info = {0, 0}, and
 * group_starts[0] = 0 if group_starts is given.  The device function then returns ENOSPC for
 * tmp_bytes below ebpf_batch_group_tmp_bytes(count, key_bits), EINVAL for a NULL tmp_dev where
 * that is not 0 — both known on the host, before the device is looked at and before any launch —
 * then ENODEV (no GPU, or no such device), ENOMEM (no scratch) or EIO.  Neither changes the
 * calling thread's current HIP device. */
size_t ebpf_batch_group_tmp_bytes(uint64_t count, uint32_t key_bits);
int ebpf_batch_group(const uint64_t *ret, const uint8_t *faults, uint64_t count,
		     uint32_t key_shift, uint32_t key_bits, uint32_t *index,
		     uint64_t group_cap, uint64_t *group_keys, uint64_t *group_starts,
		     uint64_t *info);
int ebpf_batch_group_dev(int device, const uint64_t *ret_dev, const uint8_t *faults_dev,
			 uint64_t count, uint32_t key_shift, uint32_t key_bits,
			 uint32_t *index_dev, uint64_t group_cap, uint64_t *group_keys_dev,
			 uint64_t *group_starts_dev, uint64_t *info_dev,
			 void *tmp_dev, size_t tmp_bytes, void *stream);

/* Reducing a list per segment: how much each group carried.  Once flows lie side by side (a
 * grouped index) or classes do (a steering index), these functions reduce, per group or class, the
 * packets' lengths and a bit field of their verdicts, without per-packet data crossing to the
 * host: bytes per flow or per steering class, the OR of a flags field over a flow, a flow's
 * largest sequence number, the sum of a payload-length field per backend:
 *
 *   ebpf_batch_group_dev(dev, ret, faults, batch.count, 0, 32, index, cap, keys, starts, info,
 *                        tmp, tmp_bytes, s);
 *   sums = {bytes, sum, NULL, max, NULL};                          (cap entries each)
 *   ebpf_batch_reduce_dev(dev, &batch, ret, batch.count, 32, 16, index, batch.count, starts, cap,
 *                         info, &sums, s);
 *   (read info and the sums' first min(info[0], cap) entries)
 *
 * List and segments: index[0 .. n) is any list of packets of the batch — a grouped index, a
 *   steering index, the caller's own; duplicates and any order are fine.  Segment g is
 *   index[seg_starts[g] .. seg_starts[g + 1]).  The number R of segments reduced is seg_cap when
 *   nseg is NULL (the steering case: seg_starts = starts, seg_cap = EBPF_HIST_BINS); else *nseg
 *   when *nseg <= seg_cap; else seg_cap - 1 (0 for seg_cap == 0): a short group table holds no end
 *   for its last group.  So ebpf_batch_group_dev's group_starts, group_cap and info (as nseg) plug
 *   in as they stand, after it on the same stream, with nothing read on the host, and the result
 *   is complete iff info[0] <= group_cap, as the table's is.  seg_starts[0 .. R] is read: it is
 *   non-decreasing and seg_starts[R] <= n.  Entries at or past R of any output are not written.
 *   Positions of the list that no segment covers take no part: those before seg_starts[0] and
 *   those at or past seg_starts[R] (the faulted tail [U, count) of a grouped index).
 * Per listed entry j, with i = index[j]: its length is the gather's len_j (the batch's packet i by
 *   the run functions' rule: 0 for an end below the start or 2^32 bytes or more past it, and 0 for
 *   i >= count); its value is (ret[i] >> val_shift) & (2^val_bits - 1), with 1 <= val_bits <= 64
 *   and val_shift + val_bits <= 64.  An entry with i >= count has no value: it is left out of sum,
 *   min, max and bits.  faults is not consulted: a faulted packet's ret is what the run functions
 *   left there.
 * Outputs (struct ebpf_batch_sums): each member is NULL (not wanted: it costs nothing) or has
 *   seg_cap entries.  For g < R: bytes[g] = the sum of the segment's lengths; sum[g] = the sum of
 *   its values modulo 2^64; min[g], max[g] = its smallest and largest value as unsigned numbers;
 *   bits[g] = the OR of its values.  A segment with no entry, or no entry that has a value, gives
 *   the identities: bytes 0, sum 0, min UINT64_MAX, max 0, bits 0.
 * Which arguments may be NULL: batch iff out->bytes is NULL; ret iff sum, min, max and bits all
 *   are; with all five NULL the call succeeds and does nothing.  batch->data is never read, and
 *   of batch->offsets only the listed packets' entries.
 * The output is a function of the inputs alone: it does not depend on what the output arrays held
 * on entry, and two calls on the same input give the same bytes.
 *
 * ebpf_batch_reduce: host buffers, a plain loop per segment; no GPU needed (the statement of what
 *   the device function computes).  It also returns EINVAL, with nothing written, when
 *   seg_starts[0 .. R] is not non-decreasing or seg_starts[R] > n.
 * ebpf_batch_reduce_dev: every pointer (batch->offsets, ret_dev, index_dev, seg_starts_dev,
 *   nseg_dev and the members of *out; batch and out themselves are host structs) is device memory
 *   on `device`; enqueued on `stream` (hipStream_t, NULL = default stream), returns without
 *   synchronising and never waits for the device.  It cannot look at the table: for one that is
 *   not non-decreasing or that ends past n, the first R entries of the outputs are unspecified,
 *   but every position is clamped to n: nothing outside index[0 .. n), ret[0 .. count), the listed
 *   packets' offsets entries and seg_starts[0 .. R] is read, and nothing but those output entries
 *   is written.  The cost follows the list's length and the table's, not the shape of the
 *   segments: one segment over the whole list, n segments of one entry and thousands of empty
 *   segments at one position take about the time of the reads.  Temporary storage is the
 *   library's, per stream, shared with ebpf_batch_steer_dev and ebpf_batch_group_dev: 96 bytes per
 *   4,096 list entries.  The outputs may not overlap the inputs or each other.  ret_dev,
 *   seg_starts_dev, nseg_dev, batch->offsets and the outputs must be 8-byte aligned, index_dev
 *   4-byte aligned, as their types say.
 * Both return 0; EINVAL for a NULL out, for val_bits outside [1, 64] or val_shift + val_bits > 64
 * when ret is used (sum, min, max or bits wanted), a NULL ret or batch where an output needs it, a
 * batch that the run functions would refuse, batch->count != count when batch is given, a NULL
 * index with n > 0, a NULL seg_starts with seg_cap > 0; then E2BIG for n, count or seg_cap above
 * 0xffffffff.  All of these are known on the host, before the device is looked at.  The device
 * function then returns ENODEV (no GPU, or no such device), ENOMEM (no scratch) or EIO.  Neither
 * changes the calling thread's current HIP device. */
struct ebpf_batch_sums {   /* each NULL (not wanted) or seg_cap entries */
	uint64_t *bytes;   /* sum of the listed packets' lengths */
	uint64_t *sum;     /* sum of the value field, modulo 2^64 */
	uint64_t *min;     /* smallest value, unsigned; UINT64_MAX for no value */
	uint64_t *max;     /* largest value, unsigned; 0 for no value */
	uint64_t *bits;    /* OR of the values */
};
int ebpf_batch_reduce(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
		      uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
		      const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		      const struct ebpf_batch_sums *out);
int ebpf_batch_reduce_dev(int device, const struct ebpf_pkt_batch *batch, const uint64_t *ret_dev,
			  uint64_t count, uint32_t val_shift, uint32_t val_bits,
			  const uint32_t *index_dev, uint64_t n, const uint64_t *seg_starts_dev,
			  uint64_t seg_cap, const uint64_t *nseg_dev,
			  const struct ebpf_batch_sums *out, void *stream);

/* Running totals per segment: where a packet stands inside its group.  The per-position
 * counterpart of the reduce: for every position of the list, how many entries of its segment came
 * before it, how many bytes they carried and what their values add up to, in list order (a
 * grouped index keeps a flow's packets in arrival order), and whether the entry passes a byte
 * budget of its segment.  A byte quota per flow or backend with tail drop in arrival order, "the
 * first K packets of every flow", a running sequence offset:
 *
 *   ebpf_batch_group_dev(dev, ret, faults, batch.count, 0, 32, index, cap, keys, starts, info,
 *                        tmp, tmp_bytes, s);
 *   scans = {rank, NULL, NULL, over};                              (batch.count entries each)
 *   ebpf_batch_scan_dev(dev, &batch, NULL, batch.count, 0, 0, index, batch.count, starts, cap,
 *                       info, budgets, &scans, s);
 *   (packet index[j] is within its flow's quota iff over[j] == 0; rank[j] < K samples a flow)
 *
 * List, segments and R: exactly as for ebpf_batch_reduce.  index[0 .. n) is any list of packets
 *   of the batch; segment g is index[seg_starts[g] .. seg_starts[g + 1]); R is seg_cap when nseg is
 *   NULL, else *nseg when *nseg <= seg_cap, else seg_cap - 1 (0 for seg_cap == 0).
 *   ebpf_batch_group_dev's group_starts, group_cap and info (as nseg) plug in as they stand, after
 *   it on the same stream; so does a steering table.  seg_starts[0 .. R] is read: it is
 *   non-decreasing and seg_starts[R] <= n.
 * Per position j of segment g (seg_starts[g] <= j < seg_starts[g + 1], g < R), with i = index[j],
 *   len_j and the value as the reduce has them (the length 0 for an end below the start, for an
 *   end 2^32 bytes or more past it and for i >= count; the value (ret[i] >> val_shift) &
 *   (2^val_bits - 1), and an entry with i >= count has none and adds 0):
 *     rank[j]         = j - seg_starts[g]: the entries of the segment before this one;
 *     bytes_before[j] = the sum of their lengths;
 *     sum_before[j]   = the sum of their values, modulo 2^64;
 *     over[j]         = 1 iff bytes_before[j] + len_j > budgets[g], else 0 (the sum cannot wrap: at
 *                       most 2^32 entries of less than 2^32 bytes each).
 *   budgets has seg_cap entries, of which [0, R) are read.  So for the last position of a segment
 *   bytes_before + len_j is the reduce's bytes[g], and the same for sum.  faults is not consulted.
 * Positions that no segment covers, those before seg_starts[0] and those at or past seg_starts[R]
 *   (the faulted tail of a grouped index; every position when R == 0): every wanted output is 0
 *   there.  So every wanted output is written in full, [0, n), and nothing at or past entry n is.
 * Outputs (struct ebpf_batch_scans): each member is NULL (not wanted: it costs nothing) or has n
 *   entries, by list position.
 * Which arguments may be NULL: batch iff bytes_before and over both are; ret iff sum_before is;
 *   budgets iff over is; with all four outputs NULL the call succeeds and does nothing.
 *   batch->data is never read, and of batch->offsets only the listed packets' entries.
 * The output is a function of the inputs alone: it does not depend on what the output arrays held
 * on entry, and two calls on the same input give the same bytes.
 *
 * ebpf_batch_scan: host buffers, a plain loop; no GPU needed (the statement of what the device
 *   function computes).  It also returns EINVAL, with nothing written, when seg_starts[0 .. R] is
 *   not non-decreasing or seg_starts[R] > n.
 * ebpf_batch_scan_dev: every pointer (batch->offsets, ret_dev, index_dev, seg_starts_dev,
 *   nseg_dev, budgets_dev and the members of *out; batch and out themselves are host structs) is
 *   device memory on `device`; enqueued on `stream` (hipStream_t, NULL = default stream), returns
 *   without synchronising and never waits for the device.  It cannot look at the table: for one
 *   that is not non-decreasing or that ends past n the outputs are unspecified, but nothing
 *   outside index[0 .. n), ret[0 .. count), the listed packets' offsets entries, seg_starts[0 .. R]
 *   and budgets[0 .. R) is read, and nothing outside the outputs' [0, n) is written.  The cost
 *   follows the list's length, not the shape of the segments; a budget is fetched once per segment
 *   and tile of 4,096 positions that the segment touches, not per position.  Temporary storage
 *   is the library's, per stream, shared with ebpf_batch_steer_dev, ebpf_batch_group_dev and
 *   ebpf_batch_reduce_dev: 72 bytes per 4,096 list entries (none for rank alone).  The outputs
 *   may not overlap the inputs or each other.  ret_dev, seg_starts_dev, nseg_dev, budgets_dev,
 *   batch->offsets, bytes_before and sum_before must be 8-byte aligned, index_dev and rank 4-byte
 *   aligned, as their types say; over may have any alignment.
 * Both return 0; EINVAL for a NULL out, for val_bits outside [1, 64] or val_shift + val_bits > 64
 * when sum_before is wanted, a NULL ret, batch or budgets where an output needs it, a batch that
 * the run functions would refuse, batch->count != count when batch is given, a NULL index with
 * n > 0, a NULL seg_starts with seg_cap > 0; then E2BIG for n, count or seg_cap above 0xffffffff.
 * All of these are known on the host, before the device is looked at.  The device function then
 * returns ENODEV (no GPU, or no such device), ENOMEM (no scratch) or EIO.  Neither changes the
 * calling thread's current HIP device. */
struct ebpf_batch_scans {      /* each NULL (not wanted: it costs nothing) or n entries, by list position */
	uint32_t *rank;         /* entries of the same segment before this one */
	uint64_t *bytes_before; /* sum of their lengths */
	uint64_t *sum_before;   /* sum of their values, modulo 2^64 */
	uint8_t  *over;         /* 1 iff bytes_before + own length > the segment's budget */
};
int ebpf_batch_scan(const struct ebpf_pkt_batch *batch, const uint64_t *ret, uint64_t count,
		    uint32_t val_shift, uint32_t val_bits, const uint32_t *index, uint64_t n,
		    const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		    const uint64_t *budgets, const struct ebpf_batch_scans *out);
int ebpf_batch_scan_dev(int device, const struct ebpf_pkt_batch *batch, const uint64_t *ret_dev,
			uint64_t count, uint32_t val_shift, uint32_t val_bits,
			const uint32_t *index_dev, uint64_t n, const uint64_t *seg_starts_dev,
			uint64_t seg_cap, const uint64_t *nseg_dev, const uint64_t *budgets_dev,
			const struct ebpf_batch_scans *out, void *stream);

/* Keeping part of a list: a stable compaction that carries the segments along.  The scan leaves
 * flags and ranks per list position; this turns them, or a bit field of the verdicts, into lists
 * that every other list function takes — the entries that pass a test (kept) and those that do
 * not (dropped), each in list order, each with a table of its own — with nothing per packet read
 * on the host.  A byte quota per flow, what passed forwarded and what was dropped counted per flow:
 *
 *   scans = {rank, NULL, NULL, over};
 *   ebpf_batch_scan_dev(dev, &batch, NULL, batch.count, 0, 0, index, batch.count, starts, cap,
 *                       info, budgets, &scans, s);
 *   test = {over, NULL, 0, NULL, 0, 0, 0, 0};       (test = {NULL, rank, K, ...}: K packets a flow)
 *   parts = {kept, kept_starts, dropped, dropped_starts};
 *   ebpf_batch_filter_dev(dev, &test, batch.count, index, batch.count, starts, cap, info, &parts,
 *                         kd, s);
 *   ebpf_batch_gather_dev(dev, &batch, kept, batch.count, 64, out, ...);   (slots past kd[0]: zeros)
 *   sums = {bytes, NULL, NULL, NULL, NULL};
 *   ebpf_batch_reduce_dev(dev, &batch, NULL, batch.count, 0, 0, dropped, batch.count,
 *                         dropped_starts, cap, info, &sums, s);
 *
 * List, segments and R: exactly as for ebpf_batch_reduce and ebpf_batch_scan.  index[0 .. n) is any
 *   list of packets of the batch; R is seg_cap when nseg is NULL, else *nseg when *nseg <= seg_cap,
 *   else seg_cap - 1 (0 for seg_cap == 0).  ebpf_batch_group_dev's group_starts, group_cap and info
 *   (as nseg) plug in as they stand, after it on the same stream; so does a steering table.
 *   seg_starts[0 .. R] is read: it is non-decreasing and seg_starts[R] <= n.  A position j takes
 *   part iff a segment covers it: seg_starts[0] <= j < min(seg_starts[R], n); with R == 0 (a
 *   non-NULL seg_starts with seg_cap == 0 included) nothing takes part.
 *   seg_starts == NULL is an unsegmented list: it needs seg_cap == 0 and nseg == NULL, every
 *   position of [0, n) takes part, and kept_starts and dropped_starts must be NULL.
 * Test (struct ebpf_batch_test): a conjunction; a NULL member is no test.  A position j that takes
 *   part passes iff every given member's test holds, with i = index[j]:
 *     flags (n entries, by list position):  flags[j] == 0;
 *     rank  (n entries, by list position):  rank[j] < rank_below;
 *     ret   (count entries, by packet):     i < count and val_lo <= v <= val_hi as unsigned
 *           numbers, v = (ret[i] >> val_shift) & (2^val_bits - 1), 1 <= val_bits <= 64 and
 *           val_shift + val_bits <= 64.  An entry with i >= count has no value: it fails.
 *           val_lo > val_hi is legal: nothing passes.
 *   With all three NULL every position that takes part passes.  faults is not consulted.
 * Outputs (struct ebpf_batch_parts): each member is NULL (not wanted: it costs nothing).  Let K be
 *   the number of positions that take part and pass, D the number that take part and fail.
 *     info[0] = K, info[1] = D: 2 entries, always written.
 *     kept[0 .. K) = index[j] of the passing positions, in list order (a stable compaction);
 *       kept[K .. n) = EBPF_NO_PACKET.  n entries, written in full, as the group's index is:
 *       every list function treats an entry >= count as a packet of length 0 that has no value
 *       and is never written to, so (kept, n) is a list as it stands.
 *     dropped[0 .. D) likewise of the failing positions; dropped[D .. n) = EBPF_NO_PACKET.
 *     kept_starts[g], for g <= R = the number of passing positions j with
 *       seg_starts[0] <= j < min(seg_starts[g], n).  So kept_starts[0] = 0, kept_starts[R] = K, and
 *       segment g of the kept list is kept[kept_starts[g] .. kept_starts[g + 1]), maybe empty:
 *       (kept, n, kept_starts, seg_cap, nseg) is a list with a table for ebpf_batch_reduce_dev and
 *       ebpf_batch_scan_dev, after this call on the same stream with the same seg_cap and nseg.
 *       seg_cap + 1 entries, of which [0 .. R] are written; entries past R are not.
 *     dropped_starts[g] likewise of the failing positions; dropped_starts[R] = D.
 *   With all four NULL only info is written (a count).  n == 0 succeeds: info = {0, 0} and the
 *   tables' [0 .. R] are 0.
 * The output is a function of the inputs alone: it does not depend on what the outputs held on
 * entry, and two calls on the same input give the same bytes.  The outputs may not overlap the
 * inputs or each other.
 *
 * ebpf_batch_filter: host buffers, a plain loop; no GPU needed (the statement of what the device
 *   function computes).  It also returns EINVAL, with nothing written, when seg_starts[0 .. R] is
 *   not non-decreasing or seg_starts[R] > n.
 * ebpf_batch_filter_dev: every pointer (the members of *test and *out, index_dev, seg_starts_dev,
 *   nseg_dev and info_dev; test and out themselves are host structs) is device memory on
 *   `device`; enqueued on `stream` (hipStream_t, NULL = default stream), returns without
 *   synchronising and never waits for the device.  It cannot look at the table: for one that is
 *   not non-decreasing or that ends past n the outputs are unspecified, but every position is
 *   clamped: nothing outside flags[0 .. n), rank[0 .. n), index[0 .. n), ret[0 .. count) and
 *   seg_starts[0 .. R] is read, and nothing outside kept[0 .. n), dropped[0 .. n), the tables'
 *   [0 .. R] and info[0 .. 2) is written.  The cost follows the list's length and the table's, not
 *   the shape of the segments or how many entries pass.  Temporary storage is the library's, per
 *   stream, shared with ebpf_batch_steer_dev, ebpf_batch_group_dev, ebpf_batch_reduce_dev and
 *   ebpf_batch_scan_dev: 516 bytes per 4,096 list entries (a bit per position and a count per
 *   tile) and 16 bytes a call.  rank, index_dev, kept and dropped must be 4-byte aligned, ret,
 *   seg_starts_dev, nseg_dev, info_dev and the tables 8-byte aligned, as their types say; flags may
 *   have any alignment.
 * Both return 0; EINVAL for a NULL test, out or info, for val_bits outside [1, 64] or val_shift +
 * val_bits > 64 when test->ret is given, a NULL index with n > 0, a NULL seg_starts with
 * seg_cap > 0 or with nseg given, kept_starts or dropped_starts given with a NULL seg_starts; then
 * E2BIG for n, count or seg_cap above 0xffffffff.  All of these are known on the host, before the
 * device is looked at.  The device function then returns ENODEV (no GPU, or no such device),
 * ENOMEM (no scratch) or EIO.  Neither changes the calling thread's current HIP device. */
#define EBPF_NO_PACKET 0xffffffffu  /* a list entry that names no packet: >= any count */

struct ebpf_batch_test {      /* a conjunction; a NULL member is no test */
	const uint8_t  *flags;    /* n entries by list position: passes iff flags[j] == 0        */
	const uint32_t *rank;     /* n entries by list position: passes iff rank[j] < rank_below */
	uint32_t        rank_below;
	const uint64_t *ret;      /* count entries by packet: passes iff index[j] < count and    */
	uint32_t        val_shift, val_bits;   /* val_lo <= (ret[i] >> val_shift) & mask <= val_hi */
	uint64_t        val_lo, val_hi;
};
struct ebpf_batch_parts {     /* each NULL (not wanted: it costs nothing) */
	uint32_t *kept;           /* n entries, written in full */
	uint64_t *kept_starts;    /* seg_cap + 1 entries, [0 .. R] written */
	uint32_t *dropped;        /* n entries, written in full */
	uint64_t *dropped_starts; /* seg_cap + 1 entries, [0 .. R] written */
};
int ebpf_batch_filter(const struct ebpf_batch_test *test, uint64_t count, const uint32_t *index,
		      uint64_t n, const uint64_t *seg_starts, uint64_t seg_cap, const uint64_t *nseg,
		      const struct ebpf_batch_parts *out, uint64_t *info);
int ebpf_batch_filter_dev(int device, const struct ebpf_batch_test *test, uint64_t count,
			  const uint32_t *index_dev, uint64_t n, const uint64_t *seg_starts_dev,
			  uint64_t seg_cap, const uint64_t *nseg_dev,
			  const struct ebpf_batch_parts *out, uint64_t *info_dev, void *stream);

/* Carrying totals across batches: a table keyed by the flow key, kept on the device.  A group
 * number is a position in one batch's group_keys; what outlives the batch — the bytes a flow has
 * used of a quota, a per-flow counter, a "last seen" stamp — is kept by key, in a sorted table:
 * keys strictly ascending as unsigned numbers, a value beside each.  A batch's group_keys are
 * strictly ascending too (a radix sort wrote them), so looking a batch up in the table and folding
 * a batch's per-group sums into it are merges of two sorted sequences: no hashing, no atomics, no
 * insertion order.  A byte quota per flow that holds across batches, with tables cur and next:
 *
 *   ebpf_batch_group_dev(dev, ret, faults, batch.count, 0, 32, index, cap, keys, starts, info,
 *                        tmp, tmp_bytes, s);
 *   ebpf_batch_lookup_dev(dev, &cur, keys, cap, info, EBPF_LOOKUP_REMAINING, 0, quota, budgets,
 *                         NULL, s);                    (budgets[g] = quota - the bytes used, or 0)
 *   ebpf_batch_scan_dev(... budgets, &scans, s);  ebpf_batch_filter_dev(... over ... &parts, kd, s);
 *   sums = {bytes, NULL, NULL, NULL, NULL};
 *   ebpf_batch_reduce_dev(dev, &batch, NULL, batch.count, 0, 0, kept, batch.count, kept_starts,
 *                         cap, info, &sums, s);        (bytes[g] = what flow g sent in this batch)
 *   ebpf_batch_accumulate_dev(dev, &cur, keys, bytes, cap, info, EBPF_ACC_ADD, 0, UINT64_MAX,
 *                             &next, tinfo, s);        (then swap cur and next)
 *
 * The table (struct ebpf_key_table, a host struct): keys and vals have cap entries each, vals[p]
 *   belongs to keys[p], and *n is the number of keys the table has, or would need (snprintf's
 *   rule).  N = min(*n, cap) entries are valid and keys[0 .. N) is strictly ascending.  A table that
 *   an accumulate left short (*n > cap) is its first cap entries, as a short group table is.  An
 *   empty table is *n == 0.  keys and vals may be NULL iff cap == 0; so may n, which then reads as
 *   0 and is not written.  cap is at most 0xffffffff: a table position is 32 bits.
 * The batch's side: keys has key_cap entries, of which R are used, exactly the R of
 *   ebpf_batch_reduce: key_cap when nkeys is NULL, else *nkeys when *nkeys <= key_cap, else
 *   key_cap - 1 (0 for key_cap == 0).  So ebpf_batch_group_dev's group_keys, group_cap and info,
 *   and the members of the ebpf_batch_sums of a reduce that followed it, plug in as they stand,
 *   after those calls on the same stream: entry g of each belongs to the same flow.
 *
 * Lookup, for g < R: p = the position of keys[g] in the table, if it is there;
 *     pos_out[g]  = p, or EBPF_NO_ENTRY when it is not;
 *     v           = table->vals[p], or `missing` when it is not;
 *     vals_out[g] = v for EBPF_LOOKUP_VALUE; for EBPF_LOOKUP_REMAINING limit - v when v < limit,
 *                   else 0.  With a table of the bytes used per flow and missing = 0 that is the
 *                   scan's budgets.
 *   Entries at or past R of either output are not written.  Either output may be NULL: it is not
 *   wanted and costs nothing; with both NULL the call succeeds and does nothing.  The looked-up
 *   keys may be in any order and may repeat; only the table must be sorted.
 *
 * Accumulate: keys[0 .. R) is strictly ascending and adds[g] belongs to keys[g].  The candidates
 *   are the union of the N keys of `in` and the batch's R keys, in ascending key order; a
 *   candidate's value is
 *     in->vals[p] op adds[g]  for a key in both (keys[g] == in->keys[p]),
 *     in->vals[p]             for a key in the table alone,
 *     adds[g]                 for a key in the batch alone,
 *   with op one of EBPF_ACC_ADD (modulo 2^64), EBPF_ACC_MIN, EBPF_ACC_MAX (unsigned) and
 *   EBPF_ACC_OR: the reduce's sum, min, max and bits.  A candidate is kept iff keep_lo <= value <=
 *   keep_hi as unsigned numbers: 0 and UINT64_MAX keep everything; keep_lo > keep_hi is legal and
 *   keeps nothing.  That is how a table stays bounded: a "last seen" table with EBPF_ACC_MAX and
 *   keep_lo = now - age forgets idle flows, and a call with R == 0 is a pure prune.  `in` NULL is an
 *   empty table.  With M the number of kept candidates:
 *     out->keys[0 .. min(M, out->cap)) and out->vals likewise hold the kept candidates in ascending
 *       key order; entries at or past min(M, out->cap) are not written;
 *     *out->n = M even when M > out->cap: the table is complete iff *out->n <= out->cap;
 *     info (3 entries, always written): info[0] = M; info[1] = the kept candidates whose key was
 *       not in `in`; info[2] = the candidates left out by the keep range.
 *   out (its arrays and n) may not overlap `in`, the batch's arrays or info: the caller keeps two
 *   tables and swaps them.
 * The output is a function of the inputs alone: it does not depend on what the outputs held on
 * entry, and two calls on the same input give the same bytes.
 *
 * ebpf_batch_lookup, ebpf_batch_accumulate: host buffers (the tables' pointers too), plain loops;
 *   no GPU needed (the statement of what the device functions compute).  Because they can look,
 *   they also return EINVAL, with nothing written, when a table's keys[0 .. N) is not strictly
 *   ascending, and the accumulate when keys[0 .. R) is not.  ebpf_batch_accumulate returns ENOSPC
 *   when M > out->cap, with everything that fits, *out->n and info written, as ebpf_batch_group
 *   does.
 * ebpf_batch_lookup_dev, ebpf_batch_accumulate_dev: every pointer inside the structs and every
 *   array (keys_dev, adds_dev, nkeys_dev, the outputs, info_dev; the structs themselves are host
 *   memory) is device memory on `device`; enqueued on `stream` (hipStream_t, NULL = default
 *   stream), they return without synchronising and never wait for the device.  A short output table
 *   returns 0: the caller compares info[0] with its cap after the stream.  They cannot look at the
 *   order of their inputs: for a table or, in the accumulate, keys that are not strictly ascending
 *   the outputs are unspecified, but every access is clamped: every search ends and stays inside its
 *   sequence whatever that holds; nothing outside the tables' [0, N), keys[0 .. R), adds[0 .. R),
 *   *n and *nkeys is read; and nothing outside vals_out[0 .. R), pos_out[0 .. R), out's
 *   [0, min(M', out->cap)) for the M' written to *out->n, *out->n and info[0 .. 3) is written.
 *   The cost follows cap and key_cap (the kernels are launched over them), not N and R.
 *   Temporary storage is the library's, per stream, shared with ebpf_batch_steer_dev,
 *   ebpf_batch_group_dev, ebpf_batch_reduce_dev, ebpf_batch_scan_dev and ebpf_batch_filter_dev:
 *   none for the lookup; for the accumulate 648 bytes per 4,096 entries of in->cap and per 4,096
 *   of key_cap (a bit per entry, a count per 64 entries and two per tile) and 32 bytes a call.
 *   Every array is 8-byte aligned, pos_out 4-byte aligned, as their types say.
 * All return 0; EINVAL for a NULL table or out, a NULL info, an unknown mode or op, NULL keys with
 * key_cap > 0, NULL adds with key_cap > 0, NULL keys, vals or n in a table with cap > 0; then E2BIG
 * for key_cap or a table's cap above 0xffffffff.  All of these are known on the host, before the
 * device is looked at.  The device functions then return ENODEV (no GPU, or no such device), ENOMEM
 * (no scratch) or EIO.  None changes the calling thread's current HIP device. */
#define EBPF_NO_ENTRY 0xffffffffu   /* pos_out of a key that the table does not hold */
#define EBPF_LOOKUP_VALUE     0u    /* vals_out[g] = v */
#define EBPF_LOOKUP_REMAINING 1u    /* vals_out[g] = v < limit ? limit - v : 0 */
#define EBPF_ACC_ADD 0u             /* modulo 2^64 */
#define EBPF_ACC_MIN 1u             /* unsigned */
#define EBPF_ACC_MAX 2u             /* unsigned */
#define EBPF_ACC_OR  3u

struct ebpf_key_table {   /* a host struct; the pointers are host memory for the host functions,
                             device memory on `device` for the _dev ones */
	uint64_t *keys;   /* cap entries; [0, N) strictly ascending as unsigned numbers */
	uint64_t *vals;   /* cap entries; vals[p] belongs to keys[p] */
	uint64_t  cap;
	uint64_t *n;      /* 1 entry: the number of keys the table has, or would need */
};
int ebpf_batch_lookup(const struct ebpf_key_table *table, const uint64_t *keys, uint64_t key_cap,
		      const uint64_t *nkeys, uint32_t mode, uint64_t missing, uint64_t limit,
		      uint64_t *vals_out, uint32_t *pos_out);
int ebpf_batch_lookup_dev(int device, const struct ebpf_key_table *table, const uint64_t *keys_dev,
			  uint64_t key_cap, const uint64_t *nkeys_dev, uint32_t mode,
			  uint64_t missing, uint64_t limit, uint64_t *vals_out_dev,
			  uint32_t *pos_out_dev, void *stream);
int ebpf_batch_accumulate(const struct ebpf_key_table *in, const uint64_t *keys,
			  const uint64_t *adds, uint64_t key_cap, const uint64_t *nkeys, uint32_t op,
			  uint64_t keep_lo, uint64_t keep_hi, const struct ebpf_key_table *out,
			  uint64_t *info);
int ebpf_batch_accumulate_dev(int device, const struct ebpf_key_table *in,
			      const uint64_t *keys_dev, const uint64_t *adds_dev, uint64_t key_cap,
			      const uint64_t *nkeys_dev, uint32_t op, uint64_t keep_lo,
			      uint64_t keep_hi, const struct ebpf_key_table *out, uint64_t *info_dev,
			      void *stream);

/* Rolling a table up: the entries of a keyed sequence reduced per key prefix, on the device.  The
 * tables above answer per exact key; the question is often one level up.  With dst << 32 | src as
 * the key, the entries under one dst are the distinct sources that reached it; a table of bytes
 * per host gives bytes per /24.  The keys are sorted, so the entries that share a prefix lie in one
 * run, and the result is again a sorted table: it goes to the top, a lookup, an accumulate or a
 * second rollup, on the same stream:
 *
 *   rolls = {dsts, nsrc, bytes, NULL, NULL, NULL, NULL};
 *   ebpf_batch_rollup_dev(dev, cur.keys, cur.vals, cur.cap, cur.n, 0, 32, 0, 64, out_cap, &rolls,
 *                         rinfo, s);           (per dst: its distinct sources, its bytes)
 *   ebpf_batch_top_dev(dev, dsts, nsrc, out_cap, rinfo, EBPF_TOP_LARGEST, 0, 64, 10, &tops, tinfo,
 *                      s);                     (the 10 destinations with the most sources)
 *   ebpf_batch_rollup_dev(dev, group_keys, bytes, group_cap, info, EBPF_ROLLUP_SEGMENTS, 8, 0, 64,
 *                         out_cap, &rolls, rinfo, s);     (this batch's hosts, per /24)
 *
 * Entries: ebpf_batch_top's rule.  keys and vals have cap entries each, of which N take part.
 *   n NULL: N = cap.  Otherwise N = min(*n, cap), the table's rule; with EBPF_ROLLUP_SEGMENTS N is
 *   the R of ebpf_batch_reduce (*n when *n <= cap, else cap - 1, and 0 for cap == 0).  So a table
 *   plugs in as (t.keys, t.vals, t.cap, t.n), a batch as (group_keys, a member of the reduce's
 *   sums, group_cap, the group's info) with the flag, each as it stands, after its producer on the
 *   same stream.  cap is at most 0xffffffff: a position is 32 bits.
 * Prefix: c(p) = keys[p] >> key_shift, 0 <= key_shift <= 63.  key_shift 0 is legal: over strictly
 *   ascending keys every entry is then its own run.
 * Runs: a run is a maximal stretch of adjacent positions of [0, N) with equal c: position p begins
 *   a run iff p == 0 or c(p) != c(p - 1).  That is defined for any keys, sorted or not, and neither
 *   function refuses any.  The output keys are strictly ascending, so that the output is a table,
 *   iff the input keys are non-decreasing.  C is the number of runs.
 * Value: v(p) = (vals[p] >> val_shift) & (2^val_bits - 1), 1 <= val_bits <= 64 and val_shift +
 *   val_bits <= 64, the reduce's field.  vals may be NULL iff sum, min, max and bits all are; the
 *   field is checked only when vals is used.
 * Outputs (struct ebpf_batch_rolls): each member is NULL (not wanted: it costs nothing) or has
 *   out_cap entries, starts out_cap + 1.  For run r < min(C, out_cap), of positions [a, b):
 *     keys[r] = c(a); count[r] = b - a (for a table: the distinct keys under the prefix);
 *     sum[r], min[r], max[r], bits[r] = the sum modulo 2^64, the smallest, the largest (unsigned)
 *       and the OR of v over [a, b);
 *     starts[r] = a.
 *   Entries at or past min(C, out_cap) are not written, but starts[C] = N is, iff C <= out_cap (the
 *   group table's rule: run r is positions [starts[r], starts[r + 1])).  Every run is reduced
 *   whole even when the outputs are short, so short outputs are a table by the table's rule: its
 *   first out_cap entries.
 *   info (2 entries, always written): info[0] = C even when C > out_cap (snprintf's rule: the
 *   outputs are complete iff info[0] <= out_cap); info[1] = N.  So (out->keys, out->count or
 *   out->sum ..., out_cap, info) is an ebpf_key_table with n = info.
 *   N == 0: info = {0, 0} and starts[0] = 0.  With all members NULL only info is written: the
 *   number of prefixes.  out_cap == 0 is legal, with members or without: nothing but info (and
 *   starts[0] for N == 0) is written.
 * The output is a function of the inputs alone: it does not depend on what the outputs held on
 * entry, and two calls on the same input give the same bytes.  The outputs may not overlap the
 * inputs or each other.
 *
 * ebpf_batch_rollup: host buffers, one pass; no GPU needed (the statement of what the device
 *   function computes).  It returns ENOSPC when C > out_cap, with everything that fits and info
 *   written, as ebpf_batch_group does.
 * ebpf_batch_rollup_dev: keys_dev, vals_dev, n_dev, the members of *out and info_dev (out itself
 *   is a host struct) are device memory on `device`, 8-byte aligned; enqueued on `stream`
 *   (hipStream_t, NULL = default stream), returns without synchronising and never waits for the
 *   device.  Short outputs return 0: the caller compares info[0] with out_cap after the stream.
 *   Every access is clamped: nothing outside keys[0 .. N), vals[0 .. N) and *n is read, and nothing
 *   outside the members' [0, min(C, out_cap)), starts[0 .. min(C, out_cap)] (its last entry only
 *   when C <= out_cap) and info[0 .. 2) is written.  The cost follows cap (the kernels are launched
 *   over it), not N, C or the lengths of the runs.  Temporary storage is the library's, per stream,
 *   shared with ebpf_batch_steer_dev, ebpf_batch_group_dev, ebpf_batch_reduce_dev,
 *   ebpf_batch_scan_dev, ebpf_batch_filter_dev, ebpf_batch_accumulate_dev and ebpf_batch_top_dev:
 *   128 bytes per 4,096 entries of cap (a tile's runs and what is open at its edges), at least 128
 *   bytes a call.
 * Both return 0; EINVAL for a NULL out or info, unknown bits in flags, key_shift above 63, and,
 * when an output reads the values, val_bits outside [1, 64] or val_shift + val_bits > 64; EINVAL
 * for NULL keys with cap > 0, and for NULL vals with cap > 0 when an output reads the values; then
 * E2BIG for cap or out_cap above 0xffffffff.  All of these are known on the host, before the
 * device is looked at, and nothing is written.  The device function then returns ENODEV (no GPU,
 * or no such device), ENOMEM (no scratch) or EIO.  Neither changes the calling thread's current
 * HIP device. */
#define EBPF_ROLLUP_SEGMENTS 0x1u   /* count the input's entries by the reduce's rule, not the table's */

struct ebpf_batch_rolls {      /* each NULL (not wanted: it costs nothing) */
	uint64_t *keys;    /* out_cap entries: the run's prefix, keys[p] >> key_shift            */
	uint64_t *count;   /* out_cap entries: the entries of the run (the distinct keys below it) */
	uint64_t *sum;     /* out_cap entries: sum of the value field, modulo 2^64               */
	uint64_t *min;     /* out_cap entries: smallest value field, unsigned                    */
	uint64_t *max;     /* out_cap entries: largest value field, unsigned                     */
	uint64_t *bits;    /* out_cap entries: OR of the value fields                            */
	uint64_t *starts;  /* out_cap + 1 entries: the run's first position in the input         */
};
int ebpf_batch_rollup(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
		      uint32_t flags, uint32_t key_shift, uint32_t val_shift, uint32_t val_bits,
		      uint64_t out_cap, const struct ebpf_batch_rolls *out, uint64_t *info);
int ebpf_batch_rollup_dev(int device, const uint64_t *keys_dev, const uint64_t *vals_dev,
			  uint64_t cap, const uint64_t *n_dev, uint32_t flags, uint32_t key_shift,
			  uint32_t val_shift, uint32_t val_bits, uint64_t out_cap,
			  const struct ebpf_batch_rolls *out, uint64_t *info_dev, void *stream);

/* The heaviest entries: the k best entries of a keyed sequence by a bit field of its values, found
 * on the device.  A table of per-flow totals answers "which flows carried the most?", a "last seen"
 * table "which K flows were idle the longest?" (the K smallest stamps, to evict them), and a few
 * KB cross to the host instead of the table:
 *
 *   tops = {top_keys, top_bytes, NULL};
 *   ebpf_batch_top_dev(dev, cur.keys, cur.vals, cur.cap, cur.n, EBPF_TOP_LARGEST, 0, 64, 10,
 *                      &tops, tinfo, s);                (the 10 heaviest flows of the table)
 *   ebpf_batch_top_dev(dev, group_keys, bytes, group_cap, info, EBPF_TOP_SEGMENTS, 0, 64, 10,
 *                      &tops, tinfo, s);                (the 10 heaviest flows of this batch)
 *
 * Entries: keys and vals have cap entries each, of which N take part.  n NULL: N = cap.  Otherwise
 *   N = min(*n, cap), the table's rule; with EBPF_TOP_SEGMENTS N is the R of ebpf_batch_reduce (*n
 *   when *n <= cap, else cap - 1, and 0 for cap == 0), because a reduce that followed a short group
 *   table left entry cap - 1 unwritten.  So a table plugs in as (t.keys, t.vals, t.cap, t.n), a
 *   batch as (group_keys, a member of the reduce's sums, group_cap, the group's info) with the
 *   flag, and any array of counts as (NULL, counts, cap, NULL), each as it stands, after its
 *   producer on the same stream.  cap is at most 0xffffffff: a position is 32 bits.
 * Field: f(p) = (vals[p] >> val_shift) & (2^val_bits - 1), 1 <= val_bits <= 64 and val_shift +
 *   val_bits <= 64, compared as unsigned numbers.  Bits outside the field take no part.
 * Order: by f descending (EBPF_TOP_LARGEST) or ascending (EBPF_TOP_SMALLEST); entries of equal
 *   field by ascending position p (for a table: by ascending key).  That is a total order: every
 *   input has exactly one right answer.
 * Outputs (struct ebpf_batch_tops): with m = min(k, N) and p_j the j-th position in that order, for
 *   j < m: keys[j] = keys[p_j], vals[j] = vals[p_j] (the whole word, not the field), pos[j] = p_j.
 *   Each member is NULL (not wanted: it costs nothing) or has k entries; entries at or past m are
 *   not written.  keys may be NULL iff out->keys is.  k is at most EBPF_TOP_MAX; k == 0 is valid.
 *   info (4 entries, always written): info[0] = m; info[1] = N; info[2] = f(p_(m-1)), the cut;
 *   info[3] = the entries not taken whose field equals the cut, so the cut fell inside a tie iff it
 *   is not 0.  info[2] and info[3] are 0 for m == 0.  With all three members NULL only info is
 *   written: the k-th largest or smallest field, a percentile.
 * The output is a function of the inputs alone: it does not depend on what the outputs held on
 * entry, and two calls on the same input give the same bytes.  The outputs may not overlap the
 * inputs or each other.
 *
 * ebpf_batch_top: host buffers, a partial sort over positions; no GPU needed (the statement of
 *   what the device function computes).
 * ebpf_batch_top_dev: keys_dev, vals_dev, n_dev, the members of *out and info_dev (out itself is a
 *   host struct) are device memory on `device`; enqueued on `stream` (hipStream_t, NULL = default
 *   stream), returns without synchronising and never waits for the device.  Every access is
 *   clamped: nothing outside keys[0 .. N), vals[0 .. N) and *n is read, and nothing outside the
 *   outputs' [0 .. m) and info[0 .. 4) is written.  The cost follows cap (the kernels are launched
 *   over it) and val_bits (a pass over the values per 8 bits of the field, and two more), not N or
 *   k.  Temporary storage is the library's, per stream, shared with ebpf_batch_steer_dev,
 *   ebpf_batch_group_dev, ebpf_batch_reduce_dev, ebpf_batch_scan_dev, ebpf_batch_filter_dev and
 *   ebpf_batch_accumulate_dev: 1,040 bytes per 4,096 entries of cap up to 1,024 such tiles (a
 *   digit's 256 counts and four words), 16 bytes per 4,096 entries past them (the counts are then
 *   shared by a run of tiles), and 49,216 bytes a call (EBPF_TOP_MAX candidates of 12 bytes).
 *   Every array is 8-byte aligned, pos 4-byte aligned, as their types say.
 * Both return 0; EINVAL for a NULL out or info, unknown bits in flags, val_bits outside [1, 64] or
 * val_shift + val_bits > 64, NULL vals with cap > 0, out->keys given with NULL keys; then E2BIG for
 * cap above 0xffffffff or k above EBPF_TOP_MAX.  All of these are known on the host, before the
 * device is looked at.  The device function then returns ENODEV (no GPU, or no such device),
 * ENOMEM (no scratch) or EIO.  Neither changes the calling thread's current HIP device. */
#define EBPF_TOP_MAX      4096u  /* k is at most one tile */
#define EBPF_TOP_LARGEST  0x0u
#define EBPF_TOP_SMALLEST 0x1u
#define EBPF_TOP_SEGMENTS 0x2u   /* count the entries by the reduce's rule, not the table's */

struct ebpf_batch_tops {         /* each NULL (not wanted: it costs nothing) or k entries */
	uint64_t *keys;  /* keys[p_j] */
	uint64_t *vals;  /* vals[p_j], the whole word, not the field */
	uint32_t *pos;   /* p_j */
};
int ebpf_batch_top(const uint64_t *keys, const uint64_t *vals, uint64_t cap, const uint64_t *n,
		   uint32_t flags, uint32_t val_shift, uint32_t val_bits, uint64_t k,
		   const struct ebpf_batch_tops *out, uint64_t *info);
int ebpf_batch_top_dev(int device, const uint64_t *keys_dev, const uint64_t *vals_dev, uint64_t cap,
		       const uint64_t *n_dev, uint32_t flags, uint32_t val_shift, uint32_t val_bits,
		       uint64_t k, const struct ebpf_batch_tops *out, uint64_t *info_dev, void *stream);

/* Gathering packets into a dense batch: a list of n packets of `batch` (a class of a steered
 * batch, the whole steering index, any list of the caller's own: duplicates and any order are
 * fine) copied, in list order, into `out`.  A class can then leave the device on its own (a TX
 * ring, one copy to the host), and a second-stage program gets a dense batch:
 *
 *   ebpf_batch_gather_dev(dev, &batch, index + starts[b], k, 64, out, k * 64, NULL, s);
 *   sub = {out, NULL, k, 64, 0};             (16-byte-aligned out: the staged kernel)
 *   ebpf_prog_run_batch_dev(ep2, dev, &sub, ret2, faults2, hist2, s);
 *
 * Packet index[j] has the (start, end) that ebpf_batch_select_dev would write for it, whatever
 * form `batch` has; its length len_j is end - start, or 0 when end < start or end - start >= 2^32
 * (the run functions' rule), and 0 for an index >= batch->count.  All offsets are 64-bit: packets
 * may lie 4 GiB or more from batch->data and the output may exceed 4 GiB.
 *
 * Strided form (out_stride > 0; out_offsets must be NULL): slot j is bytes [j * out_stride,
 *   (j + 1) * out_stride) of out and holds the packet's first min(len_j, out_stride) bytes, then
 *   zero bytes up to the slot's end (out_stride below the length snaps the packet, as a capture's
 *   snaplen does).  Needs n * out_stride <= out_bytes.  {out, NULL, n, out_stride, 0} is then a
 *   batch; with out_stride 64 and out 16-byte aligned it takes the staged kernel.
 * Packed form (out_stride == 0; out_offsets has n + 1 entries): out_offsets[0] = 0,
 *   out_offsets[j + 1] = out_offsets[j] + len_j, and packet j's bytes lie at out + out_offsets[j]:
 *   a tight pack, every length kept exactly, so a second stage faults on exactly the same loads.
 *   {out, out_offsets, n, 0, 0} is then an offsets-form batch.  out_offsets is always written in
 *   full, and no byte at or past out + out_bytes is written: out_offsets[n] is the size needed and
 *   the output is complete iff out_offsets[n] <= out_bytes (snprintf's rule).
 * Both: only bytes of [out, out + n * out_stride), or of [out, out + min(out_offsets[n],
 * out_bytes)), are written; out may have any alignment; out overlapping batch->data is undefined.
 * Only the listed packets' bytes, index[0 .. n) and the listed packets' offsets entries are read; a
 * listed packet of length 0 reads no data.  The output is a function of the inputs alone.  Gathering
 * a whole steering index with n = count reorders the batch by class in one call: class b then lies
 * at out + starts[b] * out_stride, or at out_offsets[starts[b] .. starts[b+1]].
 *
 * ebpf_batch_gather: host buffers; no GPU needed (the statement of what the device function
 *   computes).  Packed form: ENOSPC when out_offsets[n] > out_bytes, with out_offsets and the
 *   bytes that fit written.
 * ebpf_batch_gather_dev: batch->data, batch->offsets, index_dev, out_dev and out_offsets_dev are
 *   device memory on `device`; enqueued on `stream` (hipStream_t, NULL = default stream), returns
 *   without synchronising, so the packed form always returns 0 and the caller compares
 *   out_offsets_dev[n] with out_bytes after the stream.  A fixed-stride batch gathered at its own
 *   stride, a multiple of 16, with data and out 16-byte aligned, moves 16 bytes a lane; everything
 *   else goes through a general copy with the same results.  The packed form's temporary storage
 *   is the library's, per stream, shared with ebpf_batch_steer_dev (8 bytes per 4,096 entries).
 * Both return 0; EINVAL (a batch that the run functions would refuse; a NULL index or out with
 * n > 0; out_offsets given with out_stride > 0, or NULL with out_stride == 0; n * out_stride >
 * out_bytes); E2BIG for n > 0xffffffff.  n == 0 succeeds (the packed form writes out_offsets[0]
 * = 0).  The device function then returns ENODEV (no GPU, or no such device), ENOMEM (no scratch)
 * or EIO.  Neither changes the calling thread's current HIP device. */
int ebpf_batch_gather(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n,
		      uint32_t out_stride, void *out, uint64_t out_bytes, uint64_t *out_offsets);
int ebpf_batch_gather_dev(int device, const struct ebpf_pkt_batch *batch,
			  const uint32_t *index_dev, uint64_t n, uint32_t out_stride,
			  void *out_dev, uint64_t out_bytes, uint64_t *out_offsets_dev,
			  void *stream);

/* Scattering a dense batch back: the inverse of the gather, and the merge of a second stage's
 * results.  A second-stage program may store into its packets and returns a verdict of its own;
 * after a gathered second stage the rewritten bytes lie in the dense copy and ret2 / faults2 are
 * indexed by list position.  These functions put both back where the batch keeps them, so that the
 * pipeline ends with one batch and one ret array in packet order:
 *
 *   ebpf_batch_gather_dev(dev, &batch, index + starts[b], k, 64, out, k * 64, NULL, s);
 *   ebpf_prog_run_batch_dev(ep2, dev, &sub, ret2, faults2, NULL, s);      (sub as above)
 *   ebpf_batch_scatter_dev(dev, &batch, index + starts[b], k, 64, out, k * 64, NULL, s);
 *   ebpf_batch_merge_dev(dev, ret, faults, batch.count, index + starts[b], k, ret2, faults2, s);
 *
 * Scatter writes into batch->data through the const pointer, as the run functions do for a program
 * that stores into its packets.  Packet index[j] has the (start, len_j) that ebpf_batch_gather
 * uses, whatever form `batch` has: the length-0 rule for an end below the start or 2^32 or more
 * past it, and length 0 for an index >= batch->count.
 *
 * Strided form (in_stride > 0; in_offsets must be NULL): slot j is in + j * in_stride and k_j =
 *   min(len_j, in_stride).  Needs n * in_stride <= in_bytes.
 * Packed form (in_stride == 0; in_offsets has n + 1 entries): slot j is bytes [in_offsets[j],
 *   in_offsets[j + 1]) of in, read as an offsets-form batch reads them: its length m_j follows the
 *   same length-0 rule and is then cut so that no byte at or past in + in_bytes is read; k_j =
 *   min(len_j, m_j).  {in, in_offsets} as a packed gather left them scatter back exactly what was
 *   gathered, also after a truncated gather (out_offsets[n] > out_bytes).
 * Both: bytes [start, start + k_j) of batch->data become slot j's first k_j bytes; a packet longer
 * than its slot keeps its remaining bytes.  No other byte of batch->data is written: not the gaps
 * between packets, not an unlisted neighbour that shares 16 bytes with a listed packet, not a
 * packet's bytes past k_j.  Only the slots' first k_j bytes, index[0 .. n), in_offsets[0 .. n] and
 * the listed packets' offsets entries are read; a slot's padding is never read.  A steering list
 * names every packet once.  If a packet is listed more than once, or listed packets overlap, every
 * affected byte ends as the corresponding byte of one of the candidates, which one is unspecified
 * (the rule for stores into overlapping packets above); where the candidates agree — a
 * deterministic second stage over a gathered list with duplicates — the result is exact.  `in`
 * overlapping batch->data is undefined.
 *
 * Merge: for j < n with index[j] < count, ret[index[j]] = ret2[j] and, if faults is given,
 * faults[index[j]] = faults2 ? faults2[j] : 0.  An index >= count writes nothing, and nothing
 * outside ret[0 .. count) and faults[0 .. count) is written.  Of duplicate listings one's value
 * lands whole.  The merged histogram is `starts` of a second ebpf_batch_steer_dev over the merged
 * ret / faults (bin b = starts[b + 1] - starts[b]), which also lists the final classes.
 *
 * ebpf_batch_scatter, ebpf_batch_merge: host buffers; no GPU needed (the statement of what the
 *   device functions compute, and the step for a caller of ebpf_prog_run_batch).
 * ebpf_batch_scatter_dev, ebpf_batch_merge_dev: every pointer (batch->data, batch->offsets
 *   included) is device memory on `device`; enqueued on `stream` (hipStream_t, NULL = default
 *   stream), return without synchronising, need no temporary storage.  A fixed-stride batch
 *   scattered from its own stride, a multiple of 16, with data and in 16-byte aligned, moves 16
 *   bytes a lane; everything else goes through a general copy with the same results.
 * Scatter returns 0; EINVAL (a batch that the run functions would refuse; a NULL index or in with
 * n > 0; in_offsets given with in_stride > 0, or NULL with in_stride == 0; n * in_stride >
 * in_bytes); E2BIG for n > 0xffffffff.  Merge returns 0; EINVAL for a NULL ret, ret2 or index
 * with n > 0; E2BIG for n > 0xffffffff.  n == 0 succeeds.  The device functions then return
 * ENODEV (no GPU, or no such device) or EIO.  None changes the calling thread's current HIP
 * device. */
int ebpf_batch_scatter(const struct ebpf_pkt_batch *batch, const uint32_t *index, uint64_t n,
		       uint32_t in_stride, const void *in, uint64_t in_bytes,
		       const uint64_t *in_offsets);
int ebpf_batch_scatter_dev(int device, const struct ebpf_pkt_batch *batch,
			   const uint32_t *index_dev, uint64_t n, uint32_t in_stride,
			   const void *in_dev, uint64_t in_bytes,
			   const uint64_t *in_offsets_dev, void *stream);
int ebpf_batch_merge(uint64_t *ret, uint8_t *faults, uint64_t count, const uint32_t *index,
		     uint64_t n, const uint64_t *ret2, const uint8_t *faults2);
int ebpf_batch_merge_dev(int device, uint64_t *ret_dev, uint8_t *faults_dev, uint64_t count,
			 const uint32_t *index_dev, uint64_t n, const uint64_t *ret2_dev,
			 const uint8_t *faults2_dev, void *stream);

/* Select the device used by ebpf_prog_run_batch for the calling thread. */
int ebpf_gpu_set_device(int device);

/* Device path used by subsequent launches (all bit-identical):
 *   0 = default: the program compiled to gfx950 code (copy-and-patch of the assembly
 *       interpreter's handlers); a program too large for the code area runs on the assembly
 *       interpreter.  Launches fail with ENOSYS if the code object cannot be loaded.
 *   1 = the portable HIP interpreter (correctness baseline).
 *   2 = the hand-written gfx950 assembly interpreter. */
int ebpf_gpu_set_variant(int variant);

/* Measurement hook (extension): the calling thread's next ebpf_prog_run_batch_dev records
 * `start_event` at the start of the launch's kernel and `stop_event` at its end, on the launch
 * stream, so that hipEventElapsedTime gives the kernel's own duration (a launch is one kernel:
 * the verdict histogram is reduced inside it).  Both are hipEvent_t of the HIP runtime the
 * library runs on; NULL, NULL cancels.  Returns 0, or EINVAL if only one is NULL. */
int ebpf_gpu_time_next_launch(void *start_event, void *stop_event);

/* Instruction semantics of a program (extension: the reference has only the first).
 *   EBPF_SEM_REFERENCE (default): the reference interpreter's, quirks included
 *       (ebpf_interpreter.c:23-372: cumulative stepping, MOV64 adds, NEG ignores dst, NEG64 is
 *       dst - imm, logical ARSH, DIV/MOD by zero faults).
 *   EBPF_SEM_STANDARD: standard eBPF as compilers emit it: sequential pc (a jump goes to
 *       pc + 1 + off), MOV64 moves (imm sign-extended), NEG/NEG64 negate dst, arithmetic ARSH,
 *       DIV by zero gives 0 and MOD by zero leaves dst (32-bit ops: truncated), and the JMP32
 *       class (opcode class 0x06, compares of the low 32 bits).  Loops: in a device batch a
 *       packet may take 2^20 backward jumps (taken jumps whose target is at or before their own
 *       slot); the next one stops it with EBPF_FAULT_LOOP.  Map writes inside loops: see "Map
 *       writes in a device batch" and "Stores into map values" above (16 logged writes per
 *       packet; counter updates as additions).  ebpf_prog_run runs any program unbounded.
 * Applies to ebpf_prog_run and to device batches.  Returns 0, EINVAL (bad argument) or EBUSY
 * (the program was already translated for a device). */
#define EBPF_SEM_REFERENCE 0
#define EBPF_SEM_STANDARD 1
int ebpf_prog_set_semantics(struct ebpf_prog *ep, int semantics);

/* Information about the translated device program. */
struct ebpf_dprog_info {
	uint32_t nslots;       /* prog_len / 8 */
	uint32_t nentries;     /* executed-state entries after translation */
	uint32_t nmaps;        /* array maps resolved from LDDW immediates */
	uint32_t max_stack;    /* deepest statically known stack access (bytes below r10) */
};
int ebpf_prog_device_info(struct ebpf_prog *ep, struct ebpf_dprog_info *info);

/* What ran, and what it cost to get there (extension; measurement and diagnostics). */
#define EBPF_EXEC_COMPILED 0     /* the program compiled to gfx950 code (variant 0) */
#define EBPF_EXEC_HIP 1          /* the portable HIP interpreter (variant 1) */
#define EBPF_EXEC_INTERPRETER 2  /* the gfx950 assembly interpreter (variant 2, or variant 0 on a
                                    program too large for the code area) */
struct ebpf_dexec_info {
	int32_t exec;          /* EBPF_EXEC_* of the last launch on `device`; -1 = none yet */
	int32_t layout;        /* its kernel: 1 = staged fixed 64-B packets, 0 = general; -1 =
	                          none */
	double translate_ms;   /* host time of the state-tree translation (once per program) */
	double build_ms;       /* compile (COMPILED) or lower + link (INTERPRETER) time for that
	                          kernel on that device, paid at its first launch; 0 for HIP */
};
int ebpf_prog_device_exec(struct ebpf_prog *ep, int device, struct ebpf_dexec_info *info);

/* Diagnostics: the program as compiled for variant 0, raw gfx950 instruction bytes, for packet
 * `layout` 1 (fixed 64-B packets) or 0 (any stride / offsets); others EINVAL.  Host only (no
 * GPU needed; map base addresses are then 0).  *len: in = size of buf, out = bytes of code.  buf == NULL just
 * sizes.  Returns 0, ENOSPC (buf too small), E2BIG (program too large to compile). */
int ebpf_prog_device_code(struct ebpf_prog *ep, int layout, void *buf, size_t *len);

/* Human-readable description of the last error on this thread ("" if none). */
const char *ebpf_gpu_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* EBPF_AMD_EBPF_GPU_H */
