"""ctypes binding of the engine's C-ABI library (lib/libebpf.so).

The Python layer mirrors the reference's plugin interface: an ``Env`` owns a ``struct
ebpf_config`` laid out like tests/test_common.hpp:59-75 of the reference (program type 0
"test"; map types 0..3 = array, percpu array, hashtable, percpu hashtable; helpers 0..2 =
map_lookup_elem / map_update_elem / map_delete_elem), ``Map`` and ``Prog`` wrap the map and
program objects with the reference's errno conventions.  Batch runs go to the GPU through
include/ebpf_gpu.h; if the library is missing, loading fails loudly.
"""
import ctypes
import errno
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# EBPF_LIB: an alternative build of the same library (A/B experiments under tools/)
LIB_PATH = os.environ.get("EBPF_LIB") or os.path.join(HERE, "lib", "libebpf.so")

EBPF_TYPE_MAX = 64
EBPF_NAME_MAX = 64
EBPF_HIST_BINS = 257

MAP_TYPE_ARRAY, MAP_TYPE_PERCPU_ARRAY, MAP_TYPE_HASHTABLE, MAP_TYPE_PERCPU_HASHTABLE = range(4)
SEM_REFERENCE, SEM_STANDARD = 0, 1
HELPER_LOOKUP, HELPER_UPDATE, HELPER_DELETE, HELPER_OTHER = range(4)
EBPF_ANY, EBPF_NOEXIST, EBPF_EXIST = 0, 1, 2

FAULT_NAMES = ["NONE", "BAD_OPCODE", "DIV_ZERO", "MEM", "SLOT", "HELPER", "HELPER_UNSUPPORTED",
               "BAD_REG", "LOOP", "MAP_WRITE", "BAD_MAP", "WRITES"]


class ProgAttr(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("prog", ctypes.c_void_p),
                ("prog_len", ctypes.c_uint32), ("data", ctypes.c_void_p)]


class MapAttr(ctypes.Structure):
    _fields_ = [("type", ctypes.c_uint32), ("key_size", ctypes.c_uint32),
                ("value_size", ctypes.c_uint32), ("max_entries", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


_PREDFN = ctypes.CFUNCTYPE(ctypes.c_bool, ctypes.c_void_p)


class ProgType(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * EBPF_NAME_MAX), ("is_map_usable", _PREDFN),
                ("is_helper_usable", _PREDFN)]


class HelperType(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * EBPF_NAME_MAX), ("fn", ctypes.c_void_p)]


class Config(ctypes.Structure):
    _fields_ = [("prog_types", ctypes.c_void_p * EBPF_TYPE_MAX),
                ("map_types", ctypes.c_void_p * EBPF_TYPE_MAX),
                ("helper_types", ctypes.c_void_p * EBPF_TYPE_MAX),
                ("preprocessor_type", ctypes.c_void_p)]


class PktBatch(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("count", ctypes.c_uint64), ("stride", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class BatchSums(ctypes.Structure):
    """struct ebpf_batch_sums: the outputs of a reduce call, each NULL or seg_cap u64"""
    _fields_ = [("bytes", ctypes.c_void_p), ("sum", ctypes.c_void_p), ("min", ctypes.c_void_p),
                ("max", ctypes.c_void_p), ("bits", ctypes.c_void_p)]


class BatchScans(ctypes.Structure):
    """struct ebpf_batch_scans: the outputs of a scan call, each NULL or n entries"""
    _fields_ = [("rank", ctypes.c_void_p), ("bytes_before", ctypes.c_void_p),
                ("sum_before", ctypes.c_void_p), ("over", ctypes.c_void_p)]


class BatchTest(ctypes.Structure):
    """struct ebpf_batch_test: the tests of a filter call, a conjunction; a NULL member is none"""
    _fields_ = [("flags", ctypes.c_void_p), ("rank", ctypes.c_void_p),
                ("rank_below", ctypes.c_uint32), ("ret", ctypes.c_void_p),
                ("val_shift", ctypes.c_uint32), ("val_bits", ctypes.c_uint32),
                ("val_lo", ctypes.c_uint64), ("val_hi", ctypes.c_uint64)]


class BatchParts(ctypes.Structure):
    """struct ebpf_batch_parts: the outputs of a filter call, each NULL or n (the lists) or
    seg_cap + 1 (their tables) entries"""
    _fields_ = [("kept", ctypes.c_void_p), ("kept_starts", ctypes.c_void_p),
                ("dropped", ctypes.c_void_p), ("dropped_starts", ctypes.c_void_p)]


class KeyTable(ctypes.Structure):
    """struct ebpf_key_table: cap keys, strictly ascending, cap values beside them, and the
    number of keys the table has or would need"""
    _fields_ = [("keys", ctypes.c_void_p), ("vals", ctypes.c_void_p), ("cap", ctypes.c_uint64),
                ("n", ctypes.c_void_p)]


class BatchRolls(ctypes.Structure):
    """struct ebpf_batch_rolls: the outputs of a rollup call, each NULL or out_cap entries (starts
    out_cap + 1)"""
    _fields_ = [("keys", ctypes.c_void_p), ("count", ctypes.c_void_p), ("sum", ctypes.c_void_p),
                ("min", ctypes.c_void_p), ("max", ctypes.c_void_p), ("bits", ctypes.c_void_p),
                ("starts", ctypes.c_void_p)]


class BatchTops(ctypes.Structure):
    """struct ebpf_batch_tops: the outputs of a top call, each NULL or k entries"""
    _fields_ = [("keys", ctypes.c_void_p), ("vals", ctypes.c_void_p), ("pos", ctypes.c_void_p)]


class BatchStats(ctypes.Structure):
    _fields_ = [("packets", ctypes.c_uint64), ("faulted", ctypes.c_uint64),
                ("hist", ctypes.c_uint64 * EBPF_HIST_BINS), ("kernel_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class DexecInfo(ctypes.Structure):
    _fields_ = [("exec", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("translate_ms", ctypes.c_double), ("build_ms", ctypes.c_double)]


EXEC_NAMES = {0: "compiled", 1: "hip", 2: "interpreter"}


class PcapInfo(ctypes.Structure):
    _fields_ = [("linktype", ctypes.c_uint32), ("snaplen", ctypes.c_uint32),
                ("nanosecond", ctypes.c_uint32), ("byte_swapped", ctypes.c_uint32),
                ("truncated", ctypes.c_uint64), ("bytes", ctypes.c_uint64)]


class DprogInfo(ctypes.Structure):
    _fields_ = [("nslots", ctypes.c_uint32), ("nentries", ctypes.c_uint32),
                ("nmaps", ctypes.c_uint32), ("max_stack", ctypes.c_uint32)]


# Every function include/ebpf.h and include/ebpf_gpu.h declare: name -> (restype, argtypes)
_VP, _U32, _U64, _I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
FUNCS = {
    "ebpf_init": (_I, []), "ebpf_deinit": (_I, []),
    "ebpf_env_create": (_I, [_VP, _VP]), "ebpf_env_destroy": (_I, [_VP]),
    "ebpf_obj_acquire": (None, [_VP]), "ebpf_obj_release": (None, [_VP]),
    "ebpf_prog_create": (_I, [_VP, _VP, _VP]), "ebpf_prog_destroy": (None, [_VP]),
    "ebpf_prog_run": (_U64, [_VP, _VP]),
    "ebpf_map_create": (_I, [_VP, _VP, _VP]), "ebpf_map_lookup_elem": (_VP, [_VP, _VP]),
    "ebpf_map_update_elem": (_I, [_VP, _VP, _VP, _U64]),
    "ebpf_map_delete_elem": (_I, [_VP, _VP]),
    "ebpf_map_lookup_elem_from_user": (_I, [_VP, _VP, _VP]),
    "ebpf_map_update_elem_from_user": (_I, [_VP, _VP, _VP, _U64]),
    "ebpf_map_delete_elem_from_user": (_I, [_VP, _VP]),
    "ebpf_map_get_next_key_from_user": (_I, [_VP, _VP, _VP]),
    "ebpf_map_destroy": (None, [_VP]),
    # ebpf_gpu.h
    "ebpf_gpu_device_count": (_I, []), "ebpf_gpu_set_device": (_I, [_I]), "ebpf_dev_init": (_I, [_I]),
    "ebpf_gpu_set_variant": (_I, [_I]), "ebpf_gpu_time_next_launch": (_I, [_VP, _VP]), "ebpf_gpu_last_error": (ctypes.c_char_p, []),
    "ebpf_prog_prepare_device": (_I, [_VP, _I]),
    "ebpf_prog_run_batch": (_I, [_VP, _VP, _VP, _VP, _VP]),
    "ebpf_prog_run_batch_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "ebpf_prog_run_batch_multi": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP]),
    "ebpf_prog_run_batch_multi_dev": (_I, [_VP, _I, _VP, _VP, _VP, _VP, _VP, _VP]),
    "ebpf_prog_device_info": (_I, [_VP, _VP]),
    "ebpf_prog_device_exec": (_I, [_VP, _I, _VP]),
    "ebpf_prog_device_code": (_I, [_VP, _I, _VP, ctypes.POINTER(ctypes.c_size_t)]),
    "ebpf_prog_set_semantics": (_I, [_VP, _I]),
    "ebpf_pcap_batch": (_I, [_VP, ctypes.c_size_t, _I, _VP, _VP]),
    "ebpf_pcap_batch_free": (None, [_VP]),
    "ebpf_pcap_extents": (_I, [_VP, ctypes.c_size_t, _I, _VP, _VP]),
    "ebpf_prog_run_batch_async": (_I, [_VP, _VP, _VP, _VP, ctypes.POINTER(_VP)]),
    "ebpf_batch_wait": (_I, [_VP, _VP]),
    "ebpf_batch_steer": (_I, [_VP, _VP, _U64, _VP, _VP]),
    "ebpf_batch_steer_dev": (_I, [_I, _VP, _VP, _U64, _VP, _VP, _VP]),
    "ebpf_batch_select_dev": (_I, [_I, _VP, _VP, _U64, _VP, _VP]),
    "ebpf_batch_group_tmp_bytes": (ctypes.c_size_t, [_U64, _U32]),
    "ebpf_batch_group": (_I, [_VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _VP, _VP]),
    "ebpf_batch_group_dev": (_I, [_I, _VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _VP, _VP, _VP,
                                  ctypes.c_size_t, _VP]),
    "ebpf_batch_reduce": (_I, [_VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _U64, _VP, _VP]),
    "ebpf_batch_reduce_dev": (_I, [_I, _VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _U64, _VP, _VP,
                                   _VP]),
    "ebpf_batch_scan": (_I, [_VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _U64, _VP, _VP, _VP]),
    "ebpf_batch_scan_dev": (_I, [_I, _VP, _VP, _U64, _U32, _U32, _VP, _U64, _VP, _U64, _VP, _VP, _VP,
                                 _VP]),
    "ebpf_batch_filter": (_I, [_VP, _U64, _VP, _U64, _VP, _U64, _VP, _VP, _VP]),
    "ebpf_batch_filter_dev": (_I, [_I, _VP, _U64, _VP, _U64, _VP, _U64, _VP, _VP, _VP, _VP]),
    "ebpf_batch_lookup": (_I, [_VP, _VP, _U64, _VP, _U32, _U64, _U64, _VP, _VP]),
    "ebpf_batch_lookup_dev": (_I, [_I, _VP, _VP, _U64, _VP, _U32, _U64, _U64, _VP, _VP, _VP]),
    "ebpf_batch_accumulate": (_I, [_VP, _VP, _VP, _U64, _VP, _U32, _U64, _U64, _VP, _VP]),
    "ebpf_batch_accumulate_dev": (_I, [_I, _VP, _VP, _VP, _U64, _VP, _U32, _U64, _U64, _VP, _VP,
                                       _VP]),
    "ebpf_batch_rollup": (_I, [_VP, _VP, _U64, _VP, _U32, _U32, _U32, _U32, _U64, _VP, _VP]),
    "ebpf_batch_rollup_dev": (_I, [_I, _VP, _VP, _U64, _VP, _U32, _U32, _U32, _U32, _U64, _VP, _VP,
                                   _VP]),
    "ebpf_batch_top": (_I, [_VP, _VP, _U64, _VP, _U32, _U32, _U32, _U64, _VP, _VP]),
    "ebpf_batch_top_dev": (_I, [_I, _VP, _VP, _U64, _VP, _U32, _U32, _U32, _U64, _VP, _VP, _VP]),
    "ebpf_batch_gather": (_I, [_VP, _VP, _U64, _U32, _VP, _U64, _VP]),
    "ebpf_batch_gather_dev": (_I, [_I, _VP, _VP, _U64, _U32, _VP, _U64, _VP, _VP]),
    "ebpf_batch_scatter": (_I, [_VP, _VP, _U64, _U32, _VP, _U64, _VP]),
    "ebpf_batch_scatter_dev": (_I, [_I, _VP, _VP, _U64, _U32, _VP, _U64, _VP, _VP]),
    "ebpf_batch_merge": (_I, [_VP, _VP, _U64, _VP, _U64, _VP, _VP]),
    "ebpf_batch_merge_dev": (_I, [_I, _VP, _VP, _U64, _VP, _U64, _VP, _VP, _VP]),
}
DATA_SYMBOLS = ["emt_array", "emt_percpu_array", "emt_hashtable", "emt_percpu_hashtable",
                "eht_map_lookup_elem", "eht_map_update_elem", "eht_map_delete_elem"]

_lib = None


BATCH_HIST_OVERWRITE = 0x1  # include/ebpf_gpu.h EBPF_BATCH_HIST_OVERWRITE
BATCH_EXTENTS = 0x2         # EBPF_BATCH_EXTENTS: offsets holds (start, end) pairs
STEER_STARTS = EBPF_HIST_BINS + 1  # EBPF_STEER_STARTS: entries of a steering call's starts
EBPF_NO_PACKET = 0xffffffff  # EBPF_NO_PACKET: a list entry that names no packet
STEER_TILE = 4096           # csrc/host/steer.h STEER_TILE: packets per workgroup of the kernels
EBPF_NO_ENTRY = 0xffffffff  # EBPF_NO_ENTRY: the position of a key that a table does not hold
LOOKUP_VALUE, LOOKUP_REMAINING = 0, 1          # EBPF_LOOKUP_*: the modes of a lookup
ACC_ADD, ACC_MIN, ACC_MAX, ACC_OR = range(4)   # EBPF_ACC_*: the ops of an accumulate
ROLLUP_SEGMENTS = 1                            # EBPF_ROLLUP_SEGMENTS: N by the reduce's rule
ROLLS = ("keys", "count", "sum", "min", "max", "bits", "starts")   # ebpf_batch_rolls' members
TOP_MAX = 4096                                 # EBPF_TOP_MAX: the most entries a top call takes
TOP_LARGEST, TOP_SMALLEST, TOP_SEGMENTS = 0, 1, 2   # EBPF_TOP_*: the flags of a top call


def _pkt_batch(data_ptr, offsets_ptr, count, stride, extents=False, hist_overwrite=False):
    """The ebpf_pkt_batch of a call: where the packets are, and the two flags."""
    return PktBatch(data_ptr, offsets_ptr, count, stride,
                    (BATCH_EXTENTS if extents else 0) |
                    (BATCH_HIST_OVERWRITE if hist_overwrite else 0))


class _AsyncJob:
    """An ebpf_prog_run_batch_async job and the buffers it writes (see Prog.run_batch_async)."""

    def __init__(self, data, count, offsets, want_faults):
        self.data = data
        self.offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        self.ret = np.zeros(count, dtype=np.uint64)
        self.faults = np.zeros(count, dtype=np.uint8) if want_faults else None
        self.handle = None

    def wait(self):
        st = BatchStats()
        h, self.handle = self.handle, None
        _check(lib().ebpf_batch_wait(h, ctypes.byref(st)), "ebpf_batch_wait")
        return self.ret, self.faults, st


class PcapBatch:
    """ebpf_pcap_batch: a classic pcap capture (bytes) as a library-allocated batch in offsets
    form.  ``batch`` is the ebpf_pkt_batch to hand to the run functions; ``data()`` /
    ``offsets()`` copy it out; ``free()`` (or the context manager) releases it."""

    def __init__(self, capture, pinned=False, extents=False):
        # (extents: ebpf_pcap_extents, the batch is the capture itself; it is kept here)
        self.buf = np.frombuffer(bytes(capture), dtype=np.uint8)
        buf = self.buf
        self.batch = PktBatch()
        self.info = PcapInfo()
        fn = lib().ebpf_pcap_extents if extents else lib().ebpf_pcap_batch
        _check(fn(buf.ctypes.data if len(buf) else None, len(buf), 1 if pinned else 0,
                  ctypes.byref(self.batch), ctypes.byref(self.info)),
               "ebpf_pcap_extents" if extents else "ebpf_pcap_batch")

    @property
    def count(self):
        return int(self.batch.count)

    def offsets(self):
        n = 2 * self.count if self.batch.flags & BATCH_EXTENTS else self.count + 1
        return np.ctypeslib.as_array((ctypes.c_uint64 * n).from_address(
            self.batch.offsets)).copy()

    def data(self):
        if self.batch.flags & BATCH_EXTENTS:
            return self.buf.copy()
        n = int(self.info.bytes)
        if n == 0:
            return np.zeros(0, dtype=np.uint8)
        return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(self.batch.data)).copy()

    def free(self):
        if self.batch.data is not None or self.batch.offsets is not None:
            lib().ebpf_pcap_batch_free(ctypes.byref(self.batch))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def lib():
    """Load lib/libebpf.so (raises OSError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("native library not built: %s (run __graft_entry__.build())" % LIB_PATH)
        # torch (when installed) bundles its own HIP runtime under the same soname: loaded
        # first, it is the one the library binds to as well.  Loaded the other way round, a
        # process gets two HIP runtimes and whichever initialises second sees no GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in FUNCS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def addr_of(symbol):
    return ctypes.addressof(ctypes.c_char.in_dll(lib(), symbol))


def last_error():
    return (lib().ebpf_gpu_last_error() or b"").decode()


class EbpfError(RuntimeError):
    def __init__(self, code, what):
        super().__init__("%s failed: %s (%d) %s" % (what, errno.errorcode.get(code, "?"), code,
                                                    last_error()))
        self.code = code


def _check(code, what):
    if code != 0:
        raise EbpfError(code, what)


_always = _PREDFN(lambda _p: True)


class Env:
    """ebpf_env with the reference test suite's configuration (tests/test_common.hpp:59-75),
    plus helper 3: a helper with no device implementation (CALL 3 faults HELPER_UNSUPPORTED
    on the device)."""

    def __init__(self, helpers=None):
        L = lib()
        self._ptype = ProgType(b"test", _always, _always)
        self._other = HelperType(b"other", None)
        self.config = Config()
        self.config.prog_types[0] = ctypes.addressof(self._ptype)
        for i, s in enumerate(["emt_array", "emt_percpu_array", "emt_hashtable",
                               "emt_percpu_hashtable"]):
            self.config.map_types[i] = addr_of(s)
        hl = helpers if helpers is not None else {
            HELPER_LOOKUP: addr_of("eht_map_lookup_elem"),
            HELPER_UPDATE: addr_of("eht_map_update_elem"),
            HELPER_DELETE: addr_of("eht_map_delete_elem"),
            HELPER_OTHER: ctypes.addressof(self._other)}
        for i, a in hl.items():
            self.config.helper_types[i] = a
        self.ptr = ctypes.c_void_p()
        _check(L.ebpf_env_create(ctypes.byref(self.ptr), ctypes.byref(self.config)),
               "ebpf_env_create")

    def destroy(self):
        return lib().ebpf_env_destroy(self.ptr)


class Map:
    def __init__(self, env, max_entries, value_size, key_size=4, type=MAP_TYPE_ARRAY):
        self.env = env
        self.value_size, self.max_entries = value_size, max_entries
        attr = MapAttr(type, key_size, value_size, max_entries, 0)
        self.ptr = ctypes.c_void_p()
        _check(lib().ebpf_map_create(env.ptr, ctypes.byref(self.ptr), ctypes.byref(attr)),
               "ebpf_map_create")

    @property
    def handle(self):
        return self.ptr.value

    def update(self, key, value_bytes, flags=EBPF_ANY):
        k = ctypes.c_uint32(key)
        v = ctypes.create_string_buffer(bytes(value_bytes), self.value_size)
        return lib().ebpf_map_update_elem_from_user(self.ptr, ctypes.byref(k), v, flags)

    def fill(self, data):
        """data: bytes of max_entries * value_size."""
        for k in range(self.max_entries):
            _check(self.update(k, data[k * self.value_size:(k + 1) * self.value_size]),
                   "map update")

    def lookup(self, key):
        k = ctypes.c_uint32(key)
        v = ctypes.create_string_buffer(self.value_size)
        err = lib().ebpf_map_lookup_elem_from_user(self.ptr, ctypes.byref(k), v)
        return err, v.raw

    def destroy(self):
        lib().ebpf_map_destroy(self.ptr)


class HashMap:
    """A hashtable (or percpu hashtable) map with byte-string keys (ebpf_map_hashtable.c)."""

    def __init__(self, env, key_size, value_size, max_entries, percpu=False):
        self.env = env
        self.key_size, self.value_size, self.max_entries = key_size, value_size, max_entries
        t = MAP_TYPE_PERCPU_HASHTABLE if percpu else MAP_TYPE_HASHTABLE
        attr = MapAttr(t, key_size, value_size, max_entries, 0)
        self.ptr = ctypes.c_void_p()
        _check(lib().ebpf_map_create(env.ptr, ctypes.byref(self.ptr), ctypes.byref(attr)),
               "ebpf_map_create")

    @property
    def handle(self):
        return self.ptr.value

    def update(self, key, value_bytes, flags=EBPF_ANY):
        k = ctypes.create_string_buffer(bytes(key), self.key_size)
        v = ctypes.create_string_buffer(bytes(value_bytes), self.value_size)
        return lib().ebpf_map_update_elem_from_user(self.ptr, k, v, flags)

    def fill(self, keys, values):
        """keys: uint8 [n, key_size]; values: uint8 [n, value_size] (EBPF_ANY updates)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, self.key_size)
        values = np.ascontiguousarray(values, dtype=np.uint8).reshape(-1, self.value_size)
        f = lib().ebpf_map_update_elem_from_user
        kp, vp = keys.ctypes.data, values.ctypes.data
        for i in range(len(keys)):
            _check(f(self.ptr, kp + i * self.key_size, vp + i * self.value_size, EBPF_ANY),
                   "map update")

    def lookup(self, key):
        k = ctypes.create_string_buffer(bytes(key), self.key_size)
        v = ctypes.create_string_buffer(self.value_size)
        err = lib().ebpf_map_lookup_elem_from_user(self.ptr, k, v)
        return err, v.raw

    def delete(self, key):
        k = ctypes.create_string_buffer(bytes(key), self.key_size)
        return lib().ebpf_map_delete_elem_from_user(self.ptr, k)

    def destroy(self):
        lib().ebpf_map_destroy(self.ptr)


def patch_relocs(code, relocs, handles):
    b = bytearray(code)
    for slot, k in relocs:
        h = handles[k] & 0xffffffffffffffff
        b[slot * 8 + 4: slot * 8 + 8] = (h & 0xffffffff).to_bytes(4, "little")
        b[slot * 8 + 12: slot * 8 + 16] = (h >> 32).to_bytes(4, "little")
    return bytes(b)


class Prog:
    def __init__(self, env, code, prog_type=0):
        self.env = env
        self._buf = ctypes.create_string_buffer(bytes(code), len(code))
        attr = ProgAttr(prog_type, ctypes.addressof(self._buf), len(code), None)
        self.ptr = ctypes.c_void_p()
        _check(lib().ebpf_prog_create(env.ptr, ctypes.byref(self.ptr), ctypes.byref(attr)),
               "ebpf_prog_create")

    def destroy(self):
        lib().ebpf_prog_destroy(self.ptr)

    def info(self):
        i = DprogInfo()
        _check(lib().ebpf_prog_device_info(self.ptr, ctypes.byref(i)), "ebpf_prog_device_info")
        return i

    def exec_info(self, device=0):
        """What the last launch on ``device`` ran (ebpf_prog_device_exec): (exec name or None,
        layout, translate ms, build ms)."""
        i = DexecInfo()
        _check(lib().ebpf_prog_device_exec(self.ptr, device, ctypes.byref(i)),
               "ebpf_prog_device_exec")
        return EXEC_NAMES.get(i.exec), i.layout, i.translate_ms, i.build_ms

    def set_semantics(self, semantics):
        """SEM_REFERENCE (default) or SEM_STANDARD (ebpf_gpu.h ebpf_prog_set_semantics)."""
        _check(lib().ebpf_prog_set_semantics(self.ptr, semantics), "ebpf_prog_set_semantics")

    def prepare(self, device=0):
        _check(lib().ebpf_prog_prepare_device(self.ptr, device), "ebpf_prog_prepare_device")

    def run_cpu(self, packet):
        """Single packet through ebpf_prog_run (the API's per-packet CPU entry point)."""
        buf = ctypes.create_string_buffer(bytes(packet), len(packet))
        return lib().ebpf_prog_run(buf, self.ptr), buf.raw

    def run_batch(self, data, count, stride=0, offsets=None, want_faults=True, extents=False):
        """Host buffers: returns (ret u64[count], faults u8[count], stats).  ``data`` (a
        contiguous uint8 numpy array) is modified in place if the program stores to packets.
        ``extents``: ``offsets`` holds (start, end) pairs (EBPF_BATCH_EXTENTS)."""
        assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
        ret = np.zeros(count, dtype=np.uint64)
        faults = np.zeros(count, dtype=np.uint8) if want_faults else None
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        b = _pkt_batch(data.ctypes.data, None if offs is None else offs.ctypes.data,
                       count, stride, extents)
        st = BatchStats()
        _check(lib().ebpf_prog_run_batch(self.ptr, ctypes.byref(b), ret.ctypes.data,
                                         None if faults is None else faults.ctypes.data,
                                         ctypes.byref(st)), "ebpf_prog_run_batch")
        return ret, faults, st

    def run_batch_async(self, data, count, stride=0, offsets=None, want_faults=True):
        """ebpf_prog_run_batch_async: returns a job; job.wait() -> (ret, faults, stats) as
        run_batch.  ``data`` (and ``offsets``) must stay alive until the wait (the job keeps
        references)."""
        assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
        job = _AsyncJob(data, count, offsets, want_faults)
        b = _pkt_batch(data.ctypes.data, None if job.offs is None else job.offs.ctypes.data,
                       count, stride)
        h = ctypes.c_void_p()
        _check(lib().ebpf_prog_run_batch_async(self.ptr, ctypes.byref(b), job.ret.ctypes.data,
                                               None if job.faults is None else job.faults.ctypes.data,
                                               ctypes.byref(h)), "ebpf_prog_run_batch_async")
        job.handle = h
        return job

    def run_pcap(self, pcap, want_faults=True):
        """ebpf_prog_run_batch over a PcapBatch as the library built it (its own buffers, pinned
        or not).  Returns (ret, faults, stats) like run_batch."""
        ret = np.zeros(pcap.count, dtype=np.uint64)
        faults = np.zeros(pcap.count, dtype=np.uint8) if want_faults else None
        st = BatchStats()
        _check(lib().ebpf_prog_run_batch(self.ptr, ctypes.byref(pcap.batch), ret.ctypes.data,
                                         None if faults is None else faults.ctypes.data,
                                         ctypes.byref(st)), "ebpf_prog_run_batch")
        return ret, faults, st

    def run_batch_multi(self, devices, data, count, stride=0, offsets=None, want_faults=True,
                        extents=False):
        """ebpf_prog_run_batch_multi: host buffers sharded over ``devices`` (a list of device
        indices, repeats allowed).  Returns (ret, faults, stats) like run_batch."""
        assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
        ret = np.zeros(count, dtype=np.uint64)
        faults = np.zeros(count, dtype=np.uint8) if want_faults else None
        offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        b = _pkt_batch(data.ctypes.data, None if offs is None else offs.ctypes.data,
                       count, stride, extents)
        devs = (ctypes.c_int * len(devices))(*devices)
        st = BatchStats()
        _check(lib().ebpf_prog_run_batch_multi(self.ptr, len(devices), devs, ctypes.byref(b),
                                               ret.ctypes.data,
                                               None if faults is None else faults.ctypes.data,
                                               ctypes.byref(st)), "ebpf_prog_run_batch_multi")
        return ret, faults, st

    def run_batch_multi_dev(self, devices, shards, rets, faults=None, hists=None, streams=None,
                            hist_overwrite=False):
        """ebpf_prog_run_batch_multi_dev.  ``shards``: [(data_ptr, count, stride, offsets_ptr)]
        per device; ``rets`` / ``faults`` / ``hists`` / ``streams``: per-device pointers (ints)."""
        n = len(devices)
        arr = (PktBatch * n)()
        for d, (dp, cnt, stride, op) in enumerate(shards):
            arr[d] = _pkt_batch(dp, op, cnt, stride, hist_overwrite=hist_overwrite)
        P = ctypes.c_void_p * n
        _check(lib().ebpf_prog_run_batch_multi_dev(
            self.ptr, n, (ctypes.c_int * n)(*devices), arr, P(*rets),
            None if faults is None else P(*faults), None if hists is None else P(*hists),
            None if streams is None else P(*streams)), "ebpf_prog_run_batch_multi_dev")

    def device_code(self, layout=1):
        """The program compiled for variant 0 (raw gfx950 code bytes); works without a GPU."""
        n = ctypes.c_size_t(0)
        _check(lib().ebpf_prog_device_code(self.ptr, layout, None, ctypes.byref(n)),
               "ebpf_prog_device_code")
        buf = (ctypes.c_uint8 * max(1, n.value))()
        _check(lib().ebpf_prog_device_code(self.ptr, layout, buf, ctypes.byref(n)),
               "ebpf_prog_device_code")
        return bytes(buf)[: n.value]

    def run_batch_dev(self, device, data_ptr, count, stride, ret_ptr, offsets_ptr=None,
                      faults_ptr=None, hist_ptr=None, stream=None, hist_overwrite=False,
                      extents=False):
        """Device pointers (ints); asynchronous on ``stream`` (hipStream_t as int or None).
        ``hist_overwrite``: the histogram is set to this batch's counts instead of added to."""
        b = _pkt_batch(data_ptr, offsets_ptr, count, stride, extents, hist_overwrite=hist_overwrite)
        _check(lib().ebpf_prog_run_batch_dev(self.ptr, device, ctypes.byref(b), ret_ptr,
                                             faults_ptr, hist_ptr, stream),
               "ebpf_prog_run_batch_dev")


    def launcher(self, device, data_ptr, count, stride, ret_ptr, offsets_ptr=None,
                 faults_ptr=None, stream=None, hist_overwrite=False):
        """A prebound ebpf_prog_run_batch_dev for a bench loop: returns ``launch(hist_ptr)``
        whose only per-call work is the C call itself (batch descriptor and argument
        conversion done once here).  Raises EbpfError on a non-zero return."""
        b = _pkt_batch(data_ptr, offsets_ptr, count, stride, hist_overwrite=hist_overwrite)
        f = lib().ebpf_prog_run_batch_dev
        args = (self.ptr, device, ctypes.byref(b), ret_ptr, faults_ptr)
        st = stream

        def launch(hist_ptr):
            rc = f(*args, hist_ptr, st)
            if rc:
                raise EbpfError(rc, "ebpf_prog_run_batch_dev")
        launch.batch = b  # keeps the descriptor alive with the closure
        return launch


def gpu_count():
    return lib().ebpf_gpu_device_count()


def dev_init(ndev=0):
    """ebpf_dev_init: load the kernels on devices 0..ndev-1 (0: all); raises EbpfError."""
    _check(lib().ebpf_dev_init(ndev), "ebpf_dev_init")


def time_next_launch(start_event, stop_event):
    """The calling thread's next run_batch_dev records these hipEvent_t handles (ints, or None
    to cancel) around the interpreter kernel alone (include/ebpf_gpu.h)."""
    _check(lib().ebpf_gpu_time_next_launch(start_event, stop_event), "ebpf_gpu_time_next_launch")


def steer(ret, faults=None):
    """ebpf_batch_steer on host arrays: (index u32[count], starts u64[STEER_STARTS]);
    index[starts[b]:starts[b + 1]] are the packets of verdict class b, in ascending order."""
    ret = np.ascontiguousarray(ret, dtype=np.uint64)
    if faults is not None:
        faults = np.ascontiguousarray(faults, dtype=np.uint8)
        assert len(faults) == len(ret)
    index = np.zeros(len(ret), dtype=np.uint32)
    starts = np.zeros(STEER_STARTS, dtype=np.uint64)
    _check(lib().ebpf_batch_steer(ret.ctypes.data if len(ret) else None,
                                  None if faults is None or not len(ret) else faults.ctypes.data,
                                  len(ret), index.ctypes.data if len(ret) else None,
                                  starts.ctypes.data), "ebpf_batch_steer")
    return index, starts


def steer_dev(device, ret_ptr, faults_ptr, count, index_ptr, starts_ptr, stream=None):
    """ebpf_batch_steer_dev: device pointers (ints); asynchronous on ``stream``."""
    _check(lib().ebpf_batch_steer_dev(device, ret_ptr, faults_ptr, count, index_ptr, starts_ptr,
                                      stream), "ebpf_batch_steer_dev")


def select_dev(device, data_ptr, count, stride, index_ptr, n, extents_ptr, offsets_ptr=None,
               stream=None, extents=False):
    """ebpf_batch_select_dev: the (start, end) pairs of packets index[0..n) of the batch
    (data_ptr, count, stride, offsets_ptr, extents) as run_batch_dev takes it, written to
    ``extents_ptr`` (2n u64); device pointers (ints); asynchronous on ``stream``."""
    b = _pkt_batch(data_ptr, offsets_ptr, count, stride, extents)
    _check(lib().ebpf_batch_select_dev(device, ctypes.byref(b), index_ptr, n, extents_ptr,
                                       stream), "ebpf_batch_select_dev")


def group_tmp_bytes(count, key_bits):
    """ebpf_batch_group_tmp_bytes: the bytes of temporary device storage a group_dev call needs"""
    return int(lib().ebpf_batch_group_tmp_bytes(count, key_bits))


def group(ret, faults=None, key_shift=0, key_bits=32, group_cap=None):
    """ebpf_batch_group on host arrays: the packets sorted stably by the key
    (ret >> key_shift) & (2**key_bits - 1), faulted packets last.  Returns (index u32[count],
    group_keys u64[group_cap], group_starts u64[group_cap + 1], info u64[2] = (groups,
    unfaulted), code) with code 0 or errno.ENOSPC (more groups than ``group_cap``; the tables
    then hold what fits).  ``group_cap`` None sizes the tables to fit."""
    ret = np.ascontiguousarray(ret, dtype=np.uint64)
    n = len(ret)
    if faults is not None:
        faults = np.ascontiguousarray(faults, dtype=np.uint8)
        assert len(faults) == n
    cap = n if group_cap is None else group_cap
    index = np.zeros(n, dtype=np.uint32)
    group_keys = np.zeros(cap, dtype=np.uint64)
    group_starts = np.zeros(cap + 1, dtype=np.uint64)
    info = np.zeros(2, dtype=np.uint64)
    code = lib().ebpf_batch_group(ret.ctypes.data if n else None,
                                  None if faults is None or not n else faults.ctypes.data, n,
                                  key_shift, key_bits, index.ctypes.data if n else None, cap,
                                  group_keys.ctypes.data if cap else None,
                                  group_starts.ctypes.data, info.ctypes.data)
    if code not in (0, errno.ENOSPC):
        raise EbpfError(code, "ebpf_batch_group")
    return index, group_keys, group_starts, info, code


def group_dev(device, ret_ptr, faults_ptr, count, key_shift, key_bits, index_ptr, group_cap,
              group_keys_ptr, group_starts_ptr, info_ptr, tmp_ptr, tmp_bytes, stream=None):
    """ebpf_batch_group_dev: device pointers (ints); ``tmp_ptr`` is the caller's temporary
    storage of at least group_tmp_bytes(count, key_bits); asynchronous on ``stream``."""
    _check(lib().ebpf_batch_group_dev(device, ret_ptr, faults_ptr, count, key_shift, key_bits,
                                      index_ptr, group_cap, group_keys_ptr, group_starts_ptr,
                                      info_ptr, tmp_ptr, tmp_bytes, stream),
           "ebpf_batch_group_dev")


SUMS = ("bytes", "sum", "min", "max", "bits")   # struct ebpf_batch_sums' members, in order


def reduce(index, seg_starts, ret=None, val_shift=0, val_bits=64, count=None, stride=0,
           offsets=None, extents=False, nseg=None, want=SUMS):
    """ebpf_batch_reduce on host arrays: per segment index[seg_starts[g]:seg_starts[g + 1]] of the
    list, the outputs named in ``want``: "bytes" (the packets' lengths, of the batch (count,
    stride, offsets, extents) as run_batch takes it; no packet data is needed), and "sum", "min",
    "max", "bits" of the field (ret >> val_shift) & (2**val_bits - 1).  ``seg_starts`` has
    seg_cap + 1 entries; ``nseg`` (None: every one of the seg_cap segments) is the number of
    segments as ebpf_batch_group's info[0] gives it.  Returns (bytes, sum, min, max, bits, code):
    u64[seg_cap] each, or None where not wanted; entries at or past the segments reduced are 0.
    code is 0 or errno.EINVAL for a table that decreases or ends past the list."""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    seg_starts = np.ascontiguousarray(seg_starts, dtype=np.uint64)
    cap = max(len(seg_starts) - 1, 0)
    if ret is not None:
        ret = np.ascontiguousarray(ret, dtype=np.uint64)
    if count is None:
        count = 0 if ret is None else len(ret)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    b = None
    if "bytes" in want:   # (data: never read, but a batch with packets names some)
        b = _pkt_batch(1 if count else None, None if offs is None else offs.ctypes.data,
                       count, stride, extents)
    outs = [np.zeros(cap, dtype=np.uint64) if name in want else None for name in SUMS]
    sums = BatchSums(*[None if o is None or not cap else o.ctypes.data for o in outs])
    ns = None if nseg is None else np.array([nseg], dtype=np.uint64)
    code = lib().ebpf_batch_reduce(None if b is None else ctypes.byref(b),
                                   None if ret is None or not len(ret) else ret.ctypes.data,
                                   count, val_shift, val_bits,
                                   index.ctypes.data if len(index) else None, len(index),
                                   seg_starts.ctypes.data if len(seg_starts) else None, cap,
                                   None if ns is None else ns.ctypes.data, ctypes.byref(sums))
    if code not in (0, errno.EINVAL):
        raise EbpfError(code, "ebpf_batch_reduce")
    return (*outs, code)


def reduce_dev(device, ret_ptr, count, val_shift, val_bits, index_ptr, n, seg_starts_ptr, seg_cap,
               nseg_ptr=None, bytes_ptr=None, sum_ptr=None, min_ptr=None, max_ptr=None,
               bits_ptr=None, stride=0, offsets_ptr=None, extents=False, data_ptr=None,
               stream=None):
    """ebpf_batch_reduce_dev: device pointers (ints); the outputs that are wanted are given, each
    seg_cap u64.  The batch (count, stride, offsets_ptr, extents) as run_batch_dev takes it is
    needed for ``bytes_ptr`` alone; ``data_ptr`` is never read (None: a stand-in).  Asynchronous
    on ``stream``."""
    b = None
    if bytes_ptr is not None:
        b = _pkt_batch(data_ptr or (1 if count else None), offsets_ptr, count, stride, extents)
    sums = BatchSums(bytes_ptr, sum_ptr, min_ptr, max_ptr, bits_ptr)
    _check(lib().ebpf_batch_reduce_dev(device, None if b is None else ctypes.byref(b), ret_ptr,
                                       count, val_shift, val_bits, index_ptr, n, seg_starts_ptr,
                                       seg_cap, nseg_ptr, ctypes.byref(sums), stream),
           "ebpf_batch_reduce_dev")


SCANS = ("rank", "bytes_before", "sum_before", "over")   # struct ebpf_batch_scans' members, in order
_SCAN_TYPES = {"rank": np.uint32, "bytes_before": np.uint64, "sum_before": np.uint64,
               "over": np.uint8}


def scan(index, seg_starts, ret=None, val_shift=0, val_bits=64, count=None, stride=0,
         offsets=None, extents=False, nseg=None, budgets=None, want=SCANS):
    """ebpf_batch_scan on host arrays: per position j of the list, within its segment
    index[seg_starts[g]:seg_starts[g + 1]], the outputs named in ``want``: "rank" (the segment's
    entries before j), "bytes_before" (their lengths, of the batch (count, stride, offsets,
    extents) as run_batch takes it; no packet data is needed), "sum_before" (their values of the
    field (ret >> val_shift) & (2**val_bits - 1)) and "over" (1 iff bytes_before plus the entry's
    own length passes ``budgets[g]``; budgets has seg_cap entries).  ``seg_starts`` and ``nseg``
    are as reduce() takes them.  Returns (rank u32[n], bytes_before u64[n], sum_before u64[n],
    over u8[n], code), None where not wanted; positions that no segment covers hold 0.  code is 0
    or errno.EINVAL for a table that decreases or ends past the list."""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    seg_starts = np.ascontiguousarray(seg_starts, dtype=np.uint64)
    cap = max(len(seg_starts) - 1, 0)
    n = len(index)
    if ret is not None:
        ret = np.ascontiguousarray(ret, dtype=np.uint64)
    if count is None:
        count = 0 if ret is None else len(ret)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    if budgets is not None:
        budgets = np.ascontiguousarray(budgets, dtype=np.uint64)
        assert len(budgets) == cap
    b = None
    if "bytes_before" in want or "over" in want:   # (data: never read)
        b = _pkt_batch(1 if count else None, None if offs is None else offs.ctypes.data,
                       count, stride, extents)
    outs = [np.zeros(n, dtype=_SCAN_TYPES[name]) if name in want else None for name in SCANS]
    scans = BatchScans(*[None if o is None else o.ctypes.data or 1 for o in outs])
    ns = None if nseg is None else np.array([nseg], dtype=np.uint64)
    code = lib().ebpf_batch_scan(None if b is None else ctypes.byref(b),
                                 None if ret is None else ret.ctypes.data or 1,
                                 count, val_shift, val_bits, index.ctypes.data if n else None, n,
                                 seg_starts.ctypes.data if len(seg_starts) else None, cap,
                                 None if ns is None else ns.ctypes.data,
                                 None if budgets is None else budgets.ctypes.data or 1,
                                 ctypes.byref(scans))
    if code not in (0, errno.EINVAL):
        raise EbpfError(code, "ebpf_batch_scan")
    return (*outs, code)


def scan_dev(device, ret_ptr, count, val_shift, val_bits, index_ptr, n, seg_starts_ptr, seg_cap,
             nseg_ptr=None, budgets_ptr=None, rank_ptr=None, bytes_before_ptr=None,
             sum_before_ptr=None, over_ptr=None, stride=0, offsets_ptr=None, extents=False,
             data_ptr=None, stream=None):
    """ebpf_batch_scan_dev: device pointers (ints); the outputs that are wanted are given, each n
    entries (rank u32, bytes_before and sum_before u64, over u8).  The batch (count, stride,
    offsets_ptr, extents) as run_batch_dev takes it is needed for ``bytes_before_ptr`` and
    ``over_ptr`` alone, ``budgets_ptr`` (seg_cap u64) for ``over_ptr``; ``data_ptr`` is never read
    (None: a stand-in).  Asynchronous on ``stream``."""
    b = None
    if bytes_before_ptr is not None or over_ptr is not None:
        b = _pkt_batch(data_ptr or (1 if count else None), offsets_ptr, count, stride, extents)
    scans = BatchScans(rank_ptr, bytes_before_ptr, sum_before_ptr, over_ptr)
    _check(lib().ebpf_batch_scan_dev(device, None if b is None else ctypes.byref(b), ret_ptr,
                                     count, val_shift, val_bits, index_ptr, n, seg_starts_ptr,
                                     seg_cap, nseg_ptr, budgets_ptr, ctypes.byref(scans), stream),
           "ebpf_batch_scan_dev")


PARTS = ("kept", "kept_starts", "dropped", "dropped_starts")   # struct ebpf_batch_parts' members


def filter(index, seg_starts=None, flags=None, rank=None, rank_below=0, ret=None, val_shift=0,
           val_bits=64, val_lo=0, val_hi=(1 << 64) - 1, count=None, nseg=None, want=PARTS):
    """ebpf_batch_filter on host arrays: the entries of the list whose position passes every test
    that is given — ``flags[j] == 0``, ``rank[j] < rank_below``, and val_lo <= (ret[index[j]] >>
    val_shift) & (2**val_bits - 1) <= val_hi — in list order, and those that fail, with the tables
    of the segments they inherit.  ``seg_starts`` and ``nseg`` are as reduce() takes them;
    ``seg_starts`` None is an unsegmented list (no tables then).  Returns (kept u32[n],
    kept_starts u64[seg_cap + 1], dropped u32[n], dropped_starts u64[seg_cap + 1], info u64[2] =
    (kept, dropped), code), None where not wanted (``want`` names them); the lists' tails hold
    EBPF_NO_PACKET, table entries past the segments 0.  code is 0 or errno.EINVAL for a table that
    decreases or ends past the list."""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    n = len(index)
    if seg_starts is not None:
        seg_starts = np.ascontiguousarray(seg_starts, dtype=np.uint64)
        assert len(seg_starts) >= 1
    cap = 0 if seg_starts is None else len(seg_starts) - 1
    if flags is not None:
        flags = np.ascontiguousarray(flags, dtype=np.uint8)
        assert len(flags) == n
    if rank is not None:
        rank = np.ascontiguousarray(rank, dtype=np.uint32)
        assert len(rank) == n
    if ret is not None:
        ret = np.ascontiguousarray(ret, dtype=np.uint64)
    if count is None:
        count = 0 if ret is None else len(ret)
    test = BatchTest(None if flags is None else flags.ctypes.data or 1,
                     None if rank is None else rank.ctypes.data or 1, rank_below,
                     None if ret is None else ret.ctypes.data or 1, val_shift, val_bits,
                     val_lo, val_hi)
    if seg_starts is None:
        want = [k for k in want if not k.endswith("_starts")]
    outs = [(np.zeros(cap + 1 if k.endswith("_starts") else n,
                      dtype=np.uint64 if k.endswith("_starts") else np.uint32)
             if k in want else None) for k in PARTS]
    parts = BatchParts(*[None if o is None else o.ctypes.data or 1 for o in outs])
    info = np.zeros(2, dtype=np.uint64)
    ns = None if nseg is None else np.array([nseg], dtype=np.uint64)
    code = lib().ebpf_batch_filter(ctypes.byref(test), count, index.ctypes.data if n else None, n,
                                   None if seg_starts is None else seg_starts.ctypes.data, cap,
                                   None if ns is None else ns.ctypes.data, ctypes.byref(parts),
                                   info.ctypes.data)
    if code not in (0, errno.EINVAL):
        raise EbpfError(code, "ebpf_batch_filter")
    return (*outs, info, code)


def filter_dev(device, count, index_ptr, n, seg_starts_ptr, seg_cap, info_ptr, nseg_ptr=None,
               flags_ptr=None, rank_ptr=None, rank_below=0, ret_ptr=None, val_shift=0,
               val_bits=64, val_lo=0, val_hi=(1 << 64) - 1, kept_ptr=None, kept_starts_ptr=None,
               dropped_ptr=None, dropped_starts_ptr=None, stream=None):
    """ebpf_batch_filter_dev: device pointers (ints); the tests that are given apply, the outputs
    that are wanted are given (kept and dropped n u32, their tables seg_cap + 1 u64);
    ``info_ptr`` (2 u64) gets the numbers kept and dropped.  ``seg_starts_ptr`` None: an
    unsegmented list.  Asynchronous on ``stream``."""
    test = BatchTest(flags_ptr, rank_ptr, rank_below, ret_ptr, val_shift, val_bits, val_lo, val_hi)
    parts = BatchParts(kept_ptr, kept_starts_ptr, dropped_ptr, dropped_starts_ptr)
    _check(lib().ebpf_batch_filter_dev(device, ctypes.byref(test), count, index_ptr, n,
                                       seg_starts_ptr, seg_cap, nseg_ptr, ctypes.byref(parts),
                                       info_ptr, stream), "ebpf_batch_filter_dev")


def _key_table(keys, vals, n):
    """(KeyTable, the arrays it points into) of host arrays; n None: every entry is valid"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    assert len(keys) == len(vals)
    cnt = np.array([len(keys) if n is None else n], dtype=np.uint64)
    cap = len(keys)
    return KeyTable(keys.ctypes.data if cap else None, vals.ctypes.data if cap else None, cap,
                    cnt.ctypes.data), (keys, vals, cnt)


def lookup(table_keys, table_vals, keys, mode=LOOKUP_VALUE, missing=0, limit=0, n=None,
           nkeys=None, want=("vals", "pos")):
    """ebpf_batch_lookup on host arrays: ``keys`` (any order) looked up in the table
    (``table_keys`` strictly ascending, ``table_vals`` beside them; ``n`` (None: all) is the
    table's *n).  ``nkeys`` (None: every key) is the number of keys as ebpf_batch_group's info[0]
    gives it.  Returns (vals u64[key_cap], pos u32[key_cap], code), None where not wanted: per key
    the table's value or ``missing`` (LOOKUP_VALUE), or what is left of ``limit`` after it
    (LOOKUP_REMAINING), and its position or EBPF_NO_ENTRY; entries at or past the keys used are 0.
    code is 0 or errno.EINVAL for a table that is not strictly ascending."""
    table, hold = _key_table(table_keys, table_vals, n)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    cap = len(keys)
    vals = np.zeros(cap, dtype=np.uint64) if "vals" in want else None
    pos = np.zeros(cap, dtype=np.uint32) if "pos" in want else None
    nk = None if nkeys is None else np.array([nkeys], dtype=np.uint64)
    code = lib().ebpf_batch_lookup(ctypes.byref(table), keys.ctypes.data if cap else None, cap,
                                   None if nk is None else nk.ctypes.data, mode, missing, limit,
                                   None if vals is None else vals.ctypes.data or 1,
                                   None if pos is None else pos.ctypes.data or 1)
    if code not in (0, errno.EINVAL):
        raise EbpfError(code, "ebpf_batch_lookup")
    return vals, pos, code


def lookup_dev(device, table_keys_ptr, table_vals_ptr, table_cap, table_n_ptr, keys_ptr, key_cap,
               nkeys_ptr=None, mode=LOOKUP_VALUE, missing=0, limit=0, vals_out_ptr=None,
               pos_out_ptr=None, stream=None):
    """ebpf_batch_lookup_dev: device pointers (ints); the table is (keys, vals, cap, n), the
    outputs that are wanted are given (vals_out key_cap u64, pos_out key_cap u32).  Asynchronous
    on ``stream``."""
    table = KeyTable(table_keys_ptr, table_vals_ptr, table_cap, table_n_ptr)
    _check(lib().ebpf_batch_lookup_dev(device, ctypes.byref(table), keys_ptr, key_cap, nkeys_ptr,
                                       mode, missing, limit, vals_out_ptr, pos_out_ptr, stream),
           "ebpf_batch_lookup_dev")


def accumulate(table_keys, table_vals, keys, adds, op=ACC_ADD, keep_lo=0, keep_hi=(1 << 64) - 1,
               out_cap=None, n=None, nkeys=None):
    """ebpf_batch_accumulate on host arrays: the table (``table_keys`` None: no table; ``n`` as
    lookup() takes it) merged with the batch's ``keys`` (strictly ascending) and ``adds`` under
    ``op``, the candidates whose value lies in [keep_lo, keep_hi] kept.  ``out_cap`` (None: room
    for every candidate) is the new table's cap.  Returns (out_keys u64[out_cap], out_vals
    u64[out_cap], out_n, info u64[3] = (kept, kept and new, left out), code): entries at or past
    min(out_n, out_cap) are 0.  code is 0, errno.ENOSPC for out_n > out_cap, or errno.EINVAL for a
    table or keys that are not strictly ascending."""
    table, hold = (None, None) if table_keys is None else _key_table(table_keys, table_vals, n)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    adds = np.ascontiguousarray(adds, dtype=np.uint64)
    cap = len(keys)
    assert len(adds) == cap
    if out_cap is None:
        out_cap = cap + (0 if table is None else table.cap)
    out, (okeys, ovals, on) = _key_table(np.zeros(out_cap, dtype=np.uint64),
                                         np.zeros(out_cap, dtype=np.uint64), 0)
    info = np.zeros(3, dtype=np.uint64)
    nk = None if nkeys is None else np.array([nkeys], dtype=np.uint64)
    code = lib().ebpf_batch_accumulate(None if table is None else ctypes.byref(table),
                                       keys.ctypes.data if cap else None,
                                       adds.ctypes.data if cap else None, cap,
                                       None if nk is None else nk.ctypes.data, op, keep_lo,
                                       keep_hi, ctypes.byref(out), info.ctypes.data)
    if code not in (0, errno.EINVAL, errno.ENOSPC):
        raise EbpfError(code, "ebpf_batch_accumulate")
    return okeys, ovals, int(on[0]), info, code


def accumulate_dev(device, in_table, keys_ptr, adds_ptr, key_cap, out_table, info_ptr,
                   nkeys_ptr=None, op=ACC_ADD, keep_lo=0, keep_hi=(1 << 64) - 1, stream=None):
    """ebpf_batch_accumulate_dev: device pointers (ints); ``in_table`` (None: no table) and
    ``out_table`` are (keys_ptr, vals_ptr, cap, n_ptr); ``info_ptr`` (3 u64) gets the numbers kept,
    kept and new, and left out.  Asynchronous on ``stream``."""
    tin = None if in_table is None else KeyTable(*in_table)
    tout = KeyTable(*out_table)
    _check(lib().ebpf_batch_accumulate_dev(device, None if tin is None else ctypes.byref(tin),
                                           keys_ptr, adds_ptr, key_cap, nkeys_ptr, op, keep_lo,
                                           keep_hi, ctypes.byref(tout), info_ptr, stream),
           "ebpf_batch_accumulate_dev")


def rollup(keys, vals, key_shift, flags=0, val_shift=0, val_bits=64, out_cap=None, n=None,
           want=ROLLS):
    """ebpf_batch_rollup on host arrays: the runs of equal ``key >> key_shift`` of ``keys`` reduced
    (``vals`` beside them, or None when no output of ``want`` reads them: sum, min, max, bits).
    ``n`` (None: every entry) is *n: the table's count, or with ROLLUP_SEGMENTS ebpf_batch_group's
    info[0].  ``out_cap`` (None: room for every run) is the outputs' size.  Returns ({member: u64
    array of the min(C, out_cap) entries written; starts one more when C <= out_cap}, info u64[2]
    = (C, N), code) with the members not wanted absent; code is 0 or errno.ENOSPC for C >
    out_cap."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    cap = len(keys)
    if vals is not None:
        vals = np.ascontiguousarray(vals, dtype=np.uint64)
        assert len(vals) == cap
    want = tuple(w for w in ROLLS if w in want and
                 (vals is not None or w not in ("sum", "min", "max", "bits")))
    if out_cap is None:
        out_cap = cap
    out = {w: np.zeros(out_cap + (w == "starts"), dtype=np.uint64) for w in want}
    rolls = BatchRolls(*[out[w].ctypes.data or 1 if w in out else None for w in ROLLS])
    info = np.zeros(2, dtype=np.uint64)
    cnt = None if n is None else np.array([n], dtype=np.uint64)
    code = lib().ebpf_batch_rollup(keys.ctypes.data if cap else None,
                                   vals.ctypes.data if vals is not None and cap else None, cap,
                                   None if cnt is None else cnt.ctypes.data, flags, key_shift,
                                   val_shift, val_bits, out_cap, ctypes.byref(rolls),
                                   info.ctypes.data)
    if code not in (0, errno.ENOSPC):
        raise EbpfError(code, "ebpf_batch_rollup")
    C = int(info[0])
    m = min(C, out_cap)
    return ({w: out[w][:m + (w == "starts" and C <= out_cap)] for w in want}, info, code)


def rollup_dev(device, keys_ptr, vals_ptr, cap, n_ptr, key_shift, out_cap, info_ptr, flags=0,
               val_shift=0, val_bits=64, keys_out_ptr=None, count_ptr=None, sum_ptr=None,
               min_ptr=None, max_ptr=None, bits_ptr=None, starts_ptr=None, stream=None):
    """ebpf_batch_rollup_dev: device pointers (ints); the sequence is (keys, vals, cap, n), the
    outputs that are wanted are given (out_cap u64 each, starts out_cap + 1); ``info_ptr`` (2 u64)
    gets C and N.  Asynchronous on ``stream``."""
    rolls = BatchRolls(keys_out_ptr, count_ptr, sum_ptr, min_ptr, max_ptr, bits_ptr, starts_ptr)
    _check(lib().ebpf_batch_rollup_dev(device, keys_ptr, vals_ptr, cap, n_ptr, flags, key_shift,
                                       val_shift, val_bits, out_cap, ctypes.byref(rolls), info_ptr,
                                       stream),
           "ebpf_batch_rollup_dev")


def top(keys, vals, k, flags=TOP_LARGEST, val_shift=0, val_bits=64, n=None,
        want=("keys", "vals", "pos")):
    """ebpf_batch_top on host arrays: the ``k`` best entries of ``vals`` (``keys`` beside them, or
    None) by the field (val_shift, val_bits), largest first, or smallest with TOP_SMALLEST, equal
    fields by position.  ``n`` (None: every entry) is *n: the table's count, or with TOP_SEGMENTS
    ebpf_batch_group's info[0].  Returns (keys u64[m], vals u64[m], pos u32[m], info u64[4] = (m,
    N, the cut, the entries of the cut's field left out)), None where not wanted."""
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    cap = len(vals)
    if keys is not None:
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert len(keys) == cap
    out = {"keys": np.zeros(k, dtype=np.uint64) if "keys" in want and keys is not None else None,
           "vals": np.zeros(k, dtype=np.uint64) if "vals" in want else None,
           "pos": np.zeros(k, dtype=np.uint32) if "pos" in want else None}
    tops = BatchTops(*[None if out[f] is None else out[f].ctypes.data or 1
                       for f in ("keys", "vals", "pos")])
    info = np.zeros(4, dtype=np.uint64)
    cnt = None if n is None else np.array([n], dtype=np.uint64)
    _check(lib().ebpf_batch_top(keys.ctypes.data if keys is not None and cap else None,
                                vals.ctypes.data if cap else None, cap,
                                None if cnt is None else cnt.ctypes.data, flags, val_shift,
                                val_bits, k, ctypes.byref(tops), info.ctypes.data),
           "ebpf_batch_top")
    m = int(info[0])
    return tuple(None if out[f] is None else out[f][:m] for f in ("keys", "vals", "pos")) + (info,)


def top_dev(device, keys_ptr, vals_ptr, cap, n_ptr, k, info_ptr, flags=TOP_LARGEST, val_shift=0,
            val_bits=64, keys_out_ptr=None, vals_out_ptr=None, pos_out_ptr=None, stream=None):
    """ebpf_batch_top_dev: device pointers (ints); the sequence is (keys, vals, cap, n), the outputs
    that are wanted are given (k entries each: keys_out and vals_out u64, pos_out u32);
    ``info_ptr`` (4 u64) gets m, N, the cut and the entries of the cut's field left out.
    Asynchronous on ``stream``."""
    tops = BatchTops(keys_out_ptr, vals_out_ptr, pos_out_ptr)
    _check(lib().ebpf_batch_top_dev(device, keys_ptr, vals_ptr, cap, n_ptr, flags, val_shift,
                                    val_bits, k, ctypes.byref(tops), info_ptr, stream),
           "ebpf_batch_top_dev")


def gather(data, count, index, out_stride=0, stride=0, offsets=None, extents=False,
           out_bytes=None):
    """ebpf_batch_gather on host arrays: packets ``index`` of the batch (data, count, stride,
    offsets, extents) as run_batch takes it.  Strided form (``out_stride`` > 0): returns
    (out u8[len(index) * out_stride], None, 0).  Packed form (``out_stride`` 0): returns
    (out u8[out_bytes], out_offsets u64[len(index) + 1], code) with code 0 or errno.ENOSPC;
    ``out_bytes`` None sizes the output to fit."""
    assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"]
    index = np.ascontiguousarray(index, dtype=np.uint32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    b = _pkt_batch(data.ctypes.data, None if offs is None else offs.ctypes.data,
                   count, stride, extents)
    n = len(index)
    f = lib().ebpf_batch_gather
    if out_stride:
        out = np.zeros(n * out_stride, dtype=np.uint8)
        _check(f(ctypes.byref(b), index.ctypes.data, n, out_stride, out.ctypes.data, out.nbytes,
                 None), "ebpf_batch_gather")
        return out, None, 0
    out_offsets = np.zeros(n + 1, dtype=np.uint64)
    if out_bytes is None:   # (snprintf's rule: a first call with no room says how much is needed)
        code = f(ctypes.byref(b), index.ctypes.data, n, 0, np.zeros(1, dtype=np.uint8).ctypes.data,
                 0, out_offsets.ctypes.data)
        if code not in (0, errno.ENOSPC):
            raise EbpfError(code, "ebpf_batch_gather")
        out_bytes = int(out_offsets[n])
    out = np.zeros(max(out_bytes, 1), dtype=np.uint8)
    code = f(ctypes.byref(b), index.ctypes.data, n, 0, out.ctypes.data, out_bytes,
             out_offsets.ctypes.data)
    if code not in (0, errno.ENOSPC):
        raise EbpfError(code, "ebpf_batch_gather")
    return out[:out_bytes], out_offsets, code


def gather_dev(device, data_ptr, count, stride, index_ptr, n, out_stride, out_ptr, out_bytes,
               out_offsets_ptr=None, offsets_ptr=None, stream=None, extents=False):
    """ebpf_batch_gather_dev: packets index[0..n) of the batch (data_ptr, count, stride,
    offsets_ptr, extents) as run_batch_dev takes it, copied to ``out_ptr``: slots of
    ``out_stride`` bytes, or (``out_stride`` 0) packed, with their n + 1 offsets written to
    ``out_offsets_ptr``; device pointers (ints); asynchronous on ``stream``."""
    b = _pkt_batch(data_ptr, offsets_ptr, count, stride, extents)
    _check(lib().ebpf_batch_gather_dev(device, ctypes.byref(b), index_ptr, n, out_stride, out_ptr,
                                       out_bytes, out_offsets_ptr, stream),
           "ebpf_batch_gather_dev")


def scatter(data, count, index, dense, in_stride=0, stride=0, offsets=None, extents=False,
            in_offsets=None, in_bytes=None):
    """ebpf_batch_scatter on host arrays: the slots of ``dense`` (``in_stride`` bytes each, or
    packed at ``in_offsets``) written back, in place, into packets ``index`` of the batch (data,
    count, stride, offsets, extents) as run_batch takes it.  ``in_bytes`` None: all of
    ``dense``."""
    assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"] and data.flags["WRITEABLE"]
    dense = np.ascontiguousarray(dense, dtype=np.uint8)
    index = np.ascontiguousarray(index, dtype=np.uint32)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    in_offs = None if in_offsets is None else np.ascontiguousarray(in_offsets, dtype=np.uint64)
    b = _pkt_batch(data.ctypes.data, None if offs is None else offs.ctypes.data,
                   count, stride, extents)
    _check(lib().ebpf_batch_scatter(ctypes.byref(b), index.ctypes.data, len(index), in_stride,
                                    dense.ctypes.data, len(dense) if in_bytes is None else in_bytes,
                                    None if in_offs is None else in_offs.ctypes.data),
           "ebpf_batch_scatter")


def scatter_dev(device, data_ptr, count, stride, index_ptr, n, in_stride, in_ptr, in_bytes,
                in_offsets_ptr=None, offsets_ptr=None, stream=None, extents=False):
    """ebpf_batch_scatter_dev: the slots at ``in_ptr`` (``in_stride`` bytes each, or
    (``in_stride`` 0) packed at the n + 1 offsets of ``in_offsets_ptr``) written back into packets
    index[0..n) of the batch (data_ptr, count, stride, offsets_ptr, extents); device pointers
    (ints); asynchronous on ``stream``."""
    b = _pkt_batch(data_ptr, offsets_ptr, count, stride, extents)
    _check(lib().ebpf_batch_scatter_dev(device, ctypes.byref(b), index_ptr, n, in_stride, in_ptr,
                                        in_bytes, in_offsets_ptr, stream),
           "ebpf_batch_scatter_dev")


def merge(ret, faults, index, ret2, faults2=None):
    """ebpf_batch_merge on host arrays, in place: ret[index[j]] = ret2[j] and (``faults`` given)
    faults[index[j]] = faults2[j], or 0 without ``faults2``."""
    assert ret.dtype == np.uint64 and ret.flags["C_CONTIGUOUS"] and ret.flags["WRITEABLE"]
    assert faults is None or (faults.dtype == np.uint8 and faults.flags["C_CONTIGUOUS"]
                              and len(faults) == len(ret))
    index = np.ascontiguousarray(index, dtype=np.uint32)
    ret2 = np.ascontiguousarray(ret2, dtype=np.uint64)
    if faults2 is not None:
        faults2 = np.ascontiguousarray(faults2, dtype=np.uint8)
        assert len(faults2) == len(index)
    assert len(ret2) == len(index)
    _check(lib().ebpf_batch_merge(ret.ctypes.data, None if faults is None else faults.ctypes.data,
                                  len(ret), index.ctypes.data, len(index), ret2.ctypes.data,
                                  None if faults2 is None else faults2.ctypes.data),
           "ebpf_batch_merge")


def merge_dev(device, ret_ptr, faults_ptr, count, index_ptr, n, ret2_ptr, faults2_ptr=None,
              stream=None):
    """ebpf_batch_merge_dev: device pointers (ints); asynchronous on ``stream``."""
    _check(lib().ebpf_batch_merge_dev(device, ret_ptr, faults_ptr, count, index_ptr, n, ret2_ptr,
                                      faults2_ptr, stream), "ebpf_batch_merge_dev")


def set_variant(v):
    _check(lib().ebpf_gpu_set_variant(v), "ebpf_gpu_set_variant")
