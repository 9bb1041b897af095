"""Steering a batch by verdict on the device (include/ebpf_gpu.h: ebpf_batch_steer_dev,
ebpf_batch_select_dev; csrc/hip/steer.hip) against numpy's stable sort and against the host
function.  A stable partition has one right answer: every comparison is exact.

Shapes: T = native.STEER_TILE packets go to one workgroup, a quarter of them to each of its four
waves in 64-packet chunks, so the counts sit around 64, 256 and T; above 256 tiles the tile scan
takes its second level, which 2M + 5 packets (513 tiles) reach."""
import functools

import numpy as np
import pytest

import pyoracle
from generic_ebpf_amd import native as _native
from test_steer import U64, expected

pytestmark = pytest.mark.gpu

T = _native.STEER_TILE
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
BIG = (2 << 20) + 5
PATTERNS = ["one", "two", "mod257", "div64", "rand4", "rand257", "only256", "clamp"]
CLAMP = np.array([254, 255, 256, 1 << 32, (1 << 64) - 1, 7], dtype=U64)


@functools.lru_cache(maxsize=None)
def pattern(name, n):
    """(ret, faults) of n packets; a faulted packet has ret 0 but in "clamp", where every 11th
    packet is faulted with its ret left as it is"""
    i = np.arange(n, dtype=np.int64)
    g = np.random.default_rng(n + len(name))
    if name == "clamp":
        ret = CLAMP[i % len(CLAMP)]
        faults = np.where(i % 11 == 10, 5, 0).astype(np.uint8)
        return ret, faults
    cls = {"one": lambda: np.full(n, 3), "two": lambda: np.where(i % 2 == 0, 9, 2),
           "mod257": lambda: i % 257, "div64": lambda: (i // 64) % 257,
           "rand4": lambda: g.choice([0, 1, 17, 255], n), "rand257": lambda: g.integers(0, 257, n),
           "only256": lambda: np.full(n, 256)}[name]()
    faults = np.where(cls == 256, 1 + i % 11, 0).astype(np.uint8)
    return np.where(cls == 256, 0, cls).astype(U64), faults


@functools.lru_cache(maxsize=None)
def want(name, n, with_faults):
    """numpy's answer, checked once against the host function"""
    ret, faults = pattern(name, n)
    index, starts = expected(ret, faults if with_faults else None)
    h_index, h_starts = _native.steer(ret, faults if with_faults else None)
    np.testing.assert_array_equal(h_starts, starts)
    np.testing.assert_array_equal(h_index, index)
    return index, starts


class Dev:
    """one steering call's device buffers; outputs pre-filled with a value no result holds"""

    def __init__(self, ret, faults):
        import torch
        dev = torch.device("cuda:0")
        self.n = len(ret)
        self.ret = torch.from_numpy(np.ascontiguousarray(ret).view(np.int64)).to(dev)
        self.faults = None if faults is None else torch.from_numpy(faults).to(dev)
        self.index = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        self.starts = torch.full((258,), -1, dtype=torch.int64, device=dev)

    def enqueue(self, gpu, stream):
        gpu.steer_dev(0, self.ret.data_ptr() if self.n else None,
                      None if self.faults is None or not self.n else self.faults.data_ptr(),
                      self.n, self.index.data_ptr() if self.n else None, self.starts.data_ptr(),
                      stream.cuda_stream)

    def result(self):
        return (self.index.cpu().numpy().view(np.uint32)[:self.n],
                self.starts.cpu().numpy().view(U64))


def steer(gpu, ret, faults):
    import torch
    d = Dev(ret, faults)
    d.enqueue(gpu, torch.cuda.current_stream())
    torch.cuda.synchronize()
    return d.result()


def check(gpu, name, n, with_faults):
    ret, faults = pattern(name, n)
    index, starts = steer(gpu, ret, faults if with_faults else None)
    w_index, w_starts = want(name, n, with_faults)
    np.testing.assert_array_equal(starts, w_starts, err_msg="%s %d" % (name, n))
    np.testing.assert_array_equal(index, w_index, err_msg="%s %d" % (name, n))


@pytest.mark.parametrize("count", COUNTS)
def test_steer_counts_and_patterns(gpu, count):
    for name in PATTERNS:
        for with_faults in (True, False):
            check(gpu, name, count, with_faults)


@pytest.mark.parametrize("name", PATTERNS)
def test_steer_two_level_scan(gpu, name):
    check(gpu, name, BIG, True)
    if name in ("only256", "clamp"):
        check(gpu, name, BIG, False)


def test_steer_same_call_twice(gpu):
    ret, faults = pattern("rand257", 3 * T + 17)
    a = steer(gpu, ret, faults)
    b = steer(gpu, ret, faults)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    np.testing.assert_array_equal(a[0], want("rand257", 3 * T + 17, True)[0])


def test_steer_scratch_grows_on_a_stream(gpu):
    """a fresh stream: its scratch starts at one tile's row and must reach 257 tiles' rows, then
    513 tiles' with the segment rows, while the earlier calls are still in flight"""
    import torch
    s = torch.cuda.Stream()
    runs = [Dev(*pattern("rand4", 257)), Dev(*pattern("rand257", 256 * T + 1)),
            Dev(*pattern("mod257", BIG)), Dev(*pattern("two", 65))]
    with torch.cuda.stream(s):
        for d in runs:
            d.enqueue(gpu, s)
    s.synchronize()
    for d, (name, n) in zip(runs, [("rand4", 257), ("rand257", 256 * T + 1), ("mod257", BIG),
                                   ("two", 65)]):
        index, starts = d.result()
        np.testing.assert_array_equal(starts, want(name, n, True)[1], err_msg=name)
        np.testing.assert_array_equal(index, want(name, n, True)[0], err_msg=name)


def test_steer_two_streams_at_once(gpu):
    """each stream has its own scratch: two calls in flight do not share rows"""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [("rand257", BIG), ("div64", BIG), ("rand4", 3 * T + 17), ("mod257", 3 * T + 17)]
    runs = [Dev(*pattern(name, n)) for name, n in cases]
    torch.cuda.synchronize()
    for k, d in enumerate(runs):
        s = (s1, s2)[k % 2]
        with torch.cuda.stream(s):
            d.enqueue(gpu, s)
    torch.cuda.synchronize()
    for d, (name, n) in zip(runs, cases):
        index, starts = d.result()
        np.testing.assert_array_equal(starts, want(name, n, True)[1], err_msg=name)
        np.testing.assert_array_equal(index, want(name, n, True)[0], err_msg=name)


# ---------------------------------------------------------------- a real batch, and stage two

NREAL = 4096 + 37


@functools.lru_cache(maxsize=None)
def _c4_packets():
    from generic_ebpf_amd import workloads
    return workloads.packets_l2l3(NREAL, 64)


class C4Run:
    """C4 over NREAL packets on the device (EBPF_BATCH_HIST_OVERWRITE), steered"""

    def __init__(self, gpu, env, variant):
        import torch
        from generic_ebpf_amd import workloads
        dev = torch.device("cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        lay = workloads.prog_c4()
        self.data = torch.from_numpy(_c4_packets().reshape(-1)).to(dev)
        self.ret = torch.full((NREAL,), -1, dtype=torch.int64, device=dev)
        self.faults = torch.zeros(NREAL, dtype=torch.uint8, device=dev)
        self.hist = torch.full((257,), 4242, dtype=torch.int64, device=dev)
        self.index = torch.full((NREAL,), -1, dtype=torch.int32, device=dev)
        self.starts = torch.full((258,), -1, dtype=torch.int64, device=dev)
        m = gpu.Map(env, 256, 8)
        m.fill(workloads.c4_map_values().tobytes())
        p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, [m.handle]))
        try:
            gpu.set_variant(variant)
            p.run_batch_dev(0, self.data.data_ptr(), NREAL, 64, self.ret.data_ptr(), None,
                            self.faults.data_ptr(), self.hist.data_ptr(), st, hist_overwrite=True)
            gpu.steer_dev(0, self.ret.data_ptr(), self.faults.data_ptr(), NREAL,
                          self.index.data_ptr(), self.starts.data_ptr(), st)
            torch.cuda.synchronize()
        finally:
            gpu.set_variant(0)
            p.destroy()
            m.destroy()


@pytest.mark.parametrize("variant", [0, 1])
def test_steer_real_batch_and_stage_two(gpu, env, variant):
    import torch
    from generic_ebpf_amd import workloads
    r = C4Run(gpu, env, variant)
    ret = r.ret.cpu().numpy().view(U64)
    faults = r.faults.cpu().numpy()
    index = r.index.cpu().numpy().view(np.uint32)
    starts = r.starts.cpu().numpy().view(U64)
    w_index, w_starts = expected(ret, faults)
    np.testing.assert_array_equal(starts, w_starts)
    np.testing.assert_array_equal(index, w_index)
    # the feature's classes are the epilogue's bins
    np.testing.assert_array_equal(np.diff(starts.astype(np.int64)), r.hist.cpu().numpy())
    assert (np.diff(starts.astype(np.int64)) > 0).sum() > 4

    # stage two: C3 over the most populated class, selected in place
    b = int(np.argmax(np.diff(starts.astype(np.int64))))
    lo, n = int(starts[b]), int(starts[b + 1] - starts[b])
    dev = r.data.device
    st = torch.cuda.current_stream().cuda_stream
    ext = torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    gpu.select_dev(0, r.data.data_ptr(), NREAL, 64, r.index.data_ptr() + 4 * lo, n, ext.data_ptr(),
                   stream=st)
    ret2 = torch.full((n,), -1, dtype=torch.int64, device=dev)
    flt2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    lay = workloads.prog_c3()
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        gpu.set_variant(variant)
        p.run_batch_dev(0, r.data.data_ptr(), n, 0, ret2.data_ptr(), ext.data_ptr(),
                        flt2.data_ptr(), None, st, extents=True)
        torch.cuda.synchronize()
    finally:
        gpu.set_variant(0)
        p.destroy()
    members = w_index[lo:lo + n].astype(np.int64)
    np.testing.assert_array_equal(ext.cpu().numpy().reshape(n, 2),
                                  np.stack([members * 64, members * 64 + 64], axis=1))
    gathered = np.ascontiguousarray(_c4_packets()[members])
    w_ret, w_flt, _, _ = pyoracle.OracleProgram(lay.code, lay.relocs, []).run(gathered, n, 64)
    np.testing.assert_array_equal(flt2.cpu().numpy(), w_flt)
    np.testing.assert_array_equal(ret2.cpu().numpy().view(U64), w_ret)


# ---------------------------------------------------------------- select

NSEL = 1000


def _sources():
    """(name, count, stride, offsets or None, extents flag, numpy (start, end) of every packet)"""
    g = np.random.default_rng(8)
    i = np.arange(NSEL, dtype=np.int64)
    lens = g.integers(0, 101, NSEL)
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pairs = np.stack([csr[:-1], csr[1:]], axis=1)[g.permutation(NSEL)]
    return [("stride64", NSEL, 64, None, False, np.stack([i * 64, i * 64 + 64], axis=1)),
            ("csr", NSEL, 0, csr, False, np.stack([csr[:-1], csr[1:]], axis=1)),
            ("extents", NSEL, 0, pairs.reshape(-1), True, pairs)]


@pytest.mark.parametrize("src", _sources(), ids=lambda s: s[0])
def test_select_sources(gpu, src):
    """the extents written for every class of a steered batch, and for a list with indices at
    and past count"""
    import torch
    name, count, stride, offs, extents, pairs = src
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    ret, faults = pattern("rand4", count)
    d = Dev(ret, faults)
    d.enqueue(gpu, torch.cuda.current_stream())
    data = torch.zeros(16, dtype=torch.uint8, device=dev)   # (never read by select)
    d_off = None if offs is None else torch.from_numpy(np.ascontiguousarray(offs)).to(dev)
    w_index, w_starts = want("rand4", count, True)
    outs = []
    for b in (0, 1, 17, 255, 256):
        lo, n = int(w_starts[b]), int(w_starts[b + 1] - w_starts[b])
        out = torch.full((2 * max(n, 1),), -1, dtype=torch.int64, device=dev)
        gpu.select_dev(0, data.data_ptr(), count, stride, d.index.data_ptr() + 4 * lo, n,
                       out.data_ptr() if n else None, None if d_off is None else d_off.data_ptr(),
                       st, extents=extents)
        outs.append((lo, n, out))
    odd = np.array([5, count, 0, count - 1, 0xffffffff, count + 7, 5], dtype=np.uint32)
    d_odd = torch.from_numpy(odd.view(np.int32)).to(dev)
    o_odd = torch.full((2 * len(odd),), -1, dtype=torch.int64, device=dev)
    gpu.select_dev(0, data.data_ptr(), count, stride, d_odd.data_ptr(), len(odd), o_odd.data_ptr(),
                   None if d_off is None else d_off.data_ptr(), st, extents=extents)
    torch.cuda.synchronize()
    assert sum(n for _, n, _ in outs) == count
    for lo, n, out in outs:
        np.testing.assert_array_equal(out.cpu().numpy()[:2 * n].reshape(n, 2),
                                      pairs[w_index[lo:lo + n].astype(np.int64)])
    w_odd = np.array([pairs[k] if k < count else (0, 0) for k in odd.tolist()])
    np.testing.assert_array_equal(o_odd.cpu().numpy().reshape(-1, 2), w_odd)
