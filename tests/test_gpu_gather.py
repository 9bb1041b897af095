"""Gathering packets into a dense batch on the device (include/ebpf_gpu.h: ebpf_batch_gather_dev;
csrc/hip/gather.hip) against the numpy rules of test_gather.py, which that file checks against
the host function.  A copy has one right answer: every comparison is exact.

Every output lies PAD bytes into a device buffer filled with 0xA5 and is followed by PAD more, so
a write before `out`, past the output's end or past out_bytes shows up.

Shapes.  The row path gives stride/16 lanes to a packet and 4 x 256 such 16-byte units to a
workgroup per trip: the list lengths sit around 16, 64, 256 and 4096.  The general path gives a
workgroup 256 list entries and walks their destination range in 16-byte chunks aligned in memory:
packets of 0..3 bytes put many into one chunk, out offsets 1, 8 and 15 move the chunk grid against
the slots, and lengths 63, 64, 65 sit on both sides of a chunk boundary.  The packed form scans
4,096 entries a tile and takes its second level above 256 tiles, which 2M + 5 entries reach."""
import functools

import numpy as np
import pytest

import pyoracle
from generic_ebpf_amd import native as _native
from test_gather import (G4, NSEL, PAD, SENTINEL, Src, U64, check_frame, expected, lists, sources,
                         spans)

pytestmark = pytest.mark.gpu

ROW_COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
BIG = (2 << 20) + 5


class DevSrc:
    """a batch in device memory, its data `shift` bytes into a 256-byte-aligned allocation"""

    def __init__(self, src, shift=0):
        import torch
        dev = torch.device("cuda:0")
        self.src = src
        self.buf = torch.zeros(shift + len(src.data) + 16, dtype=torch.uint8, device=dev)
        self.buf[shift:shift + len(src.data)] = torch.from_numpy(src.data).to(dev)
        self.data_ptr = self.buf.data_ptr() + shift
        self.offs = None
        if src.offsets is not None:
            self.offs = torch.from_numpy(np.ascontiguousarray(src.offsets, dtype=U64)
                                         .view(np.int64)).to(dev)


class Call:
    """one ebpf_batch_gather_dev call into a framed output, enqueued on `stream`; check() after
    the stream compares the frame and the offsets with the numpy rules"""

    def __init__(self, gpu, dsrc, index, out_stride, out_bytes=None, shift=0, stream=None,
                 d_index=None, want=None, data_ptr=None):
        import torch
        dev = torch.device("cuda:0")
        src = dsrc.src
        self.index = np.ascontiguousarray(index, dtype=np.uint32)
        n = self.n = len(self.index)
        self.want, self.want_offs = want or expected(src, self.index, out_stride, out_bytes)
        total = n * out_stride if out_stride else int(self.want_offs[n])
        self.out_bytes = total if out_bytes is None else out_bytes
        self.lead = PAD + shift
        self.buf = torch.full((self.lead + max(total, self.out_bytes) + PAD,), SENTINEL,
                              dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.out_ptr = self.buf.data_ptr() + self.lead
        self.offs = None if out_stride else torch.full((n + 2,), 0x5a5a5a5a5a5a5a5a,
                                                       dtype=torch.int64, device=dev)
        self.d_index = d_index
        if d_index is None:
            self.d_index = torch.from_numpy(self.index.view(np.int32)).to(dev) if n else None
        self.what = "%s stride %d n %d shift %d" % (src.name, out_stride, n, shift)
        st = (stream or torch.cuda.current_stream()).cuda_stream
        gpu.gather_dev(0, dsrc.data_ptr if data_ptr is None else data_ptr, src.count, src.stride,
                       self.d_index.data_ptr() if n else None, n, out_stride,
                       self.out_ptr if n else None, self.out_bytes,
                       None if self.offs is None else self.offs.data_ptr(),
                       None if dsrc.offs is None else dsrc.offs.data_ptr(), st,
                       extents=src.extents)

    def result(self):
        return self.buf.cpu().numpy(), None if self.offs is None else self.offs.cpu().numpy()

    def check(self):
        buf, offs = self.result()
        check_frame(buf, self.lead, self.want, self.what)
        if offs is not None:
            np.testing.assert_array_equal(offs[:self.n + 1].view(U64), self.want_offs,
                                          err_msg=self.what)
            assert offs[self.n + 1] == 0x5a5a5a5a5a5a5a5a, self.what


def run_all(calls):
    import torch
    torch.cuda.synchronize()
    for c in calls:
        c.check()


# ---------------------------------------------------------------- row path


@functools.lru_cache(maxsize=None)
def _row_src(stride):
    g = np.random.default_rng(stride)
    return Src("stride%d" % stride, g.integers(0, 256, NSEL * stride, dtype=np.uint8), NSEL, stride,
               None, False)


def _row_list(n, seed):
    """duplicates (n above the batch's count forces them) and indices at and past count"""
    g = np.random.default_rng(seed)
    index = g.integers(0, NSEL + 40, n).astype(np.uint32)
    index[::97] = 0xffffffff
    if n > 2:
        index[1] = NSEL
        index[2] = NSEL - 1
    return index


@pytest.mark.parametrize("stride", [64, 16, 128])
def test_gather_rows(gpu, stride):
    src = _row_src(stride)
    aligned, off4 = DevSrc(src), DevSrc(src, shift=4)
    assert aligned.data_ptr % 16 == 0 and off4.data_ptr % 16 == 4
    calls = []
    for n in ROW_COUNTS:
        index = _row_list(n, n)
        want = expected(src, index, stride)
        calls.append(Call(gpu, aligned, index, stride, want=want))            # the row path
        calls.append(Call(gpu, off4, index, stride, want=want))               # data + 4: general
        calls.append(Call(gpu, aligned, index, stride, shift=4, want=want))   # out + 4: general
    run_all(calls)


# ---------------------------------------------------------------- general path


@functools.lru_cache(maxsize=None)
def _general_sources():
    from generic_ebpf_amd import workloads
    g = np.random.default_rng(21)
    lens = g.integers(0, 201, NSEL)
    lens[[0, 1, 2, 3, 4, NSEL - 1]] = [0, 1, 63, 64, 65, 64]
    lens[500:505] = [65, 0, 64, 63, 1]
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    data = g.integers(0, 256, int(csr[-1]) + 16, dtype=np.uint8)
    idata, ioffs, sizes = workloads.packets_imix(NSEL)
    ext = np.stack([ioffs[:-1], ioffs[:-1] + sizes], axis=1).reshape(-1).astype(U64)
    return (Src("csr200", data, NSEL, 0, csr, False), Src("imix", idata, NSEL, 0, ext, True))


@functools.lru_cache(maxsize=None)
def _tiny_src():
    """5,000 packets of 0..3 bytes: many share one 16-byte chunk, and a long list stays small"""
    g = np.random.default_rng(22)
    lens = g.integers(0, 4, 5000)
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    return Src("tiny", g.integers(1, 256, int(csr[-1]) + 16, dtype=np.uint8), 5000, 0, csr, False)


@pytest.mark.parametrize("k", [0, 1], ids=["csr200", "imix"])
def test_gather_general_strided(gpu, k):
    src = _general_sources()[k]
    dsrc = DevSrc(src)
    calls = []
    for name, index in lists(src.count).items():
        for out_stride in (1, 7, 60, 64, 128):
            want = expected(src, index, out_stride)
            for shift in (0, 1, 8):
                calls.append(Call(gpu, dsrc, index, out_stride, shift=shift, want=want))
    run_all(calls)


@pytest.mark.parametrize("k", [0, 1], ids=["csr200", "imix"])
def test_gather_packed(gpu, k):
    src = _general_sources()[k]
    dsrc = DevSrc(src)
    calls = []
    for name, index in lists(src.count).items():
        want = expected(src, index, 0)
        for shift in (0, 1, 15):
            calls.append(Call(gpu, dsrc, index, 0, shift=shift, want=want))
        # out_bytes inside a packet, at a packet's end, and 0
        offs = want[1].astype(np.int64)
        j = int(np.flatnonzero(np.diff(offs) > 2)[len(index) // 4])
        for out_bytes in (int(offs[j]) + 1, int(offs[j + 1]), 0):
            calls.append(Call(gpu, dsrc, index, 0, out_bytes=out_bytes, shift=1))
            assert len(calls[-1].want) == out_bytes < offs[-1]
    run_all(calls)


def test_gather_packed_tiny_and_empty_packets(gpu):
    tiny = _tiny_src()
    dtiny = DevSrc(tiny)
    calls = []
    for shift in (0, 1, 15):
        calls.append(Call(gpu, dtiny, np.arange(1000, 1300), 0, shift=shift))
        calls.append(Call(gpu, dtiny, np.arange(1000, 1300), 7, shift=shift))
    assert 300 < len(calls[0].want) < 900
    # all-zero lengths: an empty run of the offsets form, and a list of indices past the batch
    zeros = Src("zeros", tiny.data, 700, 0, np.full(701, 33, dtype=U64), False)
    dz = DevSrc(zeros)
    calls.append(Call(gpu, dz, np.arange(700), 0, shift=1))
    calls.append(Call(gpu, dz, np.arange(700), 16, shift=1))
    calls.append(Call(gpu, dtiny, np.full(300, 0xffffffff, dtype=np.uint32), 0))
    assert len(calls[-1].want) == 0 and not calls[-1].want_offs.any()
    # an empty list, and an empty batch
    calls.append(Call(gpu, dtiny, [], 0))
    calls.append(Call(gpu, dtiny, [], 64))
    empty = DevSrc(Src("empty", tiny.data, 0, 64, None, False))
    calls.append(Call(gpu, empty, [0, 7, 0xffffffff], 0))
    calls.append(Call(gpu, empty, [0, 7, 0xffffffff], 64))
    run_all(calls)
    assert calls[-4].offs.cpu().numpy()[0] == 0


@functools.lru_cache(maxsize=None)
def _deep():
    """2M + 5 list entries over the tiny packets: 513 tiles, the scan's second level"""
    src = _tiny_src()
    index = np.random.default_rng(23).integers(0, src.count + 3, BIG).astype(np.uint32)
    return index, expected(src, index, 0)


def test_gather_packed_two_level_scan(gpu):
    index, want = _deep()
    c = Call(gpu, DevSrc(_tiny_src()), index, 0, shift=1, want=want)
    run_all([c])
    assert int(want[1][-1]) > BIG


# ---------------------------------------------------------------- far packets

SIZE = G4 + (2 << 20)


def test_gather_far_packets(gpu):
    """one zero-filled 4 GiB + 2 MiB buffer with a handful of packets written past 4 GiB (and one
    across it); the host's copy is lazily backed, only the touched pages cost memory.  A wrong
    address or length formed from these inputs stays inside the allocation: starts lie at most
    1 MiB past 4 GiB and no length exceeds 1,500."""
    import torch
    dev = torch.device("cuda:0")
    g = np.random.default_rng(24)
    lens = [0, 1, 15, 16, 17, 64, 100, 777, 1500, 33, 64, 5]
    starts = [G4 + 4096 * (k + 1) + int(g.integers(0, 64)) for k in range(len(lens))]
    starts[-3], starts[-2], starts[-1] = G4 - 20, 8192 + 3, 70000   # across 4 GiB; two near ones
    host = np.zeros(SIZE, dtype=np.uint8)
    buf = torch.zeros(SIZE, dtype=torch.uint8, device=dev)
    try:
        for s, ln in zip(starts, lens):
            host[s:s + ln] = g.integers(1, 256, ln, dtype=np.uint8)
            buf[s:s + ln] = torch.from_numpy(host[s:s + ln]).to(dev)
        pairs = [(s, s + ln) for s, ln in zip(starts, lens)]
        pairs += [(G4 + 9000, G4 + 8000), (4096, 4096 + G4), (1 << 20, (1 << 20) + G4 + 77)]
        src = Src("far", host, len(pairs), 0, np.array(pairs, dtype=U64).reshape(-1), True)
        assert spans(src)[1].tolist() == lens + [0, 0, 0]
        dsrc = DevSrc(Src("far", np.zeros(0, dtype=np.uint8), src.count, 0, src.offsets, True))
        dsrc.src = src
        index = np.array([12, 7, 0, 13, 8, 14, 9, 1, 2, 3, 4, 5, 6, 10, 11, 8, 12, 40],
                         dtype=np.uint32)
        calls = [Call(gpu, dsrc, index, st, shift=sh, data_ptr=buf.data_ptr())
                 for st, sh in ((0, 0), (0, 5), (64, 0), (200, 3), (1500, 8))]
        # the row path with its packets past 4 GiB: the buffer as 64-byte packets
        nrows = SIZE // 64
        drows = DevSrc(Src("far64", np.zeros(0, dtype=np.uint8), nrows, 64, None, False))
        ridx = np.array([s // 64 for s in starts] + [nrows - 1, nrows], dtype=np.uint32)
        assert ridx.max() > (1 << 26)
        at = np.minimum(ridx.astype(np.int64), nrows - 1)
        want = host[at[:, None] * 64 + np.arange(64)[None, :]]
        want[ridx >= nrows] = 0
        calls.append(Call(gpu, drows, ridx, 64, data_ptr=buf.data_ptr(),
                          want=(want.reshape(-1), None)))
        run_all(calls)
        assert calls[-1].want.any() and calls[0].want.any()
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- determinism and streams


def test_gather_same_call_twice(gpu):
    src = _general_sources()[1]
    dsrc = DevSrc(src)
    index = lists(src.count)["dups"]
    for out_stride in (0, 64):
        a, b = Call(gpu, dsrc, index, out_stride, shift=1), Call(gpu, dsrc, index, out_stride, shift=1)
        run_all([a, b])
        ra, rb = a.result(), b.result()
        assert ra[0].tobytes() == rb[0].tobytes()
        assert out_stride or ra[1].tobytes() == rb[1].tobytes()


def test_gather_scratch_grows_on_a_stream(gpu):
    """a fresh stream: its scratch starts at one tile's sum and must reach 74 tiles', then 513
    tiles' with the segment sums, while the earlier calls are still in flight"""
    import torch
    src = _tiny_src()
    dsrc = DevSrc(src)
    deep_index, deep_want = _deep()
    g = np.random.default_rng(25)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        calls = [Call(gpu, dsrc, g.integers(0, src.count, 100), 0, stream=s),
                 Call(gpu, dsrc, g.integers(0, src.count, 300001), 0, stream=s),
                 Call(gpu, dsrc, deep_index, 0, stream=s, want=deep_want),
                 Call(gpu, dsrc, g.integers(0, src.count, 65), 0, stream=s)]
    s.synchronize()
    run_all(calls)


def test_gather_two_streams_at_once(gpu):
    """each stream has its own scratch: two packed gathers in flight do not share tile sums"""
    import torch
    src = _tiny_src()
    dsrc = DevSrc(src)
    deep_index, deep_want = _deep()
    g = np.random.default_rng(26)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    lists_ = [(deep_index, deep_want), (deep_index[::-1].copy(), None),
              (g.integers(0, src.count, 3 * 4096 + 17), None), (g.integers(0, src.count, 70000), None)]
    torch.cuda.synchronize()
    calls = []
    for k, (index, want) in enumerate(lists_):
        s = (s1, s2)[k % 2]
        with torch.cuda.stream(s):
            calls.append(Call(gpu, dsrc, index, 0, stream=s, want=want))
    run_all(calls)


# ---------------------------------------------------------------- a real batch, end to end


def _run_c3(gpu, env, variant, data_ptr, n, stride, offsets_ptr=None, extents=False):
    """C3 over a device batch: (ret, faults, layout of the kernel that ran)"""
    import torch
    from generic_ebpf_amd import workloads
    dev = torch.device("cuda:0")
    ret = torch.full((n,), -1, dtype=torch.int64, device=dev)
    flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    lay = workloads.prog_c3()
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        gpu.set_variant(variant)
        p.run_batch_dev(0, data_ptr, n, stride, ret.data_ptr(), offsets_ptr, flt.data_ptr(), None,
                        torch.cuda.current_stream().cuda_stream, extents=extents)
        torch.cuda.synchronize()
        layout = p.exec_info(0)[1]
    finally:
        gpu.set_variant(0)
        p.destroy()
    return ret.cpu().numpy().view(U64), flt.cpu().numpy(), layout


def _c3_oracle(packets):
    from generic_ebpf_amd import workloads
    lay = workloads.prog_c3()
    rows = np.ascontiguousarray(packets)
    ret, flt, _, _ = pyoracle.OracleProgram(lay.code, lay.relocs, []).run(rows, len(rows), 64)
    return ret, flt


@pytest.mark.parametrize("variant", [0, 1])
def test_gather_class_and_stage_two(gpu, env, variant):
    import torch
    from test_gpu_steer import C4Run, NREAL, _c4_packets
    r = C4Run(gpu, env, variant)
    dev = r.data.device
    st = torch.cuda.current_stream().cuda_stream
    index = r.index.cpu().numpy().view(np.uint32)
    starts = r.starts.cpu().numpy().view(U64).astype(np.int64)
    b = int(np.argmax(np.diff(starts)))
    lo, n = int(starts[b]), int(starts[b + 1] - starts[b])
    members = index[lo:lo + n].astype(np.int64)
    gathered = _c4_packets()[members]
    w_ret, w_flt = _c3_oracle(gathered)

    out = torch.full((n * 64 + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    gpu.gather_dev(0, r.data.data_ptr(), NREAL, 64, r.index.data_ptr() + 4 * lo, n, 64,
                   out.data_ptr(), n * 64, stream=st)
    ret, flt, layout = _run_c3(gpu, env, variant, out.data_ptr(), n, 64)
    np.testing.assert_array_equal(out.cpu().numpy()[:n * 64], gathered.reshape(-1))
    assert (out[n * 64:] == SENTINEL).all()
    np.testing.assert_array_equal(flt, w_flt)
    np.testing.assert_array_equal(ret, w_ret)

    ext = torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    gpu.select_dev(0, r.data.data_ptr(), NREAL, 64, r.index.data_ptr() + 4 * lo, n, ext.data_ptr(),
                   stream=st)
    e_ret, e_flt, e_layout = _run_c3(gpu, env, variant, r.data.data_ptr(), n, 0, ext.data_ptr(),
                                     extents=True)
    np.testing.assert_array_equal(e_flt, flt)
    np.testing.assert_array_equal(e_ret, ret)
    if variant == 0:
        assert layout == 1 and e_layout == 0

    # the whole steering index in one call: the batch reordered by class
    whole = torch.full((NREAL * 64,), SENTINEL, dtype=torch.uint8, device=dev)
    gpu.gather_dev(0, r.data.data_ptr(), NREAL, 64, r.index.data_ptr(), NREAL, 64,
                   whole.data_ptr(), NREAL * 64, stream=st)
    s_ret, s_flt, s_layout = _run_c3(gpu, env, variant, whole.data_ptr() + lo * 64, n, 64)
    np.testing.assert_array_equal(whole.cpu().numpy(), _c4_packets()[index.astype(np.int64)].reshape(-1))
    np.testing.assert_array_equal(s_flt, flt)
    np.testing.assert_array_equal(s_ret, ret)
    if variant == 0:
        assert s_layout == 1


def test_gather_imix_snapshot(gpu, env):
    """variable-length traffic snapped to its first 64 bytes feeds the staged kernel"""
    import torch
    src = _general_sources()[1]
    dsrc = DevSrc(src)
    index = np.concatenate([np.arange(0, src.count, 2), [5, 5, 999]]).astype(np.uint32)
    s, ln = spans(src)
    assert ln.min() >= 64 and len(np.unique(ln)) == 3
    c = Call(gpu, dsrc, index, 64)
    run_all([c])
    snap = src.data[(s[index.astype(np.int64)][:, None] + np.arange(64)[None, :])]
    np.testing.assert_array_equal(c.want, snap.reshape(-1))
    w_ret, w_flt = _c3_oracle(snap)
    ret, flt, layout = _run_c3(gpu, env, 0, c.out_ptr, len(index), 64)
    assert layout == 1
    np.testing.assert_array_equal(flt, w_flt)
    np.testing.assert_array_equal(ret, w_ret)
