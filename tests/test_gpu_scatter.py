"""Scattering a dense batch back and merging a second stage's results on the device
(include/ebpf_gpu.h: ebpf_batch_scatter_dev, ebpf_batch_merge_dev; csrc/hip/scatter.hip) against
the numpy rules of test_scatter.py, which that file checks against the host functions.  A copy has
one right answer: every comparison is exact.

The batch's data lies PAD + shift bytes into a device buffer filled with 0xA5 and is followed by
PAD more; the whole buffer is compared, so a byte written outside a listed packet's first k_j
bytes — a gap, an unlisted neighbour inside the same 16 bytes, the frame — shows up.  The dense
input lies in_shift bytes into a framed buffer of its own, which must come back unchanged.

Shapes.  The row path gives stride/16 lanes to a packet and 4 x 256 such 16-byte units to a
workgroup per trip: the list lengths sit around 16, 64, 256 and 4096.  The general path gives a
workgroup 256 list entries and walks their packets' 16-byte chunks aligned in memory: packets of
0..3 bytes put many, listed and not, into one chunk; batch shifts 1, 8 and 15 move the chunk grid
against the packets and dense shifts 1 and 15 misalign every 16-byte load; lengths 15, 16, 17, 63,
64 and 65 are a piece alone, exactly one chunk, and both sides of a chunk boundary."""
import functools
import itertools

import numpy as np
import pytest

from test_gather import G4, NSEL, PAD, SENTINEL, Src, U64, check_frame, expected, sources, spans
from test_scatter import FLIP, RET_GUARD, copied, expected_merge, expected_scatter, scatter_lists

pytestmark = pytest.mark.gpu

ROW_COUNTS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097]
NROWS = 5000
BIG = (2 << 20) + 5
SHIFTS = list(itertools.product((0, 1, 8, 15), (0, 1, 15)))   # (batch base, dense base)


def _dev():
    import torch
    return torch.device("cuda:0")


def framed(data, shift):
    """a device buffer of 0xA5 with `data` PAD + shift bytes in: (buffer, lead)"""
    import torch
    lead = PAD + shift
    host = np.full(lead + len(data) + PAD, SENTINEL, dtype=np.uint8)
    host[lead:lead + len(data)] = data
    buf = torch.from_numpy(host).to(_dev())
    assert buf.data_ptr() % 16 == 0
    return buf, lead


class DevBatch:
    """a batch whose data lies `shift` bytes off a 16-byte boundary inside a framed device buffer;
    fresh() gives a call its own copy to write into"""

    def __init__(self, src, shift=0):
        import torch
        self.src = src
        self.template, self.lead = framed(src.data, shift)
        self.offs = None
        if src.offsets is not None:
            self.offs = torch.from_numpy(np.ascontiguousarray(src.offsets, dtype=U64)
                                         .view(np.int64)).to(_dev())

    def fresh(self):
        return self.template.clone()


class Call:
    """one ebpf_batch_scatter_dev call into a fresh copy of the batch, enqueued on `stream`;
    check() after the stream compares the whole framed buffer with the numpy rules"""

    def __init__(self, gpu, dbatch, index, dense, in_stride, in_offsets=None, in_bytes=None,
                 in_shift=0, stream=None, want=None):
        import torch
        src = dbatch.src
        self.index = np.ascontiguousarray(index, dtype=np.uint32)
        n = self.n = len(self.index)
        dense = np.ascontiguousarray(dense, dtype=np.uint8)
        self.in_bytes = len(dense) if in_bytes is None else in_bytes
        self.want = want
        if want is None:
            self.want = expected_scatter(src, self.index, dense, in_stride, in_offsets, self.in_bytes)
        self.lead = dbatch.lead
        self.buf = dbatch.fresh()
        self.dense, self.in_lead = framed(dense, in_shift)
        self.dense_before = self.dense.clone()
        self.d_index = torch.from_numpy(self.index.view(np.int32)).to(_dev()) if n else None
        self.d_in_offs = None
        if in_offsets is not None:
            self.d_in_offs = torch.from_numpy(np.ascontiguousarray(in_offsets, dtype=U64)
                                              .view(np.int64)).to(_dev())
        self.what = "%s in_stride %d n %d shifts %d %d" % (src.name, in_stride, n,
                                                           self.lead - PAD, in_shift)
        st = (stream or torch.cuda.current_stream()).cuda_stream
        gpu.scatter_dev(0, self.buf.data_ptr() + self.lead, src.count, src.stride,
                        self.d_index.data_ptr() if n else None, n, in_stride,
                        self.dense.data_ptr() + self.in_lead if n else None, self.in_bytes,
                        None if self.d_in_offs is None else self.d_in_offs.data_ptr(),
                        None if dbatch.offs is None else dbatch.offs.data_ptr(), st,
                        extents=src.extents)

    def result(self):
        return self.buf.cpu().numpy()

    def check(self):
        import torch
        check_frame(self.result(), self.lead, self.want, self.what)
        assert torch.equal(self.dense, self.dense_before), self.what + ": the input changed"


def run_all(calls):
    import torch
    torch.cuda.synchronize()
    for c in calls:
        c.check()


def _random_dense(g, n, in_stride, own_offsets):
    """(dense bytes, in_offsets or None) for a list of n entries"""
    if in_stride:
        return g.integers(0, 256, n * in_stride, dtype=np.uint8), None
    return g.integers(0, 256, int(own_offsets[-1]), dtype=np.uint8), own_offsets


# ---------------------------------------------------------------- row path


@functools.lru_cache(maxsize=None)
def _row_src(stride):
    g = np.random.default_rng(stride)
    return Src("stride%d" % stride, g.integers(0, 256, NROWS * stride, dtype=np.uint8), NROWS,
               stride, None, False)


def _row_list(n, seed):
    """distinct indices inside the batch, and some at and past count (which write nothing)"""
    g = np.random.default_rng(seed)
    index = g.permutation(NROWS)[:n].astype(np.uint32)
    index[5::97] = 0xffffffff
    if n > 2:
        index[1] = NROWS
        index[2] = NROWS + 9
    return index


@pytest.mark.parametrize("stride", [64, 16, 128])
def test_scatter_rows(gpu, stride):
    src = _row_src(stride)
    aligned, off4 = DevBatch(src), DevBatch(src, shift=4)
    g = np.random.default_rng(100 + stride)
    calls = []
    for n in ROW_COUNTS:
        index = _row_list(n, n)
        dense = g.integers(0, 256, n * stride, dtype=np.uint8)
        want = expected_scatter(src, index, dense, stride)
        calls.append(Call(gpu, aligned, index, dense, stride, want=want))             # the row path
        calls.append(Call(gpu, off4, index, dense, stride, want=want))                # data + 4
        calls.append(Call(gpu, aligned, index, dense, stride, in_shift=4, want=want))  # in + 4
    run_all(calls)
    assert (calls[-3].result()[PAD:PAD + len(src.data)] != src.data).sum() > 4000 * stride * 0.9


# ---------------------------------------------------------------- general path


@functools.lru_cache(maxsize=None)
def _general_sources():
    """the csr and extents sources of test_gather.py, IMIX as extents over its padded layout, and
    packets of 0..200 bytes with the lengths around a chunk forced in"""
    from generic_ebpf_amd import workloads
    g = np.random.default_rng(21)
    lens = g.integers(0, 201, NSEL)
    lens[:9] = [0, 1, 15, 16, 17, 63, 64, 65, 64]
    lens[500:508] = [65, 0, 64, 63, 1, 17, 16, 15]
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    data = g.integers(0, 256, int(csr[-1]) + 16, dtype=np.uint8)
    idata, ioffs, sizes = workloads.packets_imix(NSEL)
    ext = np.stack([ioffs[:-1], ioffs[:-1] + sizes], axis=1).reshape(-1).astype(U64)
    base = sources()
    return (base[1], base[2], Src("imix", idata, NSEL, 0, ext, True),
            Src("edges", data, NSEL, 0, csr, False))


@functools.lru_cache(maxsize=None)
def _tiny_src():
    """5,000 packets of 0..3 bytes: many share one 16-byte chunk, and a long list stays small"""
    g = np.random.default_rng(22)
    lens = g.integers(0, 4, 5000)
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    return Src("tiny", g.integers(1, 256, int(csr[-1]) + 16, dtype=np.uint8), 5000, 0, csr, False)


@pytest.mark.parametrize("k", [0, 1, 2, 3], ids=["csr", "extents", "imix", "edges"])
def test_scatter_general(gpu, k):
    """every list in every form with the shifts taken in turn, then every pair of shifts on the
    class list, packed and at in_stride 60"""
    src = _general_sources()[k]
    batches = {s: DevBatch(src, s) for s in (0, 1, 8, 15)}
    g = np.random.default_rng(50 + k)
    turn = itertools.cycle(SHIFTS)
    calls = []
    ls = scatter_lists(src.count)
    for name, index in ls.items():
        own = expected(src, index, 0)[1]
        for in_stride in (7, 60, 64, 128, 0):
            dense, in_offs = _random_dense(g, len(index), in_stride, own)
            want = expected_scatter(src, index, dense, in_stride, in_offs)
            shift, in_shift = next(turn)
            calls.append(Call(gpu, batches[shift], index, dense, in_stride, in_offs,
                              in_shift=in_shift, want=want))
    index = ls["class"]
    own = expected(src, index, 0)[1]
    for in_stride in (60, 0):
        dense, in_offs = _random_dense(g, len(index), in_stride, own)
        want = expected_scatter(src, index, dense, in_stride, in_offs)
        for shift, in_shift in SHIFTS:
            calls.append(Call(gpu, batches[shift], index, dense, in_stride, in_offs,
                              in_shift=in_shift, want=want))
    # slots of lengths of their own: shorter and longer than the packets, empty ones among them
    other = np.concatenate([[0], np.cumsum(g.integers(0, 121, len(index)))]).astype(U64)
    dense = g.integers(0, 256, int(other[-1]), dtype=np.uint8)
    calls.append(Call(gpu, batches[1], index, dense, 0, other, in_shift=15))
    run_all(calls)
    assert (calls[-1].result()[PAD + 1:PAD + 1 + len(src.data)] != src.data).sum() > 1000


def test_scatter_packed_cut_by_in_bytes(gpu):
    """a truncated packed gather's {in, in_offsets}: in_bytes inside a packet, at a packet's end,
    and 0; what lies behind in_bytes in the caller's buffer is not used"""
    src = _general_sources()[3]
    index = scatter_lists(src.count)["whole"]
    offs = expected(src, index, 0)[1]
    o = offs.astype(np.int64)
    j = int(np.flatnonzero(np.diff(o) > 2)[len(index) // 2])
    g = np.random.default_rng(60)
    dense = g.integers(0, 256, int(o[-1]), dtype=np.uint8)
    calls = []
    for (shift, in_shift), in_bytes in zip(SHIFTS[3:], (int(o[j]) + 1, int(o[j + 1]), 0,
                                                        int(o[j]) + 17)):
        want = expected_scatter(src, index, dense, 0, offs, in_bytes)
        assert len(copied(src, index, 0, offs, in_bytes)[0]) == in_bytes
        calls.append(Call(gpu, DevBatch(src, shift), index, dense, 0, offs, in_bytes=in_bytes,
                          in_shift=in_shift, want=want))
    run_all(calls)


def test_scatter_tiny_packets_and_unlisted_neighbours(gpu):
    """every other packet of the 0..3-byte source: the unlisted packets between the listed ones,
    inside the same 16 bytes, keep their bytes"""
    tiny = _tiny_src()
    index = np.arange(0, tiny.count, 2, dtype=np.uint32)
    own = expected(tiny, index, 0)[1]
    g = np.random.default_rng(61)
    calls = []
    for in_stride in (0, 7, 2):
        dense, in_offs = _random_dense(g, len(index), in_stride, own)
        want = expected_scatter(tiny, index, dense, in_stride, in_offs)
        for shift, in_shift in SHIFTS:
            calls.append(Call(gpu, DevBatch(tiny, shift), index, dense, in_stride, in_offs,
                              in_shift=in_shift, want=want))
    s, ln = spans(tiny)
    assert ln[1::2].sum() > 3000 and ln[0::2].sum() > 3000
    # a tile of the general path and one entry more; all-zero lengths; an empty batch
    for n in (255, 256, 257):
        for src in (tiny, _general_sources()[3]):
            idx = np.random.default_rng(n).permutation(src.count)[:n]
            for in_stride, (shift, in_shift) in ((0, SHIFTS[4]), (60, SHIFTS[11])):
                dense, in_offs = _random_dense(g, n, in_stride, expected(src, idx, 0)[1])
                calls.append(Call(gpu, DevBatch(src, shift), idx, dense, in_stride, in_offs,
                                  in_shift=in_shift))
    zeros = Src("zeros", tiny.data, 700, 0, np.full(701, 33, dtype=U64), False)
    calls.append(Call(gpu, DevBatch(zeros, 1), np.arange(700), np.zeros(700 * 16, np.uint8), 16,
                      want=tiny.data))
    calls.append(Call(gpu, DevBatch(tiny), np.full(300, 0xffffffff, dtype=np.uint32),
                      np.zeros(300 * 8, np.uint8), 8, want=tiny.data))
    empty = Src("empty", tiny.data, 0, 64, None, False)
    calls.append(Call(gpu, DevBatch(empty), [0, 7, 0xffffffff], np.zeros(192, np.uint8), 64,
                      want=tiny.data))
    calls.append(Call(gpu, DevBatch(tiny), [], np.zeros(0, np.uint8), 64, want=tiny.data))
    calls.append(Call(gpu, DevBatch(tiny), [], np.zeros(0, np.uint8), 0, np.zeros(1, dtype=U64),
                      want=tiny.data))
    run_all(calls)


# ---------------------------------------------------------------- far packets

SIZE = G4 + (2 << 20)


def test_scatter_far_packets(gpu):
    """one zero-filled 4 GiB + 2 MiB buffer as the batch's data, its packets past 4 GiB (and one
    across it), laid out as test_gather_far_packets does.  A wrong address or length formed from
    these inputs stays inside the allocation: starts lie at most 1 MiB past 4 GiB and no length
    exceeds 1,500.  Dense bytes are 1..255, the buffer zero: the bytes of every packet with 64 on
    each side, and the count of non-zero bytes of the whole buffer, say what was written."""
    import torch
    dev = _dev()
    g = np.random.default_rng(24)
    lens = [0, 1, 15, 16, 17, 64, 100, 777, 1500, 33, 64, 5]
    starts = [G4 + 4096 * (k + 1) + int(g.integers(0, 64)) for k in range(len(lens))]
    starts[-3], starts[-2], starts[-1] = G4 - 20, 8192 + 3, 70000   # across 4 GiB; two near ones
    pairs = [(s, s + ln) for s, ln in zip(starts, lens)]
    pairs += [(G4 + 9000, G4 + 8000), (4096, 4096 + G4), (1 << 20, (1 << 20) + G4 + 77)]
    ext = torch.from_numpy(np.array(pairs, dtype=U64).reshape(-1).view(np.int64)).to(dev)
    index = np.array([12, 7, 0, 13, 8, 14, 9, 1, 2, 3, 4, 5, 6, 10, 11, 40], dtype=np.uint32)
    d_index = torch.from_numpy(index.view(np.int32)).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(SIZE, dtype=torch.uint8, device=dev)

    def check(places, what):
        """places: (start, bytes expected there); everything else must still be zero"""
        torch.cuda.synchronize()
        for s, want in places:
            got = buf[s - 64:s + len(want) + 64].cpu().numpy()
            np.testing.assert_array_equal(got[64:64 + len(want)], want, err_msg=what)
            assert not got[:64].any() and not got[64 + len(want):].any(), what
        assert int(torch.count_nonzero(buf)) == sum(len(w) for _, w in places), what
        for s, want in places:
            buf[s:s + len(want)] = 0

    try:
        for in_stride, shift in ((0, 0), (0, 5), (64, 0), (200, 3), (1500, 8)):
            n = len(index)
            lj = np.array([lens[i] if i < len(lens) else 0 for i in index], dtype=np.int64)
            if in_stride:
                at = np.arange(n, dtype=np.int64) * in_stride
                k, total, d_offs = np.minimum(lj, in_stride), n * in_stride, None
            else:
                offs = np.concatenate([[0], np.cumsum(lj)])
                at, k, total = offs[:-1], lj, int(offs[-1])
                d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
            dense = g.integers(1, 256, total, dtype=np.uint8)
            d_dense, lead = framed(dense, shift)
            gpu.scatter_dev(0, buf.data_ptr(), len(pairs), 0, d_index.data_ptr(), n, in_stride,
                            d_dense.data_ptr() + lead, total,
                            None if d_offs is None else d_offs.data_ptr(), ext.data_ptr(), st,
                            extents=True)
            check([(starts[i], dense[at[j]:at[j] + k[j]]) for j, i in enumerate(index)
                   if i < len(lens)], "in_stride %d shift %d" % (in_stride, shift))
        # the row path with its packets past 4 GiB: the buffer as 64-byte packets
        nrows = SIZE // 64
        ridx = np.array([s // 64 for s in starts] + [nrows - 1, nrows], dtype=np.uint32)
        assert ridx.max() > (1 << 26) and len(set(ridx.tolist())) == len(ridx)
        dense = g.integers(1, 256, len(ridx) * 64, dtype=np.uint8)
        d_dense, lead = framed(dense, 0)
        d_ridx = torch.from_numpy(ridx.view(np.int32)).to(dev)
        gpu.scatter_dev(0, buf.data_ptr(), nrows, 64, d_ridx.data_ptr(), len(ridx), 64,
                        d_dense.data_ptr() + lead, len(dense), stream=st)
        check([(int(r) * 64, dense[64 * j:64 * j + 64]) for j, r in enumerate(ridx[:-1])], "rows")
    finally:
        del buf
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- merge


class MergeCall:
    """one ebpf_batch_merge_dev call on framed device copies of ret and faults"""

    def __init__(self, gpu, ret, faults, index, ret2, faults2, stream=None):
        import torch
        dev = _dev()
        count, n = len(ret), len(index)
        index = np.ascontiguousarray(index, dtype=np.uint32)
        self.count = count
        self.want = expected_merge(ret, faults, index, ret2, faults2)
        r = np.full(count + 16, RET_GUARD, dtype=U64)
        r[8:8 + count] = ret
        self.ret = torch.from_numpy(r.view(np.int64)).to(dev)
        self.faults = None if faults is None else framed(faults, 3)[0]
        self.keep = [torch.from_numpy(index.view(np.int32)).to(dev),
                     torch.from_numpy(np.ascontiguousarray(ret2, dtype=U64).view(np.int64)).to(dev),
                     None if faults2 is None else torch.from_numpy(faults2).to(dev)]
        st = (stream or torch.cuda.current_stream()).cuda_stream
        gpu.merge_dev(0, self.ret.data_ptr() + 64,
                      None if faults is None else self.faults.data_ptr() + PAD + 3, count,
                      self.keep[0].data_ptr() if n else None, n,
                      self.keep[1].data_ptr() if n else None,
                      None if faults2 is None or not n else self.keep[2].data_ptr(), st)

    def check(self):
        r = self.ret.cpu().numpy().view(U64)
        assert (r[:8] == RET_GUARD).all() and (r[8 + self.count:] == RET_GUARD).all()
        np.testing.assert_array_equal(r[8:8 + self.count], self.want[0])
        if self.faults is not None:
            check_frame(self.faults.cpu().numpy(), PAD + 3, self.want[1], "faults")


def test_merge_counts(gpu):
    g = np.random.default_rng(70)
    ret = g.integers(0, 1 << 63, NROWS).astype(U64)
    faults = g.integers(0, 4, NROWS).astype(np.uint8)
    calls = []
    for n in ROW_COUNTS:
        index = _row_list(n, 1000 + n)
        ret2 = g.integers(0, 1 << 63, n).astype(U64)
        faults2 = g.integers(1, 9, n).astype(np.uint8)
        for f in (faults, None):
            for f2 in (faults2, None):
                calls.append(MergeCall(gpu, ret, f, index, ret2, f2))
    calls.append(MergeCall(gpu, ret[:0], faults[:0], [0, 7, 0xffffffff], [1, 2, 3], None))
    run_all(calls)
    assert (calls[-5].want[0] != ret).sum() > 4000


def test_merge_long_list(gpu):
    g = np.random.default_rng(71)
    count = BIG + 90
    ret = g.integers(0, 1 << 63, count).astype(U64)
    faults = g.integers(0, 4, count).astype(np.uint8)
    index = g.permutation(count + 40)[:BIG].astype(np.uint32)   # (some at and past count)
    assert (index >= count).any()
    c = MergeCall(gpu, ret, faults, index, g.integers(0, 1 << 63, BIG).astype(U64),
                  g.integers(1, 9, BIG).astype(np.uint8))
    run_all([c])


# ---------------------------------------------------------------- ordering and determinism


def test_scatter_same_call_twice(gpu):
    src = _general_sources()[2]
    db = DevBatch(src, 1)
    index = scatter_lists(src.count)["whole"]
    g = np.random.default_rng(80)
    for in_stride in (0, 64):
        dense, in_offs = _random_dense(g, len(index), in_stride, expected(src, index, 0)[1])
        a = Call(gpu, db, index, dense, in_stride, in_offs, in_shift=1)
        b = Call(gpu, db, index, dense, in_stride, in_offs, in_shift=1)
        run_all([a, b])
        assert a.result().tobytes() == b.result().tobytes()


def test_scatter_two_streams_at_once(gpu):
    """two streams, each with scatters into batches of its own"""
    import torch
    tiny, edges = _tiny_src(), _general_sources()[3]
    g = np.random.default_rng(81)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    calls = []
    for k in range(6):
        s, src = ((s1, tiny), (s2, edges))[k % 2]
        index = g.permutation(src.count)[:src.count - 7 * k]
        in_stride = (0, 60, 7)[k // 2]
        dense, in_offs = _random_dense(g, len(index), in_stride, expected(src, index, 0)[1])
        with torch.cuda.stream(s):
            calls.append(Call(gpu, DevBatch(src, k), index, dense, in_stride, in_offs, in_shift=k,
                              stream=s))
    run_all(calls)


def test_scatter_follows_gather_on_a_stream(gpu):
    """gather, a kernel that rewrites the dense batch, scatter: enqueued back to back on one
    stream with no synchronisation between them"""
    import torch
    rows, edges = _row_src(64), _general_sources()[3]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    checks = []
    with torch.cuda.stream(s):
        for src, in_stride in ((rows, 64), (edges, 0), (edges, 60)):
            index = scatter_lists(src.count)["class"]
            n = len(index)
            db = DevBatch(src)
            buf = db.fresh()
            d_index = torch.from_numpy(index.view(np.int32)).to(_dev())
            want_dense, offs = expected(src, index, in_stride)
            size = len(want_dense)
            dense = torch.zeros(size + 16, dtype=torch.uint8, device=_dev())
            d_offs = None if in_stride else torch.zeros(n + 1, dtype=torch.int64, device=_dev())
            args = (d_index.data_ptr(), n, in_stride, dense.data_ptr(), size,
                    None if d_offs is None else d_offs.data_ptr(),
                    None if db.offs is None else db.offs.data_ptr(), s.cuda_stream)
            gpu.gather_dev(0, buf.data_ptr() + db.lead, src.count, src.stride, *args)
            dense.bitwise_xor_(FLIP)
            gpu.scatter_dev(0, buf.data_ptr() + db.lead, src.count, src.stride, *args)
            checks.append((buf, db.lead, expected_scatter(src, index, want_dense ^ FLIP, in_stride,
                                                          offs), [d_index, dense, d_offs]))
    torch.cuda.synchronize()
    for buf, lead, want, _ in checks:
        check_frame(buf.cpu().numpy(), lead, want)


# ---------------------------------------------------------------- a real batch, end to end


@pytest.mark.parametrize("variant", [0, 1])
def test_scatter_and_merge_close_the_pipeline(gpu, env, variant):
    """C4, steer, gather the largest class, a storing second stage over the dense batch, scatter
    and merge: the batch, ret and faults in packet order, with the members' entries the second
    stage's.  Nothing but `starts` is read on the host between the steps.

    On variant 0 the storing second stage takes the staged kernel (layout 1): no packet read
    follows its stores, so the staged registers' going stale cannot matter
    (asm_runtime.cpp asm_program_stores_last)."""
    import torch
    from test_gpu_addressing import _loaded, _oracle, _store_prog
    from test_gpu_steer import C4Run, NREAL, _c4_packets
    r = C4Run(gpu, env, variant)
    dev = r.data.device
    st = torch.cuda.current_stream().cuda_stream
    ret1 = r.ret.cpu().numpy().view(U64).copy()
    flt1 = r.faults.cpu().numpy().copy()
    in_place = r.data.clone()
    starts = r.starts.cpu().numpy().view(U64).astype(np.int64)
    b = int(np.argmax(np.diff(starts)))
    lo, n = int(starts[b]), int(starts[b + 1] - starts[b])
    members_ptr = r.index.data_ptr() + 4 * lo

    pr = _store_prog()
    dense = torch.full((n * 64 + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    ret2 = torch.full((n,), -1, dtype=torch.int64, device=dev)
    flt2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    ext = torch.full((2 * n,), -1, dtype=torch.int64, device=dev)
    ret3 = torch.full((n,), -1, dtype=torch.int64, device=dev)
    flt3 = torch.zeros(n, dtype=torch.uint8, device=dev)
    with _loaded(gpu, env, pr, variant) as (p, _):
        gpu.gather_dev(0, r.data.data_ptr(), NREAL, 64, members_ptr, n, 64, dense.data_ptr(), n * 64,
                       stream=st)
        p.run_batch_dev(0, dense.data_ptr(), n, 64, ret2.data_ptr(), None, flt2.data_ptr(), None, st)
        gpu.scatter_dev(0, r.data.data_ptr(), NREAL, 64, members_ptr, n, 64, dense.data_ptr(),
                        n * 64, stream=st)
        gpu.merge_dev(0, r.ret.data_ptr(), r.faults.data_ptr(), NREAL, members_ptr, n,
                      ret2.data_ptr(), flt2.data_ptr(), st)
        torch.cuda.synchronize()
        layout = p.exec_info(0)[1]
        # the cross-check: the second stage in place over the class's extents, on a copy
        gpu.select_dev(0, in_place.data_ptr(), NREAL, 64, members_ptr, n, ext.data_ptr(), stream=st)
        p.run_batch_dev(0, in_place.data_ptr(), n, 0, ret3.data_ptr(), ext.data_ptr(),
                        flt3.data_ptr(), None, st, extents=True)
        torch.cuda.synchronize()

    members =r.index.cpu().numpy().view(np.uint32)[lo:lo + n].astype(np.int64)
    gathered = np.ascontiguousarray(_c4_packets()[members])
    w_ret2, w_flt2, after, _ = _oracle(pr, gathered, n, 64)
    after = np.asarray(after, dtype=np.uint8).reshape(n, 64)
    assert (after != gathered).any() and n > 100
    want = _c4_packets().copy()
    want[members] = after
    w_ret, w_flt = ret1.copy(), flt1.copy()
    w_ret[members], w_flt[members] = w_ret2, w_flt2
    assert (dense[n * 64:] == SENTINEL).all()
    np.testing.assert_array_equal(r.data.cpu().numpy(), want.reshape(-1))
    np.testing.assert_array_equal(r.ret.cpu().numpy().view(U64), w_ret)
    np.testing.assert_array_equal(r.faults.cpu().numpy(), w_flt)
    np.testing.assert_array_equal(in_place.cpu().numpy(), want.reshape(-1))
    np.testing.assert_array_equal(ret3.cpu().numpy().view(U64), w_ret2)
    np.testing.assert_array_equal(flt3.cpu().numpy(), w_flt2)
    if variant == 0:
        assert layout == 1   # the second stage ran on the staged kernel


@pytest.mark.parametrize("variant", [0, 1])
def test_storing_programs_and_the_staged_kernel(gpu, env, variant):
    """a dense 64-byte-stride batch: a program with no packet read behind its stores runs staged
    (layout 1 on variant 0); one that reads the byte it stored keeps the general kernel, which
    reads the packet from memory.  Results, faults and packet bytes are the oracle's either way."""
    import torch
    import stdprogs
    from test_gpu_addressing import I, P, _loaded, _oracle, _run_dev, _store_prog
    from test_gpu_steer import _c4_packets
    code, rel = stdprogs.asm([I("ldxb", 2, 1, 0), I("add64_imm", 2, imm=1), I("stxb", 1, 2, 0),
                              I("ldxb", 0, 1, 0), I("ldxb", 3, 1, 12), I("add64_reg", 0, 3),
                              I("exit")])
    n = 1000
    rows = np.ascontiguousarray(_c4_packets()[:n])
    for pr, staged in ((_store_prog(), True), (P("store_load", code, rel, [], True), False)):
        w_ret, w_flt, after, _ = _oracle(pr, rows, n, 64)
        data = torch.from_numpy(rows.reshape(-1)).to(_dev())
        with _loaded(gpu, env, pr, variant) as (p, _):
            ret, flt, _ = _run_dev(p, data.data_ptr(), n, 64)
            layout = p.exec_info(0)[1]
        np.testing.assert_array_equal(flt, w_flt, err_msg=pr.name)
        np.testing.assert_array_equal(ret, w_ret, err_msg=pr.name)
        np.testing.assert_array_equal(data.cpu().numpy(),
                                      np.asarray(after, dtype=np.uint8).reshape(-1), err_msg=pr.name)
        assert (np.asarray(after, dtype=np.uint8).reshape(-1) != rows.reshape(-1)).any()
        if variant == 0:
            assert layout == (1 if staged else 0), pr.name
