"""Reducing a list per segment on the device (include/ebpf_gpu.h: ebpf_batch_reduce_dev;
csrc/hip/reduce.hip) against the host function, which test_reduce.py checks against numpy; the
shapes come from there.  Integer results: every comparison is exact.

Shapes: T = native.STEER_TILE list positions go to one workgroup, 16 consecutive ones to a thread,
64 threads to a wave, so the list lengths sit around 64, 256 and T and the runs of 63, 64, 4095
and T drift against, and sit on, every one of those edges; 2M + 5 entries (513 tiles) make the
carry cross more than 256 tile edges.  Every output buffer is pre-filled with a value no result
holds and is GUARD entries longer than the call may write; the host function gets the same
buffers, so comparing them whole checks the unwritten tails too.  No test feeds a table that is
not non-decreasing or that ends past the list."""
import ctypes

import numpy as np
import pytest

import pyoracle
from gpu_buffers import run, up
from test_reduce import (BIG, COUNTS, GUARD, IDENTITY, MID, SEGMENTATIONS, SENTINEL, SUMS, T, U64,
                         Case, batch_form, list_of, reference, segmentation, shaped, verdicts)

pytestmark = pytest.mark.gpu

FORMS = ["stride64", "stride60", "offsets", "extents"]
WIDTHS = [1, 8, 32, 33, 64]


class Dev:
    """one reduce call's device buffers; outputs pre-filled with `fill`"""

    def __init__(self, c, fill=SENTINEL):
        import torch
        dev = torch.device("cuda:0")
        self.c, self.fill = c, fill
        self.index = up(c.index)
        self.starts = up(c.seg_starts)
        # (a batch of no packets still names a ret where values are wanted: one unused word)
        self.ret = None if c.ret is None else up(c.ret if len(c.ret) else np.zeros(1, U64))
        self.offsets = None if c.offsets is None else up(c.offsets)
        self.nseg = None if c.nseg is None else up(np.array([c.nseg], dtype=U64))
        signed = int(np.array([fill], dtype=U64).view(np.int64)[0])
        self.outs = {k: torch.full((c.cap + GUARD,), signed, dtype=torch.int64, device=dev)
                     for k in c.want}

    def enqueue(self, gpu, stream):
        c = self.c
        b = c.batch(None if self.offsets is None else self.offsets.data_ptr())
        sums = gpu.BatchSums(*[self.outs[k].data_ptr() if k in self.outs else None for k in SUMS])
        return gpu.lib().ebpf_batch_reduce_dev(
            0, ctypes.byref(b) if c.has_batch else None,
            None if self.ret is None else self.ret.data_ptr(), c.count, c.shift, c.bits,
            self.index.data_ptr() if c.n else None, c.n, self.starts.data_ptr(), c.cap,
            None if self.nseg is None else self.nseg.data_ptr(), ctypes.byref(sums),
            stream.cuda_stream)

    def result(self):
        return {k: v.cpu().numpy().view(U64) for k, v in self.outs.items()}

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers"""
        code, w = self.c.host(gpu, self.fill)
        assert code == 0, msg
        got = self.result()
        R = self.c.segments
        for k in self.c.want:
            np.testing.assert_array_equal(got[k][:R], w[k][:R], err_msg="%s: %s" % (msg, k))
            assert (got[k][R:] == U64(self.fill)).all(), "%s: %s written at or past R" % (msg, k)
        return got


@pytest.mark.parametrize("n", COUNTS)
def test_reduce_shapes(gpu, n):
    cases = [(seg, unc) for seg in SEGMENTATIONS for unc in (False, True)]
    devs = [Dev(shaped(n, seg, unc, FORMS[(k + n) % 4], WIDTHS[k % 5],
                       min((k * 5) % 31, 64 - WIDTHS[k % 5])))
            for k, (seg, unc) in enumerate(cases)]
    run(gpu, devs)
    for d, (seg, unc) in zip(devs, cases):
        d.check(gpu, "%s n=%d uncovered=%s" % (seg, n, unc))


@pytest.mark.parametrize("seg", ["whole", "runs4095"])
def test_reduce_many_tiles(gpu, seg):
    """513 tiles: a segment over all of them, and one tile edge in every run of 4095"""
    d = Dev(shaped(BIG, seg, seg == "whole", "offsets", 33, 9))
    run(gpu, [d])
    d.check(gpu, seg)


def test_reduce_many_segments_closed_in_a_tile(gpu):
    """m one-entry segments and then one long one: a tile that closes 256 segments or more writes
    them out through LDS, 2,048 at a time, so m sits around both numbers; shifted by 5 positions
    the segments' ranks drift against the threads' 16 positions"""
    n = T + 100
    count = n - 50
    cases = [(m, a) for m in (255, 256, 257, 2047, 2048, 2049, 2050, T - 6) for a in (0, 5)]
    devs = []
    for m, a in cases:
        starts = np.concatenate([np.arange(m + 1), [n - a]]).astype(U64) + U64(a)
        devs.append(Dev(Case(list_of(n, count, m), starts, verdicts(count, 33, 7), 7, 33,
                             form=batch_form(FORMS[m % 4], count))))
    run(gpu, devs)
    for d, (m, a) in zip(devs, cases):
        d.check(gpu, "%d singletons from position %d" % (m, a))


@pytest.mark.parametrize("bits", WIDTHS)
def test_reduce_value_fields(gpu, bits):
    cases = [(shift, seg) for shift in (0, 3, 31, 64 - bits) if shift + bits <= 64
             for seg in ("whole", "runs63", "random")]
    devs = [Dev(shaped(MID, seg, True, "stride60", bits, shift)) for shift, seg in cases]
    run(gpu, devs)
    for d, (shift, seg) in zip(devs, cases):
        d.check(gpu, "bits %d shift %d %s" % (bits, shift, seg))


def test_reduce_unsigned_and_wrapping(gpu):
    """values with the top bit set: minima and maxima are unsigned, and the sums wrap 2^64"""
    count = MID
    ret = verdicts(count) | (np.arange(count, dtype=U64) % U64(3) != 0).astype(U64) << U64(63)
    devs = [Dev(Case(list_of(MID, count), segmentation(seg, MID), ret, form=(64, None, False)))
            for seg in ("whole", "runs63", "singletons")]
    run(gpu, devs)
    got = [d.check(gpu, "top bit") for d in devs]
    vals = ret[devs[0].c.index[devs[0].c.index < count].astype(np.int64)]
    assert int(vals.astype(object).sum()) > 1 << 64
    assert got[0]["sum"][0] == int(vals.astype(object).sum()) % (1 << 64)
    assert got[0]["max"][0] >= 1 << 63 and got[0]["min"][0] < 1 << 63
    assert got[0]["max"][0] == vals.max() and got[0]["min"][0] == vals.min()


@pytest.mark.parametrize("form", FORMS)
def test_reduce_lengths(gpu, form):
    devs = [Dev(shaped(MID, seg, False, form, want=want))
            for seg in ("whole", "runs63", "singletons") for want in (SUMS, ("bytes",))]
    run(gpu, devs)
    got = [d.check(gpu, form) for d in devs]
    np.testing.assert_array_equal(got[0]["bytes"], got[1]["bytes"])
    if form == "extents":   # packets of 2^32 - 1 bytes: no 32-bit sum holds a segment's
        assert got[0]["bytes"][0] > 1 << 40 and got[2]["bytes"][:100].max() > 1 << 32


def test_reduce_ignores_what_the_outputs_held(gpu):
    c = shaped(MID, "random", True, "offsets", 33, 7)
    a, b = Dev(c, SENTINEL), Dev(c, 0x0123456789abcdef)
    run(gpu, [a, b])
    ra, rb = a.check(gpu, "first fill"), b.check(gpu, "second fill")
    for k in SUMS:
        assert ra[k][:c.segments].tobytes() == rb[k][:c.segments].tobytes()


def test_reduce_each_output_alone(gpu):
    wants = [(k,) for k in SUMS] + [("min", "bits"), ("bytes", "max")]
    devs = [Dev(shaped(MID, "runs63", True, "extents", 33, 7, want=w)) for w in wants]
    c = shaped(MID, "many_empty", False, want=("bytes",))
    c.ret = None                      # nothing asks for a value
    devs.append(Dev(c))
    c = shaped(MID, "many_empty", False, want=("sum", "min", "max", "bits"))
    c.has_batch = False               # nothing asks for a length
    devs.append(Dev(c))
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "want %s" % (d.c.want,))
    # all five NULL: nothing to do
    import torch
    d = Dev(shaped(MID, "runs63", False, want=()))
    assert d.enqueue(gpu, torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()


def test_reduce_segment_count_from_device_memory(gpu):
    """G below, equal to and above the cap: above, R = cap - 1 and entry cap - 1 stays"""
    cap = len(segmentation("runs63", MID)) - 1
    devs = [Dev(shaped(MID, "runs63", False, nseg=g)) for g in (0, 1, cap - 1, cap, cap + 1, 1 << 40)]
    devs.append(Dev(Case(list_of(9, 9), [4], verdicts(9), form=(64, None, False), nseg=3)))
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "nseg %d" % d.c.nseg)
        if d.c.nseg > cap and d.c.cap:
            assert d.c.segments == cap - 1 and got["bytes"][cap - 1] == SENTINEL
            assert got["bytes"][cap - 2] != SENTINEL


def test_reduce_no_list(gpu):
    devs = [Dev(shaped(0, seg, False)) for seg in ("whole", "empties", "steering")]
    c = Case(list_of(50, 1), segmentation("runs63", 50), np.zeros(1, dtype=U64), count=0,
             form=(64, None, False))   # a list over a batch of no packets: no lengths, no values
    devs.append(Dev(c))
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "n %d count %d" % (d.c.n, d.c.count))
        for k in SUMS:
            assert (got[k][:d.c.cap] == U64(IDENTITY[k])).all()


# ---------------------------------------------------------------- after a run, on one stream

NREAL = 2 * T + 37


def _real_batch():
    """packets of 40 to 64 bytes in offsets form"""
    from generic_ebpf_amd import workloads
    pk = workloads.packets_l2l3(NREAL, 64)
    lens = 40 + np.arange(NREAL) % 25
    data = np.concatenate([pk[i, :lens[i]] for i in range(NREAL)])
    return pk, data, np.concatenate([[0], np.cumsum(lens)]).astype(U64)


def _program(load, at):
    from generic_ebpf_amd import workloads
    from generic_ebpf_amd.workloads import I, R0, R1
    return workloads.assemble([I(load, R0, R1, at), I("exit")])


def test_reduce_after_group_on_one_stream(gpu, env):
    """run, group by a 16-bit field of the verdict, reduce the rest of it per group: nothing is
    read on the host but info and the sums"""
    import torch
    pk, data, offsets = _real_batch()
    lay = _program("ldxw", 12)
    w_ret, w_flt, _, _ = pyoracle.OracleProgram(lay.code, lay.relocs, []).run(
        data, NREAL, 0, offsets=offsets)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_data, d_offs = up(data), up(offsets)
    ret = torch.full((NREAL,), -1, dtype=torch.int64, device=dev)
    flt = torch.zeros(NREAL, dtype=torch.uint8, device=dev)
    cap = NREAL
    index = torch.full((NREAL,), -1, dtype=torch.int32, device=dev)
    gkeys = torch.zeros(cap, dtype=torch.int64, device=dev)
    gstarts = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    info = torch.zeros(2, dtype=torch.int64, device=dev)
    tmp_bytes = gpu.group_tmp_bytes(NREAL, 16)
    tmp = torch.zeros(max(tmp_bytes, 8), dtype=torch.uint8, device=dev)
    signed = int(np.array([SENTINEL], dtype=U64).view(np.int64)[0])
    outs = {k: torch.full((cap + GUARD,), signed, dtype=torch.int64, device=dev) for k in SUMS}
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        p.run_batch_dev(0, d_data.data_ptr(), NREAL, 0, ret.data_ptr(), d_offs.data_ptr(),
                        flt.data_ptr(), None, st)
        gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), NREAL, 16, 16, index.data_ptr(), cap,
                      gkeys.data_ptr(), gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(),
                      tmp_bytes, st)
        gpu.reduce_dev(0, ret.data_ptr(), NREAL, 0, 16, index.data_ptr(), NREAL,
                       gstarts.data_ptr(), cap, info.data_ptr(), *[outs[k].data_ptr() for k in SUMS],
                       offsets_ptr=d_offs.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    got_ret = ret.cpu().numpy().view(U64)
    np.testing.assert_array_equal(got_ret, w_ret)
    assert not w_flt.any()
    G, U = (int(v) for v in info.cpu())
    assert U == NREAL and 100 < G <= cap
    keys = (got_ret >> U64(16)) & U64(0xffff)
    vals = got_ret & U64(0xffff)
    lens = np.diff(offsets)
    for k, v in outs.items():
        v = v.cpu().numpy().view(U64)
        assert (v[G:] == SENTINEL).all(), k
        outs[k] = v[:G]
    for g, key in enumerate(gkeys.cpu().numpy().view(U64)[:G]):
        m = keys == key          # the group's packets, whatever their order
        assert outs["bytes"][g] == lens[m].sum() and outs["sum"][g] == vals[m].sum()
        assert outs["min"][g] == vals[m].min() and outs["max"][g] == vals[m].max()
        assert outs["bits"][g] == np.bitwise_or.reduce(vals[m])
    assert outs["bytes"].sum() == lens.sum()


def test_reduce_after_steer_on_one_stream(gpu, env):
    """run, steer, reduce with the steering table: bytes per verdict class"""
    import torch
    pk, data, offsets = _real_batch()
    lay = _program("ldxb", 20)
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    d_data, d_offs = up(data), up(offsets)
    ret = torch.full((NREAL,), -1, dtype=torch.int64, device=dev)
    flt = torch.zeros(NREAL, dtype=torch.uint8, device=dev)
    index = torch.full((NREAL,), -1, dtype=torch.int32, device=dev)
    starts = torch.zeros(gpu.STEER_STARTS, dtype=torch.int64, device=dev)
    signed = int(np.array([SENTINEL], dtype=U64).view(np.int64)[0])
    bins = gpu.EBPF_HIST_BINS
    out = torch.full((bins + GUARD,), signed, dtype=torch.int64, device=dev)
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        p.run_batch_dev(0, d_data.data_ptr(), NREAL, 0, ret.data_ptr(), d_offs.data_ptr(),
                        flt.data_ptr(), None, st)
        gpu.steer_dev(0, ret.data_ptr(), flt.data_ptr(), NREAL, index.data_ptr(),
                      starts.data_ptr(), st)
        gpu.reduce_dev(0, None, NREAL, 0, 0, index.data_ptr(), NREAL, starts.data_ptr(), bins,
                       bytes_ptr=out.data_ptr(), offsets_ptr=d_offs.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    got_ret = ret.cpu().numpy().view(U64)
    np.testing.assert_array_equal(got_ret, pk[:, 20])
    lens = np.diff(offsets)
    out = out.cpu().numpy().view(U64)
    assert (out[bins:] == SENTINEL).all()
    want = np.bincount(np.minimum(got_ret, 255).astype(np.int64), weights=None, minlength=bins)
    per_class = np.array([lens[np.minimum(got_ret, 255) == b].sum() for b in range(bins)])
    np.testing.assert_array_equal(out[:bins], per_class.astype(U64))
    assert out[:bins].sum() == lens.sum() and (out[:bins] != 0).sum() == (want != 0).sum() > 100
    c = Case(index.cpu().numpy().view(np.uint32), starts.cpu().numpy().view(U64), None,
             count=NREAL, form=(0, offsets, False), want=("bytes",))
    np.testing.assert_array_equal(out[:bins], reference(c)["bytes"])
