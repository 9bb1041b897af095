"""Running totals per segment on the device (include/ebpf_gpu.h: ebpf_batch_scan_dev;
csrc/hip/scan.hip) against the host function, which test_scan.py checks against numpy; the shapes
come from test_reduce.py.  Integer results: every comparison is exact.

Shapes: T = native.STEER_TILE list positions go to one workgroup, 16 consecutive ones to a thread,
64 threads to a wave, so the list lengths sit around 64, 256 and T and the runs of 63, 64, 4095
and T drift against, and sit on, every one of those edges; 2M + 5 entries (513 tiles) make the
carry cross more than 256 tile edges, and 1,025 tiles plus 3 entries give a thread of the carry
kernel two tiles to walk.  Every output buffer is pre-filled with a value no result holds and is
GUARD entries longer than the call may write; the host function gets the same buffers, so
comparing them whole checks the zeros where no segment is and the unwritten tails too.  No test
feeds a table that is not non-decreasing or that ends past the list."""
import ctypes

import numpy as np
import pytest

import pyoracle
from gpu_buffers import run, up
from test_reduce import (BIG, COUNTS, GUARD, MID, SEGMENTATIONS, T, U64, Case, batch_form,
                         list_of, segmentation, verdicts)
from test_scan import FILL, FORMS, SCANS, TYPES, budgets_of, host, places, shaped

pytestmark = pytest.mark.gpu

WIDTHS = [1, 8, 32, 33, 64]
OTHER = {"rank": 0x01234567, "bytes_before": 0x0123456789abcdef,
         "sum_before": 0x0123456789abcdef, "over": 0xa7}


class Dev:
    """one scan call's device buffers; outputs pre-filled with `fill`"""

    def __init__(self, c, budgets=None, fill=FILL):
        self.c, self.fill = c, fill
        if budgets is None and "over" in c.want:
            budgets = budgets_of(c)
        self.host_budgets = budgets
        self.index = up(c.index)
        self.starts = up(c.seg_starts)
        # (a batch of no packets still names a ret where values are wanted: one unused word)
        self.ret = None if c.ret is None else up(c.ret if len(c.ret) else np.zeros(1, U64))
        self.offsets = None if c.offsets is None else up(c.offsets)
        self.nseg = None if c.nseg is None else up(np.array([c.nseg], dtype=U64))
        self.budgets = None if budgets is None else up(
            budgets if len(budgets) else np.zeros(1, U64))
        self.outs = {k: up(np.full(c.n + GUARD, fill[k], dtype=TYPES[k]))
                     for k in c.want}

    def enqueue(self, gpu, stream):
        c = self.c
        b = c.batch(None if self.offsets is None else self.offsets.data_ptr())
        scans = gpu.BatchScans(*[self.outs[k].data_ptr() if k in self.outs else None
                                 for k in SCANS])
        return gpu.lib().ebpf_batch_scan_dev(
            0, ctypes.byref(b) if c.has_batch else None,
            None if self.ret is None else self.ret.data_ptr(), c.count, c.shift, c.bits,
            self.index.data_ptr() if c.n else None, c.n, self.starts.data_ptr(), c.cap,
            None if self.nseg is None else self.nseg.data_ptr(),
            None if self.budgets is None else self.budgets.data_ptr(), ctypes.byref(scans),
            stream.cuda_stream)

    def result(self):
        return {k: v.cpu().numpy().view(TYPES[k]) for k, v in self.outs.items()}

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers, GUARD and all"""
        code, w = host(gpu, self.c, self.host_budgets, self.fill)
        assert code == 0, msg
        got = self.result()
        for k in self.c.want:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


@pytest.mark.parametrize("n", COUNTS)
def test_scan_shapes(gpu, n):
    cases = [(seg, unc) for seg in SEGMENTATIONS for unc in (False, True)]
    devs = [Dev(shaped(n, seg, unc, FORMS[(k + n) % 4], WIDTHS[k % 5],
                       min((k * 5) % 31, 64 - WIDTHS[k % 5])))
            for k, (seg, unc) in enumerate(cases)]
    run(gpu, devs)
    for d, (seg, unc) in zip(devs, cases):
        d.check(gpu, "%s n=%d uncovered=%s" % (seg, n, unc))


@pytest.mark.parametrize("seg", ["whole", "runs4095"])
def test_scan_many_tiles(gpu, seg):
    """513 tiles: a segment over all of them, and one tile edge in every run of 4095"""
    d = Dev(shaped(BIG, seg, seg == "whole", "offsets", 33, 9))
    run(gpu, [d])
    got = d.check(gpu, seg)
    if seg == "whole":
        assert got["rank"][BIG - 8] == BIG - 8 - 5 and got["over"][:BIG].any()


def test_scan_carry_walks_two_tiles_a_thread(gpu):
    """past 1,024 tiles a thread of the carry kernel walks more than one"""
    n = 1025 * T + 3
    count = 1 << 20
    c = Case(list_of(n, count), segmentation("runs4095", n), None, count=count,
             form=batch_form("stride60", count), want=("rank", "bytes_before"))
    d = Dev(c)
    run(gpu, [d])
    d.check(gpu, "1025 tiles, runs of 4095")
    c = Case(c.index, segmentation("whole", n, True), None, count=count,
             form=batch_form("stride60", count), want=("rank", "bytes_before"))
    d = Dev(c)
    run(gpu, [d])
    got = d.check(gpu, "1025 tiles, one segment")
    assert got["bytes_before"][n - 8] > 60 * 1024 * T * 9 // 10


def test_scan_many_segments_begin_in_a_tile(gpu):
    """m one-entry segments and then one long one, around the reduce's staging thresholds;
    shifted by 5 positions the segments' ranks drift against the threads' 16 positions"""
    n = T + 100
    count = n - 50
    cases = [(m, a) for m in (255, 256, 257, 2047, 2048, 2049, T - 6) for a in (0, 5)]
    devs = []
    for m, a in cases:
        starts = np.concatenate([np.arange(m + 1), [n - a]]).astype(U64) + U64(a)
        devs.append(Dev(Case(list_of(n, count, m), starts, verdicts(count, 33, 7), 7, 33,
                             form=batch_form(FORMS[m % 4], count), want=SCANS)))
    run(gpu, devs)
    for d, (m, a) in zip(devs, cases):
        d.check(gpu, "%d singletons from position %d" % (m, a))


def test_scan_many_empty_segments_at_a_tile_edge(gpu):
    devs = [Dev(shaped(n, "many_empty", unc, form)) for n in (MID, T, T + 1)
            for unc in (False, True) for form in ("offsets", "stride60")]
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "many_empty n=%d" % d.c.n)


@pytest.mark.parametrize("bits", WIDTHS)
def test_scan_value_fields(gpu, bits):
    cases = [(shift, seg) for shift in (0, 3, 31, 64 - bits) if shift + bits <= 64
             for seg in ("whole", "runs63", "random")]
    devs = [Dev(shaped(MID, seg, True, "stride60", bits, shift)) for shift, seg in cases]
    run(gpu, devs)
    for d, (shift, seg) in zip(devs, cases):
        d.check(gpu, "bits %d shift %d %s" % (bits, shift, seg))


def test_scan_sums_wrap_and_bytes_pass_32_bits(gpu):
    count = MID
    ret = verdicts(count) | U64(1 << 63)
    devs = [Dev(Case(list_of(MID, count), segmentation(seg, MID), ret,
                     form=batch_form("extents", count), want=SCANS))
            for seg in ("whole", "runs63", "runsT")]
    run(gpu, devs)
    got = [d.check(gpu, "top bit") for d in devs]
    assert got[0]["bytes_before"][MID - 1] > 1 << 40 and got[1]["bytes_before"][:MID].max() > 1 << 32
    vals = ret[np.minimum(devs[0].c.index, count - 1).astype(np.int64)].astype(object)
    assert int(vals[:MID - 1].sum()) > 1 << 64     # (more than the modulus: it wrapped)


@pytest.mark.parametrize("form", FORMS)
def test_scan_lengths_and_budgets(gpu, form):
    """budgets of 0, of exactly a running total, of UINT64_MAX and of half a segment, by the
    segment's number (test_scan.budgets_of)"""
    cases = [(seg, unc, want) for seg in ("whole", "runs63", "singletons", "random", "steering")
             for unc, want in ((False, SCANS), (True, ("bytes_before", "over")))]
    devs = [Dev(shaped(MID, seg, unc, form, want=want)) for seg, unc, want in cases]
    run(gpu, devs)
    for d, (seg, unc, want) in zip(devs, cases):
        got = d.check(gpu, "%s %s" % (form, seg))
        assert got["over"][:MID].any()
        assert seg == "whole" or not got["over"][:MID].all()   # (its one budget is 0)


def test_scan_ignores_what_the_outputs_held(gpu):
    c = shaped(MID, "random", True, "offsets", 33, 7)
    a, b = Dev(c, fill=FILL), Dev(c, fill=OTHER)
    run(gpu, [a, b])
    ra, rb = a.check(gpu, "first fill"), b.check(gpu, "second fill")
    for k in SCANS:
        assert ra[k][:c.n].tobytes() == rb[k][:c.n].tobytes()
        assert (rb[k][c.n:] == OTHER[k]).all()


def test_scan_each_output_alone(gpu):
    wants = [(k,) for k in SCANS] + [("rank", "over"), ("bytes_before", "sum_before"),
                                     ("sum_before", "over")]
    devs = [Dev(shaped(MID, seg, True, "extents", 33, 7, want=w)) for w in wants
            for seg in ("runs63", "runsT", "whole")]
    c = shaped(MID, "many_empty", False, want=("rank",))
    c.ret, c.has_batch = None, False      # nothing asks for a value or a length
    devs.append(Dev(c))
    c = shaped(MID, "runs4095", False, want=("rank",))
    c.ret, c.has_batch = None, False
    devs.append(Dev(c))
    c = shaped(MID, "many_empty", False, want=("bytes_before", "over"))
    c.ret = None
    devs.append(Dev(c))
    c = shaped(MID, "many_empty", False, want=("sum_before",))
    c.has_batch = False
    devs.append(Dev(c))
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "want %s" % (d.c.want,))
    # all four NULL: nothing to do
    import torch
    d = Dev(shaped(MID, "runs63", False, want=()))
    assert d.enqueue(gpu, torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()


def test_scan_segment_count_from_device_memory(gpu):
    """G below, equal to and above the cap: above, R = cap - 1 and the last group's positions are
    uncovered"""
    cap = len(segmentation("runs63", MID)) - 1
    devs = [Dev(shaped(MID, "runs63", False, nseg=g)) for g in (0, 1, cap - 1, cap, cap + 1, 1 << 40)]
    devs.append(Dev(Case(list_of(9, 9), [4], verdicts(9), form=(64, None, False), nseg=3,
                         want=SCANS)))
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "nseg %d" % d.c.nseg)
        end = int(d.c.seg_starts[d.c.segments]) if d.c.cap else 0
        assert not got["rank"][end:d.c.n].any()


def test_scan_no_list_and_no_packets(gpu):
    devs = [Dev(shaped(0, seg, False)) for seg in ("whole", "empties", "steering")]
    c = Case(list_of(50, 1), segmentation("runs63", 50), np.zeros(1, dtype=U64), count=0,
             form=(64, None, False), want=SCANS)   # a list over a batch of no packets: ranks alone
    devs.append(Dev(c))
    c = Case(list_of(MID, 1), segmentation("runs63", MID, True), np.zeros(1, dtype=U64), count=0,
             form=(64, None, False), want=SCANS)
    devs.append(Dev(c))
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "n %d count %d" % (d.c.n, d.c.count))
        assert not got["bytes_before"][:d.c.n].any() and not got["over"][:d.c.n].any()


# ---------------------------------------------------------------- after a run, on one stream

NREAL = 2 * T + 37
BUDGET = 300


def test_scan_after_group_on_one_stream(gpu, env):
    """run, group by a 16-bit field of the verdict, scan with 300 bytes a group: per group the
    packets within the quota are the longest prefix in packet order that fits"""
    import torch
    from generic_ebpf_amd import workloads
    from generic_ebpf_amd.workloads import I, R0, R1
    pk = workloads.packets_l2l3(NREAL, 64)
    lens = 40 + np.arange(NREAL) % 25
    data = np.concatenate([pk[i, :lens[i]] for i in range(NREAL)])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    lay = workloads.assemble([I("ldxw", R0, R1, 12), I("exit")])
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
    budgets = torch.full((cap,), BUDGET, dtype=torch.int64, device=dev)
    outs = {k: up(np.full(NREAL + GUARD, FILL[k], dtype=TYPES[k]))
            for k in SCANS}
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        p.run_batch_dev(0, d_data.data_ptr(), NREAL, 0, ret.data_ptr(), d_offs.data_ptr(),
                        flt.data_ptr(), None, st)
        gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), NREAL, 16, 16, index.data_ptr(), cap,
                      gkeys.data_ptr(), gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(),
                      tmp_bytes, st)
        gpu.scan_dev(0, ret.data_ptr(), NREAL, 0, 16, index.data_ptr(), NREAL,
                     gstarts.data_ptr(), cap, info.data_ptr(), budgets.data_ptr(),
                     *[outs[k].data_ptr() for k in SCANS], offsets_ptr=d_offs.data_ptr(),
                     stream=st)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    got_ret = ret.cpu().numpy().view(U64)
    np.testing.assert_array_equal(got_ret, w_ret)
    assert not w_flt.any()
    G, U = (int(v) for v in info.cpu())
    assert U == NREAL and 100 < G <= cap
    idx = index.cpu().numpy().view(np.uint32).astype(np.int64)
    outs = {k: v.cpu().numpy().view(TYPES[k]) for k, v in outs.items()}
    for k in SCANS:
        assert (outs[k][NREAL:] == FILL[k]).all(), k
        assert not outs[k][U:NREAL].any(), k          # (the faulted tail: none here)
    by_packet = {k: np.zeros(NREAL, dtype=TYPES[k]) for k in SCANS}
    for k in SCANS:
        by_packet[k][idx] = outs[k][:NREAL]
    keys = (got_ret >> U64(16)) & U64(0xffff)
    vals = got_ret & U64(0xffff)
    some_over = 0
    for key in gkeys.cpu().numpy().view(U64)[:G]:
        m = np.flatnonzero(keys == key)          # the group's packets in packet order
        total = np.cumsum(lens[m])
        within = total <= BUDGET                 # (lengths are positive: a prefix)
        np.testing.assert_array_equal(by_packet["over"][m], (~within).astype(np.uint8))
        np.testing.assert_array_equal(by_packet["rank"][m], np.arange(len(m)))
        np.testing.assert_array_equal(by_packet["bytes_before"][m], total - lens[m])
        np.testing.assert_array_equal(by_packet["sum_before"][m],
                                      np.cumsum(vals[m]) - vals[m])
        some_over += int((~within).sum())
    assert 0 < some_over < NREAL
