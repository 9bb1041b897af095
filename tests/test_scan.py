"""Running totals per segment on the host (include/ebpf_gpu.h: ebpf_batch_scan) against a numpy
reference written here — vectorised: an exclusive cumsum in unsigned 64 bits less its value at the
segment's start, which is exact modulo 2^64 — and the argument checks of ebpf_batch_scan /
ebpf_batch_scan_dev, which come before any device work and so hold without a GPU.

Ranks, byte counts, sums modulo 2^64 and flags have one right answer, so every comparison is
exact.  The shapes (list lengths, segmentations, batch forms, value fields) are test_reduce.py's;
test_gpu_scan.py checks the device function against the host function on them."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from test_reduce import (COUNTS, GUARD, SEGMENTATIONS, SENTINEL, T, U64, Case, batch_form,
                         lengths_of, list_of, segmentation, verdicts)
from test_reduce import reference as reduce_reference

SCANS = ("rank", "bytes_before", "sum_before", "over")
TYPES = {"rank": np.uint32, "bytes_before": U64, "sum_before": U64, "over": np.uint8}
FILL = {"rank": SENTINEL & 0xffffffff, "bytes_before": SENTINEL, "sum_before": SENTINEL,
        "over": SENTINEL & 0xff}       # what every output holds on entry; no result is it
FORMS = ["stride64", "stride60", "offsets", "extents"]
MAX64 = (1 << 64) - 1
FAKE = 4096   # a non-NULL pointer that nothing may dereference


def fields(c):
    """(lens u64[n], vals u64[n]) of the listed entries: 0 where an entry has none"""
    i = c.index.astype(np.int64)
    inside = i < c.count
    at = np.where(inside, i, 0)
    lens = np.zeros(c.n, dtype=U64)
    vals = np.zeros(c.n, dtype=U64)
    if c.has_batch and c.count:
        lens = np.where(inside, lengths_of(c.count, c.stride, c.offsets, c.extents)[at], U64(0))
    if c.ret is not None and c.count:
        vals = np.where(inside, (c.ret[at] >> U64(c.shift)) & U64((1 << c.bits) - 1), U64(0))
    return lens.astype(U64), vals.astype(U64)


def places(c):
    """(covered bool[n], g int[n], start int[n]): whether a segment covers a position, which,
    and where it begins (anything where none does)"""
    R, pos = c.segments, np.arange(c.n)
    if R == 0 or c.n == 0:
        z = np.zeros(c.n, dtype=np.int64)
        return np.zeros(c.n, dtype=bool), z, z
    S = c.seg_starts[:R + 1].astype(np.int64)
    covered = (pos >= S[0]) & (pos < S[R])
    g = np.minimum(np.searchsorted(S[1:], pos, side="right"), R - 1)   # the ends at or before pos
    return covered, g, np.minimum(S[g], c.n - 1)


def reference(c, budgets=None):
    """{name: array[n]}: exclusive cumsums less their value where the segment begins"""
    lens, vals = fields(c)
    covered, g, start = places(c)
    out = {k: np.zeros(c.n, dtype=TYPES[k]) for k in SCANS}
    if not c.n:
        return out
    pos = np.arange(c.n)
    ex_bytes = np.concatenate([np.zeros(1, U64), np.cumsum(lens, dtype=U64)[:-1]])
    ex_sum = np.concatenate([np.zeros(1, U64), np.cumsum(vals, dtype=U64)[:-1]])   # (wraps)
    out["rank"] = np.where(covered, pos - start, 0).astype(np.uint32)
    out["bytes_before"] = np.where(covered, ex_bytes - ex_bytes[start], U64(0)).astype(U64)
    out["sum_before"] = np.where(covered, ex_sum - ex_sum[start], U64(0)).astype(U64)
    if budgets is not None and c.segments:
        b = budgets[g].astype(U64)
        out["over"] = (covered & (out["bytes_before"] + lens > b)).astype(np.uint8)
    return out


def budgets_of(c):
    """seg_cap budgets, by the segment's number: 0; exactly the running total that includes the
    segment's middle entry (the strict `>`: that entry is within, the next longer one is not);
    UINT64_MAX; half of what the segment carries; past R anything"""
    lens, _ = fields(c)
    g = np.random.default_rng(c.n + c.cap)
    b = g.integers(0, 1 << 63, c.cap, dtype=U64)
    R = c.segments
    if R == 0:
        return b
    inc = np.concatenate([np.zeros(1, U64), np.cumsum(lens, dtype=U64)])   # (exclusive, n + 1)
    S = np.minimum(c.seg_starts[:R + 1].astype(np.int64), c.n)
    a, e = S[:-1], S[1:]
    mid = np.minimum((a + e + 1) // 2, e)
    kind = np.arange(R) % 4
    b[:R] = np.select([kind == 0, kind == 1, kind == 2],
                      [U64(0), inc[mid] - inc[a], U64(MAX64)], (inc[e] - inc[a]) // U64(2))
    return b


def host(native, c, budgets=None, fill=FILL):
    """the host function on outputs pre-filled with `fill`, GUARD entries longer than the call
    may write: (code, {name: array[n + GUARD]})"""
    outs = {k: np.full(c.n + GUARD, fill[k], dtype=TYPES[k]) for k in c.want}
    scans = native.BatchScans(*[outs[k].ctypes.data if k in outs else None for k in SCANS])
    b = c.batch(None if c.offsets is None else c.offsets.ctypes.data)
    ns = None if c.nseg is None else np.array([c.nseg], dtype=U64)
    code = native.lib().ebpf_batch_scan(
        ctypes.byref(b) if c.has_batch else None,
        None if c.ret is None else c.ret.ctypes.data, c.count, c.shift, c.bits,
        c.index.ctypes.data if c.n else None, c.n, c.seg_starts.ctypes.data, c.cap,
        None if ns is None else ns.ctypes.data,
        None if budgets is None else budgets.ctypes.data, ctypes.byref(scans))
    return code, outs


def check_host(native, c, budgets=None, msg=""):
    """the whole contract of the host function for case c"""
    if budgets is None and "over" in c.want:
        budgets = budgets_of(c)
    code, outs = host(native, c, budgets)
    assert code == 0, msg
    w = reference(c, budgets)
    covered = places(c)[0]
    for k in c.want:
        np.testing.assert_array_equal(outs[k][:c.n], w[k], err_msg="%s %s" % (msg, k))
        assert not outs[k][:c.n][~covered].any(), "%s %s: not 0 where no segment is" % (msg, k)
        assert (outs[k][c.n:] == FILL[k]).all(), "%s %s: written at or past n" % (msg, k)
    return outs


def shaped(n, seg, uncovered, form="stride64", bits=64, shift=0, want=SCANS, **kw):
    """test_reduce's case of list length n with the named segmentation, batch form and field"""
    count = max(n - n // 8, 1) if n else 0   # (a list longer than its batch repeats packets)
    return Case(list_of(n, count), segmentation(seg, n, uncovered), verdicts(count, bits, shift),
                shift, bits, form=batch_form(form, count), want=want, **kw)


# ---------------------------------------------------------------- the host function

@pytest.mark.parametrize("n", COUNTS)
def test_scan_shapes(native, n):
    for k, seg in enumerate(SEGMENTATIONS):
        for uncovered in (False, True):
            c = shaped(n, seg, uncovered, FORMS[(k + uncovered) % 4])
            check_host(native, c, msg="%s n=%d uncovered=%s" % (seg, n, uncovered))


@pytest.mark.parametrize("bits", [1, 8, 32, 33, 64])
def test_scan_value_fields(native, bits):
    for shift in (0, 3, 31, 64 - bits):
        if shift + bits > 64:
            continue
        for k, seg in enumerate(("runs63", "random", "whole")):
            check_host(native, shaped(1000, seg, True, FORMS[k], bits, shift),
                       msg="bits %d shift %d %s" % (bits, shift, seg))


def test_scan_uncovered_positions_and_the_tail(native):
    """positions before seg_starts[0] and at or past seg_starts[R] hold 0; past n nothing is
    written; with no segment at all every position is uncovered"""
    n = 1000
    c = Case(list_of(n, 100), [5, 300, 300, 990], verdicts(100), form=(64, None, False),
             want=SCANS)
    outs = check_host(native, c)
    for k in SCANS:
        assert not outs[k][:5].any() and not outs[k][990:n].any()
        assert (outs[k][n:] == FILL[k]).all()
    assert outs["rank"][5:300].tolist() == list(range(295))
    assert outs["rank"][300:990].tolist() == list(range(690))
    for starts, nseg in (([0], None), ([7], None), ([0, 500, n], 0), ([3], 5)):
        c = Case(list_of(n, 100), starts, verdicts(100), form=(64, None, False), nseg=nseg,
                 want=SCANS)
        assert c.segments == 0
        outs = check_host(native, c)
        for k in SCANS:
            assert not outs[k][:n].any()
    # seg_cap 0 takes neither a table nor budgets' entries
    out = np.full(n, 0x5a, dtype=np.uint8)
    scans = native.BatchScans(None, None, None, out.ctypes.data)
    b = c.batch(None)
    assert native.lib().ebpf_batch_scan(ctypes.byref(b), None, 100, 0, 0, c.index.ctypes.data, n,
                                        None, 0, None, FAKE, ctypes.byref(scans)) == 0
    assert not out.any()


def test_scan_nseg(native):
    """G below, equal to and above the cap, and far above: then the last table entry is no
    segment's end, and what it covered is the uncovered tail"""
    n = 1000
    cap = len(segmentation("runs63", n)) - 1
    for nseg in (0, 1, cap - 1, cap, cap + 1, cap + 1000, 1 << 40):
        c = shaped(n, "runs63", False, nseg=nseg)
        assert c.segments == (nseg if nseg <= cap else cap - 1)
        outs = check_host(native, c, msg="nseg %d" % nseg)
        end = int(c.seg_starts[c.segments])
        assert not outs["rank"][end:n].any() and not outs["bytes_before"][end:n].any()
    c = Case(list_of(9, 9), [4], verdicts(9), form=(64, None, False), nseg=3, want=SCANS)
    assert c.segments == 0
    check_host(native, c)
    # a short table: what lies past its last start is garbage, and is not looked at
    c = shaped(n, "runs63", False, nseg=cap + 5)
    c.seg_starts[cap] = 1 << 60
    assert host(native, c, budgets_of(c))[0] == 0


def test_scan_sums_wrap(native):
    top = 1 << 63
    ret = np.array([top + 5, top + 1, 3, MAX64, 7, 2], dtype=U64)
    c = Case(np.arange(6), [0, 3, 6], ret, form=(64, None, False), want=SCANS)
    outs = check_host(native, c)
    assert outs["sum_before"][:6].tolist() == [0, top + 5, 6, 0, MAX64, 6]   # two of them wrap
    count = 3000
    ret = verdicts(count) | U64(top)
    c = Case(list_of(4000, count), segmentation("runs63", 4000), ret, form=(64, None, False),
             want=SCANS)
    check_host(native, c)


def test_scan_bytes_pass_32_bits(native):
    """extents of 2^32 - 1 bytes: no 32-bit counter holds a segment's running total"""
    for seg in ("whole", "runs63"):
        c = shaped(1000, seg, False, "extents")
        outs = check_host(native, c, msg=seg)
        assert outs["bytes_before"][:1000].max() > 1 << 32
    lens = np.full(5, (1 << 32) - 1, dtype=U64)
    ext = np.stack([np.arange(5, dtype=U64), np.arange(5, dtype=U64) + lens], axis=1).reshape(-1)
    c = Case([0, 1, 2, 3, 4, 9], [0, 6], None, count=5, form=(0, ext, True),
             want=("bytes_before", "over"))
    budget = np.array([3 * ((1 << 32) - 1)], dtype=U64)
    outs = check_host(native, c, budget)
    assert outs["bytes_before"][:6].tolist() == [k * ((1 << 32) - 1) for k in range(5)] + \
        [5 * ((1 << 32) - 1)]
    assert outs["over"][:6].tolist() == [0, 0, 0, 1, 1, 1]


def test_scan_budgets(native):
    """0, exactly a running total (strictly more is over), and UINT64_MAX"""
    c = Case(np.zeros(12, dtype=np.uint32), [0, 4, 8, 12], None, count=1, form=(60, None, False),
             want=("over", "bytes_before"))
    for budgets, want in (([0, 0, 0], [1] * 12),
                          ([120, 119, 121], [0, 0, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1]),
                          ([MAX64, 240, 239], [0] * 8 + [0, 0, 0, 1]),
                          ([59, 60, 61], [1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1])):
        outs = check_host(native, c, np.array(budgets, dtype=U64))
        assert outs["over"][:12].tolist() == want, budgets
    # an entry of length 0 is within a budget of 0 until a byte came before it
    c = Case([5, 5, 0, 5, 0], [0, 5], None, count=1, form=(60, None, False), want=("over",))
    outs = check_host(native, c, np.array([0], dtype=U64))
    assert outs["over"][:5].tolist() == [0, 0, 1, 1, 1]
    for seg in ("runs63", "random", "singletons", "steering"):
        check_host(native, shaped(1000, seg, True, "offsets"), msg=seg)


def test_scan_each_output_alone_and_none(native):
    for k in SCANS:
        check_host(native, shaped(1000, "random", True, "offsets", 33, 7, want=(k,)), msg=k)
    c = shaped(1000, "random", True, want=())
    assert host(native, c) == (0, {})
    # what an output does not need may be missing
    c = shaped(1000, "random", False, want=("rank",))
    c.ret, c.has_batch = None, False
    check_host(native, c)
    c = shaped(1000, "random", False, want=("rank", "bytes_before", "over"))
    c.ret = None
    check_host(native, c)
    c = shaped(1000, "random", False, want=("rank", "bytes_before"))
    code, outs = host(native, c, None)          # no budgets
    assert code == 0
    np.testing.assert_array_equal(outs["bytes_before"][:1000], reference(c)["bytes_before"])
    c = shaped(1000, "random", False, want=("rank", "sum_before"))
    c.has_batch = False
    check_host(native, c)


def test_scan_no_list_and_no_packets(native):
    for seg in ("whole", "empties", "steering"):
        check_host(native, shaped(0, seg, False), msg=seg)
    c = Case(list_of(50, 1), segmentation("runs63", 50), np.zeros(1, dtype=U64), count=0,
             form=(64, None, False), want=SCANS)   # a batch of no packets: ranks alone
    outs = check_host(native, c)
    assert outs["rank"][:50].tolist() == [j % 63 for j in range(50)]
    assert not outs["bytes_before"][:50].any() and not outs["over"][:50].any()


def test_scan_refuses_a_bad_table(native):
    n = 1000
    for bad in ([0, 500, 499, 1000], [0, 500, 1001], [1001, 1001], [5, 4]):
        c = Case(list_of(n, 100), bad, verdicts(100), form=(64, None, False), want=SCANS)
        code, outs = host(native, c, np.zeros(c.cap, dtype=U64))
        assert code == errno.EINVAL, bad
        for k in SCANS:
            assert (outs[k] == FILL[k]).all(), bad
    # below R only: entries past the segments scanned may be anything
    c = Case(list_of(n, 100), [0, 500, 400, 3], verdicts(100), form=(64, None, False), nseg=1,
             want=SCANS)
    check_host(native, c)


def test_scan_agrees_with_the_reduce(native):
    """a segment's last position: what came before it plus its own is the reduce's total"""
    for seg, form in (("runs63", "extents"), ("random", "offsets"), ("steering", "stride60"),
                      ("many_empty", "stride64")):
        c = shaped(3 * T + 17, seg, True, form, 33, 7)
        outs = check_host(native, c, msg=seg)
        lens, vals = fields(c)
        c.want = ("bytes", "sum")
        code, sums = c.host(native)
        assert code == 0
        np.testing.assert_array_equal(sums["bytes"][:c.segments], reduce_reference(c)["bytes"])
        S = c.seg_starts.astype(np.int64)
        full = np.flatnonzero(S[1:c.segments + 1] > S[:c.segments])
        last = S[full + 1] - 1
        assert len(full) >= 2
        np.testing.assert_array_equal(outs["bytes_before"][last] + lens[last], sums["bytes"][full])
        np.testing.assert_array_equal(outs["sum_before"][last] + vals[last], sums["sum"][full])
        np.testing.assert_array_equal(outs["rank"][last], (S[full + 1] - S[full] - 1))


# ---------------------------------------------------------------- argument checks

def _call(f, dev, batch, ret, count, shift, bits, index, n, starts, cap, nseg, budgets, scans):
    b = None if batch is None else ctypes.byref(batch)
    s = None if scans is None else ctypes.byref(scans)
    if dev is None:
        return f(b, ret, count, shift, bits, index, n, starts, cap, nseg, budgets, s)
    return f(dev, b, ret, count, shift, bits, index, n, starts, cap, nseg, budgets, s, None)


def _argument_checks(native, f, dev):
    """every EINVAL / E2BIG of the header, with pointers nothing may dereference"""
    S = native.BatchScans
    every = S(FAKE, FAKE, FAKE, FAKE)
    rank, lens, vals, over = (S(FAKE, None, None, None), S(None, FAKE, None, None),
                              S(None, None, FAKE, None), S(None, None, None, FAKE))
    b = native.PktBatch(FAKE, None, 5, 64, 0)
    call = functools.partial(_call, f, dev)
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, None) == errno.EINVAL
    for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32), (0xffffffff, 2)):
        for scans in (every, vals):
            assert call(b, FAKE, 5, shift, bits, FAKE, 5, FAKE, 1, None, FAKE, scans) == errno.EINVAL
    # a batch the run functions would refuse
    for bad in (native.PktBatch(None, None, 5, 64, 0), native.PktBatch(FAKE, None, 5, 0, 0),
                native.PktBatch(FAKE, None, 5, 64, 0x80),
                native.PktBatch(FAKE, None, 5, 64, native.BATCH_EXTENTS)):
        for scans in (every, rank, vals):
            assert call(bad, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, scans) == errno.EINVAL
    assert call(b, FAKE, 6, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, every) == errno.EINVAL
    assert call(b, FAKE, 4, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, rank) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, None, 5, FAKE, 1, None, FAKE, every) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, None, 1, None, FAKE, every) == errno.EINVAL
    assert call(b, None, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, every) == errno.EINVAL
    assert call(b, None, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, vals) == errno.EINVAL
    assert call(None, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, every) == errno.EINVAL
    assert call(None, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, lens) == errno.EINVAL
    assert call(None, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, over) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, None, every) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, None, over) == errno.EINVAL
    big = native.PktBatch(FAKE, None, 1 << 32, 64, 0)
    assert call(b, FAKE, 5, 0, 64, FAKE, 1 << 32, FAKE, 1, None, FAKE, every) == errno.E2BIG
    assert call(big, FAKE, 1 << 32, 0, 64, FAKE, 5, FAKE, 1, None, FAKE, every) == errno.E2BIG
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1 << 32, None, FAKE, every) == errno.E2BIG
    assert call(None, FAKE, 1 << 32, 0, 64, FAKE, 5, FAKE, 1, None, None, vals) == errno.E2BIG
    assert call(None, None, 5, 0, 0, FAKE, 1 << 32, FAKE, 1, None, None, rank) == errno.E2BIG


def test_scan_argument_checks(native):
    f = native.lib().ebpf_batch_scan
    _argument_checks(native, f, None)
    # the field is not looked at where ret is not used, nor the budgets where over is not wanted
    b = native.PktBatch(FAKE, None, 1, 64, 0)
    out = np.full(3, SENTINEL, dtype=U64)
    index, starts = np.zeros(2, dtype=np.uint32), np.array([0, 2], dtype=U64)
    scans = native.BatchScans(None, out.ctypes.data, None, None)
    assert _call(f, None, b, None, 1, 99, 0, index.ctypes.data, 2, starts.ctypes.data, 1, None,
                 None, scans) == 0
    assert out.tolist() == [0, 64, SENTINEL]


def test_scan_dev_argument_checks(native):
    """EINVAL and E2BIG before the device is looked at; then, on a machine without a GPU (or for
    a device out of range), ENODEV with nothing dereferenced"""
    f = native.lib().ebpf_batch_scan_dev
    for dev in (0, 1 << 20):
        _argument_checks(native, f, dev)
    every = native.BatchScans(FAKE, FAKE, FAKE, FAKE)
    nothing = native.BatchScans(None, None, None, None)
    b = native.PktBatch(FAKE, None, 5, 64, 0)
    devs = [1 << 20, -1] + ([0] if native.gpu_count() == 0 else [])
    for dev in devs:
        assert _call(f, dev, b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, FAKE, FAKE, every) == errno.ENODEV
        assert _call(f, dev, None, None, 5, 0, 0, FAKE, 5, FAKE, 1, None, None,
                     nothing) == errno.ENODEV
        assert _call(f, dev, b, FAKE, 5, 0, 64, None, 0, None, 0, None, FAKE, every) == errno.ENODEV


def test_scan_wrapper(native):
    """native.scan: the arrays it returns, and a decreasing table's EINVAL"""
    c = shaped(1000, "runs63", True, "offsets", 33, 7)
    budgets = budgets_of(c)
    w = reference(c, budgets)
    got = native.scan(c.index, c.seg_starts, c.ret, 7, 33, stride=c.stride, offsets=c.offsets,
                      extents=c.extents, budgets=budgets)
    assert got[4] == 0 and tuple(native.SCANS) == SCANS
    for k, a in zip(SCANS, got[:4]):
        assert a.dtype == TYPES[k]
        np.testing.assert_array_equal(a, w[k])
    got = native.scan(c.index, c.seg_starts, want=("rank",), nseg=3)
    assert got[1] is None and got[2] is None and got[3] is None and got[4] == 0
    end = int(c.seg_starts[3])
    np.testing.assert_array_equal(got[0][:end], w["rank"][:end])
    assert not got[0][end:].any()
    assert native.scan(c.index, [3, 2], c.ret, stride=64, budgets=[0])[4] == errno.EINVAL
