"""Keeping part of a list on the host (include/ebpf_gpu.h: ebpf_batch_filter) against a numpy
reference written here — kept = index[part & pass] in list order, kept_starts = the cumsum of
part & pass sampled at min(seg_starts, n) — and the argument checks of ebpf_batch_filter /
ebpf_batch_filter_dev, which come before any device work and so hold without a GPU.

A stable compaction has one right answer, so every comparison is exact.  The shapes (list lengths,
segmentations, lists whose every 23rd entry lies past the batch) are test_reduce.py's;
test_gpu_filter.py checks the device function against the host function on them.  Every output
buffer is pre-filled with a value no result holds and is GUARD entries longer than the call may
write, and is compared whole: the EBPF_NO_PACKET tails, the table entries past R and the guard
are checked with the rest."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from test_reduce import (COUNTS, GUARD, MID, SEGMENTATIONS, SENTINEL, T, U64, list_of,
                         segmentation, verdicts)
from test_scan import budgets_of, fields
from test_scan import shaped as scan_shaped

PARTS = ("kept", "kept_starts", "dropped", "dropped_starts")
TYPES = {"kept": np.uint32, "kept_starts": U64, "dropped": np.uint32, "dropped_starts": U64,
         "info": U64}
# what every output holds on entry; no result is it (an index is below 2^32 - 1 or is that; a
# table entry or a count is at most n)
FILL = {"kept": 0x5a5a5a5a, "kept_starts": SENTINEL, "dropped": 0x5a5a5a5a,
        "dropped_starts": SENTINEL, "info": SENTINEL}
NO_PACKET = 0xffffffff
MAX64 = (1 << 64) - 1
FAKE = 4096   # a non-NULL pointer that nothing may dereference


class Case:
    """one call's inputs, on the host.  seg_starts None: an unsegmented list"""

    def __init__(self, index, seg_starts, count, flags=None, rank=None, rank_below=0, ret=None,
                 shift=0, bits=64, lo=0, hi=MAX64, nseg=None, want=PARTS):
        self.index = np.ascontiguousarray(index, dtype=np.uint32)
        self.seg_starts = None if seg_starts is None else np.ascontiguousarray(seg_starts, dtype=U64)
        self.cap = 0 if seg_starts is None else len(self.seg_starts) - 1
        self.count, self.nseg = count, nseg
        self.flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        self.rank = None if rank is None else np.ascontiguousarray(rank, dtype=np.uint32)
        self.rank_below = rank_below
        self.ret = None if ret is None else np.ascontiguousarray(ret, dtype=U64)
        self.shift, self.bits, self.lo, self.hi = shift, bits, lo, hi
        self.want = tuple(k for k in want if self.seg_starts is not None or k in ("kept", "dropped"))

    @property
    def n(self):
        return len(self.index)

    @property
    def segments(self):
        """R of the header"""
        if self.nseg is None:
            return self.cap
        return self.nseg if self.nseg <= self.cap else max(self.cap - 1, 0)

    def size(self, k):
        """the entries of output k that the call may write"""
        return {"info": 2, "kept": self.n, "dropped": self.n}.get(k, self.cap + 1)

    def test(self, native, flags_ptr, rank_ptr, ret_ptr):
        return native.BatchTest(flags_ptr, rank_ptr, self.rank_below, ret_ptr, self.shift,
                                self.bits, self.lo, self.hi)


def decisions(c):
    """(part bool[n], ok bool[n]): whether a position takes part, and whether it passes the tests"""
    n, pos = c.n, np.arange(c.n)
    if c.seg_starts is None:
        part = np.ones(n, dtype=bool)
    elif c.segments == 0:
        part = np.zeros(n, dtype=bool)
    else:
        part = (pos >= int(c.seg_starts[0])) & (pos < min(int(c.seg_starts[c.segments]), n))
    ok = np.ones(n, dtype=bool)
    if c.flags is not None:
        ok &= c.flags == 0
    if c.rank is not None:
        ok &= c.rank < c.rank_below
    if c.ret is not None:
        i = c.index.astype(np.int64)
        inside = i < c.count
        if c.count:
            v = (c.ret[np.where(inside, i, 0)] >> U64(c.shift)) & U64((1 << c.bits) - 1)
            ok &= inside & (v >= U64(c.lo)) & (v <= U64(c.hi))
        else:
            ok &= False
    return part, ok


def reference(c, fill=FILL):
    """{name: the whole buffer, guard and all} for the outputs c wants, and info"""
    part, ok = decisions(c)
    out = {k: np.full(c.size(k) + GUARD, fill[k], dtype=TYPES[k]) for k in c.want + ("info",)}
    for name, sel in (("kept", part & ok), ("dropped", part & ~ok)):
        m = int(sel.sum())
        out["info"][0 if name == "kept" else 1] = m
        if name in out:
            out[name][:m] = c.index[sel]
            out[name][m:c.n] = NO_PACKET
        if name + "_starts" in out:
            before = np.concatenate([[0], np.cumsum(sel)]).astype(U64)   # (sel is False off the cover)
            R = c.segments
            at = np.minimum(c.seg_starts[:R + 1].astype(np.int64), c.n) if R else np.zeros(1, int)
            out[name + "_starts"][:R + 1] = before[at]
    return out


def host(native, c, fill=FILL):
    """the host function on outputs pre-filled with `fill`, GUARD entries longer than the call
    may write: (code, {name: buffer})"""
    outs = {k: np.full(c.size(k) + GUARD, fill[k], dtype=TYPES[k]) for k in c.want + ("info",)}
    parts = native.BatchParts(*[outs[k].ctypes.data if k in outs else None for k in PARTS])
    test = c.test(native, *[None if a is None else a.ctypes.data or FAKE
                            for a in (c.flags, c.rank, c.ret)])
    ns = None if c.nseg is None else np.array([c.nseg], dtype=U64)
    code = native.lib().ebpf_batch_filter(
        ctypes.byref(test), c.count, c.index.ctypes.data if c.n else None, c.n,
        None if c.seg_starts is None else c.seg_starts.ctypes.data, c.cap,
        None if ns is None else ns.ctypes.data, ctypes.byref(parts), outs["info"].ctypes.data)
    return code, outs


def check_host(native, c, msg=""):
    """the whole contract of the host function for case c"""
    code, outs = host(native, c)
    assert code == 0, msg
    w = reference(c)
    for k in w:
        np.testing.assert_array_equal(outs[k], w[k], err_msg="%s %s" % (msg, k))
    return outs


# ---------------------------------------------------------------- test vectors

def _bytes(set_):
    """a flag byte per position: 0 where `set_` is False, else some non-zero byte"""
    some = np.array([1, 0x80, 0xff, 2], dtype=np.uint8)[np.arange(len(set_)) % 4]
    return np.where(set_, some, 0).astype(np.uint8)


def _field(count, bits, hi, lo=0):
    return dict(ret=verdicts(count, bits, 64 - bits if bits > 8 else 3), bits=bits,
                shift=64 - bits if bits > 8 else 3, lo=lo, hi=hi)


def vector(kind, n, count):
    """the members of a Case that make up test vector `kind` over a list of n entries"""
    g = np.random.default_rng(n * 31 + len(kind))
    pos = np.arange(n)
    u = g.random(n)
    small_rank = g.integers(0, 4, n).astype(np.uint32)
    flags = {"flags_all": np.zeros(n, bool), "flags_none": np.ones(n, bool),
             "flags_alternate": pos % 2 == 1, "flags_tile_last": pos % T != T - 1,
             "flags_first": pos != 0, "flags_wave": pos % 1024 != 517,
             "flags_half": u < 0.5, "flags_1pct": u >= 0.01}
    if kind == "none":
        return {}
    if kind in flags:
        return dict(flags=_bytes(flags[kind]))
    if kind in ("rank0", "rank1", "rank3"):
        big = pos % 7 == 3      # (an unsigned comparison: a rank with the top bit set is large)
        return dict(rank=np.where(big, 0x80000000 + pos, small_rank), rank_below=int(kind[4:]))
    if kind in ("val1", "val8", "val33", "val64"):
        bits = int(kind[3:])
        return _field(count, bits, (1 << (bits - 1)) - 1)
    if kind == "val64_top":   # (unsigned: the upper half of the 64-bit values)
        return _field(count, 64, MAX64, 1 << 63)
    if kind == "val_1pct":
        return _field(count, 33, (1 << 33) // 100)
    if kind == "val_equal":
        return _field(count, 8, 7, 7)
    if kind == "val_nothing":
        return _field(count, 8, 4, 5)
    if kind == "all_half":
        return dict(flags=_bytes(u < 0.2), rank=small_rank, rank_below=3, **_field(count, 8, 212))
    assert kind == "all_1pct"
    return dict(flags=_bytes(u < 0.8), rank=small_rank, rank_below=1, **_field(count, 8, 50))


KINDS = ["none", "flags_all", "flags_none", "flags_alternate", "flags_tile_last", "flags_first",
         "flags_wave", "flags_half", "flags_1pct", "rank0", "rank1", "rank3", "val1", "val8",
         "val33", "val64", "val64_top", "val_1pct", "val_equal", "val_nothing", "all_half",
         "all_1pct"]
WANTS = [PARTS, ("kept", "kept_starts"), ("dropped", "dropped_starts"), ("kept",),
         ("kept_starts", "dropped_starts"), ("kept", "dropped"), ("dropped_starts",)]


def shaped(n, seg, uncovered, kind, want=PARTS, nseg=None, seed=0):
    """the case of list length n with the named segmentation (None: unsegmented) and test vector"""
    count = max(n - n // 8, 1) if n else 0   # (a list longer than its batch repeats packets)
    starts = None if seg is None else segmentation(seg, n, uncovered)
    return Case(list_of(n, count, seed), starts, count, nseg=nseg, want=want,
                **vector(kind, n, count))


# ---------------------------------------------------------------- the host function

@pytest.mark.parametrize("n", COUNTS)
def test_filter_shapes(native, n):
    k = 0
    for seg in SEGMENTATIONS:
        for uncovered in (False, True):
            for kind in (KINDS[k % len(KINDS)], KINDS[(k + 7) % len(KINDS)]):
                c = shaped(n, seg, uncovered, kind, WANTS[k % len(WANTS)])
                check_host(native, c, "%s n=%d uncovered=%s %s" % (seg, n, uncovered, kind))
            k += 1


@pytest.mark.parametrize("kind", KINDS)
def test_filter_vectors(native, kind):
    """every test vector over three tiles and a bit, and what it keeps"""
    n = MID
    for seg in ("random", "runs63", None):
        c = shaped(n, seg, True, kind)
        outs = check_host(native, c, "%s %s" % (kind, seg))
        K, D = (int(v) for v in outs["info"][:2])
        assert K + D == (n if seg is None else n - 12)
        if seg is not None:
            continue
        want = {"none": n, "flags_all": n, "flags_none": 0, "flags_alternate": (n + 1) // 2,
                "flags_tile_last": n // T, "flags_first": 1, "flags_wave": (n + 506) // 1024,
                "rank0": 0, "val_nothing": 0}
        if kind in want:
            assert K == want[kind]
        elif kind.endswith("1pct"):
            assert 0 < K < n // 40
        elif kind.endswith("half") or kind in ("val1", "val8", "val33", "val64", "val64_top"):
            assert n // 3 < K < 2 * n // 3
        else:
            assert 0 < K < n


def test_filter_unsegmented(native):
    for n in COUNTS:
        for kind in ("none", "flags_half", "rank1", "val8", "all_half"):
            c = shaped(n, None, False, kind)
            assert c.want == ("kept", "dropped")
            outs = check_host(native, c, "n=%d %s" % (n, kind))
            assert int(outs["info"][0] + outs["info"][1]) == n


def test_filter_entries_past_the_batch_have_no_value(native):
    """they fail the value test whatever the bounds, and pass where ret is not given"""
    n, count = 1000, 100
    index = list_of(n, count)
    past = index >= count
    assert 20 < past.sum() < 100
    ret = np.zeros(count, dtype=U64)
    c = Case(index, [0, n], count, ret=ret, bits=64, lo=0, hi=MAX64)
    outs = check_host(native, c)
    assert int(outs["info"][1]) == past.sum()
    np.testing.assert_array_equal(outs["dropped"][:past.sum()], index[past])
    c = Case(index, [0, n], count, flags=np.zeros(n, np.uint8))
    assert int(check_host(native, c)["info"][0]) == n
    # a batch of no packets: no entry has a value
    c = Case(index, [0, n], 0, ret=np.zeros(1, dtype=U64))
    assert check_host(native, c)["info"][:2].tolist() == [0, n]


def test_filter_no_segments(native):
    """a table with seg_cap == 0, or with no segment by nseg: nothing takes part, the lists are
    all EBPF_NO_PACKET and entry 0 of the tables is 0"""
    n = 1000
    for starts, nseg in (([0], None), ([7], None), ([0, 500, n], 0), ([3], 5)):
        c = Case(list_of(n, 100), starts, 100, nseg=nseg, flags=np.zeros(n, np.uint8))
        assert c.segments == 0
        outs = check_host(native, c)
        assert outs["info"][:2].tolist() == [0, 0]
        assert (outs["kept"][:n] == NO_PACKET).all() and (outs["dropped"][:n] == NO_PACKET).all()
        assert outs["kept_starts"][0] == 0 and outs["dropped_starts"][0] == 0
        assert outs["kept_starts"][1] == SENTINEL
    # an empty cover: every entry of the tables is 0
    c = Case(list_of(n, 100), [5, 5, 5], 100)
    outs = check_host(native, c)
    assert outs["kept_starts"][:3].tolist() == [0, 0, 0] and outs["info"][:2].tolist() == [0, 0]


def test_filter_nseg(native):
    """G below, equal to and above the cap: above, the short table is one entry shorter and the
    last group's positions take no part"""
    n = 1000
    cap = len(segmentation("runs63", n)) - 1
    for nseg in (0, 1, cap - 1, cap, cap + 1, cap + 1000, 1 << 40):
        c = shaped(n, "runs63", False, "flags_half", nseg=nseg)
        R = c.segments
        assert R == (nseg if nseg <= cap else cap - 1)
        outs = check_host(native, c, "nseg %d" % nseg)
        end = int(c.seg_starts[R]) if R else 0
        assert int(outs["info"][0] + outs["info"][1]) == end
        assert outs["kept_starts"][R] == outs["info"][0]
        assert outs["dropped_starts"][R] == outs["info"][1]
        assert (outs["kept_starts"][R + 1:] == SENTINEL).all()
    # a short table: what lies past its last start is garbage, and is not looked at
    c = shaped(n, "runs63", False, "rank1", nseg=cap + 5)
    c.seg_starts[cap] = 1 << 60
    assert host(native, c)[0] == 0


def test_filter_only_info(native):
    """all four outputs NULL: a count"""
    for seg in ("random", None):
        c = shaped(MID, seg, True, "all_half", want=())
        outs = check_host(native, c)
        assert set(outs) == {"info"} and 0 < outs["info"][0] < MID


def test_filter_no_list(native):
    for seg in ("whole", "empties", "steering", None):
        outs = check_host(native, shaped(0, seg, False, "none"), str(seg))
        assert outs["info"][:2].tolist() == [0, 0]
        if seg is not None:
            assert not outs["kept_starts"][:len(SEGMENTATIONS[seg](0))].any()


def test_filter_refuses_a_bad_table(native):
    n = 1000
    for bad in ([0, 500, 499, 1000], [0, 500, 1001], [1001, 1001], [5, 4]):
        c = Case(list_of(n, 100), bad, 100, flags=np.zeros(n, np.uint8))
        code, outs = host(native, c)
        assert code == errno.EINVAL, bad
        for k in outs:
            assert (outs[k] == FILL[k]).all(), bad
    # below R only: entries past the segments may be anything
    c = Case(list_of(n, 100), [0, 500, 400, 3], 100, nseg=1)
    check_host(native, c)


# ---------------------------------------------------------------- chains on the host

def test_filter_after_scan_then_reduce(native):
    """scan (over) -> filter -> reduce over (kept, kept_starts): per segment the bytes of the
    entries within the budget; over (dropped, dropped_starts) those of the others"""
    for seg, form in (("runs63", "offsets"), ("random", "extents"), ("steering", "stride60"),
                      ("many_empty", "stride64")):
        s = scan_shaped(3 * T + 17, seg, True, form)
        budgets = budgets_of(s)
        over = native.scan(s.index, s.seg_starts, count=s.count, stride=s.stride,
                           offsets=s.offsets, extents=s.extents, budgets=budgets,
                           want=("over",))[3]
        assert over.any() and not over.all()
        kept, ks, dropped, ds, info, code = native.filter(s.index, s.seg_starts, flags=over,
                                                          count=s.count)
        assert code == 0 and int(info[0]) == int((over == 0).sum()) - 12   # (12 uncovered)
        lens = fields(s)[0]
        S = s.seg_starts.astype(np.int64)
        inside = np.zeros(s.n, bool)
        inside[S[0]:S[-1]] = True
        for lst, starts, sel in ((kept, ks, inside & (over == 0)), (dropped, ds, inside & (over != 0))):
            got = native.reduce(lst, starts, count=s.count, stride=s.stride, offsets=s.offsets,
                                extents=s.extents, want=("bytes",))
            assert got[5] == 0
            cum = np.concatenate([[0], np.cumsum(np.where(sel, lens, U64(0)), dtype=U64)])
            np.testing.assert_array_equal(got[0], cum[S[1:]] - cum[S[:-1]], err_msg=seg)


def test_filter_by_rank_samples_every_segment(native):
    """rank < K keeps the first K entries of every segment, or all it has"""
    for seg in ("runs63", "random", "singletons", "empties"):
        s = scan_shaped(3 * T + 17, seg, True)
        rank = native.scan(s.index, s.seg_starts, want=("rank",))[0]
        for K in (0, 1, 5):
            kept, ks, _, _, info, code = native.filter(s.index, s.seg_starts, rank=rank,
                                                       rank_below=K, count=s.count)
            assert code == 0
            sizes = np.diff(s.seg_starts.astype(np.int64))
            np.testing.assert_array_equal(np.diff(ks.astype(np.int64)), np.minimum(sizes, K))
            a = s.seg_starts.astype(np.int64)[:-1][sizes > 0]
            if K:
                np.testing.assert_array_equal(kept[ks.astype(np.int64)[:-1][sizes > 0]],
                                              s.index[a])
            assert (kept[int(info[0]):] == NO_PACKET).all()


# ---------------------------------------------------------------- argument checks

def _call(f, dev, test, count, index, n, starts, cap, nseg, parts, info):
    t = None if test is None else ctypes.byref(test)
    p = None if parts is None else ctypes.byref(parts)
    if dev is None:
        return f(t, count, index, n, starts, cap, nseg, p, info)
    return f(dev, t, count, index, n, starts, cap, nseg, p, info, None)


def _argument_checks(native, f, dev):
    """every EINVAL / E2BIG of the header, with pointers nothing may dereference"""
    P, Tt = native.BatchParts, native.BatchTest
    every = P(FAKE, FAKE, FAKE, FAKE)
    lists = P(FAKE, None, FAKE, None)
    plain = Tt(FAKE, FAKE, 1, None, 0, 0, 0, 0)
    call = functools.partial(_call, f, dev)
    assert call(None, 5, FAKE, 5, FAKE, 1, None, every, FAKE) == errno.EINVAL
    assert call(plain, 5, FAKE, 5, FAKE, 1, None, None, FAKE) == errno.EINVAL
    assert call(plain, 5, FAKE, 5, FAKE, 1, None, every, None) == errno.EINVAL
    for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32), (0xffffffff, 2)):
        t = Tt(None, None, 0, FAKE, shift, bits, 0, MAX64)
        assert call(t, 5, FAKE, 5, FAKE, 1, None, every, FAKE) == errno.EINVAL
        assert call(t, 5, FAKE, 5, None, 0, None, lists, FAKE) == errno.EINVAL
    assert call(plain, 5, None, 5, FAKE, 1, None, every, FAKE) == errno.EINVAL
    assert call(plain, 5, None, 1 << 32, FAKE, 1, None, every, FAKE) == errno.EINVAL
    assert call(plain, 5, FAKE, 5, None, 1, None, lists, FAKE) == errno.EINVAL
    assert call(plain, 5, FAKE, 5, None, 0, FAKE, lists, FAKE) == errno.EINVAL
    for parts in (every, P(None, FAKE, None, None), P(FAKE, None, FAKE, FAKE)):
        assert call(plain, 5, FAKE, 5, None, 0, None, parts, FAKE) == errno.EINVAL
    assert call(plain, 5, FAKE, 1 << 32, FAKE, 1, None, every, FAKE) == errno.E2BIG
    assert call(plain, 1 << 32, FAKE, 5, FAKE, 1, None, every, FAKE) == errno.E2BIG
    assert call(plain, 5, FAKE, 5, FAKE, 1 << 32, None, every, FAKE) == errno.E2BIG
    assert call(plain, 5, FAKE, 1 << 32, None, 0, None, lists, FAKE) == errno.E2BIG


def test_filter_argument_checks(native):
    f = native.lib().ebpf_batch_filter
    _argument_checks(native, f, None)
    # the field is not looked at where ret is not given; val_lo > val_hi is legal
    index = np.array([0, 1, 0], dtype=np.uint32)
    kept = np.full(4, FILL["kept"], dtype=np.uint32)
    info = np.zeros(2, dtype=U64)
    parts = native.BatchParts(kept.ctypes.data, None, None, None)
    t = native.BatchTest(None, None, 0, None, 99, 0, 9, 1)
    assert _call(f, None, t, 2, index.ctypes.data, 3, None, 0, None, parts, info.ctypes.data) == 0
    assert kept.tolist() == [0, 1, 0, FILL["kept"]] and info.tolist() == [3, 0]
    ret = np.array([5, 6], dtype=U64)
    t = native.BatchTest(None, None, 0, ret.ctypes.data, 0, 64, 9, 1)
    assert _call(f, None, t, 2, index.ctypes.data, 3, None, 0, None, parts, info.ctypes.data) == 0
    assert kept.tolist() == [NO_PACKET] * 3 + [FILL["kept"]] and info.tolist() == [0, 3]


def test_filter_dev_argument_checks(native):
    """EINVAL and E2BIG before the device is looked at; then, on a machine without a GPU (or for
    a device out of range), ENODEV with nothing dereferenced"""
    f = native.lib().ebpf_batch_filter_dev
    for dev in (0, 1 << 20):
        _argument_checks(native, f, dev)
    every = native.BatchParts(FAKE, FAKE, FAKE, FAKE)
    nothing = native.BatchParts(None, None, None, None)
    t = native.BatchTest(FAKE, FAKE, 1, FAKE, 0, 64, 0, MAX64)
    none = native.BatchTest(None, None, 0, None, 0, 0, 0, 0)
    devs = [1 << 20, -1] + ([0] if native.gpu_count() == 0 else [])
    for dev in devs:
        assert _call(f, dev, t, 5, FAKE, 5, FAKE, 1, FAKE, every, FAKE) == errno.ENODEV
        assert _call(f, dev, none, 5, FAKE, 5, None, 0, None, nothing, FAKE) == errno.ENODEV
        assert _call(f, dev, t, 5, None, 0, FAKE, 0, None, every, FAKE) == errno.ENODEV


def test_filter_wrapper(native):
    """native.filter: the arrays it returns, and a decreasing table's EINVAL"""
    c = shaped(1000, "runs63", True, "all_half")
    w = reference(c)
    got = native.filter(c.index, c.seg_starts, flags=c.flags, rank=c.rank, rank_below=c.rank_below,
                        ret=c.ret, val_shift=c.shift, val_bits=c.bits, val_lo=c.lo, val_hi=c.hi)
    assert got[5] == 0 and tuple(native.PARTS) == PARTS and native.EBPF_NO_PACKET == NO_PACKET
    for k, a in zip(PARTS, got[:4]):
        assert a.dtype == TYPES[k]
        np.testing.assert_array_equal(a, w[k][:c.size(k)])
    np.testing.assert_array_equal(got[4], w["info"][:2])
    got = native.filter(c.index, flags=c.flags, want=("kept", "kept_starts"))
    assert got[1] is None and got[2] is None and got[3] is None and got[5] == 0
    np.testing.assert_array_equal(got[0][:int(got[4][0])], c.index[c.flags == 0])
    assert native.filter(c.index, [3, 2], flags=c.flags)[5] == errno.EINVAL
