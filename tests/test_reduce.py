"""Reducing a list per segment on the host (include/ebpf_gpu.h: ebpf_batch_reduce) against a
numpy reference written here — a plain loop over the segments, exact unsigned 64-bit throughout —
and the argument checks of ebpf_batch_reduce / ebpf_batch_reduce_dev, which come before any device
work and so hold without a GPU.

Integer sums, minima, maxima and ORs have one right answer, so every comparison is exact.  The
shapes (list lengths, segmentations, batch forms, value fields) are shared with
test_gpu_reduce.py, which checks the device function against the host function on them."""
import ctypes
import errno
import functools

import numpy as np
import pytest

from generic_ebpf_amd import native as _native
from test_group import U64, garbage

T = _native.STEER_TILE
SUMS = _native.SUMS
GUARD = 8
SENTINEL = 0x5a5a5a5a5a5a5a5a   # fills every output on entry; no result of a test below has it
IDENTITY = {"bytes": 0, "sum": 0, "min": (1 << 64) - 1, "max": 0, "bits": 0}
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
MID = 3 * T + 17
BIG = (2 << 20) + 5
FAKE = 4096   # a non-NULL pointer that nothing may dereference


# ---------------------------------------------------------------- shapes

def runs(n, length):
    return np.append(np.arange(0, n, length), n).astype(U64)


def steering_table(n):
    """258 entries; classes 0, 1, 2, 7, 200, 255 and 256 share the list, the others are empty"""
    g = np.random.default_rng(n + 258)
    sizes = np.zeros(_native.EBPF_HIST_BINS, dtype=np.int64)
    cuts = np.sort(g.integers(0, n + 1, 6))
    sizes[[0, 1, 2, 7, 200, 255, 256]] = np.diff(np.concatenate([[0], cuts, [n]]))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(U64)


def many_empty(n):
    """5,000 empty segments at one position, a tile edge where the list has one: more than a
    tile's worth of segments begin where one tile ends"""
    at = T if n > T else n
    return np.concatenate([[0], np.full(5000, at), [n]]).astype(U64)


def empties_around(n):
    a, b = n // 3, n - n // 4
    return np.array([0, 0, 0, a, a, a, a, b, n, n, n], dtype=U64)


def random_lengths(n):
    g = np.random.default_rng(n)
    cuts = np.sort(g.integers(0, n + 1, max(n // 37, 3)))
    return np.concatenate([[0], cuts, [n]]).astype(U64)


SEGMENTATIONS = {
    "whole": lambda n: np.array([0, n], dtype=U64),
    "singletons": lambda n: np.arange(n + 1, dtype=U64),
    "runs63": lambda n: runs(n, 63), "runs64": lambda n: runs(n, 64),
    "runs4095": lambda n: runs(n, 4095), "runsT": lambda n: runs(n, T),
    "random": random_lengths, "empties": empties_around, "many_empty": many_empty,
    "steering": steering_table,
}


def segmentation(name, n, uncovered=False):
    """seg_starts over a list of n entries; uncovered: the first 5 and the last 7 positions (as
    far as the list has them) belong to no segment"""
    if not uncovered:
        return SEGMENTATIONS[name](n)
    a, b = min(5, n // 3), min(7, n // 3)
    return SEGMENTATIONS[name](n - a - b) + U64(a)


def batch_form(name, count):
    """(stride, offsets, extents) of a batch of `count` packets; no data: none is read"""
    g = np.random.default_rng(count + len(name))
    if name in ("stride64", "stride60"):
        return int(name[6:]), None, False
    if name == "offsets":
        lens = g.integers(0, 1501, count)
        return 0, np.concatenate([[0], np.cumsum(lens)]).astype(U64), False
    assert name == "extents"
    start = g.integers(0, 1 << 40, count, dtype=U64)
    lens = g.integers(0, 9001, count).astype(U64)
    k = np.arange(count)
    lens[k % 5 == 1] = U64((1 << 32) - 1)      # the longest packet: a few pass 2^32 together
    lens[k % 17 == 3] = U64(1 << 32)           # too long: length 0
    lens[k % 19 == 4] = U64((1 << 33) + 5)
    end = start + lens
    below = k % 13 == 2                        # an end below its start: length 0
    end[below] = start[below] - U64(1)
    end[below & (start == 0)] = 0
    return 0, np.stack([start, end], axis=1).reshape(-1).astype(U64), True


def lengths_of(count, stride, offsets, extents):
    """every packet's length by the run functions' rule"""
    if offsets is None:
        return np.full(count, stride, dtype=U64)
    s, e = (offsets[0::2], offsets[1::2]) if extents else (offsets[:-1], offsets[1:])
    s, e = s.astype(object), e.astype(object)
    return np.array([0 if b < a or b - a >= 1 << 32 else b - a for a, b in zip(s, e)],
                    dtype=U64).reshape(count)


def list_of(n, count, seed=0):
    """a list of n entries over a batch of `count` packets: any order, duplicates, and every
    23rd entry at or past the batch's end"""
    g = np.random.default_rng(n * 7 + seed)
    index = g.integers(0, max(count, 1), n).astype(np.uint32)
    past = np.arange(n) % 23 == 5
    index[past] = count + g.integers(0, 3, int(past.sum()))
    if n > 10:
        index[7] = index[3]
    return index


class Case:
    """one call's inputs, on the host"""

    def __init__(self, index, seg_starts, ret=None, shift=0, bits=64, count=None, form=None,
                 nseg=None, want=SUMS):
        self.index = np.ascontiguousarray(index, dtype=np.uint32)
        self.seg_starts = np.ascontiguousarray(seg_starts, dtype=U64)
        self.cap = len(self.seg_starts) - 1
        self.ret = None if ret is None else np.ascontiguousarray(ret, dtype=U64)
        self.count = len(self.ret) if count is None else count
        self.shift, self.bits, self.nseg, self.want = shift, bits, nseg, tuple(want)
        self.stride, self.offsets, self.extents = form if form else (0, None, False)
        self.has_batch = form is not None

    @property
    def n(self):
        return len(self.index)

    @property
    def segments(self):
        """R of the header"""
        if self.nseg is None:
            return self.cap
        return self.nseg if self.nseg <= self.cap else max(self.cap - 1, 0)

    def batch(self, offsets_ptr):
        return _native.PktBatch(1 if self.count else None, offsets_ptr, self.count, self.stride,
                                _native.BATCH_EXTENTS if self.extents else 0)

    def host(self, native, fill=SENTINEL):
        """the host function on outputs pre-filled with `fill`, GUARD entries longer than the call
        may write: (code, {name: u64[cap + GUARD]})"""
        outs = {k: np.full(self.cap + GUARD, fill, dtype=U64) for k in self.want}
        sums = native.BatchSums(*[outs[k].ctypes.data if k in outs else None for k in SUMS])
        b = self.batch(None if self.offsets is None else self.offsets.ctypes.data)
        ns = None if self.nseg is None else np.array([self.nseg], dtype=U64)
        code = native.lib().ebpf_batch_reduce(
            ctypes.byref(b) if self.has_batch else None,
            None if self.ret is None else self.ret.ctypes.data, self.count, self.shift, self.bits,
            self.index.ctypes.data if self.n else None, self.n, self.seg_starts.ctypes.data,
            self.cap, None if ns is None else ns.ctypes.data, ctypes.byref(sums))
        return code, outs


def reference(c):
    """{name: u64[R]}: a plain loop over the segments"""
    i = c.index.astype(np.int64)
    inside = i < c.count
    at = np.where(inside, i, 0)
    lens = np.zeros(c.n, dtype=U64)
    vals = np.zeros(c.n, dtype=U64)
    if c.has_batch and c.count:
        lens = np.where(inside, lengths_of(c.count, c.stride, c.offsets, c.extents)[at], U64(0))
    if c.ret is not None and c.count:
        vals = (c.ret[at] >> U64(c.shift)) & U64((1 << c.bits) - 1)
    out = {k: np.zeros(c.segments, dtype=U64) for k in SUMS}
    for g in range(c.segments):
        a, b = int(c.seg_starts[g]), int(c.seg_starts[g + 1])
        v = vals[a:b][inside[a:b]]
        out["bytes"][g] = np.add.reduce(lens[a:b], dtype=U64)
        out["sum"][g] = np.add.reduce(v, dtype=U64)           # (wraps modulo 2^64)
        out["min"][g] = v.min() if len(v) else IDENTITY["min"]
        out["max"][g] = v.max() if len(v) else 0
        out["bits"][g] = np.bitwise_or.reduce(v) if len(v) else 0
    return out


def check_host(native, c, msg=""):
    """the whole contract of the host function for case c"""
    code, outs = c.host(native)
    assert code == 0, msg
    w = reference(c)
    R = c.segments
    for k in c.want:
        np.testing.assert_array_equal(outs[k][:R], w[k], err_msg="%s %s" % (msg, k))
        assert (outs[k][R:] == SENTINEL).all(), "%s %s: written at or past R" % (msg, k)
    return outs


@functools.lru_cache(maxsize=None)
def verdicts(count, bits=64, shift=0):
    """ret of `count` packets: a random field of `bits` at `shift` under random bits around it"""
    g = np.random.default_rng(count * 64 + bits + shift)
    field = g.integers(0, 1 << bits, count, dtype=U64) if bits < 64 else \
        g.integers(0, 1 << 64, count, dtype=U64)
    return garbage(g, field, shift, bits)


def shaped(n, seg, uncovered, form="stride64", bits=64, shift=0, **kw):
    """the case of list length n with the named segmentation, batch form and value field"""
    count = max(n - n // 8, 1) if n else 0   # (a list longer than its batch repeats packets)
    return Case(list_of(n, count), segmentation(seg, n, uncovered), verdicts(count, bits, shift),
                shift, bits, form=batch_form(form, count), **kw)


# ---------------------------------------------------------------- the host function

@pytest.mark.parametrize("n", COUNTS)
def test_reduce_shapes(native, n):
    forms = ["stride64", "stride60", "offsets", "extents"]
    for k, seg in enumerate(SEGMENTATIONS):
        for uncovered in (False, True):
            c = shaped(n, seg, uncovered, forms[(k + uncovered) % 4])
            check_host(native, c, "%s n=%d uncovered=%s" % (seg, n, uncovered))


@pytest.mark.parametrize("bits", [1, 8, 32, 33, 64])
def test_reduce_value_fields(native, bits):
    for shift in (0, 3, 31, 64 - bits):
        if shift + bits > 64:
            continue
        for seg in ("runs63", "random", "whole"):
            check_host(native, shaped(1000, seg, True, "offsets", bits, shift),
                       "bits %d shift %d %s" % (bits, shift, seg))


def test_reduce_unsigned_and_wrapping(native):
    top = 1 << 63
    ret = np.array([top + 5, 3, top + 1, (1 << 64) - 1, 7, 2], dtype=U64)
    c = Case(np.arange(6), [0, 3, 6], ret, form=(64, None, False))
    outs = check_host(native, c)
    assert outs["min"][:2].tolist() == [3, 2]                  # (not the "negative" ones)
    assert outs["max"][:2].tolist() == [top + 5, (1 << 64) - 1]
    assert outs["sum"][:2].tolist() == [(2 * top + 9) % (1 << 64), 8]   # both wrap
    assert outs["bits"][0] == top | 7


def test_reduce_lengths(native):
    """every batch form; a segment of the extents form passes 2^32 bytes"""
    for form in ("stride64", "stride60", "offsets", "extents"):
        c = shaped(1000, "runs63", False, form)
        outs = check_host(native, c, form)
        if form == "extents":
            assert outs["bytes"][:c.segments].max() > 1 << 32
    # entries at or past the batch's end: length 0 and no value; duplicates count every time
    ret = np.array([10, 20, 30], dtype=U64)
    c = Case([0, 3, 1, 1, 7, 1 << 31, 2], [0, 2, 5, 6, 7], ret, form=(64, None, False))
    outs = check_host(native, c)
    assert outs["bytes"][:4].tolist() == [64, 128, 0, 64]
    assert outs["sum"][:4].tolist() == [10, 40, 0, 30]
    assert outs["min"][:4].tolist() == [10, 20, IDENTITY["min"], 30]
    assert outs["max"][:4].tolist() == [10, 20, 0, 30]


def test_reduce_empty_segments_give_identities(native):
    c = shaped(100, "many_empty", False)
    outs = check_host(native, c)
    for k in SUMS:
        assert (outs[k][1:5001] == IDENTITY[k]).all()


def test_reduce_each_output_alone_and_none(native):
    for k in SUMS:
        check_host(native, shaped(1000, "random", True, "offsets", 33, 7, want=(k,)), k)
    c = shaped(1000, "random", True, want=())
    assert c.host(native) == (0, {})
    # what an output does not need may be missing
    c = shaped(1000, "random", False, want=("bytes",))
    c.ret = None
    check_host(native, c)
    c = shaped(1000, "random", False, want=("sum", "min", "max", "bits"))
    c.has_batch = False
    check_host(native, c)


def test_reduce_no_list_and_no_segments(native):
    for seg in ("whole", "empties", "steering"):
        c = shaped(0, seg, False)
        outs = check_host(native, c)
        for k in SUMS:
            assert (outs[k][:c.cap] == IDENTITY[k]).all()
    c = Case(list_of(50, 10), [0], verdicts(10), form=(64, None, False))
    assert c.cap == 0
    check_host(native, c)
    # seg_cap 0 takes no table at all
    sums = native.BatchSums(FAKE, FAKE, FAKE, FAKE, FAKE)
    b = c.batch(None)
    assert native.lib().ebpf_batch_reduce(ctypes.byref(b), c.ret.ctypes.data, 10, 0, 64,
                                          c.index.ctypes.data, 50, None, 0, None,
                                          ctypes.byref(sums)) == 0


def test_reduce_nseg(native):
    """G below, equal to and above the cap: above, the last table entry is no segment's end"""
    n = 1000
    starts = runs(n, 63)
    cap = len(starts) - 1
    for nseg in (0, 1, cap - 1, cap, cap + 1, cap + 1000):
        c = shaped(n, "runs63", False, nseg=nseg)
        assert c.segments == (nseg if nseg <= cap else cap - 1)
        check_host(native, c, "nseg %d" % nseg)
    c = Case(list_of(9, 9), [4], verdicts(9), form=(64, None, False), nseg=3)   # cap 0, G 3
    assert c.segments == 0
    check_host(native, c)
    # a short table: what lies past its last start is garbage, and is not looked at
    c = shaped(n, "runs63", False, nseg=cap + 5)
    c.seg_starts[cap] = 1 << 60
    assert c.host(native)[0] == 0


def test_reduce_refuses_a_bad_table(native):
    n = 1000
    for bad in ([0, 500, 499, 1000], [0, 500, 1001], [1001, 1001], [5, 4]):
        c = Case(list_of(n, 100), bad, verdicts(100), form=(64, None, False))
        code, outs = c.host(native)
        assert code == errno.EINVAL, bad
        for k in SUMS:
            assert (outs[k] == SENTINEL).all(), bad
    # below R only: entries past the segments reduced may be anything
    c = Case(list_of(n, 100), [0, 500, 400, 3], verdicts(100), form=(64, None, False), nseg=1)
    check_host(native, c)


# ---------------------------------------------------------------- argument checks

def _call(f, dev, batch, ret, count, shift, bits, index, n, starts, cap, nseg, sums):
    b = None if batch is None else ctypes.byref(batch)
    s = None if sums is None else ctypes.byref(sums)
    if dev is None:
        return f(b, ret, count, shift, bits, index, n, starts, cap, nseg, s)
    return f(dev, b, ret, count, shift, bits, index, n, starts, cap, nseg, s, None)


def _argument_checks(native, f, dev):
    """every EINVAL / E2BIG of the header, with pointers nothing may dereference"""
    S = native.BatchSums
    every = S(FAKE, FAKE, FAKE, FAKE, FAKE)
    lens, vals = S(FAKE, None, None, None, None), S(None, FAKE, None, None, FAKE)
    b = native.PktBatch(FAKE, None, 5, 64, 0)
    call = functools.partial(_call, f, dev)
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, None) == errno.EINVAL
    for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32), (0xffffffff, 2)):
        for sums in (every, vals, S(None, None, FAKE, None, None), S(None, None, None, FAKE, None)):
            assert call(b, FAKE, 5, shift, bits, FAKE, 5, FAKE, 1, None, sums) == errno.EINVAL
    # a batch the run functions would refuse
    for bad in (native.PktBatch(None, None, 5, 64, 0), native.PktBatch(FAKE, None, 5, 0, 0),
                native.PktBatch(FAKE, None, 5, 64, 0x80),
                native.PktBatch(FAKE, None, 5, 64, native.BATCH_EXTENTS)):
        assert call(bad, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, every) == errno.EINVAL
        assert call(bad, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, vals) == errno.EINVAL
    assert call(b, FAKE, 6, 0, 64, FAKE, 5, FAKE, 1, None, every) == errno.EINVAL
    assert call(b, FAKE, 4, 0, 64, FAKE, 5, FAKE, 1, None, vals) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, None, 5, FAKE, 1, None, every) == errno.EINVAL
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, None, 1, None, every) == errno.EINVAL
    assert call(b, None, 5, 0, 64, FAKE, 5, FAKE, 1, None, every) == errno.EINVAL
    assert call(b, None, 5, 0, 64, FAKE, 5, FAKE, 1, None, vals) == errno.EINVAL
    assert call(None, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, every) == errno.EINVAL
    assert call(None, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, None, lens) == errno.EINVAL
    big = native.PktBatch(FAKE, None, 1 << 32, 64, 0)
    assert call(b, FAKE, 5, 0, 64, FAKE, 1 << 32, FAKE, 1, None, every) == errno.E2BIG
    assert call(big, FAKE, 1 << 32, 0, 64, FAKE, 5, FAKE, 1, None, every) == errno.E2BIG
    assert call(b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1 << 32, None, every) == errno.E2BIG
    assert call(None, FAKE, 1 << 32, 0, 64, FAKE, 5, FAKE, 1, None, vals) == errno.E2BIG


def test_reduce_argument_checks(native):
    f = native.lib().ebpf_batch_reduce
    _argument_checks(native, f, None)
    # the field is not looked at where ret is not used
    b = native.PktBatch(FAKE, None, 1, 64, 0)
    out = np.full(2, SENTINEL, dtype=U64)
    index, starts = np.zeros(1, dtype=np.uint32), np.array([0, 1], dtype=U64)
    sums = native.BatchSums(out.ctypes.data, None, None, None, None)
    assert _call(f, None, b, None, 1, 99, 0, index.ctypes.data, 1, starts.ctypes.data, 1, None,
                 sums) == 0
    assert out.tolist() == [64, SENTINEL]


def test_reduce_dev_argument_checks(native):
    """EINVAL and E2BIG before the device is looked at; then, on a machine without a GPU (or for
    a device out of range), ENODEV with nothing dereferenced"""
    f = native.lib().ebpf_batch_reduce_dev
    for dev in (0, 1 << 20):
        _argument_checks(native, f, dev)
    every = native.BatchSums(FAKE, FAKE, FAKE, FAKE, FAKE)
    nothing = native.BatchSums(None, None, None, None, None)
    b = native.PktBatch(FAKE, None, 5, 64, 0)
    devs = [1 << 20, -1] + ([0] if native.gpu_count() == 0 else [])
    for dev in devs:
        assert _call(f, dev, b, FAKE, 5, 0, 64, FAKE, 5, FAKE, 1, FAKE, every) == errno.ENODEV
        assert _call(f, dev, None, None, 5, 0, 0, FAKE, 5, FAKE, 1, None, nothing) == errno.ENODEV
        assert _call(f, dev, b, FAKE, 5, 0, 64, None, 0, None, 0, None, every) == errno.ENODEV


def test_reduce_wrapper(native):
    """native.reduce: the arrays it returns, and a decreasing table's EINVAL"""
    c = shaped(1000, "runs63", True, "offsets", 33, 7)
    w = reference(c)
    got = native.reduce(c.index, c.seg_starts, c.ret, 7, 33, stride=c.stride, offsets=c.offsets,
                        extents=c.extents)
    assert got[5] == 0
    for k, a in zip(SUMS, got[:5]):
        np.testing.assert_array_equal(a, w[k])
    got = native.reduce(c.index, c.seg_starts, c.ret, 7, 33, want=("max",), nseg=3)
    assert got[0] is None and got[1] is None and got[5] == 0
    np.testing.assert_array_equal(got[3][:3], w["max"][:3])
    assert not got[3][3:].any()
    assert native.reduce(c.index, [3, 2], c.ret, stride=64)[5] == errno.EINVAL
