"""The heaviest entries on the host (include/ebpf_gpu.h: ebpf_batch_top, csrc/host/top.cpp) against
a Python sorted(range(N), key=...) statement of the rule.  The order is total, so every input has
one right answer: every comparison is exact.  Every output buffer is pre-filled with a value no
result holds and is GUARD entries longer than the call may write, so comparing the buffers whole
checks what must not be written too.  test_gpu_top.py runs the device function against this host
function on the same buffers."""
import ctypes
import errno

import numpy as np
import pytest

U64 = np.uint64
MAXU = (1 << 64) - 1
GUARD = 8
FILL = {"keys": 0x5a5a5a5a5a5a5a5a, "vals": 0xa5a5a5a5a5a5a5a5, "pos": 0xa5a5a5a5,
        "info": 0x2222222222222222}
TYPES = {"keys": U64, "vals": U64, "pos": np.uint32, "info": U64}
LARGEST, SMALLEST, SEGMENTS = 0, 1, 2
FIELDS = [(0, 64), (0, 40), (0, 8), (0, 9), (0, 1), (24, 16), (63, 1)]
ALL = ("keys", "vals", "pos")


def u64(a):
    if isinstance(a, np.ndarray) and a.dtype.kind in "ui":
        return np.ascontiguousarray(a.astype(U64))
    return np.array([int(x) for x in a], dtype=U64)


def entries(cap, n, flags):
    """N: the entries that take part"""
    if n is None:
        return cap
    if flags & SEGMENTS:
        return n if n <= cap else max(cap - 1, 0)
    return min(n, cap)


class Top:
    """one top call; keys None: keys is NULL (and out->keys with it)"""

    def __init__(self, vals, k, flags=LARGEST, field=(0, 64), n=None, keys="ramp", want=ALL):
        self.vals = u64(vals)
        self.cap = len(self.vals)
        # a key per position that no value or position is
        self.keys = (np.arange(self.cap, dtype=U64) * U64(3) + U64(1 << 50)) if isinstance(keys, str) \
            else (None if keys is None else u64(keys))
        self.k, self.flags, self.field, self.n = k, flags, field, n
        self.want = tuple(w for w in want if w != "keys" or self.keys is not None)
        self.N = entries(self.cap, n, flags)
        self.m = min(k, self.N)

    def f(self, p):
        shift, bits = self.field
        return (int(self.vals[p]) >> shift) & ((1 << bits) - 1)

    def order(self):
        sign = 1 if self.flags & SMALLEST else -1
        return sorted(range(self.N), key=lambda p: (sign * self.f(p), p))

    def expect(self, fill=FILL):
        p = self.order()
        m = self.m
        out = {w: np.full(self.k + GUARD, fill[w], dtype=TYPES[w]) for w in self.want}
        if "keys" in out:
            out["keys"][:m] = self.keys[p[:m]]
        if "vals" in out:
            out["vals"][:m] = self.vals[p[:m]]
        if "pos" in out:
            out["pos"][:m] = p[:m]
        out["info"] = np.full(4 + GUARD, fill["info"], dtype=U64)
        cut = self.f(p[m - 1]) if m else 0
        out["info"][:4] = [m, self.N, cut, sum(1 for q in p[m:] if self.f(q) == cut) if m else 0]
        return out


def host_top(native, c, fill=FILL):
    """(code, {name: buffer}) of the host function on pre-filled, guard-extended buffers"""
    out = {w: np.full(c.k + GUARD, fill[w], dtype=TYPES[w]) for w in c.want}
    out["info"] = np.full(4 + GUARD, fill["info"], dtype=U64)
    tops = native.BatchTops(*[out[w].ctypes.data if w in c.want else None for w in ALL])
    n = None if c.n is None else np.array([c.n], dtype=U64)
    code = native.lib().ebpf_batch_top(
        None if c.keys is None else c.keys.ctypes.data or 16,   # (NULL only where keys is)
        c.vals.ctypes.data if c.cap else None, c.cap, None if n is None else n.ctypes.data,
        c.flags, c.field[0], c.field[1], c.k, ctypes.byref(tops), out["info"].ctypes.data)
    return code, out


def check_top(native, c, msg=""):
    code, got = host_top(native, c)
    assert code == 0, msg
    want = c.expect()
    for w in want:
        np.testing.assert_array_equal(got[w], want[w], err_msg="%s: %s" % (msg, w))
    return got


PATTERNS = ["random40", "random64", "equal", "ascending", "descending", "outside"]


def values(name, n, field=(0, 64), seed=0):
    """n values in one of the patterns"""
    g = np.random.default_rng(seed + 13 * n + 1)
    shift, bits = field
    if name == "random40":
        return g.integers(0, 1 << 40, n, dtype=U64)
    if name == "random64":     # with the ends of the range, and neighbours in either word
        v = g.integers(0, 1 << 63, n, dtype=U64) * U64(2) + g.integers(0, 2, n, dtype=U64)
        edge = u64([MAXU, MAXU - 1, 0, 1, 1 << 63, (1 << 63) - 1, 1 << 32, (1 << 32) - 1,
                    (2 << 32) + 1, (3 << 32) + 1, (2 << 32) + 2])
        at = g.permutation(n)[:len(edge)]
        v[at] = edge[:len(at)]
        return v
    if name == "equal":
        return np.full(n, 0x0123456789abcdef, dtype=U64)
    if name == "ascending":    # every field value several times over, in runs
        return (np.arange(n, dtype=U64) // U64(3)) << U64(shift)
    if name == "descending":
        return ((U64(n) - np.arange(n, dtype=U64)) // U64(3)) << U64(shift)
    if name == "outside":      # few distinct fields, every bit outside the field random
        mask = U64(((1 << bits) - 1) << shift)
        f = (g.integers(0, 3, n, dtype=U64) * U64(0x5555555555555555)) & mask
        noise = g.integers(0, 1 << 63, n, dtype=U64) * U64(2) + g.integers(0, 2, n, dtype=U64)
        return f | (noise & ~mask)
    raise KeyError(name)


# ---------------------------------------------------------------- orders, fields, values

@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("name", PATTERNS)
def test_orders_fields_and_patterns(native, flags, field, name):
    for n, k in ((300, 0), (300, 1), (300, 17), (300, 299), (300, 300), (300, 301), (300, 4096),
                 (1, 1), (0, 5), (0, 0)):
        check_top(native, Top(values(name, n, field), k, flags, field), "n=%d k=%d" % (n, k))


@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
def test_values_near_the_top_of_the_range(native, flags):
    """a 64-bit compare done in halves, or as signed numbers, gets these wrong"""
    v = [MAXU, MAXU - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 0, 1, 0xffffffff, 1 << 32,
         (1 << 32) + 1, (2 << 32) + 1, (2 << 32) + 2, (3 << 32) + 1, MAXU, 0]
    for k in (1, 2, 7, 14, 15):
        got = check_top(native, Top(v, k, flags))
    want = sorted(v, reverse=not flags)
    assert [int(x) for x in got["vals"][:15]] == want
    assert list(got["pos"][:2]) == ([5, 14] if flags else [0, 13])


@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
@pytest.mark.parametrize("field", [f for f in FIELDS if f != (0, 64)])
def test_values_that_differ_only_outside_the_field_tie_by_position(native, flags, field):
    shift, bits = field
    mask = ((1 << bits) - 1) << shift
    g = np.random.default_rng(9)
    noise = g.integers(0, 1 << 63, 200, dtype=U64) * U64(2) + U64(1)
    vals = (noise & U64(~mask & MAXU)) | U64(mask & 0x5555555555555555)
    assert len(set(vals.tolist())) > 100
    got = check_top(native, Top(vals, 50, flags, field))
    assert list(got["pos"][:50]) == list(range(50))
    assert list(got["info"][:4]) == [50, 200, (mask & 0x5555555555555555) >> shift, 150]


@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
def test_all_values_equal(native, flags):
    """the cut is purely by position"""
    for n, k in ((100, 0), (100, 1), (100, 99), (100, 100), (100, 101)):
        got = check_top(native, Top([7 << 20] * n, k, flags, (16, 40)))
        m = min(n, k)
        assert list(got["pos"][:m]) == list(range(m))
        assert list(got["info"][:4]) == [m, n, (7 << 4) if m else 0, n - m if m else 0]


def test_the_cut_and_its_ties(native):
    vals = [5, 9, 9, 1, 7, 9, 7, 7]
    got = check_top(native, Top(vals, 4))
    assert list(got["pos"][:4]) == [1, 2, 5, 4] and list(got["info"][:4]) == [4, 8, 7, 2]
    got = check_top(native, Top(vals, 3))
    assert list(got["info"][:4]) == [3, 8, 9, 0]
    got = check_top(native, Top(vals, 2, SMALLEST))
    assert list(got["pos"][:2]) == [3, 0] and list(got["info"][:4]) == [2, 8, 5, 0]
    got = check_top(native, Top(vals, 3, SMALLEST))
    assert list(got["pos"][:3]) == [3, 0, 4] and list(got["info"][:4]) == [3, 8, 7, 2]


# ---------------------------------------------------------------- N

@pytest.mark.parametrize("flags", [LARGEST, SEGMENTS, SMALLEST | SEGMENTS])
@pytest.mark.parametrize("n", [None, 0, 1, 19, 20, 21, 1 << 40])
def test_n_under_both_counting_rules(native, flags, n):
    """*n below, at and above cap: the table's rule takes cap entries of a short table, the
    reduce's cap - 1"""
    c = Top(values("random40", 20), 20, flags, n=n)
    short = 19 if flags & SEGMENTS else 20
    assert c.N == {None: 20, 0: 0, 1: 1, 19: 19, 20: 20, 21: short, 1 << 40: short}[n]
    got = check_top(native, c)
    assert int(got["info"][1]) == c.N
    check_top(native, Top([], 3, flags, n=n))
    check_top(native, Top([], 0, flags, n=n, keys=None))
    for k in (0, 1, 25):
        check_top(native, Top(values("random64", 20), k, flags, n=n))


# ---------------------------------------------------------------- outputs

@pytest.mark.parametrize("want", [("vals", "pos"), ("keys", "pos"), ("keys", "vals"), ("pos",),
                                  ("keys",), ()])
def test_each_output_absent(native, want):
    vals = values("random40", 500)
    check_top(native, Top(vals, 64, LARGEST, (0, 40), want=want))
    check_top(native, Top(vals, 64, SMALLEST, (8, 24), want=want))


def test_keys_may_be_null_when_they_are_not_wanted(native):
    vals = values("random40", 100)
    got = check_top(native, Top(vals, 10, keys=None))
    assert set(got) == {"vals", "pos", "info"}
    # a percentile: only info
    got = check_top(native, Top(vals, 50, SMALLEST, keys=None, want=()))
    assert int(got["info"][2]) == sorted(vals.tolist())[49]


def test_top_through_native(native):
    keys = u64([10, 20, 30, 40, 50])
    k, v, p, info = native.top(keys, [5, 9, 9, 1, 7], 3)
    assert list(k) == [20, 30, 50] and list(v) == [9, 9, 7] and list(p) == [1, 2, 4]
    assert list(info) == [3, 5, 7, 0]
    k, v, p, info = native.top(None, [5, 9, 9, 1, 7], 9, native.TOP_SMALLEST, val_bits=3, n=4)
    assert k is None and list(v) == [9, 9, 1, 5] and list(p) == [1, 2, 3, 0]
    assert list(info) == [4, 4, 5, 0]
    k, v, p, info = native.top(keys, [5, 9, 9, 1, 7], 1, native.TOP_SEGMENTS, n=9, want=("pos",))
    assert k is None and v is None and list(p) == [1] and list(info) == [1, 4, 9, 1]
    assert native.TOP_MAX == native.STEER_TILE


# ---------------------------------------------------------------- errors

def _raw(native, out="ok", info="ok", vals="ok", keys="ok", want_keys=True, cap=4, flags=0,
         shift=0, bits=64, k=2):
    """one call with some arguments made bad: (code, the message, nothing written)"""
    bufs = {w: np.full(16, 0x33, dtype=U64) for w in ("k", "v", "n", "ok", "ov", "op", "info")}
    bufs["n"][0] = 4
    before = {w: b.copy() for w, b in bufs.items()}
    tops = native.BatchTops(bufs["ok"].ctypes.data if want_keys else None, bufs["ov"].ctypes.data,
                            bufs["op"].ctypes.data)
    code = native.lib().ebpf_batch_top(
        bufs["k"].ctypes.data if keys == "ok" else None,
        bufs["v"].ctypes.data if vals == "ok" else None, cap, bufs["n"].ctypes.data, flags, shift,
        bits, k, ctypes.byref(tops) if out == "ok" else None,
        bufs["info"].ctypes.data if info == "ok" else None)
    return code, native.last_error(), all((bufs[w] == before[w]).all() for w in bufs)


def test_argument_errors_in_their_order_write_nothing(native):
    E, B = errno.EINVAL, errno.E2BIG
    assert _raw(native)[0] == 0 and not _raw(native)[2]
    # each refusal, from the last to the first, with every later one present too: the earlier wins
    bad = [("E2BIG", dict(k=4097), B), ("E2BIG", dict(cap=1 << 32), B),
           ("out->keys", dict(keys=None), E), ("vals is NULL", dict(vals=None), E),
           ("val_bits", dict(shift=60, bits=5), E), ("flags", dict(flags=4), E),
           ("out or info", dict(info=None), E)]
    later = {}
    for text, args, code in bad:
        for a in (args, dict(later, **args)):
            got, msg, untouched = _raw(native, **a)
            assert got == code and untouched, (text, a)
            assert (text in msg) if code == E else ("above" in msg), (text, a, msg)
        later.update(args)
    assert _raw(native, out=None, **later)[:1] == (E,) and "out or info" in _raw(native, out=None)[1]
    for a in (dict(bits=0), dict(bits=65), dict(shift=64, bits=1), dict(shift=1, bits=64),
              dict(flags=0x80000000), dict(flags=8, k=5000)):
        assert _raw(native, **a)[::2] == (E, True), a
    # what is valid: NULL arrays with nothing behind them, k == 0, k == EBPF_TOP_MAX, every flag
    assert _raw(native, vals=None, keys=None, want_keys=False, cap=0)[0] == 0
    assert _raw(native, keys=None, want_keys=False)[0] == 0
    assert _raw(native, k=0)[0] == 0 and _raw(native, k=4096, cap=16)[0] == 0
    assert _raw(native, flags=3, shift=63, bits=1)[0] == 0
