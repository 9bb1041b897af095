"""Rolling a table up on the host (include/ebpf_gpu.h: ebpf_batch_rollup, csrc/host/rollup.cpp)
against a Python statement of the rule: itertools.groupby over key >> key_shift.  Every input has
one right answer, so every comparison is exact.  Every output buffer is pre-filled with a value no
result holds and is GUARD entries longer than the call may write, so comparing the buffers whole
checks what must not be written too.  test_gpu_rollup.py runs the device function against this
host function on the same buffers."""
import ctypes
import errno
import itertools

import numpy as np
import pytest

U64 = np.uint64
MAXU = (1 << 64) - 1
GUARD = 8
FILL = 0x5a5a5a5a5a5a5a5a      # (no key, count, value or position of these tests)
INFO_FILL = 0x2222222222222222
SEGMENTS = 1
ALL = ("keys", "count", "sum", "min", "max", "bits", "starts")
VALUE = ("sum", "min", "max", "bits")
SHIFTS = [0, 1, 32, 63]
FIELDS = [(0, 64), (24, 16), (63, 1)]


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


class Roll:
    """one rollup call; vals None: vals is NULL (and the outputs that read it are not wanted)"""

    def __init__(self, keys, vals, shift, flags=0, field=(0, 64), n=None, out_cap=None, want=ALL):
        self.keys = u64(keys)
        self.cap = len(self.keys)
        self.vals = None if vals is None else u64(vals)
        assert self.vals is None or len(self.vals) == self.cap
        self.shift, self.flags, self.field, self.n = shift, flags, field, n
        self.want = tuple(w for w in ALL if w in want and (self.vals is not None or w not in VALUE))
        self.N = entries(self.cap, n, flags)
        self.out_cap = self.cap if out_cap is None else out_cap

    def size(self, w):
        return self.out_cap + (1 if w == "starts" else 0) + GUARD

    def runs(self):
        """[(prefix, first position, end)] of the runs, in order"""
        out, p = [], 0
        for c, g in itertools.groupby(int(k) >> self.shift for k in self.keys[:self.N].tolist()):
            m = len(list(g))
            out.append((c, p, p + m))
            p += m
        return out

    def expect(self, fill=FILL):
        shift, bits = self.field
        runs = self.runs()
        out = {w: np.full(self.size(w), fill, dtype=U64) for w in self.want}
        for r, (c, a, b) in enumerate(runs[:self.out_cap]):
            v = [] if self.vals is None else [(int(x) >> shift) & ((1 << bits) - 1)
                                              for x in self.vals[a:b].tolist()]
            row = {"keys": c, "count": b - a, "starts": a}
            if v:
                row.update(sum=sum(v) & MAXU, min=min(v), max=max(v),
                           bits=int(np.bitwise_or.reduce(u64(v))))
            for w in self.want:
                out[w][r] = row[w]
        if "starts" in out and len(runs) <= self.out_cap:
            out["starts"][len(runs)] = self.N
        out["info"] = np.full(2 + GUARD, INFO_FILL, dtype=U64)
        out["info"][:2] = [len(runs), self.N]
        return out


def host_rollup(native, c, fill=FILL):
    """(code, {name: buffer}) of the host function on pre-filled, guard-extended buffers"""
    out = {w: np.full(c.size(w), fill, dtype=U64) for w in c.want}
    out["info"] = np.full(2 + GUARD, INFO_FILL, dtype=U64)
    rolls = native.BatchRolls(*[out[w].ctypes.data if w in c.want else None for w in ALL])
    n = None if c.n is None else np.array([c.n], dtype=U64)
    code = native.lib().ebpf_batch_rollup(
        c.keys.ctypes.data if c.cap else None,
        None if c.vals is None or not c.cap else c.vals.ctypes.data, c.cap,
        None if n is None else n.ctypes.data, c.flags, c.shift, c.field[0], c.field[1], c.out_cap,
        ctypes.byref(rolls), out["info"].ctypes.data)
    return code, out


def check_rollup(native, c, msg=""):
    code, got = host_rollup(native, c)
    want = c.expect()
    assert code == (errno.ENOSPC if int(want["info"][0]) > c.out_cap else 0), msg
    assert set(got) == set(want)
    for w in want:
        np.testing.assert_array_equal(got[w], want[w], err_msg="%s: %s" % (msg, w))
    return got


def keys_of_runs(lengths, shift, seed=0):
    """non-decreasing keys whose runs under `shift` have these lengths: ascending prefixes that use
    the whole range left of the shift, and below the shift the entry's place in its run"""
    g = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    R = len(lengths)
    top = 1 << (64 - shift)
    assert R <= top
    step = max(1, min((top - 1) // max(R, 1), 1 << 40))
    prefix = np.arange(R, dtype=U64) * U64(step)
    if step > 1:
        prefix += g.integers(0, step, R, dtype=U64)
    if R:
        prefix[-1] = top - 1 if R > 1 or g.integers(0, 2) else prefix[-1]
    run = np.repeat(np.arange(R), lengths)
    within = np.arange(len(run), dtype=np.int64) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    low = within.astype(U64) & U64((1 << shift) - 1)
    return (prefix[run] << U64(shift)) | low


def random_vals(n, seed=0):
    g = np.random.default_rng(seed + 7)
    return g.integers(0, 1 << 63, n, dtype=U64) * U64(2) + g.integers(0, 2, n, dtype=U64)


def lengths_of(total, mean, seed=0):
    """geometric run lengths of this mean that sum to total"""
    g = np.random.default_rng(seed + 3)
    out, left = [], total
    while left > 0:
        m = min(left, int(g.geometric(1.0 / mean)))
        out.append(m)
        left -= m
    return out


# ---------------------------------------------------------------- prefixes and runs

@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("mean", [1.0, 1.5, 7.0])
def test_shifts_and_run_lengths(native, shift, mean):
    lens = lengths_of(300, mean, seed=shift)
    if shift == 63:
        lens = [sum(lens) - 120, 120]          # (two prefixes are all there are)
    keys = keys_of_runs(lens, shift, seed=shift)
    c = Roll(keys, random_vals(len(keys)), shift)
    assert [b - a for _, a, b in c.runs()] == lens
    got = check_rollup(native, c, "shift=%d mean=%s" % (shift, mean))
    assert int(got["info"][0]) == len(lens)
    if len(lens) > 1:
        assert int(got["keys"][len(lens) - 1]) == MAXU >> shift      # the largest prefix


def test_keys_that_differ_in_one_word_only(native):
    """a compare of either 32-bit half alone merges or splits these"""
    high = [(h << 32) | 7 for h in (0, 1, 2, 3, 0x80000000, 0xffffffff)]     # the low words equal
    low = [(5 << 32) | x for x in (0, 1, 2, 0x80000000, 0xffffffff)]         # the high words equal
    for keys, shift, C in ((high, 0, 6), (low, 0, 5), (high, 32, 6), (low, 32, 1),
                           (high, 31, 6), (low, 31, 2), (high, 33, 4), (low, 33, 1),
                           (high + low, 0, 11), (sorted(high + low), 32, 7)):
        got = check_rollup(native, Roll(keys, random_vals(len(keys)), shift), "shift=%d" % shift)
        assert int(got["info"][0]) == C, (keys, shift)


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_smallest_and_the_largest_prefix(native, shift):
    lo = [0] * 3 if shift == 0 else [0, 1, (1 << shift) - 1]
    hi = [MAXU] * 2 if shift == 0 else [MAXU - (1 << shift) + 1, MAXU]
    got = check_rollup(native, Roll(lo + hi, [1, 2, 3, 4, 5], shift))
    assert list(got["keys"][:2]) == [0, MAXU >> shift] and list(got["count"][:2]) == [3, 2]
    assert list(got["starts"][:3]) == [0, 3, 5] and list(got["sum"][:2]) == [6, 9]


def test_unsorted_keys_and_equal_neighbours_are_defined(native):
    g = np.random.default_rng(4)
    keys = g.integers(0, 6, 400, dtype=U64) << U64(8) | g.integers(0, 4, 400, dtype=U64)
    for shift in (0, 2, 8, 9):
        c = Roll(keys, random_vals(400), shift)
        got = check_rollup(native, c, "shift=%d" % shift)
        k = [int(x) for x in got["keys"][:int(got["info"][0])]]
        assert sorted(set(k)) != k                 # (a prefix comes back: not a table)
    got = check_rollup(native, Roll([9] * 50, random_vals(50), 0))
    assert list(got["info"][:2]) == [1, 50] and int(got["count"][0]) == 50
    check_rollup(native, Roll([3, 3, 2, 2, 3, 3, 3, 1], None, 0))


# ---------------------------------------------------------------- N

@pytest.mark.parametrize("flags", [0, SEGMENTS])
@pytest.mark.parametrize("n", [None, 0, 1, 19, 20, 21, 1 << 40])
def test_n_under_both_counting_rules(native, flags, n):
    """*n below, at and above cap: the table's rule takes cap entries of a short table, the
    reduce's cap - 1"""
    keys = keys_of_runs([3, 1, 4, 1, 5, 6], 8)
    c = Roll(keys, random_vals(20), 8, flags, n=n)
    short = 19 if flags & SEGMENTS else 20
    assert c.N == {None: 20, 0: 0, 1: 1, 19: 19, 20: 20, 21: short, 1 << 40: short}[n]
    got = check_rollup(native, c)
    assert int(got["info"][1]) == c.N
    if c.N == 19:
        assert int(got["count"][5]) == 5 and int(got["starts"][6]) == 19
    check_rollup(native, Roll([], [], 8, flags, n=n))
    check_rollup(native, Roll([], None, 8, flags, n=n, out_cap=3))


def test_no_entries(native):
    """cap == 0 and N == 0: info = {0, 0} and starts[0] = 0"""
    for c in (Roll([], [], 0), Roll([], None, 5, out_cap=0), Roll([], [], 5, out_cap=4),
              Roll([1, 2, 3], [1, 2, 3], 0, n=0), Roll([1, 2, 3], [1, 2, 3], 0, n=0, out_cap=0)):
        got = check_rollup(native, c)
        assert list(got["info"][:2]) == [0, 0] and int(got["starts"][0]) == 0
        assert int(got["starts"][1]) == FILL


# ---------------------------------------------------------------- outputs and values

@pytest.mark.parametrize("want", [(w,) for w in ALL] + [(), ("keys", "count", "starts"),
                                                        ("count", "sum"), ALL])
def test_each_member_alone_and_none(native, want):
    keys = keys_of_runs(lengths_of(200, 3.0), 16)
    got = check_rollup(native, Roll(keys, random_vals(200), 16, field=(8, 40), want=want))
    assert set(got) == set(want) | {"info"}


def test_vals_may_be_null_when_no_output_reads_them(native):
    keys = keys_of_runs(lengths_of(200, 3.0), 16)
    got = check_rollup(native, Roll(keys, None, 16))
    assert set(got) == {"keys", "count", "starts", "info"}
    # the field is not looked at either
    check_rollup(native, Roll(keys, None, 16, field=(70, 0)))
    check_rollup(native, Roll(keys, random_vals(200), 16, field=(70, 0), want=("count",)))


@pytest.mark.parametrize("field", FIELDS)
def test_value_fields(native, field):
    keys = keys_of_runs(lengths_of(300, 4.0), 32)
    check_rollup(native, Roll(keys, random_vals(300), 32, field=field))


def test_sum_wraps_and_the_extremes(native):
    keys = keys_of_runs([3, 2, 4, 1], 4)
    vals = [MAXU, MAXU, 5, MAXU, MAXU, 0, 0, 0, 0, 1 << 63]
    got = check_rollup(native, Roll(keys, vals, 4))
    assert list(got["sum"][:4]) == [3, MAXU - 1, 0, 1 << 63]       # modulo 2^64
    assert list(got["min"][:4]) == [5, MAXU, 0, 1 << 63]           # a minimum over all-ones
    assert list(got["max"][:4]) == [MAXU, MAXU, 0, 1 << 63]        # a maximum over zeros
    assert list(got["bits"][:4]) == [MAXU, MAXU, 0, 1 << 63]


def test_short_outputs(native):
    """out_cap below, at and above C: starts[C] is written iff C <= out_cap, a cut run is still
    whole, and ENOSPC comes with info written"""
    lens = lengths_of(300, 5.0)
    C = len(lens)
    keys, vals = keys_of_runs(lens, 12), random_vals(300)
    for cap in (0, 1, C - 1, C, C + 1, 2 * C):
        code, got = host_rollup(native, Roll(keys, vals, 12, out_cap=cap))
        check_rollup(native, Roll(keys, vals, 12, out_cap=cap), "out_cap=%d" % cap)
        assert code == (errno.ENOSPC if cap < C else 0)
        assert list(got["info"][:2]) == [C, 300]
        assert int(got["starts"][min(C, cap)]) == (300 if cap >= C else FILL)
        if 0 < cap < C:
            assert int(got["count"][cap - 1]) == lens[cap - 1]
        for want in (("count",), ()):
            check_rollup(native, Roll(keys, vals, 12, out_cap=cap, want=want))


def test_a_rollup_of_a_rollup(native):
    """the /24 table of a /32 table rolled up again is the /16 table: count as vals, with sum"""
    g = np.random.default_rng(8)
    hosts = np.unique(g.integers(0, 1 << 14, 3000, dtype=U64) * U64(37))
    byts = random_vals(len(hosts)) >> U64(20)
    a, ainfo, code = native.rollup(hosts, byts, 8)
    assert code == 0 and int(ainfo[0]) == len(a["keys"]) < len(hosts)
    b, binfo, code = native.rollup(a["keys"], a["count"], 8, want=("keys", "sum"))
    b2, _, _ = native.rollup(a["keys"], a["sum"], 8, want=("keys", "sum"))
    one, oinfo, code = native.rollup(hosts, byts, 16, want=("keys", "count", "sum"))
    assert int(binfo[0]) == int(oinfo[0]) > 1
    np.testing.assert_array_equal(b["keys"], one["keys"])
    np.testing.assert_array_equal(b["sum"], one["count"])
    np.testing.assert_array_equal(b2["sum"], one["sum"])
    assert int(one["count"].sum()) == len(hosts)


def test_rollup_through_native(native):
    keys = u64([0x100, 0x101, 0x1ff, 0x200, 0x300, 0x301])
    out, info, code = native.rollup(keys, [5, 9, 2, 1, 7, 7], 8)
    assert code == 0 and list(info) == [3, 6]
    assert list(out["keys"]) == [1, 2, 3] and list(out["count"]) == [3, 1, 2]
    assert list(out["sum"]) == [16, 1, 14] and list(out["min"]) == [2, 1, 7]
    assert list(out["max"]) == [9, 1, 7] and list(out["bits"]) == [15, 1, 7]
    assert list(out["starts"]) == [0, 3, 4, 6]
    out, info, code = native.rollup(keys, None, 8, out_cap=2)
    assert code == errno.ENOSPC and list(info) == [3, 6] and set(out) == {"keys", "count", "starts"}
    assert list(out["keys"]) == [1, 2] and list(out["starts"]) == [0, 3]
    out, info, code = native.rollup(keys, [5, 9, 2, 1, 7, 7], 0, native.ROLLUP_SEGMENTS, 1, 2, n=9,
                                    want=("count", "sum"))
    assert code == 0 and list(info) == [5, 5] and list(out["sum"]) == [2, 0, 1, 0, 3]
    assert native.ROLLS == ALL


# ---------------------------------------------------------------- errors

def _raw(native, out="ok", info="ok", vals="ok", keys="ok", values=True, cap=4, flags=0, key_shift=8,
         shift=0, bits=64, out_cap=4):
    """one call with some arguments made bad: (code, the message, nothing written)"""
    names = ("k", "v", "n", "info") + ALL
    bufs = {w: np.full(16, 0x33, dtype=U64) for w in names}
    bufs["n"][0] = 4
    before = {w: b.copy() for w, b in bufs.items()}
    rolls = native.BatchRolls(*[bufs[w].ctypes.data if values or w not in VALUE else None
                                for w in ALL])
    code = native.lib().ebpf_batch_rollup(
        bufs["k"].ctypes.data if keys == "ok" else None,
        bufs["v"].ctypes.data if vals == "ok" else None, cap, bufs["n"].ctypes.data, flags,
        key_shift, shift, bits, out_cap, ctypes.byref(rolls) if out == "ok" else None,
        bufs["info"].ctypes.data if info == "ok" else None)
    return code, native.last_error(), all((bufs[w] == before[w]).all() for w in bufs)


def test_argument_errors_in_their_order_write_nothing(native):
    E, B = errno.EINVAL, errno.E2BIG
    assert _raw(native)[0] == 0 and not _raw(native)[2]
    # each refusal, from the last to the first, with every later one present too: the earlier wins
    bad = [("above 2^32", dict(out_cap=1 << 32), B), ("above 2^32", dict(cap=1 << 32), B),
           ("vals is NULL", dict(vals=None), E), ("keys is NULL", dict(keys=None), E),
           ("val_bits", dict(shift=60, bits=5), E), ("key_shift", dict(key_shift=64), E),
           ("flags", dict(flags=2), E), ("out or info", dict(info=None), E)]
    later = {}
    for text, args, code in bad:
        for a in (args, dict(later, **args)):
            got, msg, untouched = _raw(native, **a)
            assert got == code and untouched, (text, a)
            assert text in msg, (text, a, msg)
        later.update(args)
    assert _raw(native, out=None, **later)[:1] == (E,) and "out or info" in _raw(native, out=None)[1]
    for a in (dict(bits=0), dict(bits=65), dict(shift=64, bits=1), dict(shift=1, bits=64),
              dict(flags=0x80000000), dict(key_shift=1 << 31), dict(flags=4, cap=1 << 33)):
        assert _raw(native, **a)[::2] == (E, True), a
    # what is valid: no vals and a bad field when no output reads the values, NULL arrays with
    # nothing behind them, members with out_cap == 0, the largest shift, the flag
    assert _raw(native, vals=None, values=False)[0] == 0
    assert _raw(native, values=False, shift=64, bits=0)[0] == 0
    assert _raw(native, vals=None, keys=None, cap=0)[0] == 0
    assert _raw(native, out_cap=0)[0] == errno.ENOSPC and _raw(native, out_cap=0, cap=0)[0] == 0
    assert _raw(native, flags=1, key_shift=63, shift=63, bits=1)[0] == 0
