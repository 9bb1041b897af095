"""Carrying totals across batches on the host (include/ebpf_gpu.h: ebpf_batch_lookup and
ebpf_batch_accumulate, csrc/host/table.cpp) against a Python dict statement of the rules.  A sorted
table has one right answer: every comparison is exact.  Every output buffer is pre-filled with a
value no result holds and is GUARD entries longer than the call may write, so comparing the buffers
whole checks what must not be written too.  test_gpu_table.py runs the device functions against
these host functions on the same buffers."""
import ctypes
import errno

import numpy as np
import pytest

U64 = np.uint64
MAXU = (1 << 64) - 1
GUARD = 8
FILL = {"vals": 0xa5a5a5a5a5a5a5a5, "pos": 0xa5a5a5a5, "keys": 0x5a5a5a5a5a5a5a5a,
        "n": 0x1111111111111111, "info": 0x2222222222222222}
TYPES = {"vals": U64, "pos": np.uint32, "keys": U64, "n": U64, "info": U64}
OPS = {0: lambda a, b: (a + b) & MAXU, 1: min, 2: max, 3: lambda a, b: a | b}


def used(cap, nkeys):
    """R: the keys of the batch that are used"""
    if nkeys is None:
        return cap
    return nkeys if nkeys <= cap else max(cap - 1, 0)


def u64(a):
    if isinstance(a, np.ndarray) and a.dtype.kind in "ui":
        return np.ascontiguousarray(a.astype(U64))
    return np.array([int(x) for x in a], dtype=U64)


class Table:
    """a table on the host: cap entries, of which min(n, cap) are valid; n None: all"""

    def __init__(self, keys=(), vals=None, n=None):
        self.keys = u64(keys)
        self.vals = u64(vals if vals is not None else [0] * len(self.keys))
        assert len(self.keys) == len(self.vals)
        self.cap = len(self.keys)
        self.n = self.cap if n is None else n

    @property
    def valid(self):
        return min(self.n, self.cap)

    def as_dict(self):
        return {int(k): int(v) for k, v in zip(self.keys[:self.valid], self.vals[:self.valid])}


class Look:
    """one lookup call"""

    def __init__(self, table, keys, nkeys=None, mode=0, missing=0, limit=0, want=("vals", "pos")):
        self.table, self.keys, self.nkeys = table, u64(keys), nkeys
        self.mode, self.missing, self.limit, self.want = mode, missing, limit, tuple(want)
        self.cap = len(self.keys)
        self.R = used(self.cap, nkeys)

    def expect(self, fill=FILL):
        d = self.table.as_dict()
        where = {int(k): p for p, k in enumerate(self.table.keys[:self.table.valid])}
        out = {k: np.full(self.cap + GUARD, fill[k], dtype=TYPES[k]) for k in self.want}
        for g in range(self.R):
            k = int(self.keys[g])
            v = d.get(k, self.missing)
            if "pos" in out:
                out["pos"][g] = where.get(k, 0xffffffff)
            if "vals" in out:
                out["vals"][g] = v if self.mode == 0 else (self.limit - v if v < self.limit else 0)
        return out


class Acc:
    """one accumulate call; table None: `in` is NULL"""

    def __init__(self, table, keys, adds, nkeys=None, op=0, lo=0, hi=MAXU, out_cap=None):
        self.table, self.keys, self.adds, self.nkeys = table, u64(keys), u64(adds), nkeys
        assert len(self.keys) == len(self.adds)
        self.op, self.lo, self.hi = op, lo, hi
        self.cap = len(self.keys)
        self.R = used(self.cap, nkeys)
        self.out_cap = self.cap + (table.cap if table else 0) if out_cap is None else out_cap

    def merged(self):
        """(the kept candidates in key order, those new to the table, those left out)"""
        d = self.table.as_dict() if self.table else {}
        cand = dict(d)
        for g in range(self.R):
            k, a = int(self.keys[g]), int(self.adds[g])
            cand[k] = OPS[self.op](d[k], a) if k in d else a
        kept = [(k, v) for k, v in sorted(cand.items()) if self.lo <= v <= self.hi]
        fresh = sum(1 for k, _ in kept if k not in d)
        return kept, fresh, len(cand) - len(kept)

    def expect(self, fill=FILL):
        kept, fresh, left = self.merged()
        out = {k: np.full(self.out_cap + GUARD, fill["keys"], dtype=U64) for k in ("keys", "vals")}
        m = min(len(kept), self.out_cap)
        out["keys"][:m] = u64([k for k, _ in kept[:m]])
        out["vals"][:m] = u64([v for _, v in kept[:m]])
        out["n"] = np.full(1 + GUARD, fill["n"], dtype=U64)
        out["n"][0] = len(kept)
        out["info"] = np.full(3 + GUARD, fill["info"], dtype=U64)
        out["info"][:3] = [len(kept), fresh, left]
        return out


def _ptr(a, nonempty=True):
    return a.ctypes.data if nonempty else None


def _table(native, t, hold):
    """struct ebpf_key_table of a Table on the host; hold keeps its arrays alive"""
    n = np.array([t.n], dtype=U64)
    hold += [t.keys, t.vals, n]
    return native.KeyTable(_ptr(t.keys, t.cap), _ptr(t.vals, t.cap), t.cap, n.ctypes.data)


def host_lookup(native, c, fill=FILL):
    """(code, {name: buffer}) of the host function on pre-filled, guard-extended buffers"""
    hold = []
    out = {k: np.full(c.cap + GUARD, fill[k], dtype=TYPES[k]) for k in c.want}
    nk = None if c.nkeys is None else np.array([c.nkeys], dtype=U64)
    code = native.lib().ebpf_batch_lookup(
        ctypes.byref(_table(native, c.table, hold)), _ptr(c.keys, c.cap), c.cap,
        None if nk is None else nk.ctypes.data, c.mode, c.missing, c.limit,
        out["vals"].ctypes.data if "vals" in out else None,
        out["pos"].ctypes.data if "pos" in out else None)
    return code, out


def host_accumulate(native, c, fill=FILL):
    hold = []
    out = {"keys": np.full(c.out_cap + GUARD, fill["keys"], dtype=U64),
           "vals": np.full(c.out_cap + GUARD, fill["keys"], dtype=U64),
           "n": np.full(1 + GUARD, fill["n"], dtype=U64),
           "info": np.full(3 + GUARD, fill["info"], dtype=U64)}
    nk = None if c.nkeys is None else np.array([c.nkeys], dtype=U64)
    tout = native.KeyTable(_ptr(out["keys"], c.out_cap), _ptr(out["vals"], c.out_cap), c.out_cap,
                           out["n"].ctypes.data)
    code = native.lib().ebpf_batch_accumulate(
        None if c.table is None else ctypes.byref(_table(native, c.table, hold)),
        _ptr(c.keys, c.cap), _ptr(c.adds, c.cap), c.cap, None if nk is None else nk.ctypes.data,
        c.op, c.lo, c.hi, ctypes.byref(tout), out["info"].ctypes.data)
    return code, out


def check_lookup(native, c, msg=""):
    code, got = host_lookup(native, c)
    assert code == 0, msg
    want = c.expect()
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (msg, k))
    return got


def check_accumulate(native, c, msg=""):
    code, got = host_accumulate(native, c)
    want = c.expect()
    assert code == (errno.ENOSPC if int(want["n"][0]) > c.out_cap else 0), msg
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s: %s" % (msg, k))
    return got


# keys that a 64-bit compare done in halves gets wrong: neighbours that differ only in the high
# word, or only in the low word, and the two ends of the range
EDGE_KEYS = sorted({0, 1, 0xffffffff, 1 << 32, (1 << 32) + 1, (2 << 32) + 1, (2 << 32) + 2,
                    (3 << 32) + 1, 0x7fffffffffffffff, 1 << 63, MAXU - 1, MAXU})


def random_table(g, n, bits=20):
    keys = np.unique(g.integers(0, 1 << bits, 2 * n + 8, dtype=U64))[:n]
    assert len(keys) == n
    return Table(keys, g.integers(0, 1 << 40, n, dtype=U64))


def shared_half(g, t, r, bits=20):
    """r ascending batch keys, about half of them the table's"""
    own = g.choice(t.keys[:t.valid], min(r // 2, t.valid), replace=False) if t.valid else u64([])
    new = np.setdiff1d(g.integers(0, 1 << bits, 2 * r + 8, dtype=U64), t.keys)
    new = g.choice(new, r - len(own), replace=False)
    return np.sort(np.concatenate([own, new]).astype(U64))


# ---------------------------------------------------------------- lookup

@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("missing", [0, 7, MAXU])
@pytest.mark.parametrize("limit", [0, 1000, MAXU])
def test_lookup_modes_missing_and_limit(native, mode, missing, limit):
    """both modes; missing and limit at 0 and UINT64_MAX; REMAINING with v below, at and above
    limit; keys in any order, repeated"""
    t = Table(EDGE_KEYS, [0, 999, 1000, 1001, MAXU, MAXU - 1, 5, 0, 1, 2, 3, 4])
    keys = EDGE_KEYS[::-1] + [2, 5, 1 << 32, 1 << 32, (1 << 33), MAXU - 2, 0, 0]
    check_lookup(native, Look(t, keys, None, mode, missing, limit))


def test_lookup_high_and_low_word_neighbours(native):
    t = Table([(2 << 32) + 1, (3 << 32) + 1], [10, 20])
    keys = [(1 << 32) + 1, (2 << 32) + 0, (2 << 32) + 1, (2 << 32) + 2, (3 << 32) + 0,
            (3 << 32) + 1, (3 << 32) + 2, (4 << 32) + 1, 1, 2 << 32, 3 << 32]
    got = check_lookup(native, Look(t, keys, missing=99))
    assert list(got["pos"][:len(keys)]) == [0xffffffff] * 2 + [0] + [0xffffffff] * 2 + [1] + \
        [0xffffffff] * 5


@pytest.mark.parametrize("nkeys", [None, 0, 5, 9, 10, 11, 1 << 40])
def test_lookup_the_three_cases_of_r(native, nkeys):
    g = np.random.default_rng(3)
    t = random_table(g, 50)
    c = Look(t, shared_half(g, t, 10), nkeys, missing=3)
    assert c.R == {None: 10, 0: 0, 5: 5, 9: 9, 10: 10, 11: 9, 1 << 40: 9}[nkeys]
    check_lookup(native, c)
    check_lookup(native, Look(t, [], nkeys))


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 1 << 40])
def test_lookup_short_and_empty_tables(native, n):
    """*n below, at and above cap: above, the table is its first cap entries"""
    t = Table(range(10, 90, 10), range(1, 9), n=n)
    check_lookup(native, Look(t, [5, 10, 20, 70, 80, 85, 90], missing=77))
    check_lookup(native, Look(Table(), [5, 10], missing=77))


@pytest.mark.parametrize("want", [("vals",), ("pos",), ()])
def test_lookup_each_output_alone(native, want):
    g = np.random.default_rng(4)
    t = random_table(g, 300)
    check_lookup(native, Look(t, shared_half(g, t, 200), mode=1, limit=1 << 39, want=want))


def test_lookup_random_against_numpy(native):
    g = np.random.default_rng(5)
    t = random_table(g, 5000)
    keys = g.permutation(shared_half(g, t, 3000))
    got = check_lookup(native, Look(t, keys, missing=1))
    p = np.searchsorted(t.keys, keys)
    there = (p < t.cap) & (t.keys[np.minimum(p, t.cap - 1)] == keys)
    assert 1000 < there.sum() < 2000
    np.testing.assert_array_equal(got["pos"][:3000][there], p[there].astype(np.uint32))
    v, _, code = native.lookup(t.keys, t.vals, keys, missing=1)
    assert code == 0
    np.testing.assert_array_equal(v, got["vals"][:3000])


# ---------------------------------------------------------------- accumulate

@pytest.mark.parametrize("op", [0, 1, 2, 3])
def test_accumulate_every_op(native, op):
    """a key in both, in the table alone, in the batch alone; ADD wraps; keys 0 and UINT64_MAX"""
    t = Table(EDGE_KEYS, [MAXU, 999, 1000, 1001, MAXU, MAXU - 1, 5, 0, 1, 2, 3, 1 << 63])
    keys = [0, 2, 0xffffffff, (1 << 32) + 1, (2 << 32) + 0, (2 << 32) + 2, 1 << 63, MAXU]
    adds = [1, 2, 3, 0xf0f0, 5, MAXU, MAXU, 1 << 63]
    got = check_accumulate(native, Acc(t, keys, adds, op=op))
    assert int(got["info"][0]) == len(EDGE_KEYS) + 2 and int(got["info"][1]) == 2
    if op == 0:
        assert int(got["vals"][0]) == 0 and int(got["vals"][len(EDGE_KEYS) + 1]) == 0


@pytest.mark.parametrize("lo,hi", [(0, MAXU), (1, 0), (MAXU, 0), (1000, 5000), (0, 0),
                                   (MAXU, MAXU)])
@pytest.mark.parametrize("op", [0, 2])
def test_accumulate_keep_ranges(native, lo, hi, op):
    """keep all, none, a middle band, and the two ends"""
    g = np.random.default_rng(6)
    t = random_table(g, 400)
    t.vals = g.integers(0, 4000, 400, dtype=U64)
    t.vals[::50] = U64(MAXU)
    keys = shared_half(g, t, 300)
    adds = g.integers(0, 4000, 300, dtype=U64)
    adds[::40] = 0
    c = Acc(t, keys, adds, op=op, lo=lo, hi=hi)
    got = check_accumulate(native, c)
    if (lo, hi) == (0, MAXU):
        assert int(got["info"][2]) == 0
    if lo > hi:
        assert int(got["info"][0]) == 0 and int(got["info"][2]) > 400


def test_accumulate_a_pure_prune(native):
    """R = 0: by nkeys, and by key_cap"""
    t = Table(range(0, 100, 2), range(50))
    for c in (Acc(t, range(1, 20, 2), [1] * 10, nkeys=0, lo=10, hi=30), Acc(t, [], [], lo=10, hi=30)):
        got = check_accumulate(native, c)
        assert list(got["info"][:3]) == [21, 0, 29]


def test_accumulate_without_a_table(native):
    for keys in ([], [5], [0, 1 << 32, MAXU]):
        got = check_accumulate(native, Acc(None, keys, [7] * len(keys)))
        assert int(got["info"][1]) == len(keys)
    check_accumulate(native, Acc(Table(), [3, 4], [1, 2]))
    # a table of cap 0 may leave n NULL too
    out = np.zeros(4, dtype=U64)
    n, info = np.zeros(1, dtype=U64), np.zeros(3, dtype=U64)
    keys, adds = u64([3, 4]), u64([1, 2])
    tin = native.KeyTable(None, None, 0, None)
    tout = native.KeyTable(out[:2].ctypes.data, out[2:].ctypes.data, 2, n.ctypes.data)
    assert native.lib().ebpf_batch_accumulate(ctypes.byref(tin), keys.ctypes.data, adds.ctypes.data,
                                              2, None, 0, 0, MAXU, ctypes.byref(tout),
                                              info.ctypes.data) == 0
    assert list(out) == [3, 4, 1, 2] and int(n[0]) == 2


@pytest.mark.parametrize("short", [1, 2, 100, "all"])
def test_accumulate_short_output_tables(native, short):
    """M = cap + 1 and M >> cap, cap 0: ENOSPC, what fits written, *n and info = M, guard whole"""
    g = np.random.default_rng(7)
    t = random_table(g, 300)
    keys = shared_half(g, t, 200)
    c = Acc(t, keys, g.integers(1, 100, 200, dtype=U64))
    M = len(c.merged()[0])
    c.out_cap = 0 if short == "all" else M - short
    code, got = host_accumulate(native, c)
    assert code == errno.ENOSPC
    check_accumulate(native, c)
    c.out_cap = M
    assert host_accumulate(native, c)[0] == 0


@pytest.mark.parametrize("n", [0, 1, 39, 40, 41, 1 << 50])
def test_accumulate_short_input_table(native, n):
    """a table that an accumulate left short (*n > cap) is its first cap entries"""
    t = Table(range(100, 500, 10), range(40), n=n)
    check_accumulate(native, Acc(t, range(95, 600, 15), range(1, 35)))


@pytest.mark.parametrize("nkeys", [None, 0, 1, 19, 20, 21, 1 << 40])
def test_accumulate_the_three_cases_of_r(native, nkeys):
    g = np.random.default_rng(8)
    t = random_table(g, 30)
    c = Acc(t, shared_half(g, t, 20), range(1, 21), nkeys=nkeys)
    assert c.R == {None: 20, 0: 0, 1: 1, 19: 19, 20: 20, 21: 19, 1 << 40: 19}[nkeys]
    check_accumulate(native, c)


PATTERNS = ["below", "above", "identical", "interleaved", "random", "ends", "words"]


def pattern(name, n, r, seed=0):
    """(table, batch keys) of n and r entries in one of the key patterns"""
    g = np.random.default_rng(seed + n * 7 + r)
    vals = g.integers(0, 1 << 40, n, dtype=U64)
    if name == "below":
        return Table(np.arange(n, dtype=U64) * U64(3) + U64(r + 5), vals), np.arange(r, dtype=U64)
    if name == "above":
        return Table(np.arange(n, dtype=U64) * U64(3), vals), np.arange(r, dtype=U64) + U64(3 * n + 5)
    if name == "identical":
        keys = np.arange(max(n, r), dtype=U64) * U64(0x100000001) + U64(1)
        return Table(keys[:n], vals), keys[:r]
    if name == "interleaved":
        return Table(np.arange(n, dtype=U64) * U64(2), vals), np.arange(r, dtype=U64) * U64(2) + U64(1)
    if name == "random":
        bits = max(int(n + r).bit_length() + 2, 8)
        t = random_table(g, n, bits)
        t.vals = vals
        return t, shared_half(g, t, r, bits)
    if name == "ends":   # one shared key at each end, nothing else shared
        keys = np.arange(n, dtype=U64) * U64(4) + U64(8)
        b = np.arange(r, dtype=U64) * U64(4) + U64(9)
        if n and r:
            b[0] = keys[0]
        if n > 1 and r > 1:
            b[-1] = keys[-1] = max(int(keys[-1]), int(b[-1])) + 1
        return Table(keys, vals), b
    if name == "words":  # neighbours that differ only in the high word, or only in the low word
        keys = (np.arange(n, dtype=U64) // U64(2) << U64(32)) + (np.arange(n, dtype=U64) % U64(2))
        b = (np.arange(r, dtype=U64) // U64(3) << U64(32)) + (np.arange(r, dtype=U64) % U64(3))
        return Table(keys, vals), b
    raise KeyError(name)


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("n,r", [(0, 0), (0, 9), (9, 0), (1, 1), (64, 17), (17, 64), (300, 300)])
def test_accumulate_key_patterns(native, name, n, r):
    t, keys = pattern(name, n, r)
    assert (np.diff(t.keys.astype(object)) > 0).all() and (np.diff(keys.astype(object)) > 0).all()
    check_accumulate(native, Acc(t, keys, np.arange(r) + 1, op=0))
    check_lookup(native, Look(t, keys[::-1], mode=1, limit=1 << 39))


def test_accumulate_through_native(native):
    """native.accumulate and native.lookup: two batches into a table, then looked up"""
    k1, v1, n1, info, code = native.accumulate(None, None, [3, 5, 9], [30, 50, 90])
    assert code == 0 and n1 == 3 and list(info) == [3, 3, 0]
    k2, v2, n2, info, code = native.accumulate(k1, v1, [1, 5, 9, 11], [1, 1, 1, 1], n=n1, out_cap=5)
    assert code == 0 and n2 == 5 and list(info) == [5, 2, 0]
    assert list(k2) == [1, 3, 5, 9, 11] and list(v2) == [1, 30, 51, 91, 1]
    vals, pos, code = native.lookup(k2, v2, [11, 2, 5], native.LOOKUP_REMAINING, 0, 60, n=n2)
    assert code == 0 and list(vals) == [59, 60, 9] and list(pos) == [4, native.EBPF_NO_ENTRY, 2]
    _, _, n3, info, code = native.accumulate(k2, v2, [], [], keep_lo=40, out_cap=1, n=n2)
    assert code == errno.ENOSPC and n3 == 2 and list(info) == [2, 0, 3]


# ---------------------------------------------------------------- errors

def _raw(native, table="ok", out="ok", info="ok", keys="ok", adds="ok", key_cap=4, mode=0, op=0,
         tcap=4, tnull=None, ocap=8, onull=None):
    """one lookup and one accumulate call with one argument made bad: (codes, buffers)"""
    bufs = {k: np.full(16, 0x33, dtype=U64) for k in ("tk", "tv", "tn", "k", "a", "ok", "ov",
                                                       "on", "info", "vals")}
    bufs["tk"][:4] = [1, 2, 3, 4]
    bufs["k"][:4] = [2, 3, 5, 6]
    bufs["tn"][0] = 4
    before = {k: v.copy() for k, v in bufs.items()}

    def tab(keys, vals, cap, n, null):
        m = {"keys": keys.ctypes.data, "vals": vals.ctypes.data, "n": n.ctypes.data}
        if null:
            m[null] = None
        return native.KeyTable(m["keys"], m["vals"], cap, m["n"])
    tin = tab(bufs["tk"], bufs["tv"], tcap, bufs["tn"], tnull)
    tout = tab(bufs["ok"], bufs["ov"], ocap, bufs["on"], onull)
    L = native.lib()
    kp = bufs["k"].ctypes.data if keys == "ok" else None
    ap = bufs["a"].ctypes.data if adds == "ok" else None
    ip = bufs["info"].ctypes.data if info == "ok" else None
    a = L.ebpf_batch_lookup(ctypes.byref(tin) if table == "ok" else None, kp, key_cap, None, mode,
                            0, 0, bufs["vals"].ctypes.data, None)
    b = L.ebpf_batch_accumulate(ctypes.byref(tin) if table == "ok" else None, kp, ap, key_cap, None,
                                op, 0, MAXU, ctypes.byref(tout) if out == "ok" else None, ip)
    untouched = all((bufs[k] == before[k]).all() for k in bufs)
    return a, b, untouched


def test_argument_errors_write_nothing(native):
    E, B = errno.EINVAL, errno.E2BIG
    assert _raw(native)[:2] == (0, 0)
    assert _raw(native, table=None) == (E, 0, False)          # (in NULL is an empty table)
    assert _raw(native, out=None)[1:] == (E, False)           # (the lookup wrote its values)
    assert _raw(native, info=None)[1] == E
    assert _raw(native, mode=2)[0] == E and _raw(native, op=4)[1] == E
    assert _raw(native, keys=None, out=None, mode=2) == (E, E, True)
    for bad in (dict(keys=None), dict(keys=None, adds=None), dict(tnull="keys"), dict(tnull="vals"),
                dict(tnull="n"), dict(key_cap=1 << 32), dict(tcap=1 << 32),
                dict(key_cap=1 << 32, tcap=1 << 32)):
        want = B if "key_cap" in bad or "tcap" in bad else E
        assert _raw(native, **bad) == (want, want, True), bad
    for bad in (dict(adds=None), dict(onull="keys"), dict(onull="vals"), dict(onull="n"),
                dict(info=None), dict(op=4), dict(op=0xffffffff)):
        assert _raw(native, mode=7, **bad) == (E, E, True), bad
    assert _raw(native, mode=7, ocap=1 << 32) == (E, B, True)
    # EINVAL comes before E2BIG
    assert _raw(native, keys=None, tcap=1 << 32) == (E, E, True)
    assert _raw(native, mode=9, op=9, key_cap=1 << 32) == (E, E, True)
    # NULL arrays are fine where nothing is behind them
    assert _raw(native, keys=None, adds=None, key_cap=0)[:2] == (0, 0)
    assert _raw(native, tcap=0, tnull="keys")[:2] == (0, 0)
    assert _raw(native, ocap=0, onull="vals", key_cap=0, tcap=0)[1] == 0


def test_unsorted_inputs_are_refused_with_nothing_written(native):
    for keys in ([1, 3, 2, 4], [1, 2, 2, 4], [4, 3, 2, 1], [1 << 32, 1, 2, 3]):
        t = Table(keys, [1, 2, 3, 4])
        code, got = host_lookup(native, Look(t, [1, 2, 3]))
        assert code == errno.EINVAL and all((got[k] == FILL[k]).all() for k in got)
        code, got = host_accumulate(native, Acc(t, [7, 8], [1, 1]))
        assert code == errno.EINVAL
        assert all((got[k] == (FILL["keys"] if k in ("keys", "vals") else FILL[k])).all() for k in got)
        # the same keys as the batch's: refused by the accumulate, fine for the lookup
        good = Table([1, 2, 3, 4], [1, 2, 3, 4])
        code, got = host_accumulate(native, Acc(good, keys, [1, 1, 1, 1]))
        assert code == errno.EINVAL
        assert all((got[k] == (FILL["keys"] if k in ("keys", "vals") else FILL[k])).all() for k in got)
        check_lookup(native, Look(good, keys))
        # past the valid entries and past R nothing is looked at
        check_lookup(native, Look(Table(keys, [1, 2, 3, 4], n=1), [1, 2, 3]))
        check_accumulate(native, Acc(good, [7, 9, 8, 8], [1, 1, 1, 1], nkeys=2))
