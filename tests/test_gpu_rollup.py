"""Rolling a table up on the device (include/ebpf_gpu.h: ebpf_batch_rollup_dev;
csrc/hip/rollup.hip) against the host function, which test_rollup.py checks against a Python
groupby.  Every input has one right answer: every comparison is exact.

Shapes: T = native.STEER_TILE entries go to one workgroup, 16 consecutive ones to a thread and 64
to a wave's first round of loads, so N and the runs' edges sit around 16, 64 and T; 513 tiles make
the tile scan cross a wave of its threads, and 1,025 tiles plus 3 entries give a thread of it two
tiles to walk.  Every output buffer is pre-filled with a value no result holds and is GUARD entries
longer than the call may write; the host function gets the same buffers, so comparing them whole
checks what must not be written too."""
import ctypes
import errno

import numpy as np
import pytest

from generic_ebpf_amd import native as _native
from gpu_buffers import ptr, run, up
from test_rollup import (ALL, FIELDS, FILL, GUARD, INFO_FILL, SEGMENTS, U64, Roll,
                         host_rollup, keys_of_runs, lengths_of, random_vals)

pytestmark = pytest.mark.gpu

T = _native.STEER_TILE
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]
WANTS = [ALL, ("count",), ("keys", "count", "starts"), ("sum",), ("keys", "min", "max"),
         ("bits", "starts"), ()]
OTHER = 0x0123456789abcdef


class DevRoll:
    """a Roll's arrays and outputs on the device"""

    def __init__(self, c, fill=FILL, skew=False):
        self.c, self.fill = c, fill
        s = 8 if skew else 0
        self.keys = up(c.keys, s)
        self.vals = None if c.vals is None else up(c.vals, s)
        self.n = None if c.n is None else up(np.array([c.n], dtype=U64), s)
        self.outs = {w: up(np.full(c.size(w), fill, dtype=U64), s) for w in c.want}
        self.outs["info"] = up(np.full(2 + GUARD, INFO_FILL, dtype=U64), s)

    def enqueue(self, gpu, stream):
        c = self.c
        rolls = gpu.BatchRolls(*[self.outs[w].data_ptr() if w in c.want else None for w in ALL])
        return gpu.lib().ebpf_batch_rollup_dev(
            0, ptr(self.keys), None if self.vals is None else ptr(self.vals), c.cap,
            None if self.n is None else self.n.data_ptr(), c.flags, c.shift, c.field[0], c.field[1],
            c.out_cap, ctypes.byref(rolls), self.outs["info"].data_ptr(), stream.cuda_stream)

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers, GUARD and all"""
        code, w = host_rollup(gpu, self.c, self.fill)
        assert code == (errno.ENOSPC if int(w["info"][0]) > self.c.out_cap else 0), msg
        got = {k: v.cpu().numpy().view(U64) for k, v in self.outs.items()}
        assert set(got) == set(w)
        for k in w:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


def check_all(gpu, devs):
    run(gpu, devs)
    return [d.check(gpu, "case %d: cap=%d n=%s shift=%d flags=%d field=%s out_cap=%d want=%s" %
                    (i, d.c.cap, d.c.n, d.c.shift, d.c.flags, d.c.field, d.c.out_cap, d.c.want))
            for i, d in enumerate(devs)]


def case(lens, shift, seed=0, **kw):
    keys = keys_of_runs(lens, shift, seed)
    return Roll(keys, random_vals(len(keys), seed), shift, **kw)


# ---------------------------------------------------------------- sizes, shifts, members

@pytest.mark.parametrize("turn", range(4))
def test_sizes_shifts_and_members(gpu, turn):
    devs = []
    for i, n in enumerate(SIZES):
        shift = (0, 1, 32, 63)[(i + turn) % 4]
        lens = lengths_of(n, (1.0, 3.0, 50.0)[(i + turn) % 3], seed=i)
        if shift == 63:
            lens = [m for m in (n // 2, n - n // 2) if m]
        devs.append(DevRoll(case(lens, shift, i, field=FIELDS[(i + turn) % 3],
                                 want=WANTS[(i + 2 * turn) % len(WANTS)])))
        devs.append(DevRoll(case(lens, shift, i, field=FIELDS[(i + turn + 1) % 3])))
    check_all(gpu, devs)


N3 = 3 * T + 9
SHAPES = {
    "one run": [N3],
    "every entry its own": [1] * N3,
    "runs of a thread": [16] * (N3 // 16) + [N3 % 16],
    "runs of a thread, shifted": [1] + [16] * ((N3 - 1) // 16) + [(N3 - 1) % 16],
    "runs of a wave": [64] * (N3 // 64) + [N3 % 64],
    "runs of a wave, shifted": [1] + [64] * ((N3 - 1) // 64) + [(N3 - 1) % 64],
    "runs of a tile": [T, T, T, 9],
    "runs of a tile, shifted": [1, T, T, T, 8],
    "a boundary before a tile's edge": [T - 1, N3 - T + 1],
    "a boundary on a tile's edge": [T, N3 - T],
    "a boundary after a tile's edge": [T + 1, N3 - T - 1],
    "a run over a whole tile": [T - 5, 2 * T + 7, 7],
    "pairs on every tile's edge": [T - 1, 2, T - 2, 2, T - 2, 2, 8],
    "geometric 1.5": lengths_of(N3, 1.5, 1),
    "geometric 40": lengths_of(N3, 40.0, 2),
    "geometric 3000": lengths_of(N3, 3000.0, 3),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_run_shapes(gpu, name):
    lens = [m for m in SHAPES[name] if m]
    assert sum(lens) == N3
    devs = [DevRoll(case(lens, shift, 5, field=field, want=want))
            for shift, field, want in ((0, (0, 64), ALL), (1, (24, 16), ALL), (32, (63, 1), ALL),
                                       (32, (0, 64), ("count",)), (0, (0, 64), ("sum", "starts")))]
    got = check_all(gpu, devs)
    assert int(got[0]["info"][0]) == len(lens) and int(got[0]["info"][1]) == N3


# ---------------------------------------------------------------- many tiles

def _many(gpu, n):
    long_runs = lengths_of(n, 3.0 * T, 9)
    devs = [DevRoll(case(long_runs, 32, 1, out_cap=2 * len(long_runs))),
            DevRoll(case(long_runs, 0, 2, want=("count",))),
            DevRoll(case([1] * n, 0, 3, want=("keys", "count", "sum", "starts"))),
            DevRoll(Roll(keys_of_runs([1] * n, 8, 4), None, 8, want=("count",), out_cap=T + 1))]
    got = check_all(gpu, devs)
    assert int(got[0]["info"][0]) == len(long_runs) and int(got[2]["info"][0]) == n


def test_513_tiles(gpu):
    """the tile scan crosses a wave of its threads"""
    _many(gpu, 512 * T + 5)


def test_1025_tiles(gpu):
    """a thread of the tile scan walks two tiles"""
    _many(gpu, 1025 * T + 3)


# ---------------------------------------------------------------- short outputs, N

def test_short_outputs(gpu):
    """out_cap below, at and above C, with clamped stores in every tile"""
    lens = lengths_of(N3, 3.0, 6)
    C = len(lens)
    assert C > 2000
    devs = []
    for cap in (0, 1, T, C // 2, C - 1, C, C + 1):
        devs.append(DevRoll(case(lens, 16, 6, out_cap=cap)))
        devs.append(DevRoll(case(lens, 16, 6, out_cap=cap, want=("count", "max"))))
        devs.append(DevRoll(case(lens, 16, 6, out_cap=cap, want=())))
    got = check_all(gpu, devs)
    assert all(int(g["info"][0]) == C for g in got)
    assert int(got[3 * 4]["starts"][C - 1]) == FILL and int(got[3 * 5]["starts"][C]) == N3


@pytest.mark.parametrize("flags", [0, SEGMENTS])
def test_n_under_both_counting_rules_and_rubbish_past_n(gpu, flags):
    """the entries past N go on with the last run's prefix, with values that would change every
    output"""
    devs = []
    for cap in (0, 1, 300, T + 9):
        lens = lengths_of(cap, 4.0, cap)
        for n in (None, 0, 1, cap - 1, cap, cap + 1, 1 << 50):
            if n is not None and n < 0:
                continue
            c = case(lens, 12, cap, flags=flags, n=n)
            c.keys[c.N:] = c.keys[c.N - 1] if c.N else 0
            c.vals[c.N:] = (1 << 64) - 1
            devs.append(DevRoll(c))
            devs.append(DevRoll(Roll(c.keys, c.vals, 12, flags, n=n, want=("count", "sum"),
                                     out_cap=max(cap // 8, 1))))
    got = check_all(gpu, devs)
    assert {int(r["info"][1]) for r in got} >= {0, 1, 299, 300, T + 8, T + 9}


def test_no_entries_and_no_outputs(gpu):
    devs = [DevRoll(Roll([], [], 0)), DevRoll(Roll([], None, 5, out_cap=0)),
            DevRoll(Roll([], [], 5, out_cap=4)), DevRoll(Roll([1, 2, 3], [1, 2, 3], 0, n=0)),
            DevRoll(Roll([1, 2, 3], [1, 2, 3], 0, out_cap=0)),
            DevRoll(Roll([1, 2, 3], None, 0, out_cap=0, want=()))]
    got = check_all(gpu, devs)
    assert int(got[1]["starts"][0]) == 0 and list(got[5]["info"][:2]) == [3, 3]


# ---------------------------------------------------------------- the other cases

def test_unaligned_buffers(gpu):
    """every array 8 bytes past a 256-byte boundary"""
    devs = [DevRoll(case(lengths_of(n, mean, n), shift, n, n=n - 1), skew=True)
            for n, mean, shift in ((257, 2.0, 0), (T + 1, 1.0, 8), (2 * T + 5, 70.0, 32))]
    for d in devs:
        assert d.vals.data_ptr() % 256 == 8 and d.keys.data_ptr() % 256 == 8
        assert all(t.data_ptr() % 256 == 8 for t in d.outs.values())
    check_all(gpu, devs)


def test_unsorted_and_constant_keys(gpu):
    g = np.random.default_rng(4)
    n = 2 * T + 77
    keys = g.integers(0, 6, n, dtype=U64) << U64(8) | g.integers(0, 4, n, dtype=U64)
    devs = [DevRoll(Roll(keys, random_vals(n), shift)) for shift in (0, 2, 8, 9, 63)]
    devs.append(DevRoll(Roll(np.full(n, 9, dtype=U64), random_vals(n), 0)))
    devs.append(DevRoll(Roll(g.integers(0, 1 << 63, n, dtype=U64), random_vals(n), 40)))
    got = check_all(gpu, devs)
    assert list(got[5]["info"][:2]) == [1, n] and int(got[4]["info"][0]) == 1


def test_ignores_what_the_outputs_held(gpu):
    c = case(lengths_of(N3, 5.0, 7), 20, 7, out_cap=500)
    devs = [DevRoll(c, FILL), DevRoll(c, OTHER), DevRoll(c, FILL)]
    a, b, a2 = check_all(gpu, devs)
    for w in ALL:
        m = 500
        assert a[w][:m].tobytes() == b[w][:m].tobytes() and (b[w][m:] == OTHER).all()
        assert a[w].tobytes() == a2[w].tobytes()
    assert a["info"].tobytes() == b["info"].tobytes() and int(a["info"][0]) > 500


def test_two_streams_keep_their_scratch_apart(gpu):
    import torch
    cs = [case(lengths_of(20 * T + 9, mean, s), 24, s) for s, mean in ((1, 2.0), (2, 900.0))]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [[DevRoll(c) for _ in range(3)] for c in cs]
    torch.cuda.synchronize()
    for r in range(3):
        for s in (0, 1):
            assert devs[s][r].enqueue(gpu, streams[s]) == 0
    torch.cuda.synchronize()
    for s in (0, 1):
        for d in devs[s]:
            d.check(gpu, "stream %d" % s)


def test_device_argument_errors(gpu):
    """known on the host, before the device is looked at; then ENODEV"""
    L = gpu.lib()
    E, B = errno.EINVAL, errno.E2BIG
    full = gpu.BatchRolls(*[16] * 7)
    plain = gpu.BatchRolls(16, 16, None, None, None, None, 16)

    def roll(keys=16, vals=16, cap=4, flags=0, key_shift=8, shift=0, bits=64, out_cap=4, out=full,
             info=16, dev=0):
        return L.ebpf_batch_rollup_dev(dev, keys, vals, cap, None, flags, key_shift, shift, bits,
                                       out_cap, None if out is None else ctypes.byref(out), info,
                                       None)
    assert roll(out=None) == E and roll(info=None) == E and roll(flags=2) == E
    assert roll(key_shift=64) == E and roll(bits=0) == E and roll(shift=1, bits=64) == E
    assert roll(keys=None) == E and roll(vals=None) == E
    assert roll(cap=1 << 32) == B and roll(out_cap=1 << 32) == B
    assert roll(cap=1 << 32, flags=8) == E and roll(out_cap=1 << 32, keys=None) == E
    assert roll(dev=99) == errno.ENODEV and roll(dev=99, vals=None, out=plain) == errno.ENODEV
    assert roll(dev=99, vals=None, bits=0, out=plain) == errno.ENODEV
    assert roll(dev=99, keys=None, vals=None, cap=0, out_cap=0) == errno.ENODEV


# ---------------------------------------------------------------- pipelines, on one stream

def _z(k, fill=0, dtype=None):
    import torch
    return torch.full((k,), fill, dtype=dtype or torch.int64, device="cuda:0")


def _host(t):
    return t.cpu().numpy().view(U64)


def test_distinct_sources_per_destination_of_a_batch(gpu):
    """group by dst << 32 | src -> reduce(bytes) -> rollup (the reduce's count, shift 32: sources
    and bytes per destination) -> top by sources, nothing read in between: equal to the same calls
    of the host functions"""
    import torch
    g = np.random.default_rng(31)
    count, ndst, K = T + 301, 40, 10
    fan = g.integers(1, 120, ndst)                       # the sources a destination may have
    dst = g.integers(0, ndst, count)
    src = (g.integers(0, 1 << 30, count) % fan[dst]) * 7919 + 11
    ret = ((dst.astype(U64) + U64(0xc0a80000)) << U64(32)) | src.astype(U64)
    lens = (40 + 8 * g.integers(0, 4, count)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    cap, rcap = count, 64
    st = torch.cuda.current_stream().cuda_stream
    d_ret, d_offs = up(ret), up(offsets)
    index = _z(count, -1, torch.int32)
    gkeys, gstarts, info = _z(cap, 0x5a), _z(cap + 1, 0x5a), _z(2)
    tmp_bytes = gpu.group_tmp_bytes(count, 64)
    tmp = _z(max(tmp_bytes, 8), 0, torch.uint8)
    gbytes = _z(cap, 0x5a)
    rkeys, rcount, rsum, rinfo = _z(rcap, 0x5a), _z(rcap, 0x5a), _z(rcap, 0x5a), _z(2, 0x5a)
    tkeys, tvals, tpos, tinfo = _z(K, 0x5a), _z(K, 0x5a), _z(K, 0x5a, torch.int32), _z(4)
    gpu.group_dev(0, d_ret.data_ptr(), None, count, 0, 64, index.data_ptr(), cap, gkeys.data_ptr(),
                  gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(), tmp_bytes, st)
    gpu.reduce_dev(0, None, count, 0, 0, index.data_ptr(), count, gstarts.data_ptr(), cap,
                   info.data_ptr(), bytes_ptr=gbytes.data_ptr(), offsets_ptr=d_offs.data_ptr(),
                   stream=st)
    gpu.rollup_dev(0, gkeys.data_ptr(), gbytes.data_ptr(), cap, info.data_ptr(), 32, rcap,
                   rinfo.data_ptr(), gpu.ROLLUP_SEGMENTS, keys_out_ptr=rkeys.data_ptr(),
                   count_ptr=rcount.data_ptr(), sum_ptr=rsum.data_ptr(), stream=st)
    gpu.top_dev(0, rkeys.data_ptr(), rcount.data_ptr(), rcap, rinfo.data_ptr(), K,
                tinfo.data_ptr(), keys_out_ptr=tkeys.data_ptr(), vals_out_ptr=tvals.data_ptr(),
                pos_out_ptr=tpos.data_ptr(), stream=st)
    torch.cuda.synchronize()
    # the same calls on the host
    h_index, h_gkeys, h_gstarts, h_info, code = gpu.group(ret, None, 0, 64, group_cap=cap)
    assert code == 0
    h_bytes = gpu.reduce(h_index, h_gstarts, count=count, offsets=offsets, nseg=int(h_info[0]),
                         want=("bytes",))[0]
    h_roll, h_rinfo, code = gpu.rollup(h_gkeys, h_bytes, 32, gpu.ROLLUP_SEGMENTS, out_cap=rcap,
                                       n=int(h_info[0]), want=("keys", "count", "sum"))
    assert code == 0
    C = int(h_rinfo[0])
    h_top = gpu.top(h_roll["keys"], h_roll["count"], K)
    assert list(_host(rinfo)) == list(h_rinfo) and C == ndst and int(h_rinfo[1]) == int(h_info[0])
    for dev, w in ((rkeys, "keys"), (rcount, "count"), (rsum, "sum")):
        np.testing.assert_array_equal(_host(dev)[:C], h_roll[w])
        assert (_host(dev)[C:] == 0x5a).all()
    np.testing.assert_array_equal(_host(tkeys), h_top[0])
    np.testing.assert_array_equal(_host(tvals), h_top[1])
    np.testing.assert_array_equal(tpos.cpu().numpy().view(np.uint32), h_top[2])
    assert list(_host(tinfo)) == list(h_top[3])
    # and what it means: the distinct sources and the bytes of every destination
    pairs = {}
    for d, s, n in zip(dst.tolist(), src.tolist(), lens.tolist()):
        pairs.setdefault(d + 0xc0a80000, {}).setdefault(s, []).append(n)
    assert list(h_roll["keys"]) == sorted(pairs)
    assert list(h_roll["count"]) == [len(pairs[d]) for d in sorted(pairs)]
    assert list(h_roll["sum"]) == [sum(sum(v) for v in pairs[d].values()) for d in sorted(pairs)]


def test_a_carried_table_rolled_up(gpu):
    """two batches' per-flow sums accumulated into a table -> rollup of the table -> top by bytes,
    nothing read in between: equal to the same calls of the host functions"""
    import torch
    g = np.random.default_rng(32)
    st = torch.cuda.current_stream().cuda_stream
    tcap, rcap, K = 2 * T, 512, 10
    batches = []
    for b in range(2):
        keys = np.unique((g.integers(0, 200, T + 50 * b, dtype=U64) << U64(32)) |
                         g.integers(0, 64, T + 50 * b, dtype=U64))
        batches.append((keys, g.integers(1, 1 << 20, len(keys), dtype=U64)))
    tables = [[_z(tcap, 0x5a), _z(tcap, 0x5a), _z(1)] for _ in range(2)]
    keep = []
    for b, (keys, adds) in enumerate(batches):
        cur, nxt = tables[b % 2], tables[1 - b % 2]
        d_keys, d_adds, ainfo = up(keys), up(adds), _z(3)
        gpu.accumulate_dev(0, None if b == 0 else (cur[0].data_ptr(), cur[1].data_ptr(), tcap,
                                                   cur[2].data_ptr()),
                           d_keys.data_ptr(), d_adds.data_ptr(), len(keys),
                           (nxt[0].data_ptr(), nxt[1].data_ptr(), tcap, nxt[2].data_ptr()),
                           ainfo.data_ptr(), stream=st)
        keep.append((d_keys, d_adds, ainfo))
    final = tables[0]    # (two swaps)
    rkeys, rcount, rsum, rstarts, rinfo = (_z(rcap, 0x5a), _z(rcap, 0x5a), _z(rcap, 0x5a),
                                           _z(rcap + 1, 0x5a), _z(2, 0x5a))
    tkeys, tvals, tinfo = _z(K, 0x5a), _z(K, 0x5a), _z(4)
    gpu.rollup_dev(0, final[0].data_ptr(), final[1].data_ptr(), tcap, final[2].data_ptr(), 32, rcap,
                   rinfo.data_ptr(), keys_out_ptr=rkeys.data_ptr(), count_ptr=rcount.data_ptr(),
                   sum_ptr=rsum.data_ptr(), starts_ptr=rstarts.data_ptr(), stream=st)
    gpu.top_dev(0, rkeys.data_ptr(), rsum.data_ptr(), rcap, rinfo.data_ptr(), K, tinfo.data_ptr(),
                keys_out_ptr=tkeys.data_ptr(), vals_out_ptr=tvals.data_ptr(), stream=st)
    torch.cuda.synchronize()
    k1, v1, n1, _, code = gpu.accumulate(None, None, *batches[0])
    assert code == 0
    k2, v2, n2, _, code = gpu.accumulate(k1[:n1], v1[:n1], *batches[1])
    assert code == 0 and n2 > n1
    h_roll, h_rinfo, code = gpu.rollup(k2, v2, 32, out_cap=rcap, n=n2)
    assert code == 0 and list(_host(rinfo)) == list(h_rinfo) == [int(h_rinfo[0]), n2]
    C = int(h_rinfo[0])
    assert 100 < C <= 200
    for dev, w in ((rkeys, "keys"), (rcount, "count"), (rsum, "sum")):
        np.testing.assert_array_equal(_host(dev)[:C], h_roll[w])
        assert (_host(dev)[C:] == 0x5a).all()
    np.testing.assert_array_equal(_host(rstarts)[:C + 1], h_roll["starts"])
    h_top = gpu.top(h_roll["keys"], h_roll["sum"], K, want=("keys", "vals"))
    np.testing.assert_array_equal(_host(tkeys), h_top[0])
    np.testing.assert_array_equal(_host(tvals), h_top[1])
    assert list(_host(tinfo)) == list(h_top[3])
    total = {}
    for keys, adds in batches:
        for k, a in zip(keys.tolist(), adds.tolist()):
            total[k >> 32] = total.get(k >> 32, 0) + a
    assert list(h_roll["keys"]) == sorted(total) and list(h_roll["sum"]) == [total[d] for d in sorted(total)]
