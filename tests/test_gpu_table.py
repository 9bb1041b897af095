"""Carrying totals across batches on the device (include/ebpf_gpu.h: ebpf_batch_lookup_dev and
ebpf_batch_accumulate_dev; csrc/hip/table.hip) against the host functions, which test_table.py
checks against a Python dict.  A sorted table has one right answer: every comparison is exact.

Shapes: T = native.STEER_TILE entries of either sequence go to one workgroup, 16 to a thread, 64 to
a wave and to a word of bits, so the lengths sit around 16, 64 and T; 513 tiles make the tile scan
cross a wave of its threads, and 1,025 tiles plus 3 entries give a thread of it two tiles to walk.
Every output buffer is pre-filled with a value no result holds and is GUARD entries longer than the
call may write; the host function gets the same buffers, so comparing them whole checks what must
not be written too.  No test feeds the device a table or keys that are not strictly ascending."""
import ctypes
import errno

import numpy as np
import pytest

from generic_ebpf_amd import native as _native
from gpu_buffers import ptr, run, up
from test_table import (FILL, GUARD, MAXU, PATTERNS, TYPES, U64, Acc, Look, Table, host_accumulate,
                        host_lookup, pattern)

pytestmark = pytest.mark.gpu

T = _native.STEER_TILE
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]
# every size on either side, crossed sparsely
PAIRS = sorted({(SIZES[i], SIZES[(5 * i + 3) % 12]) for i in range(12)} |
               {(SIZES[(7 * i + 1) % 12], SIZES[i]) for i in range(12)} |
               {(0, 0), (T, T), (2 * T + 5, 2 * T + 5), (T + 1, T - 1)})
OTHER = {"vals": 0x0123456789abcdef, "pos": 0x01234567, "keys": 0x0123456789abcdef,
         "n": 0x0123456789abcdef, "info": 0x0123456789abcdef}


class DevTable:
    """a Table's arrays on the device"""

    def __init__(self, t, skew=0):
        self.cap = t.cap
        self.keys, self.vals = up(t.keys, skew), up(t.vals, skew)
        self.n = up(np.array([t.n], dtype=U64), skew)

    def struct(self, gpu):
        return gpu.KeyTable(ptr(self.keys), ptr(self.vals), self.cap, self.n.data_ptr())


class DevLook:
    def __init__(self, c, fill=FILL, skew=False):
        self.c, self.fill = c, fill
        self.table = DevTable(c.table, 8 if skew else 0)
        self.keys = up(c.keys, 8 if skew else 0)
        self.nkeys = None if c.nkeys is None else up(np.array([c.nkeys], dtype=U64))
        self.outs = {k: up(np.full(c.cap + GUARD, fill[k], dtype=TYPES[k]),
                            (8 if k == "vals" else 4) if skew else 0) for k in c.want}

    def enqueue(self, gpu, stream):
        c = self.c
        t = self.table.struct(gpu)
        return gpu.lib().ebpf_batch_lookup_dev(
            0, ctypes.byref(t), ptr(self.keys), c.cap,
            None if self.nkeys is None else self.nkeys.data_ptr(), c.mode, c.missing, c.limit,
            self.outs["vals"].data_ptr() if "vals" in self.outs else None,
            self.outs["pos"].data_ptr() if "pos" in self.outs else None, stream.cuda_stream)

    def check(self, gpu, msg):
        code, w = host_lookup(gpu, self.c, self.fill)
        assert code == 0, msg
        got = {k: v.cpu().numpy().view(TYPES[k]) for k, v in self.outs.items()}
        for k in w:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


class DevAcc:
    def __init__(self, c, fill=FILL, skew=False):
        self.c, self.fill = c, fill
        s = 8 if skew else 0
        self.table = None if c.table is None else DevTable(c.table, s)
        self.keys, self.adds = up(c.keys, s), up(c.adds, s)
        self.nkeys = None if c.nkeys is None else up(np.array([c.nkeys], dtype=U64))
        self.outs = {"keys": up(np.full(c.out_cap + GUARD, fill["keys"], dtype=U64), s),
                     "vals": up(np.full(c.out_cap + GUARD, fill["keys"], dtype=U64), s),
                     "n": up(np.full(1 + GUARD, fill["n"], dtype=U64), s),
                     "info": up(np.full(3 + GUARD, fill["info"], dtype=U64), s)}

    def enqueue(self, gpu, stream):
        c = self.c
        tin = None if self.table is None else self.table.struct(gpu)
        cap = c.out_cap
        tout = gpu.KeyTable(self.outs["keys"].data_ptr() if cap else None,
                            self.outs["vals"].data_ptr() if cap else None, cap,
                            self.outs["n"].data_ptr())
        return gpu.lib().ebpf_batch_accumulate_dev(
            0, None if tin is None else ctypes.byref(tin), ptr(self.keys), ptr(self.adds), c.cap,
            None if self.nkeys is None else self.nkeys.data_ptr(), c.op, c.lo, c.hi,
            ctypes.byref(tout), self.outs["info"].data_ptr(), stream.cuda_stream)

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers, GUARD and all
        (a short output table: ENOSPC on the host, 0 on the device, the same bytes)"""
        code, w = host_accumulate(gpu, self.c, self.fill)
        assert code in (0, errno.ENOSPC), msg
        assert (code == errno.ENOSPC) == (int(w["n"][0]) > self.c.out_cap), msg
        got = {k: v.cpu().numpy().view(U64) for k, v in self.outs.items()}
        for k in w:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


def adds_for(r, seed=0):
    return np.random.default_rng(seed + r).integers(0, 1 << 40, r, dtype=U64)


# ---------------------------------------------------------------- shapes and key patterns

@pytest.mark.parametrize("name", PATTERNS)
def test_accumulate_shapes(gpu, name):
    cases = [(n, r) for n, r in PAIRS]
    devs = []
    for k, (n, r) in enumerate(cases):
        t, keys = pattern(name, n, r)
        # a keep band that leaves about half out on every second case
        lo, hi = ((1 << 38), (1 << 40) + (1 << 39)) if k % 2 else (0, MAXU)
        devs.append(DevAcc(Acc(t, keys, adds_for(r), op=k % 4, lo=lo, hi=hi)))
    run(gpu, devs)
    for d, (n, r) in zip(devs, cases):
        d.check(gpu, "%s n=%d r=%d" % (name, n, r))


@pytest.mark.parametrize("name", PATTERNS)
def test_lookup_shapes(gpu, name):
    g = np.random.default_rng(11)
    devs = []
    for k, (n, r) in enumerate(PAIRS):
        t, keys = pattern(name, n, r)
        if k % 3 == 1:      # any order, with repeats
            keys = g.permutation(np.concatenate([keys, keys[:r // 3]]))[:r]
        limit = [0, 1 << 39, MAXU][k % 3]
        devs.append(DevLook(Look(t, keys, mode=k % 2, missing=[0, MAXU, 77][k % 3], limit=limit,
                                 want=[("vals", "pos"), ("vals",), ("pos",)][k % 3 if k % 5 else 0])))
    run(gpu, devs)
    for d, (n, r) in zip(devs, PAIRS):
        d.check(gpu, "%s n=%d r=%d" % (name, n, r))


def test_many_tiles_on_the_table_side(gpu):
    """513 tiles of table: the tile scan crosses a wave of its threads"""
    n, r = 512 * T + 5, 2 * T + 5
    devs = []
    for name in ("random", "interleaved"):
        t, keys = pattern(name, n, r)
        devs.append(DevAcc(Acc(t, keys, adds_for(r), lo=1 << 39, hi=MAXU)))
        devs.append(DevLook(Look(t, keys, mode=1, limit=1 << 39)))
    run(gpu, devs)
    got = [d.check(gpu, "513 tiles") for d in devs]
    assert n // 3 < int(got[0]["info"][0]) < n and int(got[0]["info"][2]) > n // 3


def test_many_tiles_on_the_batch_side(gpu):
    """1,025 tiles of keys and 3 more: a thread of the tile scan walks two tiles"""
    n, r = 2 * T + 5, 1025 * T + 3
    t, keys = pattern("interleaved", n, r)
    adds = adds_for(r)
    a = DevAcc(Acc(t, keys, adds, lo=1 << 39, hi=MAXU))
    b = DevAcc(Acc(None, keys, adds, op=2, lo=0, hi=(1 << 39) - 1))
    c = DevLook(Look(t, keys, missing=5))
    run(gpu, [a, b, c])
    got = a.check(gpu, "1025 tiles")
    assert r // 3 < int(got["info"][1]) < 2 * r // 3
    got = b.check(gpu, "1025 tiles, no table")
    assert int(got["info"][0]) + int(got["info"][2]) == r
    c.check(gpu, "1025 tiles, lookup")


# ---------------------------------------------------------------- values

def test_accumulate_add_wraps_and_every_op(gpu):
    t, keys = pattern("random", 3 * T + 9, 2 * T + 1)
    t.vals = U64(MAXU) - np.arange(t.cap, dtype=U64) % U64(5000)
    adds = np.arange(len(keys), dtype=U64) * U64(3)
    devs = [DevAcc(Acc(t, keys, adds, op=op, lo=lo, hi=hi))
            for op in range(4) for lo, hi in ((0, MAXU), (0, 4000), (MAXU - 100, MAXU))]
    run(gpu, devs)
    got = [d.check(gpu, "op %d keep [%d, %d]" % (d.c.op, d.c.lo, d.c.hi)) for d in devs]
    assert 0 < int(got[1]["info"][0]) < int(got[0]["info"][0])   # (ADD wrapped into [0, 4000])


def test_keep_ranges_drop_one_kind_of_candidate(gpu):
    """only the table-only, only the batch-only, only the combined candidates left out"""
    t, keys = pattern("random", 2 * T + 77, 2 * T - 3)
    n, r = t.cap, len(keys)
    shared = int(np.isin(keys, t.keys).sum())
    assert 0 < shared < min(n, r)
    t.vals = U64(100) + np.arange(n, dtype=U64) % U64(100)
    adds = U64(300) + np.arange(r, dtype=U64) % U64(100)
    table_only = DevAcc(Acc(t, keys, adds, op=0, lo=300, hi=MAXU))
    combined = DevAcc(Acc(t, keys, adds, op=0, lo=0, hi=399))
    t2 = Table(t.keys, t.vals | U64(1 << 20))
    batch_only = DevAcc(Acc(t2, keys, adds, op=3, lo=1 << 20, hi=MAXU))
    run(gpu, [table_only, combined, batch_only])
    assert int(table_only.check(gpu, "table-only")["info"][2]) == n - shared
    assert int(combined.check(gpu, "combined")["info"][2]) == shared
    got = batch_only.check(gpu, "batch-only")
    assert int(got["info"][2]) == r - shared and int(got["info"][1]) == 0


# ---------------------------------------------------------------- the other cases

def test_output_caps(gpu):
    """caps of 0, M - 1 and M, and more"""
    devs = []
    for n, r in ((T + 1, 65), (300, 2 * T + 5), (0, 17), (17, 0)):
        t, keys = pattern("random", n, r)
        c = Acc(t, keys, adds_for(r), lo=1 << 37, hi=MAXU)
        M = int(host_accumulate(gpu, c)[1]["n"][0])
        assert 0 < M <= n + r
        for cap in (0, 1, M - 1, M, M + 1):
            devs.append(DevAcc(Acc(t, keys, c.adds, lo=c.lo, hi=c.hi, out_cap=cap)))
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "n=%d r=%d cap=%d" % (d.c.table.cap, d.c.cap, d.c.out_cap))


def test_unaligned_buffers(gpu):
    """every array 8 bytes past a 16-byte boundary, pos 4 bytes"""
    devs = []
    for n, r in ((257, 63), (T + 1, 2 * T + 5)):
        for name in ("random", "words"):
            t, keys = pattern(name, n, r)
            devs.append(DevAcc(Acc(t, keys, adds_for(r), lo=1 << 38), skew=True))
            devs.append(DevLook(Look(t, keys, mode=1, limit=1 << 39), skew=True))
    for d in devs:
        assert d.keys.data_ptr() % 16 == 8 and d.table.keys.data_ptr() % 16 == 8
        assert d.outs["vals"].data_ptr() % 16 == 8
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "skewed")


def test_prune_no_table_and_short_input_table(gpu):
    t, keys = pattern("random", T + 9, 300)
    adds = adds_for(300)
    devs = [DevAcc(Acc(t, keys, adds, nkeys=0, lo=1 << 39)),            # R = 0 by *nkeys
            DevAcc(Acc(t, [], [], lo=1 << 39)),                         # R = 0 by key_cap
            DevAcc(Acc(None, keys, adds)), DevAcc(Acc(None, [], [])),   # `in` NULL
            DevAcc(Acc(Table(), keys, adds)),
            DevLook(Look(Table(), keys, missing=9)), DevLook(Look(t, []))]
    for n in (0, 1, T, T + 8, T + 9, T + 10, 1 << 50):                 # *n around and past cap
        short = Table(t.keys, t.vals, n=n)
        devs += [DevAcc(Acc(short, keys, adds)), DevLook(Look(short, keys, missing=9))]
    for nkeys in (0, 1, 299, 300, 301, 1 << 40):                       # the three cases of R
        devs += [DevAcc(Acc(t, keys, adds, nkeys=nkeys)), DevLook(Look(t, keys, nkeys=nkeys))]
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "n=%s nkeys=%s" % (d.c.table.n if d.c.table else None, d.c.nkeys))


def test_ignores_what_the_outputs_held(gpu):
    t, keys = pattern("random", 3 * T + 1, 2 * T + 9)
    c = Acc(t, keys, adds_for(len(keys)), lo=1 << 38, out_cap=2 * T)   # (a short output table)
    lk = Look(t, keys, mode=1, limit=1 << 39)
    devs = [DevAcc(c, FILL), DevAcc(c, OTHER), DevLook(lk, FILL), DevLook(lk, OTHER)]
    run(gpu, devs)
    a, b, p, q = [d.check(gpu, "fill") for d in devs]
    m = min(int(a["n"][0]), c.out_cap)
    assert m == c.out_cap
    for k in ("keys", "vals"):
        assert a[k][:m].tobytes() == b[k][:m].tobytes() and (b[k][m:] == OTHER["keys"]).all()
    assert a["info"][:3].tobytes() == b["info"][:3].tobytes()
    for k in ("vals", "pos"):
        assert p[k][:lk.cap].tobytes() == q[k][:lk.cap].tobytes()


def test_two_streams_keep_their_scratch_apart(gpu):
    import torch
    cs = []
    for s in (1, 2):
        t, keys = pattern("random", 20 * T + 9, 9 * T + 1, seed=s)
        cs.append(Acc(t, keys, adds_for(len(keys), s), lo=1 << 39))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [[DevAcc(c) for _ in range(4)] for c in cs]
    torch.cuda.synchronize()
    for r in range(4):
        for s in (0, 1):
            assert devs[s][r].enqueue(gpu, streams[s]) == 0
    torch.cuda.synchronize()
    for s in (0, 1):
        for d in devs[s]:
            d.check(gpu, "stream %d" % s)


def test_device_argument_errors(gpu):
    """known on the host, before the device is looked at; then ENODEV"""
    L = gpu.lib()
    t = gpu.KeyTable(16, 16, 4, 16)
    bad = gpu.KeyTable(16, None, 4, 16)
    big = gpu.KeyTable(16, 16, 1 << 32, 16)
    E, B = errno.EINVAL, errno.E2BIG
    assert L.ebpf_batch_lookup_dev(0, None, 16, 4, None, 0, 0, 0, 16, None, None) == E
    assert L.ebpf_batch_lookup_dev(0, ctypes.byref(t), 16, 4, None, 2, 0, 0, 16, None, None) == E
    assert L.ebpf_batch_lookup_dev(0, ctypes.byref(t), None, 4, None, 0, 0, 0, 16, None, None) == E
    assert L.ebpf_batch_lookup_dev(0, ctypes.byref(bad), 16, 4, None, 0, 0, 0, 16, None, None) == E
    assert L.ebpf_batch_lookup_dev(0, ctypes.byref(big), 16, 4, None, 0, 0, 0, 16, None, None) == B
    assert L.ebpf_batch_lookup_dev(0, ctypes.byref(t), 16, 1 << 32, None, 0, 0, 0, 16, None, None) == B
    assert L.ebpf_batch_lookup_dev(99, ctypes.byref(t), 16, 4, None, 0, 0, 0, 16, None, None) == errno.ENODEV

    def acc(tin=t, keys=16, adds=16, cap=4, op=0, tout=t, info=16, dev=0):
        return L.ebpf_batch_accumulate_dev(dev, None if tin is None else ctypes.byref(tin), keys,
                                           adds, cap, None, op, 0, MAXU,
                                           None if tout is None else ctypes.byref(tout), info, None)
    assert acc(tout=None) == E and acc(info=None) == E and acc(op=4) == E
    assert acc(keys=None) == E and acc(adds=None) == E and acc(tin=bad) == E and acc(tout=bad) == E
    assert acc(tin=big) == B and acc(tout=big) == B and acc(cap=1 << 32) == B
    assert acc(tin=big, op=4) == E
    assert acc(dev=99) == errno.ENODEV and acc(tin=None, dev=99) == errno.ENODEV


# ---------------------------------------------------------------- two batches, on one stream

QUOTA = 2000
FLOWS = 300


def _batch(seed, count, flows):
    """packets of 40 .. 64 bytes whose word at byte 12 is the flow"""
    g = np.random.default_rng(seed)
    flow = g.choice(flows, count).astype(np.uint32)
    lens = (40 + g.integers(0, 25, count)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    data = g.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    for k in range(4):
        data[offsets[:-1].astype(np.int64) + 12 + k] = (flow >> (8 * k)) & 0xff
    return flow, lens, offsets, data


def test_quota_across_two_batches_on_one_stream(gpu, env):
    """group -> reduce(bytes) -> lookup REMAINING -> scan(over) -> filter -> reduce(bytes of the
    kept list) -> accumulate ADD, the tables swapped between the batches, nothing read in between:
    the table and both batches' `over` equal a per-packet simulation of the quota, and the second
    batch's budgets are what the first one left"""
    import torch
    from generic_ebpf_amd import workloads
    from generic_ebpf_amd.workloads import I, R0, R1
    g = np.random.default_rng(21)
    ids = np.unique(g.integers(1, 1 << 32, FLOWS + 50, dtype=np.uint64))[:FLOWS].astype(np.uint32)
    g.shuffle(ids)
    # flows 0 .. 199 in the first batch, 100 .. 299 in the second: 100 in both
    batches = [_batch(1, 3 * T // 2 + 11, ids[:200]), _batch(2, T + 301, ids[100:])]
    lay = workloads.assemble([I("ldxw", R0, R1, 12), I("exit")])
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    cap = 256        # (flows per batch: at most 200)
    tcap = 512

    def z(k, dtype, fill=0):
        return torch.full((k,), fill, dtype=dtype, device=dev)
    tables = [[z(tcap, torch.int64, 0x5a), z(tcap, torch.int64, 0x5a), z(1, torch.int64)]
              for _ in range(2)]
    runs = []
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        for b, (flow, lens, offsets, data) in enumerate(batches):
            n = len(flow)
            d_data, d_offs = up(data), up(offsets)
            ret, flt = z(n, torch.int64, -1), z(n, torch.uint8)
            index, gkeys, gstarts = z(n, torch.int32, -1), z(cap, torch.int64), z(cap + 1, torch.int64)
            info, kd, tinfo = z(2, torch.int64), z(2, torch.int64), z(3, torch.int64)
            tmp_bytes = gpu.group_tmp_bytes(n, 32)
            tmp = z(max(tmp_bytes, 8), torch.uint8)
            gbytes, kbytes, budgets = (z(cap, torch.int64, 0x5a) for _ in range(3))
            over, kept, ks = z(n, torch.uint8, 0x5a), z(n, torch.int32), z(cap + 1, torch.int64)
            cur, nxt = tables[b % 2], tables[1 - b % 2]
            p.run_batch_dev(0, d_data.data_ptr(), n, 0, ret.data_ptr(), d_offs.data_ptr(),
                            flt.data_ptr(), None, st)
            gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), n, 0, 32, index.data_ptr(), cap,
                          gkeys.data_ptr(), gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(),
                          tmp_bytes, st)
            gpu.reduce_dev(0, None, n, 0, 0, index.data_ptr(), n, gstarts.data_ptr(), cap,
                           info.data_ptr(), bytes_ptr=gbytes.data_ptr(),
                           offsets_ptr=d_offs.data_ptr(), stream=st)
            gpu.lookup_dev(0, cur[0].data_ptr(), cur[1].data_ptr(), tcap, cur[2].data_ptr(),
                           gkeys.data_ptr(), cap, info.data_ptr(), gpu.LOOKUP_REMAINING, 0, QUOTA,
                           vals_out_ptr=budgets.data_ptr(), stream=st)
            gpu.scan_dev(0, None, n, 0, 0, index.data_ptr(), n, gstarts.data_ptr(), cap,
                         info.data_ptr(), budgets.data_ptr(), over_ptr=over.data_ptr(),
                         offsets_ptr=d_offs.data_ptr(), stream=st)
            gpu.filter_dev(0, n, index.data_ptr(), n, gstarts.data_ptr(), cap, kd.data_ptr(),
                           nseg_ptr=info.data_ptr(), flags_ptr=over.data_ptr(),
                           kept_ptr=kept.data_ptr(), kept_starts_ptr=ks.data_ptr(), stream=st)
            gpu.reduce_dev(0, None, n, 0, 0, kept.data_ptr(), n, ks.data_ptr(), cap,
                           info.data_ptr(), bytes_ptr=kbytes.data_ptr(),
                           offsets_ptr=d_offs.data_ptr(), stream=st)
            gpu.accumulate_dev(0, (cur[0].data_ptr(), cur[1].data_ptr(), tcap, cur[2].data_ptr()),
                               gkeys.data_ptr(), kbytes.data_ptr(), cap,
                               (nxt[0].data_ptr(), nxt[1].data_ptr(), tcap, nxt[2].data_ptr()),
                               tinfo.data_ptr(), nkeys_ptr=info.data_ptr(), op=gpu.ACC_ADD,
                               stream=st)
            runs.append((ret, index, info, gkeys, gbytes, budgets, over, tinfo, d_data, d_offs,
                         flt, gstarts, kd, tmp, kbytes, kept, ks))   # (all alive to the end)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    # the same quota, packet by packet
    used = {}
    for b, (flow, lens, offsets, data) in enumerate(batches):
        ret, index, info, gkeys, gbytes, budgets, over, tinfo = [x.cpu().numpy() for x in runs[b][:8]]
        np.testing.assert_array_equal(ret.view(U64), flow.astype(U64))
        left = {int(f): max(QUOTA - used.get(int(f), 0), 0) for f in np.unique(flow)}
        seen, sent, w_over = {}, {}, np.zeros(len(flow), dtype=np.uint8)
        for i, (f, n) in enumerate(zip(flow.tolist(), lens.tolist())):
            seen[f] = seen.get(f, 0) + n
            sent.setdefault(f, 0)
            if seen[f] > left[f]:
                w_over[i] = 1
            else:
                sent[f] += n
        G = int(info.view(U64)[0])
        assert G == len(left) == 200
        np.testing.assert_array_equal(gkeys.view(U64)[:G], u64_sorted(left))
        np.testing.assert_array_equal(budgets.view(U64)[:G], [left[f] for f in sorted(left)])
        np.testing.assert_array_equal(gbytes.view(U64)[:G], [seen[f] for f in sorted(left)])
        assert (budgets.view(U64)[G:] == 0x5a).all()
        got_over = np.zeros(len(flow), dtype=np.uint8)
        got_over[index.view(np.uint32)] = over
        np.testing.assert_array_equal(got_over, w_over)
        assert 0 < w_over.sum() < len(flow)
        new = sum(1 for f in sent if f not in used)
        for f, v in sent.items():
            used[f] = used.get(f, 0) + v
        assert list(tinfo.view(U64)) == [len(used), new, 0]
        if b == 1:   # what the first batch used shows in the second one's budgets
            both = [f for f in left if left[f] < QUOTA]
            assert len(both) == 100 and min(left[f] for f in both) < QUOTA // 4
    final = tables[0]    # (two swaps)
    keys, vals, n = [x.cpu().numpy().view(U64) for x in final]
    assert int(n[0]) == len(used) == FLOWS
    np.testing.assert_array_equal(keys[:FLOWS], u64_sorted(used))
    np.testing.assert_array_equal(vals[:FLOWS], [used[f] for f in sorted(used)])
    assert (keys[FLOWS:] == 0x5a).all() and max(used.values()) <= QUOTA


def u64_sorted(d):
    return np.array(sorted(d), dtype=U64)
