"""The heaviest entries on the device (include/ebpf_gpu.h: ebpf_batch_top_dev; csrc/hip/top.hip)
against the host function, which test_top.py checks against a Python sort.  The order is total:
every comparison is exact.

Shapes: T = native.STEER_TILE entries go to one workgroup, 16 to a thread, 64 to a wave and to a
ballot, and k is at most T, so N and k sit around 16, 64 and T; 513 tiles make the tile scan cross a
wave of its threads, and 1,025 tiles plus 3 entries give a thread of it two tiles to walk and a
histogram row two tiles.  Every output buffer is pre-filled with a value no result holds and is
GUARD entries longer than the call may write; the host function gets the same buffers, so comparing
them whole checks what must not be written too."""
import ctypes
import errno

import numpy as np
import pytest

from generic_ebpf_amd import native as _native
from gpu_buffers import ptr, run, up
from test_top import (ALL, FIELDS, FILL, GUARD, LARGEST, MAXU, PATTERNS, SEGMENTS, SMALLEST, TYPES,
                      U64, Top, host_top, values)

pytestmark = pytest.mark.gpu

T = _native.STEER_TILE
SIZES = [0, 1, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5]
KS = [0, 1, 63, 64, 65, T - 1, T]
# every N and every k, crossed sparsely
PAIRS = sorted({(SIZES[i], KS[(5 * i + 3) % 7]) for i in range(12)} |
               {(SIZES[(7 * i + 1) % 12], KS[i % 7]) for i in range(14)} |
               {(0, 0), (T, T), (2 * T + 5, T), (T + 1, T - 1), (T - 1, T), (2 * T + 5, 1)})
OTHER = {"keys": 0x0123456789abcdef, "vals": 0x0123456789abcdef, "pos": 0x01234567,
         "info": 0x0123456789abcdef}


class DevTop:
    """a Top's arrays and outputs on the device"""

    def __init__(self, c, fill=FILL, skew=False):
        self.c, self.fill = c, fill
        s = 8 if skew else 0
        self.keys = None if c.keys is None else up(c.keys, s)
        self.vals = up(c.vals, s)
        self.n = None if c.n is None else up(np.array([c.n], dtype=U64), s)
        self.outs = {w: up(np.full(c.k + GUARD, fill[w], dtype=TYPES[w]),
                            (4 if w == "pos" else 8) if skew else 0) for w in c.want}
        self.outs["info"] = up(np.full(4 + GUARD, fill["info"], dtype=U64), s)

    def enqueue(self, gpu, stream):
        c = self.c
        tops = gpu.BatchTops(*[self.outs[w].data_ptr() if w in c.want else None for w in ALL])
        return gpu.lib().ebpf_batch_top_dev(
            0, None if self.keys is None else self.keys.data_ptr() or 16, ptr(self.vals), c.cap,
            None if self.n is None else self.n.data_ptr(), c.flags, c.field[0], c.field[1], c.k,
            ctypes.byref(tops), self.outs["info"].data_ptr(), stream.cuda_stream)

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers, GUARD and all"""
        code, w = host_top(gpu, self.c, self.fill)
        assert code == 0, msg
        got = {k: v.cpu().numpy().view(TYPES[k]) for k, v in self.outs.items()}
        for k in w:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


def check_all(gpu, devs):
    run(gpu, devs)
    return [d.check(gpu, "cap=%d n=%s k=%d flags=%d field=%s" % (d.c.cap, d.c.n, d.c.k, d.c.flags,
                                                                 d.c.field)) for d in devs]


# ---------------------------------------------------------------- shapes, orders, fields

@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
@pytest.mark.parametrize("field", FIELDS)
def test_shapes_orders_and_fields(gpu, flags, field):
    devs = []
    for i, (n, k) in enumerate(PAIRS):
        devs.append(DevTop(Top(values(("random64", "random40")[i % 2], n, field, seed=i), k, flags,
                               field)))
    check_all(gpu, devs)


@pytest.mark.parametrize("name", PATTERNS)
def test_value_patterns(gpu, name):
    devs = []
    for i, (n, k) in enumerate(PAIRS):
        field = FIELDS[i % len(FIELDS)]
        devs.append(DevTop(Top(values(name, n, field, seed=i), k, i % 2, field)))
    check_all(gpu, devs)


@pytest.mark.parametrize("flags", [LARGEST, SMALLEST])
def test_two_values_with_the_boundary_inside_a_tile_and_on_its_edge(gpu, flags):
    """the better value from `edge` on: the taken entries begin there, and, for k past their
    number, go on from position 0"""
    n = 3 * T + 9
    devs = []
    for edge in (T, 2 * T, T + 700, 2 * T - 1, 2 * T + 1, 0, n):
        v = np.full(n, 5 << 30, dtype=U64)
        v[edge:] = (3 << 30) if flags else (9 << 30)
        for k in (1, 64, T - 1, T):
            devs.append(DevTop(Top(v, k, flags, (24, 16))))
    got = check_all(gpu, devs)
    assert int(got[3]["pos"][0]) == T and int(got[3]["pos"][T - 1]) == 2 * T - 1
    assert int(got[11]["pos"][0]) == T + 700


def test_sparse_ties(gpu):
    """the cut's value at every 1,000th position of 3T + 9, a few entries better and everything
    else worse: with e > 1 the equal entries taken lie in different tiles"""
    n = 3 * T + 9
    g = np.random.default_rng(5)
    v = g.integers(0, 1 << 20, n, dtype=U64)               # not taken
    best = g.permutation(n)[:40]
    best = best[best % 1000 != 0]
    v[best] = U64(1 << 50) + g.integers(0, 99, len(best), dtype=U64)
    v[::1000] = U64(1 << 40)                               # the cut: 13 of them, over 3 tiles
    extras = (0, 1, 2, 5, 9, 12, 13, 14)
    devs = [DevTop(Top(v, len(best) + e, LARGEST)) for e in extras]
    devs += [DevTop(Top(U64(MAXU) - v, len(best) + e, SMALLEST)) for e in extras]
    got = check_all(gpu, devs)
    for r in (got[4], got[12]):                            # e = 9, from tiles 0 and 1 (and 2: e = 12)
        m = int(r["info"][0])
        assert int(r["info"][3]) == 4 and list(r["pos"][m - 9:m]) == [1000 * j for j in range(9)]
    assert 8000 // T == 1 and 12000 // T == 2 and int(got[4]["info"][2]) == 1 << 40


# ---------------------------------------------------------------- many tiles

def _many(gpu, n):
    devs = []
    for flags in (LARGEST, SMALLEST):
        devs.append(DevTop(Top(values("random64", n), T, flags)))
        devs.append(DevTop(Top(values("random40", n), 65, flags, (0, 40), want=("pos",), keys=None)))
        devs.append(DevTop(Top(values("equal", n), T, flags, want=("pos",), keys=None)))
    got = check_all(gpu, devs)
    for r in (got[2], got[5]):      # all equal: only the first tile is taken
        assert list(r["pos"][:T]) == list(range(T)) and int(r["info"][3]) == n - T


def test_513_tiles(gpu):
    """the tile scan crosses a wave of its threads"""
    _many(gpu, 512 * T + 5)


def test_1025_tiles(gpu):
    """a thread of the tile scan walks two tiles, and a histogram row has two tiles"""
    _many(gpu, 1025 * T + 3)


# ---------------------------------------------------------------- the other cases

@pytest.mark.parametrize("flags", [LARGEST, SEGMENTS, SMALLEST | SEGMENTS])
def test_n_under_both_counting_rules(gpu, flags):
    devs = []
    for cap in (0, 1, 300, T + 9):
        v = values("random40", cap)
        for n in (None, 0, 1, cap - 1, cap, cap + 1, 1 << 50):
            if n is None or n >= 0:
                devs += [DevTop(Top(v, k, flags, (0, 40), n=n)) for k in (0, 7, T)]
    got = check_all(gpu, devs)
    assert {int(r["info"][1]) for r in got} >= {0, 1, 299, 300, T + 8, T + 9}


def test_unaligned_buffers(gpu):
    """every array 8 bytes past a 16-byte boundary, pos 4 bytes"""
    devs = [DevTop(Top(values("random64", n), k, flags, n=n - 1), skew=True)
            for n, k in ((257, 63), (T + 1, T), (2 * T + 5, 65)) for flags in (0, 1)]
    for d in devs:
        assert d.vals.data_ptr() % 16 == 8 and d.keys.data_ptr() % 16 == 8
        assert d.outs["vals"].data_ptr() % 16 == 8 and d.outs["pos"].data_ptr() % 16 == 4
    check_all(gpu, devs)


@pytest.mark.parametrize("want", [("vals", "pos"), ("keys", "pos"), ("keys", "vals"), ("pos",), ()])
def test_each_output_absent(gpu, want):
    devs = []
    for n, k in ((300, 64), (2 * T + 5, T), (T, 0)):
        v = values("outside", n, (8, 24))
        devs.append(DevTop(Top(v, k, LARGEST, (8, 24), want=want)))
        devs.append(DevTop(Top(v, k, SMALLEST, (8, 24), want=want,
                               keys=None if "keys" not in want else "ramp")))
    check_all(gpu, devs)


def test_ignores_what_the_outputs_held(gpu):
    c = Top(values("outside", 3 * T + 1, (0, 9)), T - 100, SMALLEST, (0, 9))
    devs = [DevTop(c, FILL), DevTop(c, OTHER)]
    a, b = check_all(gpu, devs)
    m = c.m
    assert m == T - 100 and int(a["info"][3]) > 0
    for w in ALL:
        assert a[w][:m].tobytes() == b[w][:m].tobytes() and (b[w][m:] == OTHER[w]).all()
    assert a["info"][:4].tobytes() == b["info"][:4].tobytes()


def test_two_streams_keep_their_scratch_apart(gpu):
    import torch
    cs = [Top(values("random40", 20 * T + 9, seed=s), T - s, s - 1, (0, 40)) for s in (1, 2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [[DevTop(c) for _ in range(4)] for c in cs]
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
    E, B = errno.EINVAL, errno.E2BIG
    tops = gpu.BatchTops(16, 16, 16)
    nokeys = gpu.BatchTops(None, 16, 16)

    def top(keys=16, vals=16, cap=4, flags=0, shift=0, bits=64, k=2, out=tops, info=16, dev=0):
        return L.ebpf_batch_top_dev(dev, keys, vals, cap, None, flags, shift, bits, k,
                                    None if out is None else ctypes.byref(out), info, None)
    assert top(out=None) == E and top(info=None) == E and top(flags=4) == E
    assert top(bits=0) == E and top(shift=1, bits=64) == E and top(vals=None) == E
    assert top(keys=None) == E
    assert top(cap=1 << 32) == B and top(k=T + 1) == B
    assert top(cap=1 << 32, flags=8) == E and top(k=T + 1, keys=None) == E
    assert top(dev=99) == errno.ENODEV and top(dev=99, keys=None, out=nokeys) == errno.ENODEV
    assert top(dev=99, vals=None, cap=0, k=0) == errno.ENODEV


# ---------------------------------------------------------------- two batches, on one stream

FLOWS = 300


def _batch(seed, count, flows):
    """packets of 40, 48, 56 or 64 bytes whose word at byte 12 is the flow"""
    g = np.random.default_rng(seed)
    flow = g.choice(flows, count).astype(np.uint32)
    lens = (40 + 8 * g.integers(0, 4, count)).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    data = g.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    for k in range(4):
        data[offsets[:-1].astype(np.int64) + 12 + k] = (flow >> (8 * k)) & 0xff
    return flow, lens, offsets, data


def _best(totals, k, smallest=False):
    """(keys, vals, the cut's ties left out) of the k best of {key: total}: ties by key"""
    order = sorted(totals, key=lambda f: (totals[f] if smallest else -totals[f], f))
    cut = totals[order[k - 1]]
    return ([f for f in order[:k]], [totals[f] for f in order[:k]],
            sum(1 for f in order[k:] if totals[f] == cut))


def pipeline_batches():
    g = np.random.default_rng(21)
    ids = np.unique(g.integers(1, 1 << 32, FLOWS + 50, dtype=np.uint64))[:FLOWS].astype(np.uint32)
    g.shuffle(ids)
    # flows 0 .. 199 in the first batch, 100 .. 299 in the second: 100 in both
    return [_batch(1, 3 * T // 2 + 11, ids[:200]), _batch(2, T + 301, ids[100:])]


def test_heaviest_flows_of_two_batches_on_one_stream(gpu, env):
    """per batch group -> reduce(bytes) -> top (the batch's 10 heaviest flows, counted by the
    reduce's rule) -> accumulate ADD, the tables swapped between the batches, then the table's 10
    largest and 10 smallest, nothing read in between: all equal a per-packet simulation"""
    import torch
    from generic_ebpf_amd import workloads
    from generic_ebpf_amd.workloads import I, R0, R1
    batches = pipeline_batches()
    lay = workloads.assemble([I("ldxw", R0, R1, 12), I("exit")])
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    cap, tcap, K = 256, 512, 10

    def z(k, dtype, fill=0):
        return torch.full((k,), fill, dtype=dtype, device=dev)

    def tops():
        return z(K, torch.int64, 0x5a), z(K, torch.int64, 0x5a), z(K, torch.int32, 0x5a), z(4, torch.int64)
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
            info, tinfo = z(2, torch.int64), z(3, torch.int64)
            tmp_bytes = gpu.group_tmp_bytes(n, 32)
            tmp = z(max(tmp_bytes, 8), torch.uint8)
            gbytes = z(cap, torch.int64, 0x5a)
            best = tops()
            cur, nxt = tables[b % 2], tables[1 - b % 2]
            p.run_batch_dev(0, d_data.data_ptr(), n, 0, ret.data_ptr(), d_offs.data_ptr(),
                            flt.data_ptr(), None, st)
            gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), n, 0, 32, index.data_ptr(), cap,
                          gkeys.data_ptr(), gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(),
                          tmp_bytes, st)
            gpu.reduce_dev(0, None, n, 0, 0, index.data_ptr(), n, gstarts.data_ptr(), cap,
                           info.data_ptr(), bytes_ptr=gbytes.data_ptr(),
                           offsets_ptr=d_offs.data_ptr(), stream=st)
            gpu.top_dev(0, gkeys.data_ptr(), gbytes.data_ptr(), cap, info.data_ptr(), K,
                        best[3].data_ptr(), gpu.TOP_SEGMENTS, keys_out_ptr=best[0].data_ptr(),
                        vals_out_ptr=best[1].data_ptr(), pos_out_ptr=best[2].data_ptr(), stream=st)
            gpu.accumulate_dev(0, (cur[0].data_ptr(), cur[1].data_ptr(), tcap, cur[2].data_ptr()),
                               gkeys.data_ptr(), gbytes.data_ptr(), cap,
                               (nxt[0].data_ptr(), nxt[1].data_ptr(), tcap, nxt[2].data_ptr()),
                               tinfo.data_ptr(), nkeys_ptr=info.data_ptr(), op=gpu.ACC_ADD,
                               stream=st)
            runs.append((best, tinfo, ret, index, info, gkeys, gbytes, d_data, d_offs, flt, gstarts,
                         tmp))   # (all alive to the end)
        final = tables[0]    # (two swaps)
        ends = []
        for flags in (gpu.TOP_LARGEST, gpu.TOP_SMALLEST):
            best = tops()
            gpu.top_dev(0, final[0].data_ptr(), final[1].data_ptr(), tcap, final[2].data_ptr(), K,
                        best[3].data_ptr(), flags, keys_out_ptr=best[0].data_ptr(),
                        vals_out_ptr=best[1].data_ptr(), pos_out_ptr=best[2].data_ptr(), stream=st)
            ends.append(best)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    # the same, packet by packet
    total, ties = {}, 0
    for b, (flow, lens, offsets, data) in enumerate(batches):
        seen = {}
        for f, n in zip(flow.tolist(), lens.tolist()):
            seen[f] = seen.get(f, 0) + n
            total[f] = total.get(f, 0) + n
        keys, vals, pos, info = [x.cpu().numpy() for x in runs[b][0]]
        wk, wv, wt = _best(seen, K)
        assert list(keys.view(U64)) == wk and list(vals.view(U64)) == wv
        assert list(pos.view(np.uint32)) == [sorted(seen).index(f) for f in wk]
        assert list(info.view(U64)) == [K, len(seen), wv[-1], wt] and len(seen) == 200
        assert list(runs[b][1].cpu().numpy().view(U64)) == [len(total), len(total) - 200 * b, 0]
        ties += wt
    assert len(total) == FLOWS
    for smallest, best in enumerate(ends):
        keys, vals, pos, info = [x.cpu().numpy() for x in best]
        wk, wv, wt = _best(total, K, smallest)
        assert list(keys.view(U64)) == wk and list(vals.view(U64)) == wv
        assert list(pos.view(np.uint32)) == [sorted(total).index(f) for f in wk]
        assert list(info.view(U64)) == [K, FLOWS, wv[-1], wt]
        ties += wt
    assert ties > 0      # (a tie fell on a cut)
