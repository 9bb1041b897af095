"""Keeping part of a list on the device (include/ebpf_gpu.h: ebpf_batch_filter_dev;
csrc/hip/filter.hip) against the host function, which test_filter.py checks against numpy; the
shapes come from test_reduce.py.  A stable compaction has one right answer: every comparison is
exact.

Shapes: T = native.STEER_TILE list positions go to one workgroup, 16 consecutive ones to a thread,
64 threads to a wave, so the list lengths sit around 16, 64, 256 and T and the runs of 63, 64, 4095
and T drift against, and sit on, every one of those edges; m singletons and then one long segment
put hundreds and thousands of table entries into one tile, many_empty thousands at the end of the
cover; 2M + 5 entries (513 tiles) make the tile scan cross a wave of its threads, and 1,025 tiles
plus 3 entries give a thread of it two tiles to walk.  Every output buffer is pre-filled with a
value no result holds and is GUARD entries longer than the call may write; the host function gets
the same buffers, so comparing them whole checks the EBPF_NO_PACKET tails, the table entries past R
and the guard too.  No test feeds a table that is not non-decreasing or that ends past the list."""
import ctypes

import numpy as np
import pytest

import pyoracle
from gpu_buffers import run, up
from test_reduce import BIG, COUNTS, GUARD, MID, SEGMENTATIONS, T, U64, list_of
from test_filter import (FILL, KINDS, NO_PACKET, PARTS, TYPES, WANTS, Case, host, shaped, vector)

pytestmark = pytest.mark.gpu

OTHER = {"kept": 0x01234567, "kept_starts": 0x0123456789abcdef, "dropped": 0x01234567,
         "dropped_starts": 0x0123456789abcdef, "info": 0x0123456789abcdef}
# the patterns that stress the compaction: all, none, one per tile at its last position, one per
# wave, half and one in a hundred at random
PATTERNS = ["flags_all", "flags_none", "flags_tile_last", "flags_wave", "flags_half", "flags_1pct"]


class Dev:
    """one filter call's device buffers; outputs pre-filled with `fill`.  skew: the lists start
    4 bytes, the tables 8 bytes and the flags 1 byte past a 16-byte boundary"""

    def __init__(self, c, fill=FILL, skew=False):
        self.c, self.fill = c, fill
        self.index = up(c.index)
        self.starts = None if c.seg_starts is None else up(c.seg_starts)
        self.nseg = None if c.nseg is None else up(np.array([c.nseg], dtype=U64))
        self.flags = None if c.flags is None else up(c.flags, 1 if skew else 0)
        self.rank = None if c.rank is None else up(c.rank, 4 if skew else 0)
        # (a batch of no packets still names a ret where values are tested: one unused word)
        self.ret = None if c.ret is None else up(c.ret if len(c.ret) else np.zeros(1, U64))
        self.outs = {k: up(np.full(c.size(k) + GUARD, fill[k], dtype=TYPES[k]),
                            (TYPES[k]().itemsize if skew else 0))
                     for k in c.want + ("info",)}

    def enqueue(self, gpu, stream):
        c = self.c
        test = c.test(gpu, *[None if a is None else a.data_ptr()
                             for a in (self.flags, self.rank, self.ret)])
        parts = gpu.BatchParts(*[self.outs[k].data_ptr() if k in self.outs else None
                                 for k in PARTS])
        return gpu.lib().ebpf_batch_filter_dev(
            0, ctypes.byref(test), c.count, self.index.data_ptr() if c.n else None, c.n,
            None if self.starts is None else self.starts.data_ptr(), c.cap,
            None if self.nseg is None else self.nseg.data_ptr(), ctypes.byref(parts),
            self.outs["info"].data_ptr(), stream.cuda_stream)

    def result(self):
        return {k: v.cpu().numpy().view(TYPES[k]) for k, v in self.outs.items()}

    def check(self, gpu, msg):
        """the whole contract: what the host function leaves in the same buffers, GUARD and all"""
        code, w = host(gpu, self.c, self.fill)
        assert code == 0, msg
        got = self.result()
        for k in w:
            np.testing.assert_array_equal(got[k], w[k], err_msg="%s: %s" % (msg, k))
        return got


@pytest.mark.parametrize("n", sorted(set(COUNTS + [15, 16, 17])))
def test_filter_shapes(gpu, n):
    cases = [(seg, unc) for seg in list(SEGMENTATIONS) + [None] for unc in (False, True)]
    devs = [Dev(shaped(n, seg, unc, KINDS[(k + n) % len(KINDS)], WANTS[k % len(WANTS)]))
            for k, (seg, unc) in enumerate(cases)]
    run(gpu, devs)
    for d, (seg, unc) in zip(devs, cases):
        d.check(gpu, "%s n=%d uncovered=%s" % (seg, n, unc))


@pytest.mark.parametrize("kind", KINDS)
def test_filter_vectors(gpu, kind):
    """every test vector, over three tiles and a bit"""
    devs = [Dev(shaped(MID, seg, True, kind)) for seg in ("random", "runs63", "steering", None)]
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, kind)
        assert int(got["info"][0] + got["info"][1]) == (MID if d.c.seg_starts is None else MID - 12)


def test_filter_many_segments_begin_in_a_tile(gpu):
    """m one-entry segments and then one long one; shifted by 5 positions they drift against the
    threads' 16 positions"""
    n = T + 100
    count = n - 50
    cases = [(m, a) for m in (255, 256, 257, 2047, 2048, 2049, T - 6) for a in (0, 5)]
    devs = []
    for k, (m, a) in enumerate(cases):
        starts = np.concatenate([np.arange(m + 1), [n - a]]).astype(U64) + U64(a)
        devs.append(Dev(Case(list_of(n, count, m), starts, count,
                             **vector(PATTERNS[2 + k % 4] if k % 3 else "all_half", n, count))))
    run(gpu, devs)
    for d, (m, a) in zip(devs, cases):
        d.check(gpu, "%d singletons from position %d" % (m, a))


def test_filter_many_empty_segments_at_the_end_of_the_cover(gpu):
    devs = [Dev(shaped(n, "many_empty", unc, kind)) for n in (MID, T, T + 1)
            for unc in (False, True) for kind in ("flags_half", "rank1")]
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "many_empty n=%d" % d.c.n)


@pytest.mark.parametrize("seg", ["whole", "runs4095"])
def test_filter_many_tiles(gpu, seg):
    """513 tiles: one segment over all of them, and one tile edge in every run of 4095; every
    pattern that stresses the compaction"""
    devs = [Dev(shaped(BIG, seg, seg == "whole", kind)) for kind in PATTERNS]
    run(gpu, devs)
    for d, kind in zip(devs, PATTERNS):
        got = d.check(gpu, "%s %s" % (seg, kind))
        if kind == "flags_tile_last":
            assert int(got["info"][0]) == (BIG - (7 if seg == "whole" else 0)) // T


def test_filter_carry_walks_two_tiles_a_thread(gpu):
    """past 1,024 tiles a thread of the tile scan walks more than one"""
    n = 1025 * T + 3
    devs = [Dev(shaped(n, "runs4095", False, "flags_half", ("kept", "kept_starts"))),
            Dev(shaped(n, "whole", True, "flags_tile_last")),
            Dev(shaped(n, None, False, "val8", ("dropped",)))]
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "1025 tiles")
    assert n // 3 < int(got["info"][1]) < 2 * n // 3


def test_filter_unaligned_buffers(gpu):
    """lists 4 bytes, tables 8 bytes and flags 1 byte past a 16-byte boundary"""
    devs = [Dev(shaped(n, seg, True, kind), skew=True) for n in (257, MID)
            for seg in ("runs63", "random") for kind in ("flags_half", "all_half", "rank3")]
    for d in devs:
        assert d.flags is None or d.flags.data_ptr() % 16 == 1
        assert d.outs["kept"].data_ptr() % 16 == 4 and d.outs["kept_starts"].data_ptr() % 16 == 8
    run(gpu, devs)
    for d in devs:
        d.check(gpu, "skewed n=%d" % d.c.n)


def test_filter_ignores_what_the_outputs_held(gpu):
    c = shaped(MID, "random", True, "all_half")
    a, b = Dev(c, fill=FILL), Dev(c, fill=OTHER)
    run(gpu, [a, b])
    ra, rb = a.check(gpu, "first fill"), b.check(gpu, "second fill")
    for k in PARTS + ("info",):
        m = c.size(k) if not k.endswith("_starts") else c.segments + 1
        assert ra[k][:m].tobytes() == rb[k][:m].tobytes()
        assert (rb[k][m:] == OTHER[k]).all()


def test_filter_two_streams_keep_their_scratch_apart(gpu):
    import torch
    cs = [shaped(40 * T + 9, "runs4095", False, "flags_half", seed=s) for s in (1, 2)]
    cs[1].flags = (cs[1].flags == 0).astype(np.uint8)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [[Dev(c) for _ in range(4)] for c in cs]
    torch.cuda.synchronize()
    for r in range(4):
        for s in (0, 1):
            assert devs[s][r].enqueue(gpu, streams[s]) == 0
    torch.cuda.synchronize()
    for s in (0, 1):
        for d in devs[s]:
            d.check(gpu, "stream %d" % s)


def test_filter_only_info_and_each_output_alone(gpu):
    wants = [(), ("kept",), ("kept_starts",), ("dropped",), ("dropped_starts",)]
    devs = [Dev(shaped(MID, seg, True, "all_half", w)) for w in wants
            for seg in ("runs63", "many_empty", None)]
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "want %s" % (d.c.want,))
        assert 0 < int(got["info"][0]) < MID


def test_filter_segment_count_from_device_memory(gpu):
    """G below, equal to and above the cap: above, R = cap - 1 and the last group's positions
    take no part; no segment at all; no list"""
    cap = len(SEGMENTATIONS["runs63"](MID)) - 1
    devs = [Dev(shaped(MID, "runs63", False, "flags_half", nseg=g))
            for g in (0, 1, cap - 1, cap, cap + 1, 1 << 40)]
    devs.append(Dev(Case(list_of(9, 9), [4], 9, nseg=3)))
    devs.append(Dev(Case(list_of(MID, 9), [0], 9)))
    devs.append(Dev(Case(list_of(MID, 9), [5, 5, 5], 9)))
    devs += [Dev(shaped(0, seg, False, "none")) for seg in ("whole", "empties", "steering", None)]
    c = shaped(MID, "random", False, "val8")
    c.count = 0     # a batch of no packets: no entry has a value
    devs.append(Dev(c))
    run(gpu, devs)
    for d in devs:
        got = d.check(gpu, "nseg %s n %d" % (d.c.nseg, d.c.n))
        if d.c.seg_starts is not None:
            end = int(d.c.seg_starts[d.c.segments]) - int(d.c.seg_starts[0]) if d.c.segments else 0
            assert int(got["info"][0] + got["info"][1]) == end


# ---------------------------------------------------------------- after a run, on one stream

NREAL = 2 * T + 37
BUDGET = 300


def test_filter_in_a_quota_pipeline_on_one_stream(gpu, env):
    """run, group by a 16-bit field of the verdict, scan with 300 bytes a group, filter by `over`,
    reduce the kept list per group and gather it, with no host read in between: the same chain
    of host functions gives the same bytes, and the gathered slots from K on are zero"""
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
    assert not w_flt.any()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    cap = NREAL

    def z(k, dtype, fill=0):
        return torch.full((k,), fill, dtype=dtype, device=dev)
    d_data, d_offs = up(data), up(offsets)
    ret, flt = z(NREAL, torch.int64, -1), z(NREAL, torch.uint8)
    index, gkeys, gstarts = z(NREAL, torch.int32, -1), z(cap, torch.int64), z(cap + 1, torch.int64)
    info, kd = z(2, torch.int64), z(2, torch.int64, 0x5a)
    tmp_bytes = gpu.group_tmp_bytes(NREAL, 16)
    tmp = z(max(tmp_bytes, 8), torch.uint8)
    budgets = z(cap, torch.int64, BUDGET)
    over = z(NREAL, torch.uint8, 0x5a)
    kept, dropped = z(NREAL, torch.int32, 0x5a5a5a5a), z(NREAL, torch.int32, 0x5a5a5a5a)
    ks, ds = z(cap + 1, torch.int64, 0x5a), z(cap + 1, torch.int64, 0x5a)
    kbytes, dbytes = z(cap, torch.int64, 0x5a), z(cap, torch.int64, 0x5a)
    dense = z(NREAL * 64, torch.uint8, 0x5a)
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        p.run_batch_dev(0, d_data.data_ptr(), NREAL, 0, ret.data_ptr(), d_offs.data_ptr(),
                        flt.data_ptr(), None, st)
        gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), NREAL, 16, 16, index.data_ptr(), cap,
                      gkeys.data_ptr(), gstarts.data_ptr(), info.data_ptr(), tmp.data_ptr(),
                      tmp_bytes, st)
        gpu.scan_dev(0, None, NREAL, 0, 0, index.data_ptr(), NREAL, gstarts.data_ptr(), cap,
                     info.data_ptr(), budgets.data_ptr(), over_ptr=over.data_ptr(),
                     offsets_ptr=d_offs.data_ptr(), stream=st)
        gpu.filter_dev(0, NREAL, index.data_ptr(), NREAL, gstarts.data_ptr(), cap, kd.data_ptr(),
                       nseg_ptr=info.data_ptr(), flags_ptr=over.data_ptr(),
                       kept_ptr=kept.data_ptr(), kept_starts_ptr=ks.data_ptr(),
                       dropped_ptr=dropped.data_ptr(), dropped_starts_ptr=ds.data_ptr(), stream=st)
        for lst, starts, out in ((kept, ks, kbytes), (dropped, ds, dbytes)):
            gpu.reduce_dev(0, None, NREAL, 0, 0, lst.data_ptr(), NREAL, starts.data_ptr(), cap,
                           info.data_ptr(), bytes_ptr=out.data_ptr(),
                           offsets_ptr=d_offs.data_ptr(), stream=st)
        gpu.gather_dev(0, d_data.data_ptr(), NREAL, 0, kept.data_ptr(), NREAL, 64,
                       dense.data_ptr(), NREAL * 64, offsets_ptr=d_offs.data_ptr(), stream=st)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    np.testing.assert_array_equal(ret.cpu().numpy().view(U64), w_ret)
    # the same chain on the host
    h_index, h_keys, h_starts, h_info, code = gpu.group(w_ret, None, 16, 16, cap)
    assert code == 0 and 100 < int(h_info[0]) <= cap and int(h_info[1]) == NREAL
    G = int(h_info[0])
    h_over = gpu.scan(h_index, h_starts, count=NREAL, offsets=offsets, nseg=G,
                      budgets=np.full(cap, BUDGET, dtype=U64), want=("over",))[3]
    h_kept, h_ks, h_dropped, h_ds, h_kd, code = gpu.filter(h_index, h_starts, flags=h_over,
                                                           count=NREAL, nseg=G)
    assert code == 0
    K, D = int(h_kd[0]), int(h_kd[1])
    assert K + D == NREAL and 0 < D < NREAL
    np.testing.assert_array_equal(info.cpu().numpy().view(U64), h_info)
    np.testing.assert_array_equal(index.cpu().numpy().view(np.uint32), h_index)
    np.testing.assert_array_equal(over.cpu().numpy(), h_over)
    np.testing.assert_array_equal(kd.cpu().numpy().view(U64), h_kd)
    np.testing.assert_array_equal(kept.cpu().numpy().view(np.uint32), h_kept)
    np.testing.assert_array_equal(dropped.cpu().numpy().view(np.uint32), h_dropped)
    np.testing.assert_array_equal(ks.cpu().numpy().view(U64)[:G + 1], h_ks[:G + 1])
    np.testing.assert_array_equal(ds.cpu().numpy().view(U64)[:G + 1], h_ds[:G + 1])
    assert (ks.cpu().numpy().view(U64)[G + 1:] == 0x5a).all()
    for lst, starts, got in ((h_kept, h_ks, kbytes), (h_dropped, h_ds, dbytes)):
        w = gpu.reduce(lst, starts, count=NREAL, offsets=offsets, nseg=G, want=("bytes",))
        assert w[5] == 0
        got = got.cpu().numpy().view(U64)
        np.testing.assert_array_equal(got[:G], w[0][:G])
        assert (got[G:] == 0x5a).all()
    assert (kbytes.cpu().numpy().view(U64)[:G] <= BUDGET).all()
    h_dense = gpu.gather(data, NREAL, h_kept, 64, offsets=offsets)[0]
    got = dense.cpu().numpy()
    np.testing.assert_array_equal(got, h_dense)
    assert not got[K * 64:].any() and got[:K * 64].any()
    assert (h_kept[K:] == NO_PACKET).all()
