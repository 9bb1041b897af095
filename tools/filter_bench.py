#!/usr/bin/env python3
"""What keeping part of a list costs (ebpf_batch_filter_dev, csrc/hip/filter.hip).

Over a device-resident batch of N packets (default 64M; run it with --packets 4194304 too) it
filters reduce_bench's four lists: the grouped index of three of group_bench's key mixes — 10-bit
uniform (1,024 groups), 32-bit uniform (a flow hash: nearly every group a packet or two), 32-bit
with 64K distinct values of Zipf-like popularity — with ebpf_batch_group_dev's table and info as
they stand, and a steering index with its 257 classes.  Per list, per test (flags alone, ranks
alone, a value field alone, all three; each passing about half and about one in a hundred of the
entries) and per call (both lists with both tables; the kept list and its table) it prints: the
call's time (device events around the call's kernels, median of --steps launches after --warmup),
the bytes the call must move over that time as a fraction of the 6.29 TB/s copy ceiling
(DESIGN.md §4.1), and the time of what a caller has without the feature, in the same session:
torch's index[mask] for each list and the cumsum of the mask sampled at seg_starts for each table
(yardstick below).  The results are checked against torch's.

The bytes model (bytes_model below), by the words used: per list entry a flag byte (1 B), a rank
(4 B), for the value test the index word and the ret word (12 B); the index word again where a list
is written (4 B) and 4 B per list written, which is written in full; per segment its start, read
twice by the tile that holds it, and 8 B per table; per tile its bits, written once and read once,
and its count, written twice and read twice (1,048 B).  Gathers are counted by the words they
use, not by the cache lines that carry them.

--rehearse checks the yardstick on CPU tensors against the host function ebpf_batch_filter and
needs no GPU.  One JSON line per measurement on stdout.  Without --rehearse it needs a GPU:
without one it fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pkgload  # noqa: E402

pkgload.load()
from generic_ebpf_amd import native  # noqa: E402
from reduce_bench import BINS, COPY_CEILING, VAL_BITS, VAL_SHIFT, key_mixes, median_ms  # noqa: E402

CALLS = {"all": native.PARTS, "kept": ("kept", "kept_starts")}
TESTS = {"flags": ("flags",), "rank": ("rank",), "value": ("value",),
         "all3": ("flags", "rank", "value")}
RATES = {"half": 0.5, "1pct": 0.01}
RANKS = 1000   # ranks are uniform below this


def bytes_model(n, segments, tests, want):
    tiles = max(-(-n // native.STEER_TILE), 1)
    lists = [k for k in want if not k.endswith("_starts")]
    tables = [k for k in want if k.endswith("_starts")]
    per_entry = ((1 if "flags" in tests else 0) + (4 if "rank" in tests else 0) +
                 (12 if "value" in tests else 0) + (4 + 4 * len(lists) if lists else 0))
    per_segment = 16 + 8 * len(tables) if tables else 0
    return n * per_entry + segments * per_segment + tiles * (2 * 512 + 6 * 4)


def bounds(tests, rate):
    """(rank_below, val_hi): every given test passes rate ** (1 / the number of tests)"""
    p = rate ** (1.0 / len(tests))
    return max(int(round(p * RANKS)), 1), max(int(p * (1 << VAL_BITS)) - 1, 0)


def yardstick(torch, tests, want, flags, rank, rank_below, ret, val_hi, index, starts, segments, n):
    """the same outputs with torch alone: {name: tensor}.  Every position of [0, starts[segments])
    takes part (starts[0] == 0, as a grouped or steered index has it)"""
    dev = index.device
    mask = torch.arange(n, device=dev) < starts[segments]
    if "flags" in tests:
        mask = mask & (flags[:n] == 0)
    if "rank" in tests:
        mask = mask & (rank[:n] < rank_below)
    if "value" in tests:
        v = (ret[index[:n].to(torch.int64)] >> VAL_SHIFT) & ((1 << VAL_BITS) - 1)
        mask = mask & (v <= val_hi)
    out = {}
    part = torch.arange(n, device=dev) < starts[segments]
    for name, sel in (("kept", mask), ("dropped", part & ~mask)):
        if name in want:
            out[name] = index[:n][sel]
        if name + "_starts" in want:
            before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                                torch.cumsum(sel, 0)])
            out[name + "_starts"] = before[starts[:segments + 1]]
    return out


def matches(torch, t_out, d_out, n, segments, fill):
    """the call's buffers against the yardstick's: lists, EBPF_NO_PACKET tails, tables, guards"""
    ok = True
    for k, v in t_out.items():
        m = len(v)
        ok = ok and bool((d_out[k][:m] == v).all())
        if k.endswith("_starts"):
            ok = ok and bool((d_out[k][m:m + 8] == fill).all())
        else:
            ok = ok and bool((d_out[k][m:n] == -1).all()) and bool((d_out[k][n:] == fill).all())
    return ok


def rehearse():
    """the yardstick on CPU tensors against the host function, on a list of a few tiles"""
    import torch
    g = np.random.default_rng(5)
    n, count = 3 * native.STEER_TILE + 17, 9000
    index = g.integers(0, count, n).astype(np.uint32)
    cuts = np.sort(g.integers(0, n + 1, 300))
    starts = np.concatenate([[0], cuts, [n - 9]]).astype(np.uint64)
    segments = len(starts) - 1
    ret = g.integers(0, 1 << 63, count, dtype=np.uint64)   # (below 2^63 for torch's int64)
    for tname, tests in TESTS.items():
        for rname, rate in RATES.items():
            rank_below, val_hi = bounds(tests, rate)
            p = rate ** (1.0 / len(tests))
            flags = (g.random(n) >= p).astype(np.uint8) * 3
            rank = g.integers(0, RANKS, n).astype(np.uint32)
            w = native.filter(index, starts,
                              flags=flags if "flags" in tests else None,
                              rank=rank if "rank" in tests else None, rank_below=rank_below,
                              ret=ret if "value" in tests else None, val_shift=VAL_SHIFT,
                              val_bits=VAL_BITS, val_lo=0, val_hi=val_hi)
            assert w[5] == 0
            t = yardstick(torch, tests, native.PARTS, torch.from_numpy(flags),
                          torch.from_numpy(rank.astype(np.int64)), rank_below,
                          torch.from_numpy(ret.view(np.int64)), val_hi,
                          torch.from_numpy(index.view(np.int32)),
                          torch.from_numpy(starts.view(np.int64)), segments, n)
            K, D = int(w[4][0]), int(w[4][1])
            assert K + D == n - 9 and abs(K / (n - 9) - rate) < 0.25 * rate + 0.01, (tname, rname, K)
            for k, host_out in zip(native.PARTS, w[:4]):
                got = t[k].numpy()
                m = len(got)
                assert m == (segments + 1 if k.endswith("_starts") else (K if k == "kept" else D))
                assert np.array_equal(got.astype(host_out.dtype), host_out[:m]), (tname, rname, k)
            print(json.dumps({"what": "filter_rehearsal", "test": tname, "rate": rname,
                              "kept": K, "dropped": D, "yardstick_matches_host": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    import torch
    if native.gpu_count() < 1:
        sys.exit("filter_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    n = a.packets
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    fill = 77
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_index = torch.zeros(n, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(2, dtype=torch.int64, device=dev)
    d_kd = torch.zeros(2, dtype=torch.int64, device=dev)
    d_tmp = torch.zeros(native.group_tmp_bytes(n, 32), dtype=torch.uint8, device=dev)
    d_rank = torch.randint(0, RANKS, (n,), generator=g, device=dev, dtype=torch.int32)
    u = torch.rand((n,), generator=g, device=dev)
    d_out = {"kept": torch.zeros(n + 8, dtype=torch.int32, device=dev),
             "dropped": torch.zeros(n + 8, dtype=torch.int32, device=dev)}

    def lists():
        """(name, ret, seg_starts, seg_cap, nseg or None, segments): d_index holds the list"""
        for name, bits, keys in key_mixes(torch, n, g, dev):
            ret = keys | (torch.randint(0, 1 << VAL_BITS, (n,), generator=g, device=dev) << VAL_SHIFT)
            del keys
            native.group_dev(0, ret.data_ptr(), d_flt.data_ptr(), n, 0, bits, d_index.data_ptr(), n,
                             None, d_starts.data_ptr(), d_info.data_ptr(), d_tmp.data_ptr(),
                             native.group_tmp_bytes(n, bits), st)
            yield name, ret, d_starts, n, d_info, int(d_info.cpu()[0])
            del ret
        ret = torch.randint(0, 256, (n,), generator=g, device=dev) | \
            (torch.randint(0, 1 << VAL_BITS, (n,), generator=g, device=dev) << VAL_SHIFT)
        classes = ret & 0xff
        native.steer_dev(0, classes.data_ptr(), None, n, d_index.data_ptr(), d_starts.data_ptr(), st)
        torch.cuda.synchronize()
        del classes
        yield "steer257", ret, d_starts, BINS, None, BINS

    for name, d_ret, starts, cap, nseg, segments in lists():
        for k in ("kept_starts", "dropped_starts"):
            d_out[k] = torch.zeros(segments + 1 + 8, dtype=torch.int64, device=dev)
        for tname, tests in TESTS.items():
            for rname, rate in RATES.items():
                rank_below, val_hi = bounds(tests, rate)
                d_flags = (u >= rate ** (1.0 / len(tests))).to(torch.uint8)
                for call, want in CALLS.items():
                    ptrs = {k + "_ptr": d_out[k].data_ptr() for k in want}
                    if "flags" in tests:
                        ptrs["flags_ptr"] = d_flags.data_ptr()
                    if "rank" in tests:
                        ptrs["rank_ptr"] = d_rank.data_ptr()
                    if "value" in tests:
                        ptrs["ret_ptr"] = d_ret.data_ptr()

                    def run():
                        native.filter_dev(0, n, d_index.data_ptr(), n, starts.data_ptr(), cap,
                                          d_kd.data_ptr(),
                                          nseg_ptr=None if nseg is None else nseg.data_ptr(),
                                          rank_below=rank_below, val_shift=VAL_SHIFT,
                                          val_bits=VAL_BITS, val_lo=0, val_hi=val_hi, stream=st,
                                          **ptrs)

                    for k in want:
                        d_out[k].fill_(fill)
                    ms, lo = median_ms(torch, run, a.steps, a.warmup)

                    def other():
                        return yardstick(torch, tests, want, d_flags, d_rank, rank_below, d_ret,
                                         val_hi, d_index, starts, segments, n)

                    t_out = other()
                    ok = matches(torch, t_out, d_out, n, segments, fill)
                    kept = int(d_kd.cpu()[0])
                    del t_out
                    t_ms, _ = median_ms(torch, other, max(a.steps // 4, 3), 1)
                    by = bytes_model(n, segments, tests, want)
                    line = {"what": "filter", "list": name, "test": tname, "rate": rname,
                            "call": call, "packets": n, "segments": segments, "kept": kept,
                            "ms": round(ms, 4), "min_ms": round(lo, 4), "model_GB": round(by / 1e9, 4),
                            "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                            "torch_ms": round(t_ms, 4), "torch_over_filter": round(t_ms / ms, 2),
                            "matches_torch": ok}
                    print(json.dumps(line), flush=True)
                    if not ok:
                        sys.exit("the results differ from torch's on list %s, test %s %s, call %s"
                                 % (name, tname, rname, call))
                del d_flags


if __name__ == "__main__":
    main()
