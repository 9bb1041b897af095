#!/usr/bin/env python3
"""What reducing a list per segment costs (ebpf_batch_reduce_dev, csrc/hip/reduce.hip).

Over a device-resident batch of N packets in offsets form (default 64M; run it with --packets
4194304 too) it reduces four lists: the grouped index of three of group_bench's key mixes — 10-bit
uniform (1,024 groups), 32-bit uniform (a flow hash: nearly every group a packet or two), 32-bit
with 64K distinct values of Zipf-like popularity — with ebpf_batch_group_dev's table and info as
they stand, and a steering index with its 257 classes.  Per list and per call (all five outputs;
bytes alone) it prints: the call's time (device events around the call's kernels, median of
--steps launches after --warmup), the bytes the call must move over that time as a fraction of the
6.29 TB/s copy ceiling, and the time of what a caller has without the feature,
in the same session: torch with segment ids from repeat_interleave, ret[index] and the offsets
gathered through the index, and index_add_ / scatter_reduce_ per statistic.  torch has no OR
reduction, so `bits` has no yardstick and is left out of that column; an op that this build
lacks for int64 is printed and left out too.  The sums are checked against torch's.

The bytes model (bytes_model below): per list entry the index word (4 B), for bytes the packet's
two offsets entries (16 B), for the value statistics its ret word (8 B); per segment its start,
read by the tile that holds it and by the pass that writes empty segments' identities (16 B), and
8 B per output wanted; the tiles' scratch rows.  Gathers are counted by the words they use, not
by the cache lines that carry them.

One JSON line per measurement on stdout, then one line with the ratio between the slowest and the
fastest list per call.  Needs a GPU: without one it fails."""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

pkgload.load()
from generic_ebpf_amd import native  # noqa: E402

COPY_CEILING = 6.29e12   # B/s, DESIGN.md §4.1
BINS = native.EBPF_HIST_BINS
VAL_SHIFT, VAL_BITS = 32, 31   # the value field: ret's upper half (below 2^63 for torch's int64)
CALLS = {"all": native.SUMS, "bytes": ("bytes",)}


def median_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
           for _ in range(steps)]
    for e0, e1 in evs:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    s = [a.elapsed_time(b) for a, b in evs]
    return float(np.median(s)), float(np.min(s))


def bytes_model(n, segments, want):
    tiles = -(-n // native.STEER_TILE)
    values = any(k != "bytes" for k in want)
    per_entry = 4 + (16 if "bytes" in want else 0) + (8 if values else 0)
    return n * per_entry + segments * (16 + 8 * len(want)) + tiles * 96 * 3


def key_mixes(torch, n, g, dev):
    """(name, key_bits, keys int64[n]): tools/group_bench.py's, the three the issue names"""
    yield "uniform10", 10, torch.randint(0, 1 << 10, (n,), generator=g, device=dev)
    yield "uniform32", 32, torch.randint(0, 1 << 32, (n,), generator=g, device=dev)
    u = torch.rand((n,), generator=g, device=dev, dtype=torch.float64)
    rank = torch.clamp(torch.exp(u * math.log(65536.0)).to(torch.int64) - 1, 0, 65535)
    yield "zipf32_64k", 32, (rank * 2654435761) & 0xffffffff


def torch_path(torch, want, ret, offs, index, starts, segments, n_listed):
    """the same sums with torch alone: {name: tensor[segments]}, and the names it cannot do"""
    out, missing = {}, []
    counts = starts[1:segments + 1] - starts[:segments]
    seg = torch.repeat_interleave(torch.arange(segments, device=ret.device), counts)
    idx = index[:n_listed].to(torch.int64)
    if "bytes" in want:
        out["bytes"] = torch.zeros(segments, dtype=torch.int64, device=ret.device).index_add_(
            0, seg, offs[idx + 1] - offs[idx])
    if len(want) > 1:
        v = (ret[idx] >> VAL_SHIFT) & ((1 << VAL_BITS) - 1)
        out["sum"] = torch.zeros(segments, dtype=torch.int64, device=ret.device).index_add_(
            0, seg, v)
        # (an empty segment keeps its start: the identities, UINT64_MAX read as int64 and 0)
        for name, op, start in (("min", "amin", -1), ("max", "amax", 0)):
            try:
                out[name] = torch.full((segments,), start, dtype=torch.int64,
                                       device=ret.device).scatter_reduce_(0, seg, v, op,
                                                                          include_self=False)
            except RuntimeError as e:
                missing.append("%s: %s" % (name, str(e).splitlines()[0]))
        missing.append("bits: torch has no OR reduction")
    return out, missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("reduce_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    n = a.packets
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    lens = torch.randint(64, 1501, (n,), generator=g, device=dev)
    d_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    del lens
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_index = torch.zeros(n, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(2, dtype=torch.int64, device=dev)
    d_tmp = torch.zeros(native.group_tmp_bytes(n, 32), dtype=torch.uint8, device=dev)
    d_out = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in native.SUMS}

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

    times = {c: {} for c in CALLS}
    for name, d_ret, starts, cap, nseg, segments in lists():
        for call, want in CALLS.items():
            ptrs = {k + "_ptr": d_out[k].data_ptr() for k in want}

            def run():
                native.reduce_dev(0, d_ret.data_ptr(), n, VAL_SHIFT, VAL_BITS, d_index.data_ptr(),
                                  n, starts.data_ptr(), cap,
                                  None if nseg is None else nseg.data_ptr(),
                                  offsets_ptr=d_offs.data_ptr(), stream=st, **ptrs)

            for k in want:
                d_out[k].fill_(-7)
            ms, lo = median_ms(torch, run, a.steps, a.warmup)
            t_out, missing = torch_path(torch, want, d_ret, d_offs, d_index, starts, segments, n)
            t_ms, _ = median_ms(torch, lambda: torch_path(torch, want, d_ret, d_offs, d_index,
                                                          starts, segments, n),
                                max(a.steps // 4, 3), 1)
            ok = all(bool((d_out[k][:segments] == v).all()) for k, v in t_out.items())
            if "bits" in want:   # no yardstick: the OR holds the maximum's bits and is no sum's
                b, m = d_out["bits"][:segments], d_out["max"][:segments]
                ok = ok and bool(((b | m) == b).all()) and bool((b < (1 << VAL_BITS)).all())
            ok = ok and bool((d_out[want[0]][segments:segments + 8] == -7).all())
            by = bytes_model(n, segments, want)
            times[call][name] = ms
            print(json.dumps({"what": "reduce", "list": name, "call": call, "packets": n,
                              "segments": segments, "ms": round(ms, 4), "min_ms": round(lo, 4),
                              "bytes": by,
                              "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                              "torch_ms": round(t_ms, 4), "torch_over_reduce": round(t_ms / ms, 2),
                              "torch_columns": sorted(t_out), "torch_left_out": missing,
                              "matches_torch": ok}), flush=True)
            del t_out
            if not ok:
                sys.exit("the sums differ from torch's on list %s, call %s" % (name, call))
    print(json.dumps({"what": "reduce_shape_ratio", "packets": n,
                      **{c: round(max(t.values()) / min(t.values()), 3) for c, t in times.items()},
                      "slowest": {c: max(t, key=t.get) for c, t in times.items()},
                      "fastest": {c: min(t, key=t.get) for c, t in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
