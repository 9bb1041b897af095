#!/usr/bin/env python3
"""What running totals per segment cost (ebpf_batch_scan_dev, csrc/hip/scan.hip).

Over a device-resident batch of N packets in offsets form (default 64M; run it with --packets
4194304 too) it scans reduce_bench's four lists: the grouped index of three of group_bench's key
mixes — 10-bit uniform (1,024 groups), 32-bit uniform (a flow hash: nearly every group a packet or
two), 32-bit with 64K distinct values of Zipf-like popularity — with ebpf_batch_group_dev's table
and info as they stand, and a steering index with its 257 classes.  Per list and per call (all
four outputs; rank and over, the quota's two; rank alone) it prints: the call's time (device
events around the call's kernels, median of --steps launches after --warmup), the bytes the call
must move over that time as a fraction of the 6.29 TB/s copy ceiling, and the
time of what a caller has without the feature, in the same session: torch with segment ids from
repeat_interleave, ret[index] and the offsets gathered through the index, a cumsum and the
subtraction of its value where the segment begins.  The results are checked against torch's.
With all four outputs it also times ebpf_batch_reduce_dev with all five of its own on the same
list: the same gathers and far fewer entries written (a context line, not a bound).

The bytes model (bytes_model below): per list entry the index word (4 B), for bytes_before or over
the packet's two offsets entries (16 B), for sum_before its ret word (8 B), and what is written
(4 B of rank, 8 B of bytes_before and of sum_before, 1 B of over); per segment its start, read
twice by the tile that holds it, and its budget (24 B); the tiles' scratch rows.  Gathers are
counted by the words they use, not by the cache lines that carry them, and the second visit of a
tile's leading positions is not counted.

One JSON line per measurement on stdout, then one line with the ratio between the slowest and the
fastest list per call.  Needs a GPU: without one it fails."""
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

CALLS = {"all": native.SCANS, "quota": ("rank", "over"), "rank": ("rank",)}
WIDTH = {"rank": 4, "bytes_before": 8, "sum_before": 8, "over": 1}
BUDGET = 4000   # bytes a segment: a few packets of 64 to 1,500 bytes


def bytes_model(n, segments, want):
    tiles = -(-n // native.STEER_TILE)
    lens = "bytes_before" in want or "over" in want
    per_entry = (4 + (16 if lens else 0) + (8 if "sum_before" in want else 0)
                 if lens or "sum_before" in want else 0)
    per_entry += sum(WIDTH[k] for k in want)
    return n * per_entry + segments * 24 + tiles * 72 * 3


def torch_path(torch, want, ret, offs, index, starts, segments, n_listed, budgets):
    """the same outputs with torch alone: {name: tensor[n_listed]}"""
    out = {}
    dev = ret.device
    counts = starts[1:segments + 1] - starts[:segments]
    seg = torch.repeat_interleave(torch.arange(segments, device=dev), counts)
    base = starts[:segments][seg]               # where each position's segment begins
    if "rank" in want:
        out["rank"] = torch.arange(n_listed, device=dev) - base
    idx = index[:n_listed].to(torch.int64)
    if "bytes_before" in want or "over" in want:
        lens = offs[idx + 1] - offs[idx]
        ex = torch.cumsum(lens, 0) - lens
        before = ex - ex[base]
        if "bytes_before" in want:
            out["bytes_before"] = before
        if "over" in want:
            out["over"] = (before + lens > budgets[seg]).to(torch.uint8)
    if "sum_before" in want:
        v = (ret[idx] >> VAL_SHIFT) & ((1 << VAL_BITS) - 1)
        ex = torch.cumsum(v, 0) - v
        out["sum_before"] = ex - ex[base]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("scan_bench needs a GPU: %s" % native.last_error())
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
    d_budgets = torch.full((n,), BUDGET, dtype=torch.int64, device=dev)
    types = {"rank": torch.int32, "bytes_before": torch.int64, "sum_before": torch.int64,
             "over": torch.uint8}
    d_out = {k: torch.zeros(n + 8, dtype=types[k], device=dev) for k in native.SCANS}
    d_sums = {k: torch.zeros(n, dtype=torch.int64, device=dev) for k in native.SUMS}

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
                native.scan_dev(0, d_ret.data_ptr(), n, VAL_SHIFT, VAL_BITS, d_index.data_ptr(), n,
                                starts.data_ptr(), cap, None if nseg is None else nseg.data_ptr(),
                                d_budgets.data_ptr(), offsets_ptr=d_offs.data_ptr(), stream=st,
                                **ptrs)

            for k in want:
                d_out[k].fill_(77)
            ms, lo = median_ms(torch, run, a.steps, a.warmup)
            t_out = torch_path(torch, want, d_ret, d_offs, d_index, starts, segments, n, d_budgets)
            ok = all(bool((d_out[k][:n] == v).all()) for k, v in t_out.items())
            ok = ok and all(bool((d_out[k][n:] == 77).all()) for k in want)
            del t_out
            t_ms, _ = median_ms(torch, lambda: torch_path(torch, want, d_ret, d_offs, d_index,
                                                          starts, segments, n, d_budgets),
                                max(a.steps // 4, 3), 1)
            by = bytes_model(n, segments, want)
            times[call][name] = ms
            line = {"what": "scan", "list": name, "call": call, "packets": n,
                    "segments": segments, "ms": round(ms, 4), "min_ms": round(lo, 4),
                    "bytes": by, "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                    "torch_ms": round(t_ms, 4), "torch_over_scan": round(t_ms / ms, 2),
                    "matches_torch": ok}
            if call == "all":   # the reduce with all five outputs, same list, same session
                sums = {k + "_ptr": d_sums[k].data_ptr() for k in native.SUMS}
                r_ms, _ = median_ms(torch, lambda: native.reduce_dev(
                    0, d_ret.data_ptr(), n, VAL_SHIFT, VAL_BITS, d_index.data_ptr(), n,
                    starts.data_ptr(), cap, None if nseg is None else nseg.data_ptr(),
                    offsets_ptr=d_offs.data_ptr(), stream=st, **sums), a.steps, a.warmup)
                line["reduce_ms"] = round(r_ms, 4)
                line["scan_over_reduce"] = round(ms / r_ms, 2)
            print(json.dumps(line), flush=True)
            if not ok:
                sys.exit("the results differ from torch's on list %s, call %s" % (name, call))
    print(json.dumps({"what": "scan_shape_ratio", "packets": n,
                      **{c: round(max(t.values()) / min(t.values()), 3) for c, t in times.items()},
                      "slowest": {c: max(t, key=t.get) for c, t in times.items()},
                      "fastest": {c: min(t, key=t.get) for c, t in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
