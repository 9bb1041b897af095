#!/usr/bin/env python3
"""What grouping a batch by a wide key costs (ebpf_batch_group_dev, csrc/hip/group.hip).

Groups a device-resident ret / faults of N packets (default 64M; run it with --packets 4194304
too) for five key mixes — 10-bit uniform (1,024 queues), 16-bit uniform, 32-bit uniform (a flow
hash), 32-bit with 64K distinct values of Zipf-like popularity, 64-bit uniform — and prints per
mix: the call's time (device events around the call's kernels, median of --steps launches after
--warmup), its passes and the time per pass, the bytes a pass moves over that time as a fraction
of the 6.29 TB/s copy ceiling, the groups found, and the time of what a caller
has without the feature: torch.sort(stable=True) of the int64 key tensor with its indices, on the
same device in the same session (the timing keys stay below 2^63 for it).  The index is checked
against that sort.

One JSON line per measurement on stdout.  Needs a GPU: without one it fails."""
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


def plan(key_bits):
    """(passes, bytes a key travels as): csrc/host/group.cpp group_plan_of"""
    return -(-key_bits // 8), 4 if key_bits <= 32 else 8


def group_bytes(n, key_bits):
    """bytes one call moves: the first pass reads ret and faults twice (9 B a packet each) and
    writes key and index; a later pass reads the keys, then keys and indices, and writes both;
    every pass's tile rows as in steer_bench; the table's two sweeps read the sorted keys (the
    table's own entries, which depend on the mix, are left out)"""
    passes, w = plan(key_bits)
    tiles = -(-n // native.STEER_TILE)
    rows = (5 if tiles > 256 else 4) * tiles * BINS * 4
    first = 2 * 9 * n + (w + 4) * n + rows
    later = (w + (w + 4) + (w + 4)) * n + rows
    return first + (passes - 1) * later + 2 * w * n


def mixes(torch, n, g, dev):
    """(name, key_bits, keys int64[n] below 2^63)"""
    yield "uniform10", 10, torch.randint(0, 1 << 10, (n,), generator=g, device=dev)
    yield "uniform16", 16, torch.randint(0, 1 << 16, (n,), generator=g, device=dev)
    yield "uniform32", 32, torch.randint(0, 1 << 32, (n,), generator=g, device=dev)
    # value number floor(65536^u) - 1 for uniform u: popularity falls off as 1 / rank
    u = torch.rand((n,), generator=g, device=dev, dtype=torch.float64)
    rank = torch.clamp(torch.exp(u * math.log(65536.0)).to(torch.int64) - 1, 0, 65535)
    yield "zipf32_64k", 32, (rank * 2654435761) & 0xffffffff
    del u, rank
    yield "uniform64", 64, torch.randint(0, (1 << 63) - 1, (n,), generator=g, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("group_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    n = a.packets
    st = torch.cuda.current_stream().cuda_stream
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_index = torch.zeros(n, dtype=torch.int32, device=dev)
    d_keys = torch.zeros(n, dtype=torch.int64, device=dev)
    d_starts = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    d_info = torch.zeros(2, dtype=torch.int64, device=dev)
    d_tmp = torch.zeros(native.group_tmp_bytes(n, 64), dtype=torch.uint8, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for name, bits, d_ret in mixes(torch, n, g, dev):
        tmp_bytes = native.group_tmp_bytes(n, bits)

        def call():
            native.group_dev(0, d_ret.data_ptr(), d_flt.data_ptr(), n, 0, bits,
                             d_index.data_ptr(), n, d_keys.data_ptr(), d_starts.data_ptr(),
                             d_info.data_ptr(), d_tmp.data_ptr(), tmp_bytes, st)

        ms, lo = median_ms(torch, call, a.steps, a.warmup)
        sort_ms, _ = median_ms(torch, lambda: torch.sort(d_ret, stable=True), a.steps, a.warmup)
        skeys, order = torch.sort(d_ret, stable=True)
        ok = bool((order == d_index.to(torch.int64)).all())
        groups, unfaulted = (int(v) for v in d_info.cpu())
        heads = int((skeys[1:] != skeys[:-1]).sum()) + 1
        ok = ok and groups == heads and unfaulted == n and int(d_starts[groups]) == n
        ok = ok and bool((d_keys[:groups] == torch.unique_consecutive(skeys)).all())
        del skeys, order
        passes, w = plan(bits)
        b = group_bytes(n, bits)
        print(json.dumps({"what": "group", "mix": name, "packets": n, "key_bits": bits,
                          "groups": groups, "passes": passes, "ms": round(ms, 4),
                          "min_ms": round(lo, 4), "ms_per_pass": round(ms / passes, 4),
                          "bytes": b, "bytes_per_pass": b // passes,
                          "copy_ceiling_frac": round(b / (ms * 1e-3) / COPY_CEILING, 4),
                          "tmp_bytes": tmp_bytes,
                          "torch_sort_stable_ms": round(sort_ms, 4),
                          "sort_over_group": round(sort_ms / ms, 2),
                          "matches_torch_sort": ok}), flush=True)
        if not ok:
            sys.exit("grouping differs from torch.sort(stable=True) on mix %s" % name)
        del d_ret


if __name__ == "__main__":
    main()
