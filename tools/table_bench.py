#!/usr/bin/env python3
"""What carrying totals across batches costs (ebpf_batch_lookup_dev and ebpf_batch_accumulate_dev,
csrc/hip/table.hip).

Per point — a table of N keys in {64K, 1M, 16M} with a batch of R = N / 4 keys of which half are
new to the table, and a batch of 1M keys into no table — it prints, for the lookup (REMAINING, the
values alone) and for the accumulate (ADD, everything kept, into a second table of N + R entries):
the call's time (device events around the call's kernels, median of --steps calls after --warmup),
the bytes the call must move over that time as a fraction of the 6.29 TB/s copy ceiling
(DESIGN.md §4.1), and the time of what a caller has without the feature, in the same session, on
the same device: torch.searchsorted and two gathers for the lookup; cat + sort +
unique_consecutive + scatter_add_ for the accumulate (yardsticks below).  The results are checked
against torch's.  Keys are below 2^44 so that torch's signed order is the unsigned one.

The bytes model (bytes_model below), by the words used: the lookup reads per key the key and the
table key it is compared with (16 B) and, where the table has the key, its value (8 B), and writes
the budget (8 B); the accumulate reads every key and value of the table and of the batch once and
writes every kept pair once (16 B each).  What the searches probe on the way, the second reading
of the keys by the placing pass and the scratch (648 B a tile) are the algorithm's, not the
problem's: they are not in the model, so the fraction says how far the call is from a copy of its
inputs to its outputs.

--rehearse checks the yardsticks on CPU tensors against the host functions and needs no GPU.  One
JSON line per measurement on stdout.  Without --rehearse it needs a GPU: without one it fails."""
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
from reduce_bench import COPY_CEILING, median_ms  # noqa: E402

POINTS = [(1 << 16, 1 << 14), (1 << 20, 1 << 18), (1 << 24, 1 << 22), (0, 1 << 20)]
KEY_BITS = 44
LIMIT = 1 << 30   # the quota of the lookup; the table's values are below 2^31


def bytes_model(what, n, r, found, kept):
    if what == "lookup":
        return r * (16 + 8) + found * 8
    return 16 * (n + r + kept)


def point(torch, g, n, r, dev):
    """(table keys, table values, batch keys, adds) of n and r entries, sorted; half of the batch's
    keys are the table's (none of them for n == 0)"""
    u = torch.unique(torch.randint(0, 1 << KEY_BITS, (n + r,), generator=g, device=dev))
    u = u[torch.randperm(len(u), generator=g, device=dev)]
    shared = r // 2 if n else 0
    n = min(n, len(u) - (r - shared))
    tkeys = torch.sort(u[:n])[0]
    own = tkeys[torch.randperm(n, generator=g, device=dev)[:shared]]
    keys = torch.sort(torch.cat([u[n:n + r - shared], own]))[0]
    tvals = torch.randint(0, 1 << 31, (n,), generator=g, device=dev)
    adds = torch.randint(0, 1 << 20, (r,), generator=g, device=dev)
    return tkeys, tvals, keys, adds


def torch_lookup(torch, tkeys, tvals, keys):
    """the budgets with torch alone"""
    if len(tkeys) == 0:
        return torch.full_like(keys, LIMIT)
    p = torch.searchsorted(tkeys, keys).clamp_(max=len(tkeys) - 1)
    v = torch.where(tkeys[p] == keys, tvals[p], torch.zeros_like(keys))
    return (LIMIT - v).clamp_(min=0)


def torch_accumulate(torch, tkeys, tvals, keys, adds):
    """the merged table with torch alone: (keys, values)"""
    k, perm = torch.sort(torch.cat([tkeys, keys]))
    uk, inv = torch.unique_consecutive(k, return_inverse=True)
    v = torch.zeros(len(uk), dtype=torch.int64, device=k.device)
    v.scatter_add_(0, inv, torch.cat([tvals, adds])[perm])
    return uk, v


def rehearse():
    """the yardsticks on CPU tensors against the host functions, over a few tiles"""
    import torch
    g = torch.Generator()
    g.manual_seed(3)
    for n, r in ((3 * native.STEER_TILE + 5, native.STEER_TILE + 9), (0, 3000)):
        tkeys, tvals, keys, adds = point(torch, g, n, r, torch.device("cpu"))
        n = len(tkeys)
        h = [x.numpy().view(np.uint64) for x in (tkeys, tvals, keys, adds)]
        vals, _, code = native.lookup(h[0], h[1], h[2], native.LOOKUP_REMAINING, 0, LIMIT)
        assert code == 0 and np.array_equal(vals.view(np.int64),
                                            torch_lookup(torch, tkeys, tvals, keys).numpy())
        ok, ov, m, info, code = native.accumulate(h[0] if n else None, h[1] if n else None, h[2], h[3])
        uk, uv = torch_accumulate(torch, tkeys, tvals, keys, adds)
        assert code == 0 and m == len(uk) == n + r - (r // 2 if n else 0)
        assert np.array_equal(ok[:m].view(np.int64), uk.numpy())
        assert np.array_equal(ov[:m].view(np.int64), uv.numpy())
        print(json.dumps({"what": "table_rehearsal", "table": n, "keys": r, "merged": m,
                          "yardsticks_match_host": True}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    import torch
    if native.gpu_count() < 1:
        sys.exit("table_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    fill = 77
    for n, r in POINTS:
        tkeys, tvals, keys, adds = point(torch, g, n, r, dev)
        n = len(tkeys)
        d_n = torch.tensor([n], dtype=torch.int64, device=dev)
        ocap = n + r
        okeys = torch.full((ocap + 8,), fill, dtype=torch.int64, device=dev)
        ovals = torch.full((ocap + 8,), fill, dtype=torch.int64, device=dev)
        d_on = torch.zeros(1, dtype=torch.int64, device=dev)
        d_info = torch.zeros(3, dtype=torch.int64, device=dev)
        budgets = torch.full((r + 8,), fill, dtype=torch.int64, device=dev)
        tab = (tkeys.data_ptr() if n else None, tvals.data_ptr() if n else None, n, d_n.data_ptr())

        def look():
            native.lookup_dev(0, *tab, keys.data_ptr(), r, None, native.LOOKUP_REMAINING, 0, LIMIT,
                              vals_out_ptr=budgets.data_ptr(), stream=st)

        def acc():
            native.accumulate_dev(0, tab, keys.data_ptr(), adds.data_ptr(), r,
                                  (okeys.data_ptr(), ovals.data_ptr(), ocap, d_on.data_ptr()),
                                  d_info.data_ptr(), op=native.ACC_ADD, stream=st)

        calls = {"lookup": (look, lambda: torch_lookup(torch, tkeys, tvals, keys)),
                 "accumulate": (acc, lambda: torch_accumulate(torch, tkeys, tvals, keys, adds))}
        for what, (run, other) in calls.items():
            ms, lo = median_ms(torch, run, a.steps, a.warmup)
            t_out = other()
            info = d_info.cpu().tolist()
            if what == "lookup":
                ok = bool((budgets[:r] == t_out).all()) and bool((budgets[r:] == fill).all())
                found, kept = int((t_out != LIMIT).sum()) if n else 0, 0
            else:
                m = len(t_out[0])
                ok = (info[0] == m == int(d_on.cpu()[0]) and info[2] == 0 and
                      bool((okeys[:m] == t_out[0]).all()) and bool((ovals[:m] == t_out[1]).all())
                      and bool((okeys[m:] == fill).all()) and bool((ovals[m:] == fill).all()))
                found, kept = 0, m
            del t_out
            t_ms, _ = median_ms(torch, other, max(a.steps // 4, 3), 1)
            by = bytes_model(what, n, r, found, kept)
            line = {"what": what, "table": n, "keys": r, "found": found, "kept": kept,
                    "ms": round(ms, 4), "min_ms": round(lo, 4), "model_GB": round(by / 1e9, 5),
                    "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                    "torch_ms": round(t_ms, 4), "torch_over_call": round(t_ms / ms, 2),
                    "matches_torch": ok}
            print(json.dumps(line), flush=True)
            if not ok:
                sys.exit("the results differ from torch's: %s, table %d, keys %d" % (what, n, r))
        del tkeys, tvals, keys, adds, okeys, ovals, budgets


if __name__ == "__main__":
    main()
