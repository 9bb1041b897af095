#!/usr/bin/env python3
"""What rolling a table up costs (ebpf_batch_rollup_dev, csrc/hip/rollup.hip).

Per point — a sorted table of N in {64K, 1M, 16M} keys whose runs under key_shift 16 have a mean
length of 1, 8 or 4,096 entries, or are one run over everything, with random 40-bit values; the
count alone (the values are not read), and all seven members — it prints the call's time (device
events around the call's kernels, median of --steps calls after --warmup), the bytes the call must
move over that time as a fraction of the 6.29 TB/s copy ceiling, and the time of
what a caller has without the feature, in the same session, on the same device:
torch.unique_consecutive with counts, and for all members its inverse with scatter_add_ and
scatter_reduce_ (torch_rollup below; torch has no scattered OR, so `bits` is left out of its side).
The call's outputs are checked equal to the host function's, whole, and torch's to them.

The bytes model (bytes_model below): the keys are read once, 8 B an entry, the values once when an
output reads them, 8 B more, and every member is written, 8 B a run.  The second reading by the
placing kernel and the tiles' rows in scratch are the algorithm's, not the problem's: they are not
in the model.

After the points of the largest table, one line per member set gives the slowest run shape's time
over the fastest's.  --rehearse checks the yardstick on CPU tensors against the host function and
needs no GPU.  One JSON line per measurement on stdout.  Without --rehearse it needs a GPU: without
one it fails."""
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

SIZES = [1 << 16, 1 << 20, 1 << 24]
MEANS = [1, 8, 4096, None]          # None: one run over everything
CALLS = {"count": ("count",), "all": native.ROLLS}
KEY_SHIFT, VAL_BITS = 16, 40
VALUE = ("sum", "min", "max", "bits")


def bytes_model(n, runs, want):
    reads = 8 * n + (8 * n if any(w in VALUE for w in want) else 0)
    return reads + 8 * runs * len(want) + (8 if "starts" in want else 0)


def point(torch, g, n, mean, dev):
    """(keys, values): n non-decreasing keys whose runs under KEY_SHIFT have about this mean
    length, and random values"""
    if mean is None:
        heads = torch.zeros(n, dtype=torch.int64, device=dev)
    elif mean == 1:
        heads = torch.ones(n, dtype=torch.int64, device=dev)
    else:
        heads = (torch.rand(n, generator=g, device=dev) < 1.0 / mean).to(torch.int64)
    prefix = torch.cumsum(heads, 0) * 3 + 5
    low = torch.arange(n, device=dev) & ((1 << KEY_SHIFT) - 1)
    return (prefix << KEY_SHIFT) | low, torch.randint(0, 1 << VAL_BITS, (n,), generator=g, device=dev)


def torch_rollup(torch, keys, vals, want):
    """the members of `want` with torch alone (no bits)"""
    if want == ("count",):
        c, count = torch.unique_consecutive(keys >> KEY_SHIFT, return_counts=True)
        return {"count": count}
    c, inv, count = torch.unique_consecutive(keys >> KEY_SHIFT, return_inverse=True,
                                             return_counts=True)
    C = len(c)
    zero = torch.zeros(C, dtype=torch.int64, device=keys.device)
    ends = torch.cumsum(count, 0)
    return {"keys": c, "count": count, "sum": zero.scatter_add(0, inv, vals),
            "min": zero.scatter_reduce(0, inv, vals, "amin", include_self=False),
            "max": zero.scatter_reduce(0, inv, vals, "amax", include_self=False),
            "starts": torch.cat([ends[:1] * 0, ends])}


def matches(got, want):
    return all(np.array_equal(got[w].cpu().numpy().view(np.uint64)[:len(want[w])], want[w])
               for w in got if w in want)


def rehearse():
    """the yardstick on CPU tensors against the host function, over a few tiles"""
    import torch
    g = torch.Generator()
    g.manual_seed(3)
    for mean in MEANS:
        keys, vals = point(torch, g, 3 * native.STEER_TILE + 5, mean, torch.device("cpu"))
        for call, want in CALLS.items():
            h, info, code = native.rollup(keys.numpy().view(np.uint64),
                                          vals.numpy().view(np.uint64) if call == "all" else None,
                                          KEY_SHIFT, val_bits=VAL_BITS, want=want)
            t = torch_rollup(torch, keys, vals, want)
            assert code == 0 and len(t["count"]) == int(info[0]) and matches(t, h)
            print(json.dumps({"what": "rollup_rehearsal", "entries": len(keys), "mean_run": mean,
                              "call": call, "runs": int(info[0]), "yardstick_matches_host": True}))


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
        sys.exit("rollup_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    fill = 77
    for n in SIZES:
        outs = {w: torch.full((n + 1 + 8,), fill, dtype=torch.int64, device=dev) for w in native.ROLLS}
        d_info = torch.zeros(2, dtype=torch.int64, device=dev)
        d_n = torch.tensor([n], dtype=torch.int64, device=dev)
        times = {c: {} for c in CALLS}
        for mean in MEANS:
            keys, vals = point(torch, g, n, mean, dev)
            h_keys, h_vals = (x.cpu().numpy().view(np.uint64) for x in (keys, vals))
            for call, want in CALLS.items():
                for o in outs.values():
                    o.fill_(fill)
                ptrs = {("keys_out" if w == "keys" else w) + "_ptr": outs[w].data_ptr() for w in want}

                def run():
                    native.rollup_dev(0, keys.data_ptr(), vals.data_ptr() if call == "all" else None,
                                      n, d_n.data_ptr(), KEY_SHIFT, n, d_info.data_ptr(),
                                      val_bits=VAL_BITS, stream=st, **ptrs)

                def other():
                    return torch_rollup(torch, keys, vals, want)
                ms, lo = median_ms(torch, run, a.steps, a.warmup)
                h, info, code = native.rollup(h_keys, h_vals if call == "all" else None, KEY_SHIFT,
                                              val_bits=VAL_BITS, want=want)
                C = int(info[0])
                ok = (code == 0 and d_info.cpu().numpy().view(np.uint64).tolist() == info.tolist() and
                      all(np.array_equal(outs[w][:len(h[w])].cpu().numpy().view(np.uint64), h[w]) and
                          bool((outs[w][len(h[w]):] == fill).all()) for w in want))
                t_ok = matches(other(), h)
                t_ms, _ = median_ms(torch, other, a.steps, a.warmup)
                by = bytes_model(n, C, want)
                times[call][str(mean)] = ms
                line = {"what": "rollup", "entries": n, "mean_run": mean, "runs": C, "call": call,
                        "launches": 3, "ms": round(ms, 4), "min_ms": round(lo, 4),
                        "model_GB": round(by / 1e9, 5),
                        "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                        "torch_ms": round(t_ms, 4), "torch_over_call": round(t_ms / ms, 2),
                        "torch_left_out": ["bits"] if call == "all" else [],
                        "matches_host": ok, "torch_matches": t_ok}
                print(json.dumps(line), flush=True)
                if not ok or not t_ok:
                    sys.exit("the results differ: %d entries, mean run %s, %s" % (n, mean, call))
            del keys, vals
        print(json.dumps({"what": "rollup_shape_ratio", "entries": n,
                          **{c: round(max(t.values()) / min(t.values()), 3) for c, t in times.items()},
                          "slowest": {c: max(t, key=t.get) for c, t in times.items()},
                          "fastest": {c: min(t, key=t.get) for c, t in times.items()}}), flush=True)
        del outs


if __name__ == "__main__":
    main()
