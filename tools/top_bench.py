#!/usr/bin/env python3
"""What the heaviest entries of a table cost (ebpf_batch_top_dev, csrc/hip/top.hip).

Per point — a table of N random 44-bit keys in {64K, 1M, 16M} with random 40-bit values, the k in
{16, 256, 4,096} largest by a field of 40 and of 64 bits, keys, values and positions wanted — it
prints the call's time (device events around the call's kernels, median of --steps calls after
--warmup), the bytes of the model over that time as a fraction of the 6.29 TB/s copy ceiling
(DESIGN.md §4.1), and the time of what a caller has without the feature, in the same session, on
the same device: torch.topk on the values and two gathers (torch_top below).  The call's outputs are
checked equal to the host function's, whole; torch's values are checked equal to them (torch's
order among equal values is its own, so its positions are not compared).

The bytes model (bytes_model below): the select reads the values once per 8 bits of the field and
the collect once more, 8 B an entry each, and the k entries taken are gathered and written (36 B
each).  The second, partial reading by the placing kernel (the tiles that hold a taken entry), the
histograms' rows and the candidates are the algorithm's, not the problem's: they are not in the
model.

--rehearse checks the yardstick on CPU tensors against the host function and needs no GPU.  One
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

SIZES = [1 << 16, 1 << 20, 1 << 24]
KS = [16, 256, 4096]
BITS = [40, 64]
KEY_BITS, VAL_BITS = 44, 40


def bytes_model(n, k, bits):
    return (-(-bits // 8) + 1) * 8 * n + k * 36


def point(torch, g, n, dev):
    """(keys, values) of a table of about n entries: unique sorted keys, random values"""
    keys = torch.unique(torch.randint(0, 1 << KEY_BITS, (n,), generator=g, device=dev))
    return keys, torch.randint(0, 1 << VAL_BITS, (len(keys),), generator=g, device=dev)


def torch_top(torch, keys, vals, k):
    """the k largest with torch alone: (keys, values, positions)"""
    v, p = torch.topk(vals, k)
    return keys[p], vals[p], p


def rehearse():
    """the yardstick on CPU tensors against the host function, over a few tiles"""
    import torch
    g = torch.Generator()
    g.manual_seed(3)
    keys, vals = point(torch, g, 3 * native.STEER_TILE + 5, torch.device("cpu"))
    for k in (16, 256, native.TOP_MAX):
        for bits in BITS:
            hk, hv, hp, info = native.top(keys.numpy().view(np.uint64), vals.numpy().view(np.uint64),
                                          k, native.TOP_LARGEST, 0, bits)
            tk, tv, tp = torch_top(torch, keys, vals, k)
            assert int(info[0]) == k and np.array_equal(hv.view(np.int64), tv.numpy())
            if int(info[3]) == 0 and len(set(hv.tolist())) == k:   # (no ties: one right answer)
                assert np.array_equal(hk.view(np.int64), tk.numpy())
                assert np.array_equal(hp.astype(np.int64), tp.numpy())
            print(json.dumps({"what": "top_rehearsal", "table": len(keys), "k": k, "val_bits": bits,
                              "yardstick_matches_host": True}))


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
        sys.exit("top_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    fill = 77
    for size in SIZES:
        keys, vals = point(torch, g, size, dev)
        n = len(keys)
        d_n = torch.tensor([n], dtype=torch.int64, device=dev)
        h_keys, h_vals = (x.cpu().numpy().view(np.uint64) for x in (keys, vals))
        for k in KS:
            okeys = torch.full((k + 8,), fill, dtype=torch.int64, device=dev)
            ovals = torch.full((k + 8,), fill, dtype=torch.int64, device=dev)
            opos = torch.full((k + 8,), fill, dtype=torch.int32, device=dev)
            d_info = torch.zeros(4, dtype=torch.int64, device=dev)
            for bits in BITS:
                def run():
                    native.top_dev(0, keys.data_ptr(), vals.data_ptr(), n, d_n.data_ptr(), k,
                                   d_info.data_ptr(), native.TOP_LARGEST, 0, bits,
                                   keys_out_ptr=okeys.data_ptr(), vals_out_ptr=ovals.data_ptr(),
                                   pos_out_ptr=opos.data_ptr(), stream=st)

                def other():
                    return torch_top(torch, keys, vals, k)
                ms, lo = median_ms(torch, run, a.steps, a.warmup)
                hk, hv, hp, info = native.top(h_keys, h_vals, k, native.TOP_LARGEST, 0, bits, n=n)
                m = int(info[0])
                ok = (m == k and d_info.cpu().numpy().view(np.uint64).tolist() == info.tolist() and
                      np.array_equal(okeys[:m].cpu().numpy().view(np.uint64), hk) and
                      np.array_equal(ovals[:m].cpu().numpy().view(np.uint64), hv) and
                      np.array_equal(opos[:m].cpu().numpy().view(np.uint32), hp) and
                      bool((okeys[m:] == fill).all()) and bool((ovals[m:] == fill).all()) and
                      bool((opos[m:] == fill).all()))
                t_ok = np.array_equal(other()[1].cpu().numpy().view(np.uint64), hv)
                t_ms, _ = median_ms(torch, other, a.steps, a.warmup)
                by = bytes_model(n, k, bits)
                line = {"what": "top", "table": n, "k": k, "val_bits": bits,
                        "launches": 2 * -(-bits // 8) + 4, "cut_ties": int(info[3]),
                        "ms": round(ms, 4), "min_ms": round(lo, 4), "model_GB": round(by / 1e9, 5),
                        "copy_ceiling_frac": round(by / (ms * 1e-3) / COPY_CEILING, 4),
                        "torch_ms": round(t_ms, 4), "torch_over_call": round(t_ms / ms, 2),
                        "matches_host": ok, "torch_values_match": t_ok}
                print(json.dumps(line), flush=True)
                if not ok or not t_ok:
                    sys.exit("the results differ: table %d, k %d, val_bits %d" % (n, k, bits))
        del keys, vals


if __name__ == "__main__":
    main()
