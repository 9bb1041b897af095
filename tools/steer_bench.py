#!/usr/bin/env python3
"""What steering a batch by verdict costs (ebpf_batch_steer_dev, csrc/hip/steer.hip).

Steers the ret of C4 over N packets (default 64M, device-resident) for three class mixes — C4's
own verdicts, uniform over 4 classes, uniform over 257 — and prints per mix: the steering time
(device events around the call's kernels, median of --steps launches after --warmup), the bytes
it moves (two reads of ret and faults, 9 B a packet each; one 4-B index write; the tile rows'
traffic) over that time as a fraction of the 6.29 TB/s copy ceiling, and the
time of what a caller can do without the feature: torch.sort(stable=True) of the int16 class
tensor with its indices, on the same device in the same session.  C4's own kernel time is
printed next to them, and (--stage2) a second stage on the most populated class: C3 over the
selected extents batch (general kernel) against C3 over the whole 64-byte-stride batch (staged
kernel), per packet.

One JSON line per measurement on stdout.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pkgload  # noqa: E402

pkgload.load()
from generic_ebpf_amd import native, workloads  # noqa: E402

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


def steer_bytes(n):
    """bytes one call moves: both sweeps read ret and faults, the scatter writes the index; a
    tile's row is written by the count, read and rewritten by the scan and read by the scatter
    and, past 256 tiles, once more by the segment sums (those, 256 rows at most, are left
    out)"""
    tiles = -(-n // native.STEER_TILE)
    return 2 * 9 * n + 4 * n + (5 if tiles > 256 else 4) * tiles * BINS * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stage2", action="store_true")
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("steer_bench needs a GPU: %s" % native.last_error())
    dev = torch.device("cuda:0")
    n = a.packets
    st = torch.cuda.current_stream().cuda_stream
    D = min(n, 1 << 20)
    base = torch.from_numpy(workloads.packets_l2l3(D, 64)).to(dev)
    data = base.repeat(-(-n // D), 1)[:n].contiguous().reshape(-1)
    d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_hist = torch.zeros(BINS, dtype=torch.int64, device=dev)
    d_index = torch.zeros(n, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(native.STEER_STARTS, dtype=torch.int64, device=dev)

    env = native.Env()
    lay = workloads.prog_c4()
    m = native.Map(env, 256, 8)
    m.fill(workloads.c4_map_values().tobytes())
    p = native.Prog(env, native.patch_relocs(lay.code, lay.relocs, [m.handle]))

    def run_c4():
        p.run_batch_dev(0, data.data_ptr(), n, 64, d_ret.data_ptr(), None, d_flt.data_ptr(),
                        d_hist.data_ptr(), st, hist_overwrite=True)

    def kernel_ms(prog_run):
        """the program's own kernel, timed by the library around its dispatch"""
        for _ in range(a.warmup):
            prog_run()
        out = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            native.time_next_launch(e0.cuda_event, e1.cuda_event)
            prog_run()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return float(np.median(out))

    c4_ms = kernel_ms(run_c4)
    print(json.dumps({"what": "c4_kernel", "packets": n, "ms": round(c4_ms, 4),
                      "layout": p.exec_info(0)[1]}), flush=True)
    c4_ret, c4_flt = d_ret.clone(), d_flt.clone()

    def steer_call():
        native.steer_dev(0, d_ret.data_ptr(), d_flt.data_ptr(), n, d_index.data_ptr(),
                         d_starts.data_ptr(), st)

    g = torch.Generator(device=dev)
    g.manual_seed(1)
    for name, nclass in (("c4", 0), ("uniform4", 4), ("uniform257", 257)):
        if nclass:   # (class 256 = a faulted packet: ret 0, its fault code set)
            cls = torch.randint(0, nclass, (n,), generator=g, device=dev)
            d_flt.copy_((cls == 256).to(torch.uint8))
            d_ret.copy_(torch.where(cls == 256, torch.zeros_like(cls), cls))
            del cls
        ms, lo = median_ms(torch, steer_call, a.steps, a.warmup)
        # the result against torch's own stable sort, and that sort's time
        c16 = torch.where(d_flt != 0, torch.full_like(d_ret, 256),
                          torch.clamp(d_ret, max=255)).to(torch.int16)
        sort_ms, _ = median_ms(torch, lambda: torch.sort(c16, stable=True), a.steps, a.warmup)
        order = torch.sort(c16, stable=True)[1]
        ok = bool((order == d_index.to(torch.int64)).all())
        classes = int((torch.diff(d_starts) > 0).sum())
        del order, c16
        b = steer_bytes(n)
        print(json.dumps({"what": "steer", "mix": name, "packets": n, "classes": classes,
                          "ms": round(ms, 4), "min_ms": round(lo, 4), "bytes": b,
                          "copy_ceiling_frac": round(b / (ms * 1e-3) / COPY_CEILING, 4),
                          "torch_sort_stable_ms": round(sort_ms, 4),
                          "sort_over_steer": round(sort_ms / ms, 2),
                          "steer_over_c4_kernel": round(ms / c4_ms, 3),
                          "matches_torch_sort": ok}), flush=True)
        if not ok:
            sys.exit("steering differs from torch.sort(stable=True) on mix %s" % name)

    if a.stage2:
        d_ret.copy_(c4_ret)
        d_flt.copy_(c4_flt)
        steer_call()
        torch.cuda.synchronize()
        starts = d_starts.cpu().numpy()
        b = int(np.argmax(np.diff(starts)))
        lo, k = int(starts[b]), int(starts[b + 1] - starts[b])
        ext = torch.zeros(2 * k, dtype=torch.int64, device=dev)
        sel_ms, _ = median_ms(torch, lambda: native.select_dev(
            0, data.data_ptr(), n, 64, d_index.data_ptr() + 4 * lo, k, ext.data_ptr(), stream=st),
            a.steps, a.warmup)
        lay3 = workloads.prog_c3()
        p3 = native.Prog(env, native.patch_relocs(lay3.code, lay3.relocs, []))
        r2 = torch.zeros(n, dtype=torch.int64, device=dev)
        whole = kernel_ms(lambda: p3.run_batch_dev(0, data.data_ptr(), n, 64, r2.data_ptr(),
                                                   None, None, None, st))
        whole_layout = p3.exec_info(0)[1]
        part = kernel_ms(lambda: p3.run_batch_dev(0, data.data_ptr(), k, 0, r2.data_ptr(),
                                                  ext.data_ptr(), None, None, st, extents=True))
        print(json.dumps({"what": "stage2_c3", "class": b, "class_packets": k,
                          "select_ms": round(sel_ms, 4),
                          "selected_ms": round(part, 4), "selected_layout": p3.exec_info(0)[1],
                          "selected_ns_per_packet": round(part * 1e6 / k, 4),
                          "whole_batch_ms": round(whole, 4), "whole_layout": whole_layout,
                          "whole_ns_per_packet": round(whole * 1e6 / n, 4)}), flush=True)
        p3.destroy()
    p.destroy()
    m.destroy()
    env.destroy()


if __name__ == "__main__":
    main()
