#!/usr/bin/env python3
"""What gathering packets into a dense batch costs (ebpf_batch_gather_dev, csrc/hip/gather.hip).

Three measurements, each timed with device events around the call (median of --steps launches
after --warmup; every timing is taken twice, and both medians are printed: their difference is
the spread a comparison has to beat):

  rows     C4 over N 64-byte packets (default 64M, device-resident), steered; the most populated
           class, then the whole steering index, gathered at stride 64 (the row path).  Bytes =
           4 (index) + 64 (read) + 64 (written) a packet, over the time, against the 6.29 TB/s
           copy ceiling.  Baseline: torch.index_select of the [N, 16] int32 view
           by the same int32 index into a preallocated output, same session; the outputs are
           compared.
  stage2   C3 over the gathered class (staged kernel), over the same class selected in place
           (ebpf_batch_select_dev: extents, general kernel) and over the whole dense batch, per
           packet, and the number of second-stage passes from which gather + staged is cheaper
           than running in place.
  general  M IMIX packets (default 4M, true sizes 64 / 576 / 1500 as extents over C5's padded
           layout) and the list of every second packet: the packed form, against a
           device-to-device copy_ of the same payload as the floor, and the 64-byte snapshot,
           with C3 over the snapshot (staged kernel) against C3 over the listed packets in place
           (extents, general kernel).  Both gathers again from a source moved by one byte, so
           that every 16-byte load is misaligned.  Bytes = per list entry 4 (index) + 16 (its
           extent) + payload read + payload written (+ 8 of out_offsets, packed form).

One JSON line per measurement on stdout.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys

import numpy as np

from steer_bench import COPY_CEILING, BINS, median_ms, native, workloads


def twice(torch, fn, a):
    return [round(median_ms(torch, fn, a.steps, a.warmup)[0], 4) for _ in range(2)]


def frac(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / COPY_CEILING, 4)


def kernel_ms(torch, a, prog_run):
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


def c3_ms(torch, a, p3, st, data_ptr, n, stride, ret, offsets_ptr=None, extents=False):
    ms = kernel_ms(torch, a, lambda: p3.run_batch_dev(0, data_ptr, n, stride, ret.data_ptr(),
                                                      offsets_ptr, None, None, st,
                                                      extents=extents))
    return ms, p3.exec_info(0)[1]


def rows_and_stage2(torch, a, env, p3):
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    n = a.packets
    D = min(n, 1 << 20)
    base = torch.from_numpy(workloads.packets_l2l3(D, 64)).to(dev)
    data = base.repeat(-(-n // D), 1)[:n].contiguous().reshape(-1)
    d_ret = torch.zeros(n, dtype=torch.int64, device=dev)
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_hist = torch.zeros(BINS, dtype=torch.int64, device=dev)
    d_index = torch.zeros(n, dtype=torch.int32, device=dev)
    d_starts = torch.zeros(native.STEER_STARTS, dtype=torch.int64, device=dev)
    lay = workloads.prog_c4()
    m = native.Map(env, 256, 8)
    m.fill(workloads.c4_map_values().tobytes())
    p = native.Prog(env, native.patch_relocs(lay.code, lay.relocs, [m.handle]))
    p.run_batch_dev(0, data.data_ptr(), n, 64, d_ret.data_ptr(), None, d_flt.data_ptr(),
                    d_hist.data_ptr(), st, hist_overwrite=True)
    native.steer_dev(0, d_ret.data_ptr(), d_flt.data_ptr(), n, d_index.data_ptr(),
                     d_starts.data_ptr(), st)
    torch.cuda.synchronize()
    starts = d_starts.cpu().numpy()
    b = int(np.argmax(np.diff(starts)))
    lo, k = int(starts[b]), int(starts[b + 1] - starts[b])
    out = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    rows = data.view(torch.int32).view(n, 16)
    sel = torch.empty((n, 16), dtype=torch.int32, device=dev)
    gather_class_ms = None
    for name, first, cnt in (("class", lo, k), ("whole", 0, n)):
        idx = d_index[first:first + cnt]
        ms = twice(torch, lambda: native.gather_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), cnt,
                                                    64, out.data_ptr(), cnt * 64, stream=st), a)
        ref = twice(torch, lambda: torch.index_select(rows, 0, idx, out=sel[:cnt]), a)
        same = bool(torch.equal(out[:cnt * 64].view(torch.int32).view(cnt, 16), sel[:cnt]))
        nbytes = cnt * (4 + 64 + 64)
        print(json.dumps({"what": "gather_rows", "list": name, "class": b if name == "class" else None,
                          "packets": cnt, "ms": ms, "bytes": nbytes,
                          "copy_ceiling_frac": [frac(nbytes, x) for x in ms],
                          "index_select_ms": ref,
                          "spread_ms": round(max(abs(ms[0] - ms[1]), abs(ref[0] - ref[1])), 4),
                          "gather_over_index_select": round(min(ms) / min(ref), 3),
                          "matches_index_select": same}), flush=True)
        if not same:
            sys.exit("gather differs from torch.index_select on the %s list" % name)
        if name == "class":
            gather_class_ms = min(ms)
    if a.only in ("all", "stage2"):
        idx = d_index[lo:lo + k]
        native.gather_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), k, 64, out.data_ptr(), k * 64,
                          stream=st)
        ext = torch.zeros(2 * k, dtype=torch.int64, device=dev)
        native.select_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), k, ext.data_ptr(), stream=st)
        r2 = torch.zeros(n, dtype=torch.int64, device=dev)
        g_ms, g_lay = c3_ms(torch, a, p3, st, out.data_ptr(), k, 64, r2)
        s_ms, s_lay = c3_ms(torch, a, p3, st, data.data_ptr(), k, 0, r2, ext.data_ptr(), True)
        w_ms, w_lay = c3_ms(torch, a, p3, st, data.data_ptr(), n, 64, r2)
        ns = lambda ms, cnt: ms * 1e6 / cnt
        gain = ns(s_ms, k) - ns(g_ms, k)
        print(json.dumps({"what": "stage2_c3", "class": b, "class_packets": k,
                          "gather_ms": gather_class_ms,
                          "gather_ns_per_packet": round(ns(gather_class_ms, k), 4),
                          "gathered_ms": round(g_ms, 4), "gathered_layout": g_lay,
                          "gathered_ns_per_packet": round(ns(g_ms, k), 4),
                          "selected_ms": round(s_ms, 4), "selected_layout": s_lay,
                          "selected_ns_per_packet": round(ns(s_ms, k), 4),
                          "whole_batch_ms": round(w_ms, 4), "whole_layout": w_lay,
                          "whole_ns_per_packet": round(ns(w_ms, n), 4),
                          "break_even_passes": round(ns(gather_class_ms, k) / gain, 2)
                          if gain > 0 else None}), flush=True)
    p.destroy()
    m.destroy()


def general(torch, a, p3):
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    n = a.imix
    h_data, h_offs, h_sizes = workloads.packets_imix_range(0, n, seed=5)
    ext = np.stack([h_offs[:-1], h_offs[:-1] + h_sizes], axis=1).reshape(-1)
    buf = torch.zeros(len(h_data) + 64, dtype=torch.uint8, device=dev)
    buf[:len(h_data)] = torch.from_numpy(h_data).to(dev)
    moved = torch.zeros(len(h_data) + 64, dtype=torch.uint8, device=dev)
    moved[1:1 + len(h_data)] = buf[:len(h_data)]
    d_ext = torch.from_numpy(ext.view(np.int64)).to(dev)
    listed = np.arange(0, n, 2)
    k = len(listed)
    idx = torch.from_numpy(listed.astype(np.int32)).to(dev)
    sizes = torch.from_numpy(h_sizes[listed].astype(np.int64)).to(dev)
    first = torch.from_numpy(h_offs[:-1][listed].astype(np.int64)).to(dev)
    payload = int(h_sizes[listed].sum())
    out = torch.empty(max(payload, k * 64) + 64, dtype=torch.uint8, device=dev)
    offs = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    want_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)])
    copy_src = torch.empty(payload, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty(payload, dtype=torch.uint8, device=dev)
    floor = twice(torch, lambda: copy_dst.copy_(copy_src), a)
    del copy_src, copy_dst
    col = torch.arange(64, device=dev)
    res = {}
    for src_name, src in (("aligned", buf), ("moved_1_byte", moved[1:])):
        ms = twice(torch, lambda: native.gather_dev(0, src.data_ptr(), n, 0, idx.data_ptr(), k, 0,
                                                    out.data_ptr(), payload, offs.data_ptr(),
                                                    d_ext.data_ptr(), st, extents=True), a)
        ok = bool(torch.equal(offs, want_offs))
        for lo_, hi_ in ((0, 2000), (k - 2000, k)):   # the first and last packets, byte by byte
            a0, a1 = int(want_offs[lo_]), int(want_offs[hi_])
            pos = torch.repeat_interleave(first[lo_:hi_] - want_offs[lo_:hi_], sizes[lo_:hi_]) + \
                torch.arange(a0, a1, device=dev)
            ok = ok and bool(torch.equal(out[a0:a1], buf[pos]))
        nbytes = k * (4 + 16 + 8) + 2 * payload
        print(json.dumps({"what": "gather_packed", "source": src_name, "packets": k,
                          "payload_bytes": payload, "ms": ms, "bytes": nbytes,
                          "copy_ceiling_frac": [frac(nbytes, x) for x in ms],
                          "copy_floor_ms": floor,
                          "copy_floor_frac": [frac(2 * payload, x) for x in floor],
                          "correct": ok}), flush=True)
        if not ok:
            sys.exit("packed gather wrong (%s source)" % src_name)
        ms = twice(torch, lambda: native.gather_dev(0, src.data_ptr(), n, 0, idx.data_ptr(), k, 64,
                                                    out.data_ptr(), k * 64, None, d_ext.data_ptr(),
                                                    st, extents=True), a)
        ok = bool(torch.equal(out[:k * 64].view(k, 64), buf[first[:, None] + col[None, :]]))
        nbytes = k * (4 + 16 + 64 + 64)
        res[src_name] = ms
        print(json.dumps({"what": "gather_snapshot64", "source": src_name, "packets": k, "ms": ms,
                          "bytes": nbytes, "copy_ceiling_frac": [frac(nbytes, x) for x in ms],
                          "correct": ok}), flush=True)
        if not ok:
            sys.exit("snapshot gather wrong (%s source)" % src_name)
    # out holds the snapshot: C3 over it, and over the listed packets in place
    sel = torch.zeros(2 * k, dtype=torch.int64, device=dev)
    native.select_dev(0, buf.data_ptr(), n, 0, idx.data_ptr(), k, sel.data_ptr(), d_ext.data_ptr(),
                      st, extents=True)
    r2 = torch.zeros(k, dtype=torch.int64, device=dev)
    r3 = torch.zeros(k, dtype=torch.int64, device=dev)
    g_ms, g_lay = c3_ms(torch, a, p3, st, out.data_ptr(), k, 64, r2)
    s_ms, s_lay = c3_ms(torch, a, p3, st, buf.data_ptr(), k, 0, r3, sel.data_ptr(), True)
    print(json.dumps({"what": "snapshot_stage2_c3", "packets": k,
                      "snapshot_ms": round(g_ms, 4), "snapshot_layout": g_lay,
                      "snapshot_ns_per_packet": round(g_ms * 1e6 / k, 4),
                      "in_place_ms": round(s_ms, 4), "in_place_layout": s_lay,
                      "in_place_ns_per_packet": round(s_ms * 1e6 / k, 4),
                      "gather_ns_per_packet": round(min(res["aligned"]) * 1e6 / k, 4),
                      "same_results": bool(torch.equal(r2, r3))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--imix", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["all", "rows", "stage2", "general"], default="all")
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("gather_bench needs a GPU: %s" % native.last_error())
    env = native.Env()
    lay3 = workloads.prog_c3()
    p3 = native.Prog(env, native.patch_relocs(lay3.code, lay3.relocs, []))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps({"what": "library", "path": os.path.relpath(native.LIB_PATH, root)}), flush=True)
    if a.only != "general":
        rows_and_stage2(torch, a, env, p3)
        torch.cuda.empty_cache()
    if a.only in ("all", "general"):
        general(torch, a, p3)
    p3.destroy()
    env.destroy()


if __name__ == "__main__":
    main()
