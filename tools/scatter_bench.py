#!/usr/bin/env python3
"""What bringing a class back costs (ebpf_batch_scatter_dev, ebpf_batch_merge_dev,
csrc/hip/scatter.hip).

Every call is timed with device events around it (median of --steps launches after --warmup;
every timing is taken twice, and both medians are printed: their difference is the spread a
comparison has to beat).  `frac` is bytes over time against the 6.29 TB/s copy ceiling
(DESIGN.md §4.1).

  rows     C4 over N 64-byte packets (default 64M, device-resident), steered; the most populated
           class, then the whole steering index, gathered at stride 64 and scattered back (the row
           path).  Bytes = 4 (index) + 64 (read) + 64 (written) a packet.  Yardsticks, same
           session: torch.index_copy_ of the same rows into the [N, 16] int32 view, and the gather
           of the same list.  The two scatters' results are compared.
  merge    ret2 / faults2 of the class into ret / faults: bytes = 4 + 9 read + 9 written an
           entry; against ret.index_copy_ (and the faults' index_copy_ on top) in the same session.
  pipeline per packet of the class: gather + C3 over the dense batch (staged kernel) + scatter +
           merge, against select + C3 in place (extents, general kernel), and the number of
           second-stage passes from which the dense route is cheaper when the class must return.
  general  M IMIX packets (default 4M, true sizes as extents over C5's padded layout) and the list
           of every second packet: packed and in_stride 64, from what the gather of the same list
           left.  Bytes = per entry 4 + packet read + packet written (+ 8 of in_offsets, packed).
           Yardstick: the gather of the same list in the same form.

One JSON line per measurement on stdout.  Needs a GPU: without one it fails."""
import argparse
import json
import os
import sys

import numpy as np

from gather_bench import c3_ms, frac, twice
from steer_bench import BINS, native, workloads


def rows_merge_pipeline(torch, a, env, p3):
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
    dense = torch.empty(n * 64, dtype=torch.uint8, device=dev)
    back = torch.zeros(n * 64, dtype=torch.uint8, device=dev)    # where the library scatters to
    ref = torch.zeros((n, 16), dtype=torch.int32, device=dev)    # where torch scatters to
    times = {}
    for name, first, cnt in (("class", lo, k), ("whole", 0, n)):
        idx = d_index[first:first + cnt]
        idx64 = idx.long()
        g_ms = twice(torch, lambda: native.gather_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), cnt,
                                                      64, dense.data_ptr(), cnt * 64, stream=st), a)
        ms = twice(torch, lambda: native.scatter_dev(0, back.data_ptr(), n, 64, idx.data_ptr(), cnt,
                                                     64, dense.data_ptr(), cnt * 64, stream=st), a)
        src_rows = dense[:cnt * 64].view(torch.int32).view(cnt, 16)
        t_ms = twice(torch, lambda: ref.index_copy_(0, idx64, src_rows), a)
        same = bool(torch.equal(back.view(torch.int32).view(n, 16), ref))
        nbytes = cnt * (4 + 64 + 64)
        times[name] = (min(g_ms), min(ms))
        print(json.dumps({"what": "scatter_rows", "list": name, "class": b if name == "class" else None,
                          "packets": cnt, "ms": ms, "bytes": nbytes,
                          "frac": [frac(nbytes, x) for x in ms],
                          "index_copy_ms": t_ms, "gather_ms": g_ms,
                          "gather_frac": [frac(nbytes, x) for x in g_ms],
                          "spread_ms": round(max(abs(ms[0] - ms[1]), abs(t_ms[0] - t_ms[1])), 4),
                          "scatter_over_index_copy": round(min(ms) / min(t_ms), 3),
                          "scatter_frac_over_gather_frac": round(min(g_ms) / min(ms), 3),
                          "matches_index_copy": same}), flush=True)
        if not same:
            sys.exit("scatter differs from torch.index_copy_ on the %s list" % name)
    del back, ref
    torch.cuda.empty_cache()

    # merge: the class's second-stage results into the batch's
    idx = d_index[lo:lo + k]
    idx64 = idx.long()
    ret2 = torch.arange(k, dtype=torch.int64, device=dev)
    flt2 = torch.ones(k, dtype=torch.uint8, device=dev)
    m_ret, m_flt = d_ret.clone(), d_flt.clone()
    t_ret, t_flt = d_ret.clone(), d_flt.clone()
    ms = twice(torch, lambda: native.merge_dev(0, m_ret.data_ptr(), m_flt.data_ptr(), n, idx.data_ptr(),
                                               k, ret2.data_ptr(), flt2.data_ptr(), st), a)
    r_ms = twice(torch, lambda: t_ret.index_copy_(0, idx64, ret2), a)
    rf_ms = twice(torch, lambda: (t_ret.index_copy_(0, idx64, ret2),
                                  t_flt.index_copy_(0, idx64, flt2)), a)
    same = bool(torch.equal(m_ret, t_ret)) and bool(torch.equal(m_flt, t_flt))
    nbytes = k * (4 + 9 + 9)
    merge_ms = min(ms)
    print(json.dumps({"what": "merge", "class": b, "entries": k, "ms": ms, "bytes": nbytes,
                      "frac": [frac(nbytes, x) for x in ms], "ret_index_copy_ms": r_ms,
                      "ret_and_faults_index_copy_ms": rf_ms,
                      "merge_over_ret_index_copy": round(min(ms) / min(r_ms), 3),
                      "merge_over_both_index_copies": round(min(ms) / min(rf_ms), 3),
                      "matches_index_copy": same}), flush=True)
    if not same:
        sys.exit("merge differs from torch.index_copy_")
    del m_ret, m_flt, t_ret, t_flt

    # the closed pipeline, per packet of the class
    native.gather_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), k, 64, dense.data_ptr(), k * 64,
                      stream=st)
    ext = torch.zeros(2 * k, dtype=torch.int64, device=dev)
    sel_ms = twice(torch, lambda: native.select_dev(0, data.data_ptr(), n, 64, idx.data_ptr(), k,
                                                    ext.data_ptr(), stream=st), a)
    r2 = torch.zeros(k, dtype=torch.int64, device=dev)
    g_ms, g_lay = c3_ms(torch, a, p3, st, dense.data_ptr(), k, 64, r2)
    s_ms, s_lay = c3_ms(torch, a, p3, st, data.data_ptr(), k, 0, r2, ext.data_ptr(), True)
    ns = lambda ms_: ms_ * 1e6 / k
    gather_ms, scatter_ms = times["class"]
    moved = gather_ms + scatter_ms + merge_ms
    gain = s_ms - g_ms
    print(json.dumps({"what": "pipeline_c3", "class": b, "class_packets": k,
                      "gather_ns": round(ns(gather_ms), 4), "staged_c3_ns": round(ns(g_ms), 4),
                      "staged_layout": g_lay, "scatter_ns": round(ns(scatter_ms), 4),
                      "merge_ns": round(ns(merge_ms), 4),
                      "dense_route_ns": round(ns(moved + g_ms), 4),
                      "select_ns": round(ns(min(sel_ms)), 4), "in_place_c3_ns": round(ns(s_ms), 4),
                      "in_place_layout": s_lay,
                      "in_place_route_ns": round(ns(min(sel_ms) + s_ms), 4),
                      "break_even_passes_gather_only": round(gather_ms / gain, 2) if gain > 0 else None,
                      "break_even_passes_class_returns":
                      round((moved - min(sel_ms)) / gain, 2) if gain > 0 else None}), flush=True)
    p.destroy()
    m.destroy()


def general(torch, a):
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    n = a.imix
    h_data, h_offs, h_sizes = workloads.packets_imix_range(0, n, seed=5)
    ext = np.stack([h_offs[:-1], h_offs[:-1] + h_sizes], axis=1).reshape(-1)
    buf = torch.zeros(len(h_data) + 64, dtype=torch.uint8, device=dev)
    buf[:len(h_data)] = torch.from_numpy(h_data).to(dev)
    d_ext = torch.from_numpy(ext.view(np.int64)).to(dev)
    listed = np.arange(0, n, 2)
    k = len(listed)
    idx = torch.from_numpy(listed.astype(np.int32)).to(dev)
    payload = int(h_sizes[listed].sum())
    dense = torch.empty(max(payload, k * 64) + 64, dtype=torch.uint8, device=dev)
    offs = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    back = torch.zeros_like(buf)
    for what, in_stride, moved in (("scatter_packed", 0, payload), ("scatter_stride64", 64, k * 64)):
        size = moved
        o_ptr = offs.data_ptr() if in_stride == 0 else None
        g_ms = twice(torch, lambda: native.gather_dev(0, buf.data_ptr(), n, 0, idx.data_ptr(), k,
                                                      in_stride, dense.data_ptr(), size, o_ptr,
                                                      d_ext.data_ptr(), st, extents=True), a)
        back.zero_()
        ms = twice(torch, lambda: native.scatter_dev(0, back.data_ptr(), n, 0, idx.data_ptr(), k,
                                                     in_stride, dense.data_ptr(), size, o_ptr,
                                                     d_ext.data_ptr(), st, extents=True), a)
        # gathering what was scattered gives the dense bytes again; nothing else was written
        again = torch.empty_like(dense)
        native.gather_dev(0, back.data_ptr(), n, 0, idx.data_ptr(), k, in_stride, again.data_ptr(),
                          size, o_ptr, d_ext.data_ptr(), st, extents=True)
        ok = bool(torch.equal(again[:size], dense[:size])) and \
            int(torch.count_nonzero(back)) == int(torch.count_nonzero(dense[:size]))
        del again
        nbytes = k * (4 + (8 if in_stride == 0 else 0)) + 2 * moved
        print(json.dumps({"what": what, "packets": k, "payload_bytes": moved, "ms": ms,
                          "bytes": nbytes, "frac": [frac(nbytes, x) for x in ms],
                          "gather_ms": g_ms, "gather_frac": [frac(nbytes, x) for x in g_ms],
                          "scatter_frac_over_gather_frac": round(min(g_ms) / min(ms), 3),
                          "correct": ok}), flush=True)
        if not ok:
            sys.exit("%s wrong" % what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 26)
    ap.add_argument("--imix", type=int, default=1 << 22)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["all", "rows", "general"], default="all")
    a = ap.parse_args()
    import torch
    if native.gpu_count() < 1:
        sys.exit("scatter_bench needs a GPU: %s" % native.last_error())
    env = native.Env()
    lay3 = workloads.prog_c3()
    p3 = native.Prog(env, native.patch_relocs(lay3.code, lay3.relocs, []))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps({"what": "library", "path": os.path.relpath(native.LIB_PATH, root)}), flush=True)
    if a.only != "general":
        rows_merge_pipeline(torch, a, env, p3)
        torch.cuda.empty_cache()
    if a.only != "rows":
        general(torch, a)
    p3.destroy()
    env.destroy()


if __name__ == "__main__":
    main()
