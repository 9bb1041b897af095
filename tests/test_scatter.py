"""Scattering a dense batch back and merging a second stage's results on the host
(include/ebpf_gpu.h: ebpf_batch_scatter, ebpf_batch_merge) against a numpy restatement of the
header's rules, and the argument checks of the four entry points, which come before any device
work and so hold without a GPU.

A copy has one right answer, so every comparison is exact.  The batch's data lies inside a larger
buffer filled with 0xA5 and is compared whole: a byte touched outside a listed packet's first k_j
bytes — a gap, an unlisted neighbour, the rest of a packet longer than its slot, the frame —
shows up."""
import ctypes
import errno

import numpy as np
import pytest

from test_gather import (FAKE, G4, PAD, SENTINEL, STRIDES, Src, U64, check_frame, expected, listed,
                         lists, sources, spans)

FLIP = 0x5C


# ---------------------------------------------------------------- the rules, in numpy


def slots(n, in_stride, in_offsets=None, in_bytes=None):
    """(start, length) of the dense side's n slots, int64: strided, or packed and read as an
    offsets-form batch reads it, then cut at in_bytes"""
    if in_stride:
        return np.arange(n, dtype=np.int64) * in_stride, np.full(n, in_stride, dtype=np.int64)
    o = np.asarray(in_offsets, dtype=np.int64)
    at, e = o[:n], o[1:n + 1]
    m = np.where((e < at) | (e - at >= G4), 0, e - at)
    if in_bytes is not None:
        m = np.minimum(m, np.maximum(in_bytes - at, 0))
    return at, m


def copied(src, index, in_stride, in_offsets=None, in_bytes=None):
    """(positions in the batch's data, positions in the dense input) of every byte that moves:
    packet index[j]'s first k_j = min(len_j, slot j's length) bytes"""
    s, ln = listed(src, index)
    at, m = slots(len(s), in_stride, in_offsets, in_bytes)
    k = np.minimum(ln, m)
    first = np.cumsum(k) - k
    ramp = np.arange(int(k.sum()), dtype=np.int64) - np.repeat(first, k)
    return np.repeat(s, k) + ramp, np.repeat(at, k) + ramp


def expected_scatter(src, index, dense, in_stride, in_offsets=None, in_bytes=None):
    """the batch's data after the scatter (listings that share a byte must agree on it)"""
    to, frm = copied(src, index, in_stride, in_offsets, in_bytes)
    data = src.data.copy()
    data[to] = np.asarray(dense, dtype=np.uint8)[frm]
    return data


def scatter_lists(count):
    """the lists without repeats: a steered class, the whole steering index, descending, and
    indices at and past count"""
    ls = lists(count)
    return {"class": ls["class"], "whole": ls["whole"], "descending": ls["descending"],
            "odd": np.array([5, count, 0, count - 1, 0xffffffff, count + 7, 6], dtype=np.uint32)}


def scatter_sources():
    """(the overlapping extents are left out: what a scatter into them leaves is unspecified)"""
    return [s for s in sources() if s.name != "overlap"]


# ---------------------------------------------------------------- the host function, framed


def run_host(native, src, index, dense, in_stride, in_offsets=None, in_bytes=None, want=None):
    """ebpf_batch_scatter into a framed copy of the batch's data; the whole frame is checked
    against the numpy rules (or `want`); returns the data after the call"""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    dense = np.ascontiguousarray(dense, dtype=np.uint8)
    n = len(index)
    if in_bytes is None:
        in_bytes = len(dense)
    if want is None:
        want = expected_scatter(src, index, dense, in_stride, in_offsets, in_bytes)
    buf = np.full(PAD + len(src.data) + PAD, SENTINEL, dtype=np.uint8)
    buf[PAD:PAD + len(src.data)] = src.data
    offs = None if src.offsets is None else np.ascontiguousarray(src.offsets, dtype=U64)
    b = native.PktBatch(buf.ctypes.data + PAD, None if offs is None else offs.ctypes.data,
                        src.count, src.stride, native.BATCH_EXTENTS if src.extents else 0)
    in_offs = None if in_offsets is None else np.ascontiguousarray(in_offsets, dtype=U64)
    keep = dense.copy()
    code = native.lib().ebpf_batch_scatter(ctypes.byref(b), index.ctypes.data if n else None, n,
                                           in_stride, dense.ctypes.data if n else None, in_bytes,
                                           None if in_offs is None else in_offs.ctypes.data)
    what = "%s in_stride %d n %d" % (src.name, in_stride, n)
    assert code == 0, what
    check_frame(buf, PAD, want, what)
    np.testing.assert_array_equal(dense, keep, err_msg=what + ": the input changed")
    return buf[PAD:PAD + len(src.data)].copy()


@pytest.mark.parametrize("src", scatter_sources(), ids=lambda s: s.name)
def test_scatter_sources_lists_and_forms(native, src):
    g = np.random.default_rng(41)
    changed = 0
    for name, index in scatter_lists(src.count).items():
        n = len(index)
        for in_stride in STRIDES:
            dense = g.integers(0, 256, n * in_stride + 5, dtype=np.uint8)
            after = run_host(native, src, index, dense, in_stride, in_bytes=n * in_stride)
            changed += int((after != src.data).sum())
        # packed: slots of the packets' own lengths, and slots of lengths of their own (shorter
        # and longer than the packets, empty ones among them)
        own = expected(src, index, 0)[1]
        other = np.concatenate([[0], np.cumsum(g.integers(0, 121, n))]).astype(U64)
        for in_offs in (own, other):
            dense = g.integers(0, 256, int(in_offs[-1]) + 5, dtype=np.uint8)
            after = run_host(native, src, index, dense, 0, in_offs, in_bytes=int(in_offs[-1]))
            changed += int((after != src.data).sum())
    assert changed > 10000


@pytest.mark.parametrize("src", scatter_sources(), ids=lambda s: s.name)
def test_scatter_round_trips(native, src):
    """gather then scatter leaves the batch as it was; with every dense byte flipped between the
    two, exactly the listed packets' first k_j bytes flip (duplicates agree, so `dups` holds)"""
    ls = dict(scatter_lists(src.count), dups=lists(src.count)["dups"])
    for name, index in ls.items():
        n = len(index)
        s, ln = listed(src, index)
        for st in STRIDES + [0]:
            dense, offs, code = native.gather(src.data, src.count, index, out_stride=st,
                                              stride=src.stride, offsets=src.offsets,
                                              extents=src.extents)
            assert code == 0
            run_host(native, src, index, dense, st, offs, want=src.data)
            k = np.minimum(ln, st) if st else ln
            want = src.data.copy()
            first = np.cumsum(k) - k
            pos = np.repeat(s, k) + np.arange(int(k.sum()), dtype=np.int64) - np.repeat(first, k)
            want[np.unique(pos)] ^= FLIP
            after = run_host(native, src, index, dense ^ FLIP, st, offs, want=want)
            np.testing.assert_array_equal(
                after, expected_scatter(src, index, dense ^ FLIP, st, offs), err_msg=name)
    # the wrapper, in place
    index = ls["class"]
    data = src.data.copy()
    dense = native.gather(src.data, src.count, index, out_stride=64, stride=src.stride,
                          offsets=src.offsets, extents=src.extents)[0]
    native.scatter(data, src.count, index, dense ^ FLIP, in_stride=64, stride=src.stride,
                   offsets=src.offsets, extents=src.extents)
    np.testing.assert_array_equal(data, expected_scatter(src, index, dense ^ FLIP, 64))


def test_scatter_of_a_truncated_gather(native):
    """{in, in_offsets} as a packed gather with too little room left them: only what was gathered
    goes back, whether the cut falls inside a packet or on a packet's end"""
    src = sources()[1]
    index = scatter_lists(src.count)["class"]
    offs = expected(src, index, 0)[1].astype(np.int64)
    j = int(np.flatnonzero(np.diff(offs) > 2)[len(index) // 2])
    s, ln = listed(src, index)
    for out_bytes in (int(offs[j]) + 1, int(offs[j + 1]), 0):
        dense, g_offs, code = native.gather(src.data, src.count, index, offsets=src.offsets,
                                            out_bytes=out_bytes)
        assert code == errno.ENOSPC and len(dense) == out_bytes < int(g_offs[-1])
        # the caller's buffer goes on behind out_bytes: nothing of it may be used
        room = np.concatenate([dense, np.full(int(g_offs[-1]) - out_bytes + 8, 0xEE, np.uint8)])
        run_host(native, src, index, room, 0, g_offs, in_bytes=out_bytes, want=src.data)
        to, frm = copied(src, index, 0, g_offs, out_bytes)
        assert len(to) == out_bytes and (len(frm) == 0 or frm.max() == out_bytes - 1)
        want = src.data.copy()
        want[to] ^= FLIP
        run_host(native, src, index, room ^ FLIP, 0, g_offs, in_bytes=out_bytes, want=want)


def test_scatter_length_zero_rules(native):
    """the degenerate extents of test_gather_length_zero_rules: a packet of length 0 takes no
    byte, wherever its start and end point; so does a degenerate slot of the packed form"""
    g = np.random.default_rng(4)
    data = g.integers(1, 256, 4096, dtype=np.uint8)
    ext = np.array([[0, 64], [300, 250], [512, 576], [1024, 1024 + G4], [2048, 2112],
                    [100, 100 + G4 - 1]], dtype=U64)
    src = Src("degenerate", data, 6, 0, ext.reshape(-1), True)
    index = np.array([1, 0, 3, 2, 4], dtype=np.uint32)   # (never the 4 GiB packet)
    for in_stride in (16, 64, 100):
        dense = g.integers(0, 256, len(index) * in_stride, dtype=np.uint8)
        after = run_host(native, src, index, dense, in_stride)
        k = min(in_stride, 64)
        touched = np.flatnonzero(after != data)
        assert len(touched) > 0 and set(touched // 512) <= {0, 1, 4} and (touched % 512 < k).all()
    dense, offs, _ = native.gather(data, 6, index, offsets=src.offsets, extents=True)
    assert offs.tolist() == [0, 0, 64, 64, 128, 192]
    run_host(native, src, index, dense ^ FLIP, 0, offs)
    # slots of the packed form: an end below the start, and an end 2^32 past it, hold nothing
    csr = Src("csr", data, 3, 0, np.array([0, 100, 200, 300], dtype=U64), False)
    in_offs = np.array([50, 20, 20 + G4, 60], dtype=U64)
    assert slots(3, 0, in_offs)[1].tolist() == [0, 0, 0]
    run_host(native, csr, [0, 1, 2], np.zeros(64, dtype=np.uint8), 0, in_offs, want=data)
    # offsets form: a decreasing entry makes one packet's end fall below its start
    dip = Src("csr_dip", data, 3, 0, np.array([0, 100, 40, 90], dtype=U64), False)
    assert spans(dip)[1].tolist() == [100, 0, 50]
    after = run_host(native, dip, [1, 2], np.zeros(128, dtype=np.uint8), 64)
    assert (after[40:90] == 0).all() and (after[90:] == data[90:]).all()


def test_scatter_empty_list_and_empty_batch(native):
    src = sources()[0]
    run_host(native, src, [], np.zeros(0, dtype=np.uint8), 64, want=src.data)
    run_host(native, src, [], np.zeros(0, dtype=np.uint8), 0, np.zeros(1, dtype=U64), want=src.data)
    empty = Src("empty", src.data, 0, 64, None, False)
    run_host(native, empty, [0, 5, 0xffffffff], np.zeros(48, dtype=np.uint8), 16, want=src.data)


# ---------------------------------------------------------------- merge

RET_GUARD = 0x5a5a5a5a5a5a5a5a


def expected_merge(ret, faults, index, ret2, faults2):
    """(ret, faults) after the merge (duplicate listings must agree)"""
    index = np.asarray(index, dtype=np.int64)
    ok = index < len(ret)
    ret = ret.copy()
    ret[index[ok]] = np.asarray(ret2, dtype=U64)[ok]
    if faults is not None:
        faults = faults.copy()
        faults[index[ok]] = 0 if faults2 is None else np.asarray(faults2, dtype=np.uint8)[ok]
    return ret, faults


def run_merge(native, ret, faults, index, ret2, faults2):
    """ebpf_batch_merge on framed copies of ret and faults, checked against numpy"""
    count, n = len(ret), len(index)
    index = np.ascontiguousarray(index, dtype=np.uint32)
    ret2 = np.ascontiguousarray(ret2, dtype=U64)
    w_ret, w_flt = expected_merge(ret, faults, index, ret2, faults2)
    r = np.full(count + 16, RET_GUARD, dtype=U64)
    r[8:8 + count] = ret
    f = None
    if faults is not None:
        f = np.full(count + 2 * PAD, SENTINEL, dtype=np.uint8)
        f[PAD:PAD + count] = faults
    code = native.lib().ebpf_batch_merge(
        r.ctypes.data + 64, None if f is None else f.ctypes.data + PAD, count,
        index.ctypes.data if n else None, n, ret2.ctypes.data if n else None,
        None if faults2 is None or not n else faults2.ctypes.data)
    assert code == 0
    assert (r[:8] == RET_GUARD).all() and (r[8 + count:] == RET_GUARD).all()
    np.testing.assert_array_equal(r[8:8 + count], w_ret)
    if f is not None:
        check_frame(f, PAD, w_flt, "faults")
    return w_ret, w_flt


def test_merge_against_numpy(native):
    g = np.random.default_rng(42)
    count = 1000
    ret = g.integers(0, 1 << 63, count).astype(U64)
    faults = g.integers(0, 4, count).astype(np.uint8)
    for name, index in scatter_lists(count).items():
        n = len(index)
        ret2 = g.integers(0, 1 << 63, n).astype(U64)
        faults2 = g.integers(1, 9, n).astype(np.uint8)
        for f in (faults, None):
            for f2 in (faults2, None):
                run_merge(native, ret, f, index, ret2, f2)
        w_ret, w_flt = run_merge(native, ret, faults, index, ret2, None)
        inside = index[index < count].astype(np.int64)
        assert (w_ret != ret).any() and (w_flt[inside] == 0).all() and faults[inside].any()
    run_merge(native, ret, faults, [], [], None)
    run_merge(native, ret[:0], faults[:0], [0, 7, 0xffffffff], [1, 2, 3], None)
    # the wrapper, in place; a whole steering index puts a class-ordered ret back in packet order
    index, starts = native.steer(ret, faults)
    r, f = np.zeros(count, dtype=U64), np.full(count, 9, dtype=np.uint8)
    native.merge(r, f, index, ret[index], faults[index])
    np.testing.assert_array_equal(r, ret)
    np.testing.assert_array_equal(f, faults)


# ---------------------------------------------------------------- argument checks


def _scatter_calls(native):
    """both entry points as f(batch, index, n, in_stride, in, in_bytes, in_offsets)"""
    L = native.lib()
    ref = lambda b: None if b is None else ctypes.byref(b)
    yield "host", lambda b, *a: L.ebpf_batch_scatter(ref(b), *a)
    for dev in (0, 1 << 20):
        yield "dev%d" % dev, lambda b, *a, d=dev: L.ebpf_batch_scatter_dev(d, ref(b), *a, None)


def test_scatter_argument_checks(native):
    """EINVAL and E2BIG with nothing dereferenced, on both entry points; on the device function
    they come before the device is looked at"""
    good = native.PktBatch(FAKE, None, 8, 64, 0)
    for name, f in _scatter_calls(native):
        assert f(None, FAKE, 1, 64, FAKE, 64, None) == errno.EINVAL, name
        for bad in (native.PktBatch(None, None, 8, 64, 0), native.PktBatch(FAKE, None, 8, 0, 0),
                    native.PktBatch(FAKE, None, 8, 64, 0x80),
                    native.PktBatch(FAKE, None, 8, 0, native.BATCH_EXTENTS)):
            assert f(bad, FAKE, 1, 64, FAKE, 64, None) == errno.EINVAL, name
        assert f(good, None, 1, 64, FAKE, 64, None) == errno.EINVAL, name
        assert f(good, FAKE, 1, 64, None, 64, None) == errno.EINVAL, name
        assert f(good, FAKE, 1, 64, FAKE, 64, FAKE) == errno.EINVAL, name   # strided + offsets
        assert f(good, FAKE, 1, 0, FAKE, 64, None) == errno.EINVAL, name    # packed, no offsets
        assert f(good, None, 0, 0, None, 0, None) == errno.EINVAL, name
        assert f(good, FAKE, 2, 64, FAKE, 127, None) == errno.EINVAL, name  # n * stride > bytes
        # (a product that does not fit 64 bits must not pass as a small one)
        assert f(good, FAKE, 0xffffffff, 0xffffffff, FAKE, 1 << 20, None) == errno.EINVAL, name
        assert f(good, FAKE, 1 << 32, 64, FAKE, 1 << 40, None) == errno.E2BIG, name
        assert f(good, FAKE, 1 << 32, 0, FAKE, 1 << 40, FAKE) == errno.E2BIG, name
    L = native.lib()
    assert L.ebpf_batch_scatter(ctypes.byref(good), None, 0, 64, None, 0, None) == 0
    assert L.ebpf_batch_scatter(ctypes.byref(good), None, 0, 0, None, 0, FAKE) == 0
    hist = native.PktBatch(FAKE, None, 8, 64, native.BATCH_HIST_OVERWRITE)
    assert L.ebpf_batch_scatter(ctypes.byref(hist), None, 0, 64, None, 0, None) == 0
    bad_dev = lambda n, st, offs: L.ebpf_batch_scatter_dev(1 << 20, ctypes.byref(good), FAKE, n, st,
                                                           FAKE, 1 << 20, offs, None)
    assert bad_dev(3, 64, None) == errno.ENODEV
    assert bad_dev(0, 64, None) == errno.ENODEV
    assert bad_dev(3, 0, FAKE) == errno.ENODEV
    assert L.ebpf_batch_scatter_dev(-1, ctypes.byref(good), FAKE, 3, 64, FAKE, 1 << 20, None,
                                    None) == errno.ENODEV
    if native.gpu_count() == 0:
        assert L.ebpf_batch_scatter_dev(0, ctypes.byref(good), FAKE, 3, 64, FAKE, 1 << 20, None,
                                        None) == errno.ENODEV


def test_merge_argument_checks(native):
    L = native.lib()
    calls = [("host", lambda *a: L.ebpf_batch_merge(*a))]
    for dev in (0, 1 << 20):
        calls.append(("dev%d" % dev, lambda *a, d=dev: L.ebpf_batch_merge_dev(d, *a, None)))
    for name, f in calls:   # f(ret, faults, count, index, n, ret2, faults2)
        assert f(None, FAKE, 8, FAKE, 1, FAKE, FAKE) == errno.EINVAL, name
        assert f(FAKE, FAKE, 8, None, 1, FAKE, FAKE) == errno.EINVAL, name
        assert f(FAKE, FAKE, 8, FAKE, 1, None, FAKE) == errno.EINVAL, name
        assert f(FAKE, None, 8, FAKE, 1 << 32, FAKE, None) == errno.E2BIG, name
    assert L.ebpf_batch_merge(None, None, 8, None, 0, None, None) == 0
    assert L.ebpf_batch_merge(FAKE, FAKE, 0, None, 0, None, None) == 0
    bad_dev = lambda n: L.ebpf_batch_merge_dev(1 << 20, FAKE, FAKE, 8, FAKE, n, FAKE, FAKE, None)
    assert bad_dev(3) == errno.ENODEV and bad_dev(0) == errno.ENODEV
    assert L.ebpf_batch_merge_dev(-1, FAKE, None, 8, FAKE, 3, FAKE, None, None) == errno.ENODEV
    if native.gpu_count() == 0:
        assert L.ebpf_batch_merge_dev(0, FAKE, None, 8, FAKE, 3, FAKE, None, None) == errno.ENODEV
