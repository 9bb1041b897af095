"""Grouping a batch by key on the host (include/ebpf_gpu.h: ebpf_batch_group) against numpy's
stable sort, and the argument checks of ebpf_batch_group / ebpf_batch_group_dev /
ebpf_batch_group_tmp_bytes, which come before any device work and so hold without a GPU.

A stable sort has one right answer, so every comparison is exact.  Keys stay unsigned 64-bit."""
import ctypes
import errno

import numpy as np
import pytest

U64 = np.uint64
SENTINEL = 0xdeadbeefdeadbeef   # fills a table's tail; no position and no test key has this value


def keys_of(ret, shift, bits):
    mask = U64((1 << bits) - 1)
    return (np.asarray(ret, dtype=U64) >> U64(shift)) & mask


def expected(ret, faults, shift, bits):
    """(index, group_keys, group_starts with the closing entry, U)"""
    ret = np.asarray(ret, dtype=U64)
    n = len(ret)
    flt = np.zeros(n, dtype=np.uint8) if faults is None else np.asarray(faults)
    k = keys_of(ret, shift, bits)
    k[flt != 0] = 0   # a faulted packet's ret is not looked at: among themselves, packet order
    o = np.argsort(k, kind="stable")
    o = o[np.argsort(flt[o] != 0, kind="stable")]
    u = int((flt == 0).sum())
    ks = k[o[:u]]
    heads = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if u else np.zeros(0, int)
    return (o.astype(np.uint32), ks[heads].astype(U64),
            np.concatenate([heads, [u]]).astype(U64), u)


def check(native, ret, faults=None, shift=0, bits=32):
    ret = np.asarray(ret, dtype=U64)
    index, gkeys, gstarts, info, code = native.group(ret, faults, shift, bits)
    w_index, w_keys, w_starts, u = expected(ret, faults, shift, bits)
    g = len(w_keys)
    assert code == 0 and info.tolist() == [g, u]
    np.testing.assert_array_equal(index, w_index)
    np.testing.assert_array_equal(gkeys[:g], w_keys)
    np.testing.assert_array_equal(gstarts[:g + 1], w_starts)
    return index, gkeys[:g], gstarts[:g + 1]


def garbage(g, field, shift, bits):
    """ret whose field at (shift, bits) is `field` and whose other bits are random"""
    field = np.asarray(field, dtype=U64)
    noise = g.integers(0, 1 << 64, len(field), dtype=U64)
    mask = U64(((1 << bits) - 1) << shift)
    return (noise & ~mask) | ((field << U64(shift)) & mask)


@pytest.mark.parametrize("count", [0, 1, 257, 100003])
def test_counts(native, count):
    g = np.random.default_rng(count)
    ret = g.integers(0, 1 << 64, count, dtype=U64)
    faults = (g.integers(0, 8, count) == 0).astype(np.uint8) * 7
    for bits in (10, 32, 64):
        index, gkeys, gstarts = check(native, ret, faults, 0, bits)
        check(native, ret, None, 0, bits)
    if count == 0:
        assert len(index) == 0 and len(gkeys) == 0 and gstarts.tolist() == [0]


@pytest.mark.parametrize("bits", [1, 8, 10, 13, 32, 64])
@pytest.mark.parametrize("shift", [0, 3, 32, 51])
def test_field_with_garbage_around_it(native, bits, shift):
    """few distinct field values under random bits above and below the field: equal fields stay in
    packet order and form one group"""
    if shift + bits > 64:
        assert native.lib().ebpf_batch_group(4096, None, 1, shift, bits, 4096, 0, None, None,
                                             4096) == errno.EINVAL
        return
    g = np.random.default_rng(bits * 64 + shift)
    n = 5003
    vals = g.integers(0, 1 << bits, 12, dtype=U64) if bits < 64 else \
        g.integers(0, 1 << 64, 12, dtype=U64)
    field = vals[g.integers(0, len(vals), n)]
    ret = garbage(g, field, shift, bits)
    faults = (np.arange(n) % 11 == 10).astype(np.uint8)
    index, gkeys, gstarts = check(native, ret, faults, shift, bits)
    assert len(gkeys) == len(np.unique(field[faults == 0])) <= 12
    np.testing.assert_array_equal(gkeys, np.unique(field[faults == 0]))
    for a, b in zip(gstarts[:-1].tolist(), gstarts[1:].tolist()):
        assert (np.diff(index[a:b].astype(np.int64)) > 0).all()
    check(native, ret, None, shift, bits)


def test_faulted_packets_with_nonzero_ret_go_last(native):
    ret = np.array([5, 1 << 63, 5, 0, 9, 2], dtype=U64)
    faults = np.array([0, 3, 0, 0, 0, 200], dtype=np.uint8)
    index, gkeys, gstarts = check(native, ret, faults, 0, 64)
    assert index.tolist() == [3, 0, 2, 4, 1, 5]
    assert gkeys.tolist() == [0, 5, 9] and gstarts.tolist() == [0, 1, 3, 4]
    index, gkeys, gstarts = check(native, ret, None, 0, 64)
    assert index.tolist() == [3, 5, 0, 2, 4, 1] and gkeys[-1] == 1 << 63


def test_all_faulted(native):
    ret = np.arange(100, dtype=U64)
    index, gkeys, gstarts = check(native, ret, np.full(100, 9, dtype=np.uint8), 0, 8)
    assert index.tolist() == list(range(100)) and len(gkeys) == 0 and gstarts.tolist() == [0]


def _raw(native, ret, faults, shift, bits, cap, with_keys=True, with_starts=True):
    """the raw call with sentinel-filled tables one entry longer than they have to be"""
    n = len(ret)
    index = np.full(n, 0xffffffff, dtype=np.uint32)
    gkeys = np.full(cap + 1, SENTINEL, dtype=U64)
    gstarts = np.full(cap + 2, SENTINEL, dtype=U64)
    info = np.full(2, SENTINEL, dtype=U64)
    code = native.lib().ebpf_batch_group(
        ret.ctypes.data, None if faults is None else faults.ctypes.data, n, shift, bits,
        index.ctypes.data, cap, gkeys.ctypes.data if with_keys else None,
        gstarts.ctypes.data if with_starts else None, info.ctypes.data)
    return code, index, gkeys, gstarts, info


def test_group_cap(native):
    g = np.random.default_rng(5)
    n = 4000
    ret = g.integers(0, 300, n).astype(U64)
    faults = (np.arange(n) % 7 == 0).astype(np.uint8)
    w_index, w_keys, w_starts, u = expected(ret, faults, 0, 16)
    G = len(w_keys)
    assert G > 100
    for cap in (G + 5, G, G - 1, 1):
        code, index, gkeys, gstarts, info = _raw(native, ret, faults, 0, 16, cap)
        m = min(G, cap)
        assert code == (0 if G <= cap else errno.ENOSPC), cap
        assert info.tolist() == [G, u]
        np.testing.assert_array_equal(index, w_index)
        np.testing.assert_array_equal(gkeys[:m], w_keys[:m])
        assert (gkeys[m:] == SENTINEL).all()
        if G <= cap:
            np.testing.assert_array_equal(gstarts[:G + 1], w_starts)
            assert (gstarts[G + 1:] == SENTINEL).all()
        else:
            np.testing.assert_array_equal(gstarts[:m], w_starts[:m])
            assert (gstarts[m:] == SENTINEL).all()
    # no keys wanted: the starts alone
    code, index, gkeys, gstarts, info = _raw(native, ret, faults, 0, 16, G, with_keys=False)
    assert code == 0 and (gkeys == SENTINEL).all()
    np.testing.assert_array_equal(gstarts[:G + 1], w_starts)
    # cap 0: sort and count; the one entry of group_starts is not G's, so it stays
    code, index, gkeys, gstarts, info = _raw(native, ret, faults, 0, 16, 0, with_keys=False)
    assert code == errno.ENOSPC and info.tolist() == [G, u] and (gstarts == SENTINEL).all()
    np.testing.assert_array_equal(index, w_index)
    code, index, gkeys, gstarts, info = _raw(native, ret, faults, 0, 16, 0, False, False)
    assert code == errno.ENOSPC and info.tolist() == [G, u]
    np.testing.assert_array_equal(index, w_index)
    # cap 0 and no group at all: complete, and the closing start is written
    allf = np.ones(n, dtype=np.uint8)
    code, index, gkeys, gstarts, info = _raw(native, ret, allf, 0, 16, 0, with_keys=False)
    assert code == 0 and info.tolist() == [0, 0] and gstarts.tolist() == [0, SENTINEL]


FAKE = 4096   # a non-NULL pointer that nothing may dereference


def test_group_argument_checks(native):
    L = native.lib()
    info = (ctypes.c_uint64 * 2)(77, 77)
    starts = (ctypes.c_uint64 * 2)(77, 77)
    f = L.ebpf_batch_group
    for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32), (60, 5), (0xffffffff, 2)):
        assert f(FAKE, None, 1, shift, bits, FAKE, 0, None, None, info) == errno.EINVAL
    assert f(FAKE, None, 1, 0, 32, FAKE, 0, None, None, None) == errno.EINVAL
    assert f(None, None, 1, 0, 32, FAKE, 0, None, None, info) == errno.EINVAL
    assert f(FAKE, None, 1, 0, 32, None, 0, None, None, info) == errno.EINVAL
    assert f(FAKE, None, 1, 0, 32, FAKE, 1, FAKE, None, info) == errno.EINVAL
    assert f(None, None, 0, 0, 32, None, 0, None, None, None) == errno.EINVAL
    assert f(FAKE, None, 1 << 32, 0, 32, FAKE, 1, FAKE, starts, info) == errno.E2BIG
    assert list(info) == [77, 77] and list(starts) == [77, 77]
    assert f(None, None, 0, 0, 32, None, 1, None, starts, info) == 0
    assert list(info) == [0, 0] and list(starts) == [0, 77]
    info[0] = info[1] = 77
    assert f(None, None, 0, 63, 1, None, 0, None, None, info) == 0 and list(info) == [0, 0]


def test_group_dev_argument_checks(native):
    """EINVAL, E2BIG and the short tmp_bytes' ENOSPC before the device is looked at; then, on a
    machine without a GPU (or for a device out of range), ENODEV with nothing dereferenced"""
    L = native.lib()
    f = L.ebpf_batch_group_dev
    need = native.group_tmp_bytes(5, 32)
    assert need > 0
    for dev in (0, 1 << 20):
        for shift, bits in ((0, 0), (0, 65), (1, 64), (64, 1), (33, 32)):
            assert f(dev, FAKE, None, 1, shift, bits, FAKE, 0, None, None, FAKE, FAKE, 1 << 20,
                     None) == errno.EINVAL
        assert f(dev, FAKE, None, 5, 0, 32, FAKE, 0, None, None, None, FAKE, need,
                 None) == errno.EINVAL
        assert f(dev, None, None, 5, 0, 32, FAKE, 0, None, None, FAKE, FAKE, need,
                 None) == errno.EINVAL
        assert f(dev, FAKE, None, 5, 0, 32, None, 0, None, None, FAKE, FAKE, need,
                 None) == errno.EINVAL
        assert f(dev, FAKE, None, 5, 0, 32, FAKE, 1, FAKE, None, FAKE, FAKE, need,
                 None) == errno.EINVAL
        assert f(dev, None, None, 0, 0, 32, None, 0, None, None, None, None, 0,
                 None) == errno.EINVAL
        assert f(dev, FAKE, FAKE, 1 << 32, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, 1 << 40,
                 None) == errno.E2BIG
        assert f(dev, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, need - 1,
                 None) == errno.ENOSPC
        assert f(dev, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, 0,
                 None) == errno.ENOSPC
        assert f(dev, FAKE, FAKE, 5, 0, 64, FAKE, 1, FAKE, FAKE, FAKE, FAKE, need,
                 None) == errno.ENOSPC            # (64-bit keys need more than 32-bit ones)
        assert f(dev, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, None, need,
                 None) == errno.EINVAL
    assert f(1 << 20, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, need,
             None) == errno.ENODEV
    assert f(-1, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, need, None) == errno.ENODEV
    assert f(1 << 20, None, None, 0, 0, 32, None, 0, None, None, FAKE, None, 0,
             None) == errno.ENODEV
    if native.gpu_count() == 0:
        assert f(0, FAKE, FAKE, 5, 0, 32, FAKE, 1, FAKE, FAKE, FAKE, FAKE, need,
                 None) == errno.ENODEV
        assert f(0, None, None, 0, 0, 32, None, 0, None, None, FAKE, None, 0,
                 None) == errno.ENODEV


def test_group_tmp_bytes(native):
    """the header's formula and bound: at most 2 * (8 + 4) bytes a packet plus a fixed term; less
    for keys of 32 bits or fewer; monotone in count; 0 for what the calls refuse"""
    fixed = 2 * (8 + 4) * 63
    counts = [0, 1, 63, 64, 65, 4095, 4096, 4097, 100003, 1 << 26, 0xffffffff]
    for bits in (1, 8, 9, 10, 16, 32, 33, 64):
        got = [native.group_tmp_bytes(n, bits) for n in counts]
        assert got[0] == 0
        assert all(a <= b for a, b in zip(got, got[1:])), bits
        w = 4 if bits <= 32 else 8
        per = w if bits <= 8 else 2 * w + 4
        for n, b in zip(counts, got):
            assert b == (n + 63) // 64 * 64 * per
            assert b <= 2 * (8 + 4) * n + fixed
            assert b >= n * w     # (the sorted keys alone)
    assert native.group_tmp_bytes(1000, 32) < native.group_tmp_bytes(1000, 33)
    assert native.group_tmp_bytes(1000, 0) == 0 and native.group_tmp_bytes(1000, 65) == 0
    assert native.group_tmp_bytes(1 << 32, 32) == 0
