"""Steering a batch by verdict on the host (include/ebpf_gpu.h: ebpf_batch_steer) against numpy's
stable sort, and the argument checks of ebpf_batch_steer / ebpf_batch_steer_dev /
ebpf_batch_select_dev, which come before any device work and so hold without a GPU.

A stable partition has one right answer, so every comparison is exact."""
import ctypes
import errno
import os
import re

import numpy as np
import pytest

U64 = np.uint64


def classes(ret, faults=None):
    """the histogram's bins: 256 for a faulted packet, else min(ret, 255)"""
    cls = np.minimum(np.asarray(ret, dtype=U64), U64(255)).astype(np.int64)
    if faults is not None:
        cls[np.asarray(faults) != 0] = 256
    return cls


def expected(ret, faults=None):
    """(index, starts) of the stable partition by class"""
    cls = classes(ret, faults)
    index = np.argsort(cls, kind="stable").astype(np.uint32)
    starts = np.searchsorted(cls[index], np.arange(258), side="left").astype(U64)
    return index, starts


def check(native, ret, faults=None):
    ret = np.asarray(ret, dtype=U64)
    index, starts = native.steer(ret, faults)
    want_index, want_starts = expected(ret, faults)
    np.testing.assert_array_equal(starts, want_starts)
    np.testing.assert_array_equal(index, want_index)
    assert starts[0] == 0 and starts[native.EBPF_HIST_BINS] == len(ret)
    np.testing.assert_array_equal(np.diff(starts.astype(np.int64)),
                                  np.bincount(classes(ret, faults), minlength=257))
    return index, starts


def test_tile_constant_matches_the_kernels(native):
    src = open(os.path.join(native.HERE, "csrc", "host", "steer.h")).read()
    assert int(re.search(r"STEER_TILE = (\d+);", src).group(1)) == native.STEER_TILE
    assert native.STEER_STARTS == native.EBPF_HIST_BINS + 1 == 258


@pytest.mark.parametrize("count", [0, 1, 257])
def test_small_counts(native, count):
    g = np.random.default_rng(count)
    ret = g.integers(0, 300, count).astype(U64)
    faults = (g.integers(0, 8, count) == 0).astype(np.uint8)
    ret[faults != 0] = 0
    index, starts = check(native, ret, faults)
    if count == 0:
        assert not starts.any() and len(index) == 0
    check(native, ret)


@pytest.mark.parametrize("nclass", [4, 257])
def test_100003_packets(native, nclass):
    g = np.random.default_rng(nclass)
    n = 100003
    cls = g.integers(0, nclass, n) if nclass == 257 else g.choice([0, 2, 3, 200], n)
    faults = (cls == 256).astype(np.uint8)
    ret = np.where(cls == 256, 0, cls).astype(U64)
    index, starts = check(native, ret, faults)
    assert (np.diff(starts.astype(np.int64)) > 0).sum() == nclass


def test_clamp_values(native):
    """254 keeps its own class; 255, 256, 2^32 and 2^64 - 1 all land in class 255"""
    vals = np.array([254, 255, 256, 1 << 32, (1 << 64) - 1], dtype=U64)
    ret = np.tile(vals, 7)
    index, starts = check(native, ret)
    assert starts[255] - starts[254] == 7 and starts[256] - starts[255] == 28
    np.testing.assert_array_equal(index[int(starts[255]):int(starts[256])],
                                  np.flatnonzero(ret >= 255))
    assert starts[256] == starts[257] == len(ret)


def test_faulted_packet_with_nonzero_ret(native):
    ret = np.array([5, 7, 5, 0, 9], dtype=U64)
    faults = np.array([0, 3, 0, 0, 0], dtype=np.uint8)
    index, starts = check(native, ret, faults)
    assert index[int(starts[256]):].tolist() == [1] and starts[8] - starts[7] == 0


def test_null_faults_puts_faulted_packets_in_class_0(native):
    """a faulted packet's ret is 0: without faults it shares class 0 with the packets that
    returned 0"""
    ret = np.array([3, 0, 0, 3, 1], dtype=U64)
    faults = np.array([0, 11, 0, 0, 0], dtype=np.uint8)
    index, starts = check(native, ret)
    assert index[:int(starts[1])].tolist() == [1, 2] and starts[257] == starts[256] == 5
    index, starts = check(native, ret, faults)
    assert index[:int(starts[1])].tolist() == [2] and index[-1] == 1


FAKE = 4096   # a non-NULL pointer that nothing may dereference


def test_steer_argument_checks(native):
    L = native.lib()
    starts = (ctypes.c_uint64 * native.STEER_STARTS)(*([77] * native.STEER_STARTS))
    assert L.ebpf_batch_steer(None, None, 1, FAKE, starts) == errno.EINVAL
    assert L.ebpf_batch_steer(FAKE, None, 1, None, starts) == errno.EINVAL
    assert L.ebpf_batch_steer(FAKE, None, 1, FAKE, None) == errno.EINVAL
    assert L.ebpf_batch_steer(None, None, 0, None, None) == errno.EINVAL
    assert L.ebpf_batch_steer(FAKE, None, 1 << 32, FAKE, starts) == errno.E2BIG
    assert list(starts) == [77] * native.STEER_STARTS
    assert L.ebpf_batch_steer(None, None, 0, None, starts) == 0
    assert list(starts) == [0] * native.STEER_STARTS


def test_steer_dev_argument_checks(native):
    """EINVAL and E2BIG before the device is looked at; then, on a machine without a GPU (or for
    a device out of range), ENODEV with nothing dereferenced"""
    L = native.lib()
    for dev in (0, 1 << 20):
        assert L.ebpf_batch_steer_dev(dev, None, None, 1, FAKE, FAKE, None) == errno.EINVAL
        assert L.ebpf_batch_steer_dev(dev, FAKE, None, 1, None, FAKE, None) == errno.EINVAL
        assert L.ebpf_batch_steer_dev(dev, FAKE, None, 1, FAKE, None, None) == errno.EINVAL
        assert L.ebpf_batch_steer_dev(dev, None, None, 0, None, None, None) == errno.EINVAL
        assert L.ebpf_batch_steer_dev(dev, FAKE, FAKE, 1 << 32, FAKE, FAKE, None) == errno.E2BIG
    assert L.ebpf_batch_steer_dev(1 << 20, FAKE, FAKE, 5, FAKE, FAKE, None) == errno.ENODEV
    assert L.ebpf_batch_steer_dev(-1, FAKE, FAKE, 5, FAKE, FAKE, None) == errno.ENODEV
    assert L.ebpf_batch_steer_dev(1 << 20, None, None, 0, None, FAKE, None) == errno.ENODEV
    if native.gpu_count() == 0:
        assert L.ebpf_batch_steer_dev(0, FAKE, FAKE, 5, FAKE, FAKE, None) == errno.ENODEV
        assert L.ebpf_batch_steer_dev(0, None, None, 0, None, FAKE, None) == errno.ENODEV


def test_select_dev_argument_checks(native):
    L = native.lib()
    good = native.PktBatch(FAKE, None, 8, 64, 0)
    for dev in (0, 1 << 20):
        sel = lambda b, idx, n, ext: L.ebpf_batch_select_dev(
            dev, None if b is None else ctypes.byref(b), idx, n, ext, None)
        assert sel(None, FAKE, 1, FAKE) == errno.EINVAL
        assert sel(native.PktBatch(None, None, 8, 64, 0), FAKE, 1, FAKE) == errno.EINVAL
        assert sel(native.PktBatch(FAKE, None, 8, 0, 0), FAKE, 1, FAKE) == errno.EINVAL
        assert sel(native.PktBatch(FAKE, None, 8, 64, 0x80), FAKE, 1, FAKE) == errno.EINVAL
        assert sel(native.PktBatch(FAKE, None, 8, 0, native.BATCH_EXTENTS), FAKE, 1,
                   FAKE) == errno.EINVAL
        assert sel(good, None, 1, FAKE) == errno.EINVAL
        assert sel(good, FAKE, 1, None) == errno.EINVAL
    bad_dev = lambda b, n: L.ebpf_batch_select_dev(1 << 20, ctypes.byref(b), FAKE, n, FAKE, None)
    assert bad_dev(good, 3) == errno.ENODEV
    assert bad_dev(good, 0) == errno.ENODEV
    assert bad_dev(native.PktBatch(FAKE, FAKE, 8, 0, native.BATCH_EXTENTS), 3) == errno.ENODEV
    if native.gpu_count() == 0:
        assert L.ebpf_batch_select_dev(0, ctypes.byref(good), FAKE, 3, FAKE, None) == errno.ENODEV
