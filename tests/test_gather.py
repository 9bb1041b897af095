"""Gathering packets into a dense batch on the host (include/ebpf_gpu.h: ebpf_batch_gather) against
a numpy restatement of the header's rules, and the argument checks of ebpf_batch_gather /
ebpf_batch_gather_dev, which come before any device work and so hold without a GPU.

A copy has one right answer, so every comparison is exact.  Outputs lie inside a larger buffer
filled with 0xA5: a write before `out`, past the end or past out_bytes shows up."""
import collections
import ctypes
import errno

import numpy as np
import pytest

from test_steer import U64, expected as steer_expected

G4 = 1 << 32
SENTINEL = 0xA5
PAD = 64
NSEL = 1000
STRIDES = [1, 7, 32, 60, 64, 128]

# a batch as the run functions take it; data a uint8 array
Src = collections.namedtuple("Src", "name data count stride offsets extents")


# ---------------------------------------------------------------- the rules, in numpy


def spans(src):
    """(start, length) of every packet of the batch, int64: the length is end - start, or 0 for
    an end below the start or 2^32 bytes or more past it"""
    if src.offsets is None:
        s = np.arange(src.count, dtype=np.int64) * src.stride
        e = s + src.stride
    elif src.extents:
        pairs = np.asarray(src.offsets, dtype=np.int64).reshape(-1, 2)
        s, e = pairs[:, 0], pairs[:, 1]
    else:
        o = np.asarray(src.offsets, dtype=np.int64)
        s, e = o[:-1], o[1:]
    ln = np.where((e < s) | (e - s >= G4), 0, e - s)
    return s, ln


def listed(src, index):
    """(start, length) of the listed packets; an index >= count has length 0"""
    index = np.asarray(index, dtype=np.int64)
    s, ln = spans(src)
    if src.count == 0:
        return np.zeros(len(index), dtype=np.int64), np.zeros(len(index), dtype=np.int64)
    ok = index < src.count
    at = np.minimum(index, src.count - 1)
    return np.where(ok, s[at], 0), np.where(ok, ln[at], 0)


def expected(src, index, out_stride, out_bytes=None):
    """(the bytes written from `out` on, out_offsets or None): strided form n * out_stride bytes;
    packed form min(out_offsets[n], out_bytes) bytes"""
    s, ln = listed(src, index)
    n = len(s)
    if out_stride:
        k = np.minimum(ln, out_stride)
        col = np.arange(out_stride, dtype=np.int64)
        mask = col[None, :] < k[:, None]
        out = np.zeros((n, out_stride), dtype=np.uint8)
        out[mask] = src.data[(s[:, None] + col[None, :])[mask]]
        return out.reshape(-1), None
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(ln, out=offs[1:])
    pos = np.repeat(s - offs[:-1], ln) + np.arange(offs[-1], dtype=np.int64)
    out = src.data[pos] if len(pos) else np.zeros(0, dtype=np.uint8)
    if out_bytes is not None:
        out = out[:out_bytes]
    return out, offs.astype(U64)


# ---------------------------------------------------------------- sources and lists


def sources(csr_max=100, seed=8):
    """the constructions of test_gpu_steer._sources over random bytes, plus extents that overlap"""
    g = np.random.default_rng(seed)
    lens = g.integers(0, csr_max + 1, NSEL)
    csr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pairs = np.stack([csr[:-1], csr[1:]], axis=1)[g.permutation(NSEL)]
    nbytes = max(64 * NSEL, int(csr[-1]))
    data = g.integers(0, 256, nbytes + 16, dtype=np.uint8)
    ov_s = g.integers(0, nbytes - 300, NSEL)
    overlap = np.stack([ov_s, ov_s + g.integers(0, 300, NSEL)], axis=1)
    return [Src("stride64", data, NSEL, 64, None, False),
            Src("csr", data, NSEL, 0, csr.astype(U64), False),
            Src("extents", data, NSEL, 0, pairs.reshape(-1).astype(U64), True),
            Src("overlap", data, NSEL, 0, overlap.reshape(-1).astype(U64), True)]


def lists(count, seed=3):
    """{name: index}: a steered class, the whole steering index, duplicates, descending, and
    indices at and past count"""
    g = np.random.default_rng(seed)
    ret = g.choice([0, 1, 17, 255], count).astype(U64)
    index, starts = steer_expected(ret)
    return {"class": index[int(starts[17]):int(starts[18])],
            "whole": index,
            "dups": g.integers(0, count, 777).astype(np.uint32),
            "descending": np.arange(count - 1, -1, -1, dtype=np.uint32)[::3],
            "odd": np.array([5, count, 0, count - 1, 0xffffffff, count + 7, 5], dtype=np.uint32)}


# ---------------------------------------------------------------- the host function, framed


def batch_of(native, src, data_ptr=None, offsets_ptr=None):
    offs = None if src.offsets is None else np.ascontiguousarray(src.offsets, dtype=U64)
    b = native.PktBatch(src.data.ctypes.data if data_ptr is None else data_ptr,
                        (None if offs is None else offs.ctypes.data) if offsets_ptr is None
                        else offsets_ptr, src.count, src.stride,
                        native.BATCH_EXTENTS if src.extents else 0)
    return b, offs


def check_frame(buf, lead, want, what=""):
    """buf = sentinel bytes, then `want` from position lead on, then sentinel bytes again"""
    assert (buf[:lead] == SENTINEL).all(), "%s: wrote before out" % what
    np.testing.assert_array_equal(buf[lead:lead + len(want)], want, err_msg=what)
    assert (buf[lead + len(want):] == SENTINEL).all(), "%s: wrote past the end" % what


def run_host(native, src, index, out_stride, out_bytes=None, shift=0):
    """ebpf_batch_gather into a framed buffer: (code, out_offsets); the frame is checked against
    the numpy rules"""
    index = np.ascontiguousarray(index, dtype=np.uint32)
    n = len(index)
    want, want_offs = expected(src, index, out_stride, out_bytes)
    total = n * out_stride if out_stride else int(want_offs[n])
    if out_bytes is None:
        out_bytes = total
    lead = PAD + shift
    buf = np.full(lead + max(total, out_bytes) + PAD, SENTINEL, dtype=np.uint8)
    offs = None if out_stride else np.full(n + 2, 0x5a5a5a5a5a5a5a5a, dtype=U64)
    b, keep = batch_of(native, src)
    code = native.lib().ebpf_batch_gather(ctypes.byref(b), index.ctypes.data if n else None, n,
                                          out_stride, buf.ctypes.data + lead, out_bytes,
                                          None if offs is None else offs.ctypes.data)
    what = "%s stride %d n %d" % (src.name, out_stride, n)
    check_frame(buf, lead, want, what)
    if offs is not None:
        np.testing.assert_array_equal(offs[:n + 1], want_offs, err_msg=what)
        assert offs[n + 1] == 0x5a5a5a5a5a5a5a5a
        assert code == (errno.ENOSPC if total > out_bytes else 0), what
    else:
        assert code == 0, what
    return code, offs


@pytest.mark.parametrize("src", sources(), ids=lambda s: s.name)
def test_gather_sources_lists_and_forms(native, src):
    for name, index in lists(src.count).items():
        for out_stride in STRIDES + [0]:
            run_host(native, src, index, out_stride, shift=(3 if name == "dups" else 0))


def test_gather_reorders_a_batch_by_class(native):
    """the whole steering index: class b lies at starts[b] * out_stride, and at
    out_offsets[starts[b] .. starts[b + 1]]"""
    src = sources()[1]
    g = np.random.default_rng(3)
    ret = g.choice([0, 1, 17, 255], src.count).astype(U64)
    index, starts = native.steer(ret)
    out, _, _ = native.gather(src.data, src.count, index, out_stride=32, offsets=src.offsets)
    packed, offs, code = native.gather(src.data, src.count, index, offsets=src.offsets)
    assert code == 0 and len(packed) == int(offs[-1]) == int(src.offsets[-1])
    for b in (0, 1, 17, 255):
        lo, hi = int(starts[b]), int(starts[b + 1])
        members = index[lo:hi]
        assert hi > lo and (ret[members] == b).all()
        np.testing.assert_array_equal(out[lo * 32:hi * 32], expected(src, members, 32)[0])
        np.testing.assert_array_equal(packed[int(offs[lo]):int(offs[hi])],
                                      expected(src, members, 0)[0])


def test_gather_length_zero_rules(native):
    """an end below its start, and an end exactly 2^32 past it, are packets of length 0: nothing
    of them is read (the second's end lies far outside the buffer)"""
    g = np.random.default_rng(4)
    data = g.integers(1, 256, 4096, dtype=np.uint8)
    ext = np.array([[0, 64], [300, 250], [512, 576], [1024, 1024 + G4], [2048, 2112],
                    [100, 100 + G4 - 1]], dtype=U64)
    src = Src("degenerate", data, 6, 0, ext.reshape(-1), True)
    s, ln = spans(src)
    assert ln.tolist() == [64, 0, 64, 0, 64, G4 - 1]
    index = np.array([1, 0, 3, 2, 3, 1, 4], dtype=np.uint32)   # (never the 4 GiB packet)
    for out_stride in (16, 64, 0):
        run_host(native, src, index, out_stride)
    _, offs = run_host(native, src, index, 0)
    assert offs[:8].tolist() == [0, 0, 64, 64, 128, 128, 128, 192]
    # offsets form: a decreasing entry makes one packet's end fall below its start
    csr = Src("csr_dip", data, 3, 0, np.array([0, 100, 40, 90], dtype=U64), False)
    assert spans(csr)[1].tolist() == [100, 0, 50]
    for out_stride in (64, 0):
        run_host(native, csr, [0, 1, 2, 1], out_stride)


def test_gather_enospc(native):
    """the packed form's snprintf rule: out_offsets in full, the bytes that fit, ENOSPC"""
    src = sources()[1]
    index = lists(src.count)["dups"]
    offs = expected(src, index, 0)[1]
    total = int(offs[-1])
    j = int(np.flatnonzero(np.diff(offs.astype(np.int64)) > 2)[300])
    for out_bytes in (int(offs[j]) + 1, int(offs[j]), 0, total - 1):
        code, _ = run_host(native, src, index, 0, out_bytes=out_bytes)
        assert code == errno.ENOSPC
    for out_bytes in (total, total + 9):
        assert run_host(native, src, index, 0, out_bytes=out_bytes)[0] == 0
    # the wrapper sizes the output by a first call
    out, o2, code = native.gather(src.data, src.count, index, offsets=src.offsets)
    assert code == 0 and len(out) == total
    np.testing.assert_array_equal(o2, offs)
    out, o2, code = native.gather(src.data, src.count, index, offsets=src.offsets, out_bytes=10)
    assert code == errno.ENOSPC and len(out) == 10 and int(o2[-1]) == total


def test_gather_empty_list_and_empty_batch(native):
    src = sources()[0]
    assert run_host(native, src, [], 64)[0] == 0
    code, offs = run_host(native, src, [], 0)
    assert code == 0 and offs[0] == 0
    empty = Src("empty", src.data, 0, 64, None, False)
    run_host(native, empty, [0, 5, 0xffffffff], 16)
    code, offs = run_host(native, empty, [0, 5, 0xffffffff], 0)
    assert offs[:4].tolist() == [0, 0, 0, 0]


FAKE = 4096   # a non-NULL pointer that nothing may dereference


def _calls(native):
    """both entry points as f(batch, index, n, out_stride, out, out_bytes, out_offsets)"""
    L = native.lib()
    ref = lambda b: None if b is None else ctypes.byref(b)
    yield "host", lambda b, *a: L.ebpf_batch_gather(ref(b), *a)
    for dev in (0, 1 << 20):
        yield "dev%d" % dev, lambda b, *a, d=dev: L.ebpf_batch_gather_dev(d, ref(b), *a, None)


def test_gather_argument_checks(native):
    """EINVAL and E2BIG with nothing dereferenced, on both entry points; on the device function
    they come before the device is looked at"""
    good = native.PktBatch(FAKE, None, 8, 64, 0)
    for name, f in _calls(native):
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
    assert L.ebpf_batch_gather(ctypes.byref(good), None, 0, 64, None, 0, None) == 0
    hist = native.PktBatch(FAKE, None, 8, 64, native.BATCH_HIST_OVERWRITE)
    assert L.ebpf_batch_gather(ctypes.byref(hist), None, 0, 64, None, 0, None) == 0
    bad_dev = lambda n, st, offs: L.ebpf_batch_gather_dev(1 << 20, ctypes.byref(good), FAKE, n, st,
                                                          FAKE, 1 << 20, offs, None)
    assert bad_dev(3, 64, None) == errno.ENODEV
    assert bad_dev(0, 64, None) == errno.ENODEV
    assert bad_dev(3, 0, FAKE) == errno.ENODEV
    assert L.ebpf_batch_gather_dev(-1, ctypes.byref(good), FAKE, 3, 64, FAKE, 1 << 20, None,
                                   None) == errno.ENODEV
    if native.gpu_count() == 0:
        assert L.ebpf_batch_gather_dev(0, ctypes.byref(good), FAKE, 3, 64, FAKE, 1 << 20, None,
                                       None) == errno.ENODEV
