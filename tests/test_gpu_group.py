"""Grouping a batch by key on the device (include/ebpf_gpu.h: ebpf_batch_group_dev;
csrc/hip/group.hip) against numpy's stable sort and against the host function.  A stable sort has
one right answer: every comparison is exact, and keys stay unsigned 64-bit throughout.

Shapes: T = native.STEER_TILE entries go to one workgroup, a quarter of them to each of its four
waves in 64-entry chunks, so the counts sit around 64, 256 and T; above 256 tiles the tile scan
takes its second level, which 2M + 5 packets (513 tiles) reach.  Every output buffer is pre-filled
with a value no result holds and is 8 entries longer than the call may write."""
import errno
import functools

import numpy as np
import pytest

import pyoracle
from generic_ebpf_amd import native as _native
from test_group import U64, expected, garbage

pytestmark = pytest.mark.gpu

T = _native.STEER_TILE
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17]
MID = 3 * T + 17
BIG = (2 << 20) + 5
PATTERNS = ["equal", "two", "div64", "div4095", "divT", "desc", "byte3", "byte1", "rand32",
            "rand1000", "rand64"]
GUARD = 8
FILL = 0xffffffffffffffff   # no position, and no key of a pattern below


@functools.lru_cache(maxsize=None)
def pattern(name, n):
    """(ret, faults, key_bits): every 11th packet is faulted with its ret left as it is"""
    i = np.arange(n, dtype=U64)
    g = np.random.default_rng(n + len(name))
    mix = (i * U64(2654435761)) >> U64(7)
    ret = {"equal": lambda: np.full(n, 7, dtype=U64),
           "two": lambda: np.where(i % U64(2) == 0, U64(9), U64(2)),
           "div64": lambda: i // U64(64), "div4095": lambda: i // U64(4095),
           "divT": lambda: i // U64(T), "desc": lambda: U64(max(n, 1) - 1) - i,
           "byte3": lambda: (mix % U64(256)) << U64(24),
           "byte1": lambda: (mix % U64(256)) << U64(8),
           "rand32": lambda: g.integers(0, 1 << 32, n, dtype=U64),
           "rand1000": lambda: g.integers(0, 1000, n, dtype=U64) * U64(4194301),
           "rand64": lambda: g.integers(0, 1 << 64, n, dtype=U64) | (i % U64(3) << U64(63)),
           }[name]().astype(U64)
    faults = np.where(np.arange(n) % 11 == 10, 5, 0).astype(np.uint8)
    return ret, faults, 64 if name == "rand64" else 32


def reference(ret, faults, shift, bits):
    """numpy's answer, checked against the host function"""
    w = expected(ret, faults, shift, bits)
    index, gkeys, gstarts, info, code = _native.group(ret, faults, shift, bits)
    g = len(w[1])
    assert code == 0 and info.tolist() == [g, w[3]]
    np.testing.assert_array_equal(index, w[0])
    np.testing.assert_array_equal(gkeys[:g], w[1])
    np.testing.assert_array_equal(gstarts[:g + 1], w[2])
    return w


@functools.lru_cache(maxsize=None)
def want(name, n, with_faults):
    ret, faults, bits = pattern(name, n)
    return reference(ret, faults if with_faults else None, 0, bits)


class Dev:
    """one grouping call's device buffers; outputs pre-filled with a value no result holds"""

    def __init__(self, ret, faults, shift, bits, cap=None, tmp_bytes=None):
        import torch
        dev = torch.device("cuda:0")
        self.n, self.shift, self.bits = len(ret), shift, bits
        self.cap = self.n if cap is None else cap
        self.ret = torch.from_numpy(np.ascontiguousarray(ret).view(np.int64)).to(dev)
        self.faults = None if faults is None else torch.from_numpy(faults).to(dev)
        self.index = torch.full((self.n + GUARD,), -1, dtype=torch.int32, device=dev)
        self.gkeys = torch.full((self.cap + GUARD,), -1, dtype=torch.int64, device=dev)
        self.gstarts = torch.full((self.cap + 1 + GUARD,), -1, dtype=torch.int64, device=dev)
        self.info = torch.full((2 + GUARD,), -1, dtype=torch.int64, device=dev)
        self.tmp_bytes = _native.group_tmp_bytes(self.n, bits) if tmp_bytes is None else tmp_bytes
        self.tmp = torch.zeros(max(self.tmp_bytes, 8), dtype=torch.uint8, device=dev)

    def enqueue(self, gpu, stream):
        n = self.n
        return gpu.lib().ebpf_batch_group_dev(
            0, self.ret.data_ptr() if n else None,
            None if self.faults is None or not n else self.faults.data_ptr(), n, self.shift,
            self.bits, self.index.data_ptr() if n else None, self.cap, self.gkeys.data_ptr(),
            self.gstarts.data_ptr(), self.info.data_ptr(), self.tmp.data_ptr(), self.tmp_bytes,
            stream.cuda_stream)

    def result(self):
        return (self.index.cpu().numpy().view(np.uint32), self.gkeys.cpu().numpy().view(U64),
                self.gstarts.cpu().numpy().view(U64), self.info.cpu().numpy().view(U64))

    def check(self, w, msg):
        """the whole contract for a call whose answer is w = expected(...)"""
        w_index, w_keys, w_starts, u = w
        index, gkeys, gstarts, info = self.result()
        G, m = len(w_keys), min(len(w_keys), self.cap)
        assert info[:2].tolist() == [G, u], msg
        assert (info[2:] == FILL).all(), msg
        np.testing.assert_array_equal(index[:self.n], w_index, err_msg=msg)
        assert (index[self.n:] == 0xffffffff).all(), msg
        np.testing.assert_array_equal(gkeys[:m], w_keys[:m], err_msg=msg)
        assert (gkeys[m:] == FILL).all(), msg
        written = G + 1 if G <= self.cap else m
        np.testing.assert_array_equal(gstarts[:written], w_starts[:written], err_msg=msg)
        assert (gstarts[written:] == FILL).all(), msg


def run(gpu, devs):
    import torch
    for d in devs:
        assert d.enqueue(gpu, torch.cuda.current_stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("count", COUNTS)
def test_group_counts_and_patterns(gpu, count):
    cases = [(name, wf) for name in PATTERNS for wf in (True, False)]
    devs = []
    for name, wf in cases:
        ret, faults, bits = pattern(name, count)
        devs.append(Dev(ret, faults if wf else None, 0, bits))
    run(gpu, devs)
    for d, (name, wf) in zip(devs, cases):
        d.check(want(name, count, wf), "%s %d faults=%s" % (name, count, wf))
    if count > T:   # a run of equal keys across a tile edge opens no group
        assert len(want("equal", count, False)[1]) == 1
        assert len(want("div4095", count, False)[1]) == -(-count // 4095)
    if count > 1:
        assert len(want("desc", count, False)[1]) == count


@pytest.mark.parametrize("bits", [1, 5, 8, 9, 10, 13, 16, 24, 32, 33, 64])
def test_group_widths_and_shifts(gpu, bits):
    """the field under random bits above and below it, at every digit split"""
    g = np.random.default_rng(bits)
    n = MID
    faults = np.where(np.arange(n) % 11 == 10, 1, 0).astype(np.uint8)
    cases, devs = [], []
    for shift in (0, 3, 32):
        if shift + bits > 64:
            continue
        vals = g.integers(0, 1 << bits, 1000, dtype=U64) if bits < 64 else \
            g.integers(0, 1 << 64, 1000, dtype=U64)
        for field in (vals[g.integers(0, len(vals), n)],                  # few values: runs
                      vals[g.integers(0, len(vals), n) % 3],             # three keys under garbage
                      g.integers(0, 1 << bits, n, dtype=U64) if bits < 64
                      else g.integers(0, 1 << 64, n, dtype=U64)):        # the whole field
            ret = garbage(g, field, shift, bits)
            cases.append((ret, shift))
            devs.append(Dev(ret, faults, shift, bits))
    run(gpu, devs)
    for d, (ret, shift) in zip(devs, cases):
        d.check(reference(ret, faults, shift, bits), "bits %d shift %d" % (bits, shift))


@pytest.mark.parametrize("count", [65, T + 1, MID])
def test_group_fault_shapes(gpu, count):
    ret, _, bits = pattern("rand1000", count)
    every = np.full(count, 3, dtype=np.uint8)
    none = np.zeros(count, dtype=np.uint8)
    devs = [Dev(ret, every, 0, bits), Dev(ret, none, 0, bits), Dev(ret, None, 0, bits)]
    run(gpu, devs)
    w = reference(ret, every, 0, bits)
    assert w[3] == 0 and len(w[1]) == 0 and w[0].tolist() == list(range(count))
    devs[0].check(w, "all faulted")
    devs[1].check(reference(ret, none, 0, bits), "none faulted")
    devs[2].check(reference(ret, None, 0, bits), "faults NULL")
    assert devs[1].result()[0].tobytes() == devs[2].result()[0].tobytes()


def test_group_caps(gpu):
    """G = count: a full table, one entry short, one entry, none; and no table at all"""
    ret, _, bits = pattern("desc", MID)
    w = want("desc", MID, False)
    G = len(w[1])
    assert G == MID
    devs = [Dev(ret, None, 0, bits, cap=c) for c in (G + 3, G, G - 1, 1, 0)]
    run(gpu, devs)
    for d in devs:
        d.check(w, "cap %d" % d.cap)
    import torch
    d = Dev(ret, None, 0, bits, cap=0)
    assert gpu.lib().ebpf_batch_group_dev(
        0, d.ret.data_ptr(), None, d.n, 0, bits, d.index.data_ptr(), 0, None, None,
        d.info.data_ptr(), d.tmp.data_ptr(), d.tmp_bytes,
        torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    d.check(w, "cap 0, NULL tables")
    # cap 0 and no group at all: the table is complete and its one start is written
    d = Dev(ret, np.ones(MID, dtype=np.uint8), 0, bits, cap=0)
    run(gpu, [d])
    d.check(expected(ret, np.ones(MID, dtype=np.uint8), 0, bits), "cap 0, G 0")
    assert d.result()[2][0] == 0


@pytest.mark.parametrize("name", ["rand32", "div64"])
def test_group_two_level_scan(gpu, name):
    ret, faults, bits = pattern(name, BIG)
    d = Dev(ret, faults, 0, bits)
    run(gpu, [d])
    d.check(want(name, BIG, True), name)


def test_group_same_call_twice(gpu):
    ret, faults, bits = pattern("rand1000", MID)
    a, b = Dev(ret, faults, 0, bits), Dev(ret, faults, 0, bits)
    run(gpu, [a])
    run(gpu, [b])
    for x, y in zip(a.result(), b.result()):
        assert x.tobytes() == y.tobytes()
    a.check(want("rand1000", MID, True), "first call")


def test_group_two_streams_at_once(gpu):
    """each stream has its own scratch and each call its own tmp: calls in flight share nothing"""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    cases = [("rand32", BIG), ("div64", BIG), ("rand1000", MID), ("rand64", MID)]
    runs = [Dev(*pattern(name, n)[:2], 0, pattern(name, n)[2]) for name, n in cases]
    torch.cuda.synchronize()
    for k, d in enumerate(runs):
        s = (s1, s2)[k % 2]
        with torch.cuda.stream(s):
            assert d.enqueue(gpu, s) == 0
    torch.cuda.synchronize()
    for d, (name, n) in zip(runs, cases):
        d.check(want(name, n, True), name)


def test_group_short_tmp_launches_nothing(gpu):
    import torch
    ret, faults, bits = pattern("rand32", MID)
    d = Dev(ret, faults, 0, bits, tmp_bytes=_native.group_tmp_bytes(MID, bits) - 1)
    assert d.enqueue(gpu, torch.cuda.current_stream()) == errno.ENOSPC
    torch.cuda.synchronize()
    index, gkeys, gstarts, info = d.result()
    assert (index == 0xffffffff).all() and (gkeys == FILL).all()
    assert (gstarts == FILL).all() and (info == FILL).all()


# ---------------------------------------------------------------- a real batch, grouped and gathered

NREAL = 4096 + 37
FIELD_AT = 12   # the ethertype, the IPv4 version byte and the TOS byte: a few hundred values


def test_group_real_batch_then_gather(gpu, env):
    """a program that returns a 32-bit field of the packet; the batch grouped by it and gathered
    over the whole index: every group's packets side by side, in arrival order"""
    import torch
    from generic_ebpf_amd import workloads
    from generic_ebpf_amd.workloads import I, R0, R1
    lay = workloads.assemble([I("ldxw", R0, R1, FIELD_AT), I("exit")])
    pk = workloads.packets_l2l3(NREAL, 64)
    w_ret, w_flt, _, _ = pyoracle.OracleProgram(lay.code, lay.relocs, []).run(pk, NREAL, 64)
    np.testing.assert_array_equal(
        w_ret, np.ascontiguousarray(pk[:, FIELD_AT:FIELD_AT + 4]).view("<u4").reshape(-1))
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    data = torch.from_numpy(pk.reshape(-1)).to(dev)
    ret = torch.full((NREAL,), -1, dtype=torch.int64, device=dev)
    flt = torch.zeros(NREAL, dtype=torch.uint8, device=dev)
    out = torch.full((NREAL * 64,), 0xee, dtype=torch.uint8, device=dev)
    d = Dev(np.zeros(NREAL, dtype=U64), None, 0, 32)
    p = gpu.Prog(env, gpu.patch_relocs(lay.code, lay.relocs, []))
    try:
        p.run_batch_dev(0, data.data_ptr(), NREAL, 64, ret.data_ptr(), None, flt.data_ptr(), None,
                        st)
        gpu.group_dev(0, ret.data_ptr(), flt.data_ptr(), NREAL, 0, 32, d.index.data_ptr(), d.cap,
                      d.gkeys.data_ptr(), d.gstarts.data_ptr(), d.info.data_ptr(),
                      d.tmp.data_ptr(), d.tmp_bytes, st)
        gpu.gather_dev(0, data.data_ptr(), NREAL, 64, d.index.data_ptr(), NREAL, 64,
                       out.data_ptr(), NREAL * 64, stream=st)
        torch.cuda.synchronize()
    finally:
        p.destroy()
    np.testing.assert_array_equal(ret.cpu().numpy().view(U64), w_ret)
    np.testing.assert_array_equal(flt.cpu().numpy(), w_flt)
    assert not w_flt.any()
    d.check(reference(w_ret, w_flt, 0, 32), "real batch")
    index, gkeys, gstarts, info = d.result()
    G = int(info[0])
    assert 100 < G < NREAL // 2 and info[1] == NREAL
    dense = out.cpu().numpy().reshape(NREAL, 64)
    field = np.ascontiguousarray(dense[:, FIELD_AT:FIELD_AT + 4]).view("<u4").reshape(-1)
    for g in range(G):
        a, b = int(gstarts[g]), int(gstarts[g + 1])
        assert b > a and (field[a:b] == gkeys[g]).all()
        members = np.flatnonzero(w_ret == gkeys[g])       # the group's packets in arrival order
        np.testing.assert_array_equal(dense[a:b], pk[members])
