"""Batch addressing edges: packets 4 GiB and more from batch->data, packets up to 2^32 - 1 bytes
long with loads at the boundaries of the offset checks, degenerate extents, and batch bases of
any alignment (include/ebpf_gpu.h: the batch descriptor and ebpf_prog_run_batch_dev).

One zero-filled buffer of SIZE = 4 GiB + 2 MiB bytes carries every batch here: on the device a
torch allocation, on the host np.zeros (backed lazily: only the pages a test touches cost
memory).  Both allocations are ALLOC = 4 GiB + 5 MiB long: the 1-MiB-stride batch of 4,100
packets spans 4 GiB + 4 MiB, and the slack behind SIZE keeps the addresses a wrong check could
form inside the allocation (below).

Safety rule of every device test: if the bounds check or address computation under test were
wrong, the address it formed would still lie inside the device allocation, so that a bug shows
as a mismatch and not as a GPU memory fault —
* packets start at least LEAD = 4 KiB into the buffer;
* a packet that is the target of an offset K >= 2^30 starts below 2 MiB - 32, so that
  packet + K + 8 (every K below 2^33 used here is at most 2^32 + 16) and packet + (K mod 2^32)
  + 8 are inside SIZE;
* the staged (LDS-DMA) kernel is never launched on a base that is not 16-byte aligned: the
  library sends such a base to the general kernel, and the tests assert that it did
  (exec_info layout 0) after a launch whose choice was made on the host before anything ran.

Expected values: the oracle on the same packets gathered contiguously (results do not depend on
where a packet lies: programs return no addresses), or, for the giant packets, values derived by
hand from marker bytes (MARK(position)) written at the read positions; a refused access is
EBPF_FAULT_MEM with ret 0.  The oracle's own 64-bit handling is pinned by a CPU test on the host
buffer against the same hand-derived values."""
import collections
import contextlib
import ctypes
import functools
import os
import time

import numpy as np
import pytest

import manywrites as mw
import pyoracle
import stdprogs

I = stdprogs.I
VARIANTS = [int(v) for v in os.environ.get("EBPF_TEST_VARIANTS", "0,1,2").split(",")]
G4 = 1 << 32
SIZE = G4 + (2 << 20)
ALLOC = G4 + (5 << 20)
LEAD = 4096
F_MEM = 3
GUARD = 0xa5

P = collections.namedtuple("P", "name code relocs maps std")


@pytest.fixture(scope="module")
def hostbuf():
    yield np.zeros(ALLOC, dtype=np.uint8)


@pytest.fixture(scope="module")
def devbuf(gpu):
    import torch
    t = torch.zeros(ALLOC, dtype=torch.uint8, device="cuda:0")
    yield t
    del t
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- programs


def _store_prog():
    """standard semantics: x = pkt[0] + pkt[12] + 1 (MEM on packets shorter than 13 bytes, before
    any store); pkt[0] = x (byte), pkt[8..11] = x * 0x01010101; r0 = x * 0x01010101"""
    code, rel = stdprogs.asm([I("ldxb", 2, 1, 0), I("ldxb", 3, 1, 12), I("add64_reg", 2, 3),
                              I("add64_imm", 2, imm=1), I("stxb", 1, 2, 0),
                              I("mul64_imm", 2, imm=0x01010101), I("stxw", 1, 2, 8),
                              I("mov64_reg", 0, 2), I("exit")])
    return P("store", code, rel, [], True)


@functools.lru_cache(maxsize=None)
def _progs(nrand):
    """C3, nrand random programs with one map (as test_general_kernels_header_staging builds
    them: some loads fault MEM, some store into the packet) and the storing program"""
    from generic_ebpf_amd import randprog, workloads
    g = np.random.default_rng(31)
    lay = workloads.prog_c3()
    out = [P("c3", lay.code, lay.relocs, [], False)]
    for k in range(nrand):
        lay = randprog.random_program(70000 + k, length=int(g.integers(10, 60)), nmaps=1,
                                      map_value_size=8)
        out.append(P("rand%d" % k, lay.code, lay.relocs,
                     [(8, 16, g.integers(0, 256, 8 * 16, dtype=np.uint8).tobytes())], False))
    out.append(_store_prog())
    return tuple(out)


def _oracle(pr, data, n, stride, offs=None):
    op = pyoracle.OracleProgram(pr.code, pr.relocs, pr.maps, semantics=1 if pr.std else 0)
    ret, flt, after, _ = op.run(data, n, stride, offs, nthreads=8)
    return ret, flt, after, [op.map_bytes(k) for k in range(len(pr.maps))]


def _hist(ret, flt):
    ok = flt == 0
    h = np.bincount(np.minimum(ret[ok], 255).astype(np.int64), minlength=257)
    h[256] = int((~ok).sum())
    return h


@contextlib.contextmanager
def _loaded(gpu, env, pr, variant):
    maps = []
    for vs, me, d in pr.maps:
        m = gpu.Map(env, me, vs)
        m.fill(d)
        maps.append(m)
    p = gpu.Prog(env, gpu.patch_relocs(pr.code, pr.relocs, [m.handle for m in maps]))
    try:
        if pr.std:
            p.set_semantics(gpu.SEM_STANDARD)
        gpu.set_variant(variant)
        yield p, maps
    finally:
        gpu.set_variant(0)
        p.destroy()
        for m in maps:
            m.destroy()


def _run_dev(p, base_ptr, n, stride, offs=None, extents=False, hist=False):
    """one device-resident launch: (ret u64[n], faults u8[n], histogram or None)"""
    import torch
    dev = torch.device("cuda:0")
    d_ret = torch.full((n,), -1, dtype=torch.int64, device=dev)
    d_flt = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_off = None
    if offs is not None:
        d_off = torch.from_numpy(np.ascontiguousarray(offs, dtype=np.uint64).view(np.int64)).to(dev)
    d_hist = torch.full((257,), 12345, dtype=torch.int64, device=dev) if hist else None
    p.run_batch_dev(0, base_ptr, n, stride, d_ret.data_ptr(),
                    None if d_off is None else d_off.data_ptr(), d_flt.data_ptr(),
                    None if d_hist is None else d_hist.data_ptr(),
                    torch.cuda.current_stream().cuda_stream, hist_overwrite=hist, extents=extents)
    torch.cuda.synchronize()
    return (d_ret.cpu().numpy().view(np.uint64), d_flt.cpu().numpy(),
            None if d_hist is None else d_hist.cpu().numpy())


# ---------------------------------------------------------------- 1, 4: far packets


class FarCase:
    """Packets (starts[i], lens[i]) in the buffer, their bytes (rows of packets_l2l3 cut to
    length) gathered contiguously for the oracle, and the oracle's results per program (computed
    once, shared by every variant and by the device and host tests)."""

    def __init__(self, starts, lens, seed, forced=()):
        from generic_ebpf_amd import workloads
        self.starts = np.asarray(starts, dtype=np.int64)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.n = len(self.starts)
        self.forced = list(forced)
        order = np.argsort(self.starts)
        ends = (self.starts + self.lens)[order]
        assert (ends[:-1] <= self.starts[order][1:]).all(), "packets overlap"
        assert self.starts.min() >= LEAD and ends.max() <= ALLOC
        self.goffs = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(self.lens, out=self.goffs[1:])
        rows = workloads.packets_l2l3(self.n, 160, seed=seed)
        self.gathered = rows[np.arange(160)[None, :] < self.lens[:, None]]
        assert len(self.gathered) == self.goffs[-1]
        # buffer position of every gathered byte
        self.idx = np.repeat(self.starts - self.goffs[:-1], self.lens) + np.arange(self.goffs[-1])
        self.extents = np.stack([self.starts, self.starts + self.lens], axis=1).reshape(-1)
        self._want = {}

    def csr(self):
        """the packets as one CSR run (they must be contiguous)"""
        assert (self.starts[1:] == self.starts[:-1] + self.lens[:-1]).all()
        return np.append(self.starts, self.starts[-1] + self.lens[-1]).astype(np.uint64)

    def want(self, pr):
        if pr.name not in self._want:
            self._want[pr.name] = _oracle(pr, self.gathered, self.n, 0, self.goffs.astype(np.uint64))[:3]
        return self._want[pr.name]

    def guards(self):
        """positions of the 64 bytes on either side of the forced packets that belong to no
        packet (a forced packet's neighbours are other forced packets or nothing)"""
        pos = set()
        for s, ln in self.forced:
            pos.update(range(s - 64, s))
            pos.update(range(s + ln, s + ln + 64))
        for s, ln in self.forced:
            pos.difference_update(range(s, s + ln))
        return np.array(sorted(q for q in pos if q < ALLOC), dtype=np.int64)


SLOT = 1024


def _scattered(seed, n, forced):
    """n packets of 0..127 bytes at random places over the whole buffer (one per 1-KiB slot, at
    least 64 bytes from the slot's edges, none in the slots around 2^32 and at the buffer's end),
    and the forced (start, length) placements among them at random positions"""
    g = np.random.default_rng(seed)
    slots = np.unique(g.integers(LEAD // SLOT, SIZE // SLOT - 1, n + 256))
    slots = slots[(slots < G4 // SLOT - 2) | (slots > G4 // SLOT + 2)]
    g.shuffle(slots)
    slots = slots[:n]
    assert len(slots) == n
    starts = slots * SLOT + g.integers(64, SLOT - 128 - 64, n)
    lens = g.integers(0, 128, n)
    for s, ln in forced:
        at = int(g.integers(0, len(starts) + 1))
        starts = np.insert(starts, at, s)
        lens = np.insert(lens, at, ln)
    return FarCase(starts, lens, seed, forced)


@functools.lru_cache(maxsize=None)
def _extents_cases():
    """The four forced placements cannot share a batch with a storing program (the one ending at
    2^32 and the one starting at 2^32 - 13 overlap), so there are two batches of 2,000 random
    packets: one with a packet ending exactly at byte 2^32, one starting exactly there and one
    ending at the buffer's last byte, the other with a packet from 2^32 - 13 across 2^32."""
    return (_scattered(1, 2000, [(G4 - 100, 100), (G4, 77), (SIZE - 91, 91)]),
            _scattered(2, 2000, [(G4 - 13, 100)]))


@functools.lru_cache(maxsize=None)
def _csr_case():
    """3,000 contiguous packets of 1..140 bytes from 2^32 - 100,000 across 2^32"""
    g = np.random.default_rng(3)
    lens = g.integers(1, 141, 3000)
    starts = G4 - 100000 + np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert starts[0] < G4 < starts[-1]
    return FarCase(starts, lens, 3, [(int(starts[0]), int(lens.sum()))])   # (guards round the run)


@functools.lru_cache(maxsize=None)
def _stride_case():
    """4,100 packets at a 1 MiB stride (4.0 GiB + 4 MiB); their first 64 bytes are the data"""
    n = 4100
    return FarCase(LEAD + (np.arange(n, dtype=np.int64) << 20), np.full(n, 64), 4)


@functools.lru_cache(maxsize=None)
def _host_extents_case():
    """two clusters of 1,500 packets, from 2^32 - 1 MiB and from just past 2^32, interleaved: the
    one chunk the host path makes of them spans under 4 MiB and starts at a byte0 near 2^32"""
    g = np.random.default_rng(5)
    k = np.arange(1500, dtype=np.int64)
    a = G4 - (1 << 20) + 256 * k + g.integers(0, 64, 1500)
    b = G4 + 64 + 256 * k + g.integers(0, 64, 1500)
    starts = np.stack([a, b], axis=1).reshape(-1)
    return FarCase(starts, g.integers(0, 128, 3000), 5)


def _check_far_dev(gpu, env, devbuf, variant, case, progs, launch):
    """Every program on the case's packets in the device buffer (put back before each: programs
    store into them): results, fault codes and the packets' bytes afterwards against the oracle;
    the guard bytes around the forced packets stay as they were.  launch(p) -> (ret, faults)."""
    import torch
    idx = torch.from_numpy(case.idx).to(devbuf.device)
    gidx = torch.from_numpy(case.guards()).to(devbuf.device)
    pristine = torch.from_numpy(case.gathered).to(devbuf.device)
    bad = []
    try:
        devbuf[gidx] = GUARD
        for pr in progs:
            want, wf, wafter = case.want(pr)
            devbuf[idx] = pristine
            with _loaded(gpu, env, pr, variant) as (p, _):
                ret, flt = launch(p)[:2]
            after = devbuf[idx].cpu().numpy()
            guards_ok = bool((devbuf[gidx] == GUARD).all())
            if not (np.array_equal(flt, wf) and np.array_equal(ret, want)
                    and np.array_equal(after, wafter) and guards_ok):
                bad.append((pr.name, int((ret != want).sum()), int((flt != wf).sum()),
                            int((after != wafter).sum()), guards_ok))
    finally:
        devbuf[idx] = 0
        devbuf[gidx] = 0
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_far_packets_extents(gpu, env, devbuf, variant):
    for case in _extents_cases():
        assert (case.starts >= G4).any() and (case.starts < 1 << 31).any()
        _check_far_dev(gpu, env, devbuf, variant, case, _progs(10),
                       lambda p: _run_dev(p, devbuf.data_ptr(), case.n, 0, case.extents, extents=True))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_far_packets_csr_offsets(gpu, env, devbuf, variant):
    case = _csr_case()
    _check_far_dev(gpu, env, devbuf, variant, case, _progs(10),
                   lambda p: _run_dev(p, devbuf.data_ptr(), case.n, 0, case.csr()))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_far_packets_fixed_stride_general(gpu, env, devbuf, variant):
    """stride 1 MiB: index x stride passes 2^32 at packet 4,096.  The programs read below byte 64
    (the oracle, on the packets' first 64 bytes at stride 64, must fault nowhere)"""
    case = _stride_case()
    progs = [pr for pr in _progs(10) if pr.name in ("c3", "store")]
    for pr in progs:
        assert not case.want(pr)[1].any()
    _check_far_dev(gpu, env, devbuf, variant, case, progs,
                   lambda p: _run_dev(p, devbuf.data_ptr() + LEAD, case.n, 1 << 20))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_far_packets_fixed_stride_64_staged(gpu, env, devbuf, variant):
    """The only full-size batch: 64M + 8,192 + 37 packets of 64 B from LEAD on, so the last 8,229
    start 4 GiB and more from batch->data (the staged kernels' LDS-DMA base).  C4 on 1M distinct
    packets tiled on the device; results against the tiled oracle's, histogram overwritten.
    Takes 0.2-0.3 s per variant on an MI355X (the oracle, the fill and the compare included)."""
    import torch
    from generic_ebpf_amd import workloads
    t0 = time.time()
    D = 1 << 20
    n = (1 << 26) + 8192 + 37
    lay = workloads.prog_c4()
    pr = P("c4", lay.code, lay.relocs, [(8, 256, workloads.c4_map_values().tobytes())], False)
    pk = workloads.packets_l2l3(D, 64)
    want, wf, _, _ = _oracle(pr, pk.reshape(-1), D, 64)
    assert not wf.any()
    region = devbuf[LEAD:LEAD + 64 * n]
    full, tail = n // D, n % D
    # the tile's period divides 2^26 packets = 2^32 bytes, so a base that lost bit 32 would read
    # the very packet it should: the packets past 2^32 are distinct packets SH.. instead
    SH = 500000
    try:
        src = torch.from_numpy(pk.reshape(-1)).to(devbuf.device)
        region[:full * D * 64].view(full, D * 64).copy_(src.unsqueeze(0).expand(full, D * 64))
        region[full * D * 64:].copy_(src[SH * 64:(SH + tail) * 64])
        d_ret = torch.full((n,), -1, dtype=torch.int64, device=devbuf.device)
        d_hist = torch.full((257,), 987654321, dtype=torch.int64, device=devbuf.device)
        with _loaded(gpu, env, pr, variant) as (p, _):
            p.run_batch_dev(0, devbuf.data_ptr() + LEAD, n, 64, d_ret.data_ptr(), None, None,
                            d_hist.data_ptr(), torch.cuda.current_stream().cuda_stream,
                            hist_overwrite=True)
            torch.cuda.synchronize()
            if variant != 1:
                assert p.exec_info(0)[1] == 1
        wt = torch.from_numpy(want.view(np.int64)).to(devbuf.device)
        bad = int((d_ret[:full * D].view(full, D) != wt.unsqueeze(0)).sum())
        bad += int((d_ret[full * D:] != wt[SH:SH + tail]).sum())
        assert bad == 0, "%d of %d packets differ from the oracle" % (bad, n)
        assert (want[SH:SH + tail] != want[:tail]).sum() > tail // 2
        h = np.bincount(np.minimum(want, 255).astype(np.int64), minlength=257) * full
        h += np.bincount(np.minimum(want[SH:SH + tail], 255).astype(np.int64), minlength=257)
        np.testing.assert_array_equal(d_hist.cpu().numpy(), h)
    finally:
        region.zero_()
        torch.cuda.synchronize()
    print("64M + 8,229 packets, variant %d: %.1f s" % (variant, time.time() - t0))


def _check_far_host(gpu, env, hostbuf, variant, case, progs, run):
    """as _check_far_dev on the host buffer through ebpf_prog_run_batch; the bytes between the
    packets stay zero"""
    lo, hi = int(case.starts.min()) - 64, int((case.starts + case.lens).max()) + 64
    bad = []
    try:
        for pr in progs:
            want, wf, wafter = case.want(pr)
            hostbuf[case.idx] = case.gathered
            with _loaded(gpu, env, pr, variant) as (p, _):
                ret, flt = run(p)[:2]
            after = hostbuf[case.idx]
            between = hostbuf[lo:hi].copy()
            between[case.idx - lo] = 0
            if not (np.array_equal(flt, wf) and np.array_equal(ret, want)
                    and np.array_equal(after, wafter) and not between.any()):
                bad.append((pr.name, int((ret != want).sum()), int((flt != wf).sum()),
                            int((after != wafter).sum()), int(between.any())))
    finally:
        hostbuf[lo:hi] = 0
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("mode", ["csr", "extents"])
def test_host_path_far_offsets(gpu, env, hostbuf, variant, mode):
    """ebpf_prog_run_batch uploads a chunk's bytes [byte0, byte1) and launches with off_base =
    byte0: here byte0 is near 2^32 and the offsets pass it"""
    progs = [pr for pr in _progs(10) if pr.name in ("c3", "store")]
    if mode == "csr":
        case = _csr_case()
        run = lambda p: p.run_batch(hostbuf, case.n, 0, case.csr())
    else:
        case = _host_extents_case()
        span = (case.starts + case.lens).max() - case.starts.min()
        assert span < (4 << 20) and case.starts.min() < G4 < case.starts.max()
        run = lambda p: p.run_batch(hostbuf, case.n, 0, case.extents.astype(np.uint64), extents=True)
    _check_far_host(gpu, env, hostbuf, variant, case, progs, run)


# ---------------------------------------------------------------- 2: huge packets


def MARK(pos):
    """the marker byte of buffer position pos (never 0)"""
    return ((pos * 2654435761 >> 11) & 0xff) | 1


SMALL = [8192 + 1 + 256 * i for i in range(9)]   # 64-byte packets (odd bases)
GA = (1 << 20) + 3                                # length 2^32 - 1
GA2 = (1 << 20) + (1 << 16) + 3                   # length 2^32 - 1
GB = (1 << 20) + (1 << 17) + 1                    # length 2^30 + 4
LEN_A, LEN_B = G4 - 1, (1 << 30) + 4
DG = (32 << 10) + 1                               # the degenerate-extents batch
KS = [56, 60, (1 << 30) - 8, (1 << 30) - 4, (1 << 30) - 3, 1 << 30,
      G4 - 9, G4 - 8, G4 - 2, G4 - 1, G4 + 16]
TS_SMALL = [0, 55, 56, G4 + 5, 1 << 63, (1 << 64) - 16]
U64 = (1 << 64) - 1


def _const_prog(K, size):
    """r2 = r1; r2 += K (an immediate, or through LDDW past 2^31); r0 = *(u<size> *)(r2 + 0)"""
    items = [I("mov64_reg", 2, 1)]
    if K < (1 << 31):
        items.append(I("add64_imm", 2, imm=K))
    else:
        items += [("lddw", 3, K), I("add64_reg", 2, 3)]
    items += [I({1: "ldxb", 4: "ldxw", 8: "ldxdw"}[size], 0, 2, 0), I("exit")]
    code, rel = stdprogs.asm(items)
    return P("const_%x_%d" % (K, size), code, rel, [], True)


def _pktv_prog():
    """t = *(u64 *)pkt; r0 = *(u8 *)(pkt + t + 8)"""
    code, rel = stdprogs.asm([I("ldxdw", 2, 1, 0), I("mov64_reg", 3, 1), I("add64_reg", 3, 2),
                              I("ldxb", 0, 3, 8), I("exit")])
    return P("pktv", code, rel, [], True)


@functools.lru_cache(maxsize=None)
def _huge_cases():
    """(bytes to write {position: byte}, [(program, extents [(start, end)], want ret, want
    faults)]).  A load of `size` bytes at offset `off` (mod 2^64) of a packet of length L is
    allowed iff off + size <= L, and then returns the marker bytes at start + off, little-endian;
    else EBPF_FAULT_MEM and 0."""
    W = {}

    def mark(pos, n=8):
        for q in range(pos, pos + n):
            if 0 <= q < SIZE:
                W[q] = MARK(q)

    def load(start, L, off, size):
        if off + size <= L:
            return int.from_bytes(bytes(MARK(start + off + j) for j in range(size)), "little"), 0
        return 0, F_MEM

    cases = []
    # constant offsets: giants among 64-byte packets
    pkts = [(SMALL[0], 64), (GB, LEN_B), (SMALL[1], 64), (GA, LEN_A), (SMALL[2], 64)]
    for s, L in pkts:
        assert LEAD <= s < (2 << 20) - 32 and s + L <= SIZE
        if L == 64:
            mark(s, 64)
        for K in KS:
            mark(s + K)
            mark(s + (K & (G4 - 1)))
    ext = [(s, s + L) for s, L in pkts]
    for K in KS:
        for size in (1, 4, 8):
            r = [load(s, L, K, size) for s, L in pkts]
            cases.append((_const_prog(K, size), ext, [x[0] for x in r], [x[1] for x in r]))
    # hand check of the table above, at the boundaries the issue names
    at = {(c[0].name, i): (c[2][i], c[3][i]) for c in cases for i in range(5)}
    assert at["const_%x_8" % ((1 << 30) - 4), 1][1] == 0 and at["const_%x_8" % ((1 << 30) - 3), 1][1] == F_MEM
    assert at["const_%x_4" % (1 << 30), 1][1] == 0 and at["const_%x_8" % (1 << 30), 1][1] == F_MEM
    assert at["const_%x_8" % (G4 - 9), 3][1] == 0 and at["const_%x_8" % (G4 - 8), 3][1] == F_MEM
    assert at["const_%x_1" % (G4 - 2), 3][1] == 0 and at["const_%x_1" % (G4 - 1), 3][1] == F_MEM
    assert all(at["const_%x_%d" % (G4 + 16, z), i][1] == F_MEM for z in (1, 4, 8) for i in range(5))
    # run-time offsets
    pkts = [(SMALL[3 + i], 64, t) for i, t in enumerate(TS_SMALL)]
    pkts[3:3] = [(GA, LEN_A, G4 - 10)]
    pkts.append((GA2, LEN_A, G4 - 9))
    tbytes = {}
    r = []
    for s, L, t in pkts:
        assert LEAD <= s < (2 << 20) - 32 and s + L <= SIZE
        off = (t + 8) & U64
        if L == 64:
            mark(s, 64)
        mark((s + off) & U64, 1)
        mark(s + (off & (G4 - 1)), 1)
        for j in range(8):
            tbytes[s + j] = (t >> (8 * j)) & 0xff
        r.append(load(s, L, off, 1))
    assert [x[1] for x in r] == [0, 0, F_MEM, 0, F_MEM, F_MEM, F_MEM, F_MEM]
    W.update(tbytes)   # (no read position of any case lies in a t field: checked below)
    cases.append((_pktv_prog(), [(s, s + L) for s, L, _ in pkts], [x[0] for x in r], [x[1] for x in r]))
    # degenerate extents: end < start, and end - start == 2^32 exactly, between ordinary packets
    ext = [(DG, DG + 64), (DG + 300, DG + 250), (DG + 512, DG + 576), (DG + 1024, DG + 1024 + G4),
           (DG + 2048, DG + 2112)]
    for s, _ in ext:
        mark(s, 64)
    code, rel = stdprogs.asm([I("ldxb", 0, 1, 3), I("exit")])
    cases.append((P("one_load", code, rel, [], True), ext,
                  [MARK(ext[0][0] + 3), 0, MARK(ext[2][0] + 3), 0, MARK(ext[4][0] + 3)],
                  [0, F_MEM, 0, F_MEM, 0]))
    code, rel = stdprogs.asm([I("mov64_imm", 0, imm=42), I("exit")])
    cases.append((P("no_load", code, rel, [], True), ext, [42] * 5, [0] * 5))
    # a position read as a marker must hold its marker: t fields lie in no such place
    for prog, ext, ret, flt in cases[:-3]:
        K, size = int(prog.name.split("_")[1], 16), int(prog.name.split("_")[2])
        for (s, e), f in zip(ext, flt):
            assert f or all(q not in tbytes for q in range(s + K, s + K + size))
    return W, cases


def _poke(buf, W, zero=False):
    pos = np.fromiter(W.keys(), dtype=np.int64, count=len(W))
    val = np.zeros(len(W), dtype=np.uint8) if zero else np.fromiter(W.values(), dtype=np.uint8, count=len(W))
    if isinstance(buf, np.ndarray):
        buf[pos] = val
    else:
        import torch
        buf[torch.from_numpy(pos).to(buf.device)] = torch.from_numpy(val).to(buf.device)


def test_oracle_huge_packets_and_offset_boundaries(hostbuf):
    """the oracle, one packet at a time in place on the host buffer (it has no extents mode: the
    length rule of the batch descriptor is applied here), against the hand-derived values"""
    W, cases = _huge_cases()
    bad = []
    try:
        _poke(hostbuf, W)
        for pr, ext, want, wf in cases:
            op = pyoracle.OracleProgram(pr.code, pr.relocs, pr.maps, semantics=1)
            r, f = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
            for i, (s, e) in enumerate(ext):
                ln = e - s if s <= e and e - s < G4 else 0
                o = np.array([s, s + ln], dtype=np.uint64)
                pyoracle.lib().oracle_run_batch(ctypes.addressof(op.p), hostbuf.ctypes.data,
                                                o.ctypes.data, 1, 0, r.ctypes.data, f.ctypes.data, 1)
                if (int(r[0]), int(f[0])) != (want[i], wf[i]):
                    bad.append((pr.name, i, hex(int(r[0])), int(f[0]), hex(want[i]), wf[i]))
    finally:
        _poke(hostbuf, W, zero=True)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_huge_packets_and_offset_boundaries(gpu, env, devbuf, variant):
    W, cases = _huge_cases()
    bad = []
    try:
        _poke(devbuf, W)
        for pr, ext, want, wf in cases:
            with _loaded(gpu, env, pr, variant) as (p, _):
                ret, flt, _ = _run_dev(p, devbuf.data_ptr(), len(ext), 0,
                                       np.array(ext, dtype=np.uint64).reshape(-1), extents=True)
            if ret.tolist() != want or flt.tolist() != wf:
                bad.append((pr.name, [hex(x) for x in ret.tolist()], flt.tolist(),
                            [hex(x) for x in want], wf))
    finally:
        _poke(devbuf, W, zero=True)
    assert not bad, bad


# ---------------------------------------------------------------- 3: base alignment

N3 = 64 * 300 + 17


@functools.lru_cache(maxsize=None)
def _align_case():
    from generic_ebpf_amd import workloads
    pk = workloads.packets_l2l3(N3, 64, seed=5).reshape(-1)
    progs = [pr for pr in _progs(10) if pr.name in ("c3", "store")]
    mk, vs, me = mw.CASES["mixed17_17"]
    lay = mk()
    init = np.random.default_rng(12).integers(0, 256, vs * me, dtype=np.uint8).tobytes()
    writer = P("mixed17_17", lay.code, lay.relocs, [(vs, me, init)], False)
    wpk = mw.packets(N3, 11).reshape(-1)
    return pk, [(pr, _oracle(pr, pk, N3, 64)) for pr in progs], wpk, writer, _oracle(writer, wpk, N3, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_base_alignment_device(gpu, env, devbuf, variant):
    """64-byte packets at data_ptr + d: any d gives the oracle's results, faults, histogram and
    packet bytes; the staged kernel (layout 1) runs only for d a multiple of 16, the general
    kernel (layout 0) for the others — the LDS-DMA never sees a misaligned source"""
    import torch
    pk, progs, wpk, writer, wwant = _align_case()
    d_pk = torch.from_numpy(pk).to(devbuf.device)
    nb = 64 * N3
    bad = []
    try:
        for d in (0, 1, 4, 8, 16, 24, 64):
            base = LEAD + d
            devbuf[base - 64:base + nb + 64] = GUARD
            for pr, (want, wf, wafter, _) in progs:
                devbuf[base:base + nb] = d_pk
                with _loaded(gpu, env, pr, variant) as (p, _):
                    ret, flt, hist = _run_dev(p, devbuf.data_ptr() + base, N3, 64, hist=True)
                    layout = p.exec_info(0)[1]
                after = devbuf[base:base + nb].cpu().numpy()
                guards = torch.cat([devbuf[base - 64:base], devbuf[base + nb:base + nb + 64]])
                # variant 1 always reports 0; c3 is the program known to take the staged kernel
                want_layout = 0 if (d % 16 or variant == 1) else 1 if pr.name == "c3" else layout
                ok = (np.array_equal(ret, want) and np.array_equal(flt, wf)
                      and np.array_equal(hist, _hist(want, wf)) and np.array_equal(after, wafter)
                      and bool((guards == GUARD).all()) and layout == want_layout)
                if not ok:
                    bad.append((d, pr.name, layout, int((ret != want).sum()), int((flt != wf).sum()),
                                int((after != wafter).sum())))
            devbuf[base - 64:base + nb + 64] = 0
        # the write log on the misaligned route: a map-writing program at d = 8
        base = LEAD + 8
        devbuf[base:base + nb] = torch.from_numpy(wpk).to(devbuf.device)
        want, wf, _, wmaps = wwant
        with _loaded(gpu, env, writer, variant) as (p, maps):
            ret, flt, _ = _run_dev(p, devbuf.data_ptr() + base, N3, 64)
            layout = p.exec_info(0)[1]
            after = b"".join(maps[0].lookup(k)[1] for k in range(maps[0].max_entries))
        assert layout == 0
        np.testing.assert_array_equal(flt, wf)
        np.testing.assert_array_equal(ret, want)
        assert after == wmaps[0] and after != writer.maps[0][2]
    finally:
        devbuf[LEAD - 64:LEAD + nb + 256] = 0
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_base_alignment_host(gpu, env, variant):
    """host buffers that start 1 and 3 bytes into their array, at stride 64 and with CSR offsets"""
    from generic_ebpf_amd import workloads
    pk, progs, _, _, _ = _align_case()
    g = np.random.default_rng(7)
    lens = g.integers(1, 141, 3000)
    offs = np.zeros(3001, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    rows = workloads.packets_l2l3(3000, 160, seed=7)
    ragged = rows[np.arange(160)[None, :] < lens[:, None]]
    bad = []
    for d in (1, 3):
        for pr, (want, wf, wafter, _) in progs:
            for data, n, stride, o, exp in ((pk, N3, 64, None, (want, wf, wafter)),
                                            (ragged, 3000, 0, offs, None)):
                if exp is None:
                    exp = _oracle(pr, data, n, stride, o)[:3]
                arr = np.full(d + len(data) + 64, GUARD, dtype=np.uint8)
                view = arr[d:d + len(data)]
                view[:] = data
                assert view.ctypes.data % 16 == d and view.flags["C_CONTIGUOUS"]
                with _loaded(gpu, env, pr, variant) as (p, _):
                    ret, flt, _ = p.run_batch(view, n, stride, o)
                if not (np.array_equal(ret, exp[0]) and np.array_equal(flt, exp[1])
                        and np.array_equal(view, exp[2]) and (arr[:d] == GUARD).all()
                        and (arr[d + len(data):] == GUARD).all()):
                    bad.append((d, pr.name, stride))
    assert not bad, bad
