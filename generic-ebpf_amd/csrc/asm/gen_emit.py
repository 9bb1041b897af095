"""The small emit helpers every other module builds its lines from: operand names, kernel-argument
operands, tests of the mode word and of dp_launch.vflags, dispatch / call / goto / fault, the
lane's index, and the layouts of the staged packet in LDS.  Lines are strings; a body is a list
of them."""
import re

from gen_abi import *  # noqa: F401,F403  (the register plan and the ABI: the names every line is made of)


def lo(r):
    return "v%d" % (2 * r)


def hi(r):
    return "v%d" % (2 * r + 1)


def pair(r):
    return "v[%d:%d]" % (2 * r, 2 * r + 1)


def v(i):
    return "v%d" % i


def vp(i):
    return "v[%d:%d]" % (i, i + 1)


def s(i):
    return "s%d" % i


def sp(i):
    return "s[%d:%d]" % (i, i + 1)


def dispatch(next_reg=12):
    """Fetch the entry at byte offset s[next_reg] (inside the entry being replaced: the offset
    is read when the load issues, and the code object is xnack-, so no replay can re-read it)
    and jump to its handler."""
    return ["s_load_dwordx8 s[8:15], s[%d:%d], s%d" % (S_PROG, S_PROG + 1, next_reg),
            "s_waitcnt lgkmcnt(0)",
            "s_setpc_b64 s[8:9]"]


_ENT_REF = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")


def early_fetch_point(body):
    """Interpreter image: where in a straight-line handler body the next entry's fetch can issue
    — right after the body's last reference to the entry SGPRs s[8:15] (the load overwrites them
    when it lands; its offset s12 is read at issue) — so that the fetch's latency overlaps the
    rest of the body.  None when the body branches, calls, or waits on a partial lgkmcnt."""
    last = -1
    for i, ln in enumerate(body):
        if ln.endswith(":") or ln.split(" ")[0] in ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz",
                                                    "s_cbranch_vccnz", "s_cbranch_execz",
                                                    "s_cbranch_execnz", "s_branch", "s_setpc_b64",
                                                    "s_swappc_b64"):
            return None
        for a, b, c in _ENT_REF.findall(ln):
            lo_, hi_ = (int(a), int(a)) if a else (int(b), int(c))
            if lo_ <= 15 and hi_ >= 8:
                last = i
    rest = body[last + 1:]
    if any("lgkmcnt(" in ln and "lgkmcnt(0)" not in ln for ln in rest):
        return None
    return last + 1


def raddr(label, pair_):
    return ["s_add_u32 %s, %s, %s-.Lcb" % (s(pair_), s(S_CB), label),
            "s_addc_u32 %s, %s, 0" % (s(pair_ + 1), s(S_CB + 1))]


def call(label):
    """Call a routine: its address is formed in the link pair, which the swap then
    overwrites with the return address (a routine that calls another saves its own link)."""
    return raddr(label, S_LINK) + ["s_swappc_b64 %s, %s" % (sp(S_LINK), sp(S_LINK))]


def goto(label):
    """Jump to a routine through the scratch pair (the link pair may be live: tail calls)."""
    return raddr(label, S_JUNK) + ["s_setpc_b64 %s" % sp(S_JUNK)]


def fault_mask(mask_sgpr_pair, code):
    """Retire the lanes in s[mask] with fault `code`; returns (or never, if none remain)."""
    out = []
    if mask_sgpr_pair != S_MASK:
        out.append("s_mov_b64 %s, %s" % (sp(S_MASK), sp(mask_sgpr_pair)))
    out += ["s_mov_b32 %s, %d" % (s(S_CODE), code)] + call(".Lr_fault")
    return out


def karg(*fields, table=LAUNCH):
    """The kernel-argument operand of an s_load that starts at the first of `fields`; a wider
    load names every field it covers, which must lie back to back."""
    off, size = table[fields[0]]
    end = off + size
    for f in fields[1:]:
        assert table[f][0] == end, "%s does not follow at 0x%x" % (f, end)
        end += table[f][1]
    return "s[0:1], 0x%x" % off


def karg_regs(*pairs):
    """karg() of a load into consecutive SGPRs, [(field, the SGPR it must land in), ...]."""
    (f0, r0) = pairs[0]
    for f, r in pairs:
        assert r == r0 + (LAUNCH[f][0] - LAUNCH[f0][0]) // 4, "%s is not loaded into s%d" % (f, r)
    return karg(*[f for f, _ in pairs])


def mode_test(bit):
    return "s_bitcmp1_b32 %s, %d" % (s(S_MODE), bit)


def mode_set(bit):
    return "s_or_b32 %s, %s, %s" % (s(S_MODE), s(S_MODE), "%d" % (1 << bit) if bit < 4 else "0x%x" % (1 << bit))


def vflags_test(bit, skip):
    """Branches to `skip` when dp_launch.vflags bit `bit` is clear (VF_OVERLAY: MODE_OVERLAY,
    copied at kernel start; other bits: loaded, clobbering S_T3)."""
    if bit == VF_OVERLAY:
        return [mode_test(MODE_OVERLAY), "s_cbranch_scc0 %s" % skip]
    return ["s_load_dword %s, %s" % (s(S_T3), karg("vflags")),
            "s_waitcnt lgkmcnt(0)",
            "s_bitcmp1_b32 %s, %d" % (s(S_T3), bit),
            "s_cbranch_scc0 %s" % skip]


def lane_index(img, dst):
    """dst = this lane's index in the wave (0..63)."""
    if img.staged:
        return ["v_lshrrev_b32 %s, 4, v%d" % (v(dst), V_L16)]
    return ["v_mbcnt_lo_u32_b32 %s, -1, 0" % v(dst), "v_mbcnt_hi_u32_b32 %s, -1, %s" % (v(dst), v(dst))]


def lane_pkt_index(img, dst):
    """dst = the packet index of this lane in the launch (general image: V_IDX)."""
    if img.staged:
        return ["v_lshrrev_b32 %s, 4, v%d" % (v(dst), V_L16),
                "v_lshl_add_u32 %s, %s, 6, %s" % (v(dst), s(S_GROUP), v(dst))]
    return ["v_mov_b32 %s, v%d" % (v(dst), V_IDX)]


def ret_slot_write(x0, x1):
    """r0 of the retiring lanes into v[44:45]; a superblock kernel (RETK > 1) moves the whole
    group's results into its slot v[V_RB + 2k], k = group % RETK, once when the group is done
    (slot_commit), not at every exit."""
    return ["v_mov_b32 v%d, %s" % (V_RES, x0), "v_mov_b32 v%d, %s" % (V_RES + 1, x1)]


def dma_lane_offsets(dst, tmp):
    """dst = lane l's byte offset inside each 1-KB DMA block of a staged group: 64 (l & 15) +
    16 (l >> 4), so DMA q's lane l fetches chunk l >> 4 of packet 16 q + (l & 15) and the LDS
    block holds chunk c of its 16 packets as 256 contiguous bytes (packet m at 16 m).  Each DMA
    instruction still covers its own 1 KB (same cache lines, lanes permuted: the same DMA rate,
    profiles/r05/staging_layout/), and the staging reads of a chunk by 16 lanes are contiguous:
    no LDS bank conflicts (in the packets' own layout lanes 64 B apart collide)."""
    return ["v_bfe_u32 %s, v%d, 4, 4" % (dst, V_L16),
            "v_bfe_u32 %s, v%d, 8, 2" % (tmp, V_L16),
            "v_lshlrev_b32 %s, 4, %s" % (tmp, tmp),
            "v_lshl_or_b32 %s, %s, 6, %s" % (dst, dst, tmp)]


def lds_pkt_dwords(base, save_exec=None):
    """Write the lane's 64 staged bytes (v22..v37) into the wave's LDS packet buffer transposed:
    dword c of lane l at S_PKTLDS + 4 l + 256 c (VGPR `base` = S_PKTLDS + 4 l).  The loads at
    run-time offsets (lds_pkt_read) then read consecutive dwords across the lanes; in the DMA's
    layout (lane l's 64 bytes at S_PKTLDS + 64 l) every lane reading the same offset hit the same
    two banks (C3L: 112M conflict cycles per launch against 9M of LDS instructions)."""
    return ["ds_write_b32 %s, v%d offset:%d" % (base, PKT0 + c, 256 * c) for c in range(16)]


def lds_pkt_read(z, d, A, B, T):
    """d = the z bytes at byte offset T (a VGPR, <= 64 - z) of the lane's packet in the transposed
    LDS buffer (lds_pkt_dwords), A = S_PKTLDS + 4 lane (clobbered): the dwords around the bytes,
    then one byte align by T's low bits (any alignment, no branch; a dword past the lane's 64
    bytes is read but never selected).  Clobbers B, R[0..2]."""
    t0, t1, t2 = v(R[0]), v(R[1]), v(R[2])
    out = ["v_lshrrev_b32 %s, 2, %s" % (B, T),
           "v_lshl_add_u32 %s, %s, 8, %s" % (B, B, A)]
    if z == 1:
        out += ["ds_read_b32 %s, %s" % (t0, B)]
    else:
        out += ["ds_read2_b32 v[%d:%d], %s offset1:64" % (R[0], R[1], B)]
    if z == 8:
        out.append("ds_read_b32 %s, %s offset:512" % (t2, B))
    out += ["s_waitcnt lgkmcnt(0)",
            "v_alignbyte_b32 %s, %s, %s, %s" % (lo(d), t0 if z == 1 else t1, t0, T)]
    if z == 8:
        out.append("v_alignbyte_b32 %s, %s, %s, %s" % (hi(d), t2, t1, T))
    else:
        if z < 4:
            out.append("v_and_b32 %s, %s, %s" % (lo(d), "0xff" if z == 1 else "0xffff", lo(d)))
        out.append("v_mov_b32 %s, 0" % hi(d))
    return out
