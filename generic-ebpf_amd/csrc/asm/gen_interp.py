#!/usr/bin/env python3
"""Generate the hand-written gfx950 (CDNA4) assembly interpreter for the device program.

Output: <out>.s (the code object source: two interpreter kernels sharing one handler set, the
handler linker kernel, the handler offset table) and <out>.h (handler family ids for the host
lowering in asm_runtime.cpp, and the ABI the kernels share with the host: kernel-argument
offsets, registers, flag bits, the template table's order).  gen_abi.py states the register plan,
the handler families and that ABI; gen_image.py reads the build knobs (EBPF_ASM_*) and describes
the three images (m1, m0, m3); gen_emit.py has the small emit helpers, gen_handlers.py the handler
bodies, gen_maps.py the map routines, gen_routines.py the routines the kernels share, gen_jit.py
the compiled-program support.  This file holds an image's kernels and group code and assembles
the image from all of them; every function whose output depends on the image takes the image as
its first argument, and only main() writes files.

Execution model (one lane = one packet, wavefront-lockstep dispatch):
  * eBPF register rK lives in v[2K:2K+1] (VGPRs, never memory);
  * every handler is specialised for its (operation, dst, src) so no register is indexed at
    run time; a dispatch is  s_load_dwordx8 entry -> s_waitcnt -> s_setpc_b64 handler;
  * the wave-uniform entry (32 B, dprog.h layout with `handler` linked to an absolute code
    address) is fetched with scalar loads (K$), so decoding costs no VALU;
  * in the staged kernel each lane's 64-B packet is loaded with 4 x global_load_dwordx4 into
    v22..v37 and packet loads at translation-time-known offsets read registers;
  * the 512-B eBPF stack lives in LDS (per-lane slice sized from the translated program);
  * lanes that disagree on a conditional jump are parked (v41 = their entry) and resumed after
    the running group retires; retirement writes r0, the fault code and an LDS histogram.
"""
import re
import sys
from typing import NamedTuple

from gen_emit import *  # noqa: F401,F403  (with gen_abi's names: what every emitted line is made of)
from gen_handlers import handler_body
from gen_image import IMAGES, SETTINGS
from gen_jit import entry_reads, jit_templates
from gen_routines import routines


def kernel(img, name, staged, jit=False):
    k = "K%s%s" % ("s" if staged else "g", "j" if jit else "")
    L = [".globl %s" % name, ".p2align 8", ".type %s,@function" % name, "%s:" % name]
    if name == "ebpf_jit_s64" and img.phased and img.slots == 16:
        # the wide kernel: the same code with 16 result slots allocated (store_phased)
        L += [".globl ebpf_jit_s64w", ".type ebpf_jit_s64w,@function", "ebpf_jit_s64w:"]
    # v0 = workitem id; wave index within the 256-lane workgroup
    L += ["v_readfirstlane_b32 %s, v0" % s(S_WAVE),
          "s_lshr_b32 %s, %s, 6" % (s(S_WAVE), s(S_WAVE)),
          "s_load_dwordx16 s[%d:%d], %s" % (S_PROG, S_PROG + 15, karg_regs(
              ("prog", S_PROG), ("maps", S_MAPS), ("data", S_DATA), ("offsets", S_OFFS),
              ("off_base", S_OFFBASE), ("ret", S_RET), ("faults", S_FAULTS), ("hist", S_HIST))),
          "s_load_dwordx8 s[%d:%d], %s" % (S_COUNT, S_COUNT + 7, karg_regs(
              ("count", S_COUNT), ("stride", S_STRIDE), ("start", S_START), ("nmaps", S_NMAPS),
              ("nentries", S_NENT), ("stack_stride", S_STKSTRIDE), ("lds_stack_base", S_LDSBASE))),
          "s_load_dword %s, %s" % (s(S_GSTRIDE), karg("total_waves")),
          "s_load_dword %s, %s" % (s(S_PKTLDS), karg("lds_pkt_base")),
          "s_mov_b64 %s, src_shared_base" % sp(S_SHARED),
          "v_mov_b32 v%d, 0x00010203" % V_SEL,
          # code base: routines are addressed relative to .Lcb
          "s_getpc_b64 %s" % sp(S_CB),
          ".L%s_pc:" % k,
          "s_add_u32 %s, %s, .Lcb-.L%s_pc" % (s(S_CB), s(S_CB), k),
          "s_addc_u32 %s, %s, 0" % (s(S_CB + 1), s(S_CB + 1)),
          "v_mbcnt_lo_u32_b32 %s, -1, 0" % v(H[0]),
          "v_mbcnt_hi_u32_b32 %s, -1, %s" % (v(H[0]), v(H[0])),
          "v_lshlrev_b32 v%d, 4, %s" % (V_L16, v(H[0])),
          "s_mov_b32 %s, -1" % s(S_PREVG),
          "s_waitcnt lgkmcnt(0)",
          "s_mov_b32 %s, %d" % (s(S_MODE), (staged << MODE_STAGED) | (jit << MODE_JIT)),
          # MODE_OVERLAY: the program reads its own stores into map values (VF_OVERLAY)
          "s_load_dword %s, %s" % (s(S_T3), karg("vflags"))] + (
          # (the general kernels of a phased image leave write phasing off)
          ["s_load_dword %s, %s" % (s(S_WPHASE), karg("wphase")) if staged else
           "s_mov_b32 %s, 0" % s(S_WPHASE),
           "s_mov_b32 %s, 0" % s(S_PEND)] if img.phased else []) + [
          "s_waitcnt lgkmcnt(0)",
          "s_bitcmp1_b32 %s, %d" % (s(S_T3), VF_OVERLAY),
          "s_cbranch_scc0 .L%s_noovl" % k,
          mode_set(MODE_OVERLAY),
          ".L%s_noovl:" % k,
          # MODE_EXTENTS: dp_launch.offsets holds (start, end) pairs (VF_EXTENTS)
          "s_bitcmp1_b32 %s, %d" % (s(S_T3), VF_EXTENTS),
          "s_cbranch_scc0 .L%s_noext" % k,
          mode_set(MODE_EXTENTS),
          ".L%s_noext:" % k]
    if staged:
        # MODE_KEEP (keep mode): the program reads its packet at run-time offsets from the LDS
        # packet buffer (LDXPKTV), so the next group's DMA waits for the group's end.  Set by
        # the host in dp_launch.vflags (VF_KEEP, still in S_T3) for compiled and interpreted
        # programs alike.  (Double-buffering the packets instead, two 4-KB buffers per wave,
        # measured slower on C3L: 0.294 against 0.284 ms, the LDS cutting 6 workgroups per CU
        # to 4; profiles/r05/keep2/)
        L += ["s_bitcmp1_b32 %s, %d" % (s(S_T3), VF_KEEP),
              "s_cbranch_scc0 .L%s_nokeep" % k,
              mode_set(MODE_KEEP),
              ".L%s_nokeep:" % k]
    if not staged:   # header staging requested by the host (dp_launch.lds_pkt_base PKTLDS_HDRSTAGE)
        L += ["s_bitcmp1_b32 %s, %d" % (s(S_PKTLDS), PKTLDS_HDRSTAGE),
              "s_cbranch_scc0 .L%s_nogs" % k,
              mode_set(MODE_HDRSTAGE),
              ".L%s_nogs:" % k,
              # PKTLDS_HDRKEEP: the staged headers are kept in the wave's LDS packet buffer too, for the
              # loads at run-time offsets (MODE_KEEP in the general kernels)
              "s_bitcmp1_b32 %s, %d" % (s(S_PKTLDS), PKTLDS_HDRKEEP),
              "s_cbranch_scc0 .L%s_nohl" % k,
              mode_set(MODE_KEEP),
              ".L%s_nohl:" % k,
              "s_and_b32 %s, %s, 0x%x" % (s(S_PKTLDS), s(S_PKTLDS), (1 << PKTLDS_HDRKEEP) - 1)]
    L += ["s_branch .Lprologue"]
    return L


def pkt_setup(idx, tag):
    """General kernels: V_PKT / V_LEN of the running lanes' packets (index in VGPR idx), and with
    header staging (MODE_HDRSTAGE) their first 64 bytes into v22..v37.  Clobbers H[1], H[4:5], R[0],
    R[2], S_JUNK; leaves exec = the running lanes (s[S_MASK] holds them meanwhile)."""
    return ["s_mov_b64 %s, exec" % sp(S_MASK),
            "s_cmp_eq_u64 %s, 0" % sp(S_OFFS),
            "s_cbranch_scc0 .Lps_offsets_%s" % tag,
            "v_mov_b32 %s, %s" % (v(H[1]), s(S_STRIDE)),
            "v_mad_u64_u32 v[%d:%d], %s, v%d, %s, %s" % (V_PKT, V_PKT + 1, sp(S_JUNK), idx,
                                                         v(H[1]), sp(S_DATA)),
            "v_mov_b32 v%d, %s" % (V_LEN, s(S_STRIDE)),
            "s_branch .Lps_stage_%s" % tag,
            ".Lps_offsets_%s:" % tag,
            # offsets[i], offsets[i + 1]; extents batches (MODE_EXTENTS): offsets[2i], offsets[2i + 1]
            mode_test(MODE_EXTENTS),
            "s_cselect_b32 %s, 16, 8" % s(S_JUNK),
            "v_mov_b32 %s, %s" % (v(H[1]), s(S_JUNK)),
            "v_mad_u64_u32 %s, %s, v%d, %s, %s" % (vp(H[4]), sp(S_JUNK), idx, v(H[1]), sp(S_OFFS)),
            "global_load_dwordx2 %s, %s, off offset:8" % (vp(R[0]), vp(H[4])),
            "global_load_dwordx2 %s, %s, off" % (vp(H[4]), vp(H[4])),
            "s_waitcnt vmcnt(0)",
            # length = end - start; an end below its start or 4 GiB past it: length 0 (every load
            # of the packet faults MEM)
            "v_sub_co_u32 v%d, vcc, %s, %s" % (V_LEN, v(R[0]), v(H[4])),
            "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(R[1]), v(R[1]), v(H[5])),
            "v_cmp_ne_u32_e32 vcc, 0, %s" % v(R[1]),
            "v_cndmask_b32 v%d, v%d, 0, vcc" % (V_LEN, V_LEN),
            "v_mov_b32 %s, %s" % (v(R[2]), s(S_OFFBASE + 1)),
            "v_sub_co_u32 %s, vcc, %s, %s" % (v(H[4]), v(H[4]), s(S_OFFBASE)),
            "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(H[5]), v(H[5]), v(R[2])),
            "v_lshl_add_u64 v[%d:%d], %s, 0, %s" % (V_PKT, V_PKT + 1, vp(H[4]), sp(S_DATA)),
            ] + [
            # header staging: the first 64 bytes of every packet at least that long into
            # v22..v37 (what the staged kernels' LDS DMA provides)
            ".Lps_stage_%s:" % tag,
            mode_test(MODE_HDRSTAGE),
            "s_cbranch_scc0 .Lps_done_%s" % tag,
            "v_cmp_lt_u32_e64 vcc, 63, v%d" % V_LEN,
            "s_and_b64 exec, %s, vcc" % sp(S_MASK),
            "s_cbranch_execz .Lps_done_%s" % tag] + [
            "global_load_dwordx4 v[%d:%d], v[%d:%d], off offset:%d" % (PKT0 + 4 * q, PKT0 + 4 * q + 3,
                                                                       V_PKT, V_PKT + 1, 16 * q)
            for q in range(4)] + [
            "s_waitcnt vmcnt(0)",
            # (MODE_KEEP: the headers also into the wave's LDS packet buffer, transposed, for
            # loads at run-time offsets: h_ldx_pktv)
            mode_test(MODE_KEEP),
            "s_cbranch_scc0 .Lps_done_%s" % tag,
            "v_mbcnt_lo_u32_b32 %s, -1, 0" % v(H[1]),
            "v_mbcnt_hi_u32_b32 %s, -1, %s" % (v(H[1]), v(H[1])),
            "v_lshl_add_u32 %s, %s, 2, %s" % (v(H[1]), v(H[1]), s(S_PKTLDS))] + lds_pkt_dwords(v(H[1])) + [
            ".Lps_done_%s:" % tag,
            "s_mov_b64 exec, %s" % sp(S_MASK)]


def slot_commit(img):
    if img.retk == 1:
        return []
    L = ["s_mov_b64 exec, -1",
         "s_and_b32 %s, %s, %s" % (s(S_BYTES), s(S_GROUP), s(S_KMASK))]
    if img.phased and img.slots == 16:
        # wide phasing (dp_launch.wphase WPHASE_WIDE, the 96-VGPR kernel): 16 slots, the superblocks
        # of a wave alternating between slots 0-7 and 8-15 (s98 bit 31 = the running half,
        # switched at each superblock's first group)
        L += ["s_cmp_eq_u32 %s, 0" % s(S_BYTES),
              "s_cbranch_scc0 .Lsc_half",
              "s_bitcmp1_b32 %s, %d" % (s(S_WPHASE), WPHASE_WIDE),
              "s_cbranch_scc0 .Lsc_half",
              "s_xor_b32 %s, %s, 0x80000000" % (s(S_PEND), s(S_PEND)),
              ".Lsc_half:",
              "s_lshr_b32 %s, %s, 28" % (s(S_T0), s(S_PEND)),
              "s_and_b32 %s, %s, 8" % (s(S_T0), s(S_T0)),
              "s_or_b32 %s, %s, %s" % (s(S_BYTES), s(S_BYTES), s(S_T0)),
              "s_bitset1_b32 %s, %s" % (s(S_PEND), s(S_BYTES))]
    elif img.phased:
        L.append("s_bitset1_b32 %s, %s" % (s(S_PEND), s(S_BYTES)))
    return L + [
            "s_lshl_b32 %s, %s, 1" % (s(S_BYTES), s(S_BYTES)),
            "s_set_gpr_idx_on %s, gpr_idx(DST)" % s(S_BYTES),
            "v_mov_b32 v%d, v%d" % (img.v_rb, V_RES),
            "v_mov_b32 v%d, v%d" % (img.v_rb + 1, V_RES + 1),
            "s_set_gpr_idx_off"]


def store_phased(img, tag, final):
    """Write phasing (dp_launch.wphase != 0, staged kernels with result slots): instead of one
    burst per superblock, a wave writes the slots of all its finished groups (S_PEND bits 0-15)
    when the GPU's constant clock is inside the write window, when the next group's slot still
    holds an unwritten group (all slots full), and at the end (`final`).  Every wave reads the same
    100-MHz counter, so the result writes of the whole GPU bunch into the windows and the packet
    reads run alone between them: HBM turns between reading and writing far less often (floor
    kernel, tools/ubench/phase.hip: 0.855 -> 0.773 ms for 64M packets).
    Slots: slot k = group & K'-1 of the wave's last superblocks; with wphase WPHASE_WIDE (wide, the
    96-VGPR kernel) a wave's superblocks alternate between slots 0-7 and 8-15 (s98 bit 31 = the
    half of S_PREVG's superblock), so 16 groups fit (0.770 -> 0.753 ms, tools/ubench/phase2.hip).
    An unwritten slot of S_PREVG's half belongs to its superblock (index <= S_PREVG's) or to the
    one `back` (index above: two superblocks back when wide, one otherwise); a slot of the other
    half to the previous superblock.  Falls through to the superblock burst when wphase is 0;
    clobbers exec, S_T0..S_T3, S_BYTES, s[60:69], R[0], R[1]."""
    P = s(S_PEND)
    L = ["s_cmp_eq_u32 %s, 0" % s(S_WPHASE),
         "s_cbranch_scc1 .Lph_off_%s" % tag] + (
        ["s_waitcnt lgkmcnt(0)"] if not final else []) + [   # (the clock read)
         "s_and_b32 %s, %s, 0xffff" % (s(S_T0), P),
         "s_cbranch_scc0 .Lsp_none_%s" % tag]                   # nothing unwritten
    if not final:
        L += [# the next group's slot is taken: write now
              "s_and_b32 %s, %s, %s" % (s(S_T0), s(S_GROUP), s(S_KMASK)),
              "s_lshr_b32 %s, %s, 28" % (s(S_T1), P),
              "s_and_b32 %s, %s, 8" % (s(S_T1), s(S_T1)),
              "s_cmp_eq_u32 %s, 0" % s(S_T0),
              "s_cbranch_scc0 .Lph_nf_%s" % tag,
              "s_bitcmp1_b32 %s, %d" % (s(S_WPHASE), WPHASE_WIDE),
              "s_cbranch_scc0 .Lph_nf_%s" % tag,
              "s_xor_b32 %s, %s, 8" % (s(S_T1), s(S_T1)),           # (a new superblock's half)
              ".Lph_nf_%s:" % tag,
              "s_or_b32 %s, %s, %s" % (s(S_T0), s(S_T0), s(S_T1)),
              "s_bitcmp1_b32 %s, %s" % (P, s(S_T0)),
              "s_cbranch_scc1 .Lph_write_%s" % tag,
              # (width, offset 0)
              "s_and_b32 %s, %s, 0x%x" % (s(S_T1), s(S_WPHASE), 0x1f << WPHASE_PERIOD_SHIFT),
              "s_and_b32 %s, %s, 0xffff" % (s(S_T2), s(S_WPHASE)),
              "s_bfe_u32 %s, %s, %s" % (s(S_T0), s(S_CLOCK), s(S_T1)),
              "s_cmp_lt_u32 %s, %s" % (s(S_T0), s(S_T2)),
              "s_cbranch_scc0 .Lsp_none_%s" % tag,
              ".Lph_write_%s:" % tag]
    L += ["s_mov_b64 exec, -1",
          "v_lshrrev_b32 %s, 1, v%d" % (v(R[0]), V_L16),                # lane * 8
          "s_andn2_b32 %s, %s, %s" % (s(S_T1), s(S_PREVG), s(S_KMASK)),  # cur: S_PREVG's superblock
          "s_add_u32 %s, %s, %s" % (s(S_T2), s(S_GSTRIDE), s(S_KMASK)),  # superblock stride
          "s_sub_u32 %s, %s, %s" % (s(S_T0), s(S_T1), s(S_T2)),         # prev: the one before
          "s_bitcmp1_b32 %s, %d" % (s(S_WPHASE), WPHASE_WIDE),
          "s_cselect_b32 %s, %s, 0" % (s(S_T2), s(S_T2)),
          "s_sub_u32 %s, %s, %s" % (s(S_T2), s(S_T0), s(S_T2)),         # back
          "s_and_b32 %s, %s, %s" % (s(S_T3), s(S_PREVG), s(S_KMASK)),   # S_PREVG's slot index
          # every packet of cur (and so of the older ones) in the batch: no per-slot bounds (all
          # but a launch's last superblock)
          "s_lshr_b32 s66, %s, 6" % s(S_COUNT),
          "s_add_u32 s67, %s, %s" % (s(S_T1), s(S_KMASK)),
          "s_cmp_lt_u32 s67, s66",
          "s_cbranch_scc0 .Lph_ragged_%s" % tag]
    # result addresses of cur, prev and back: s[60:61], s[62:63], s[64:65]
    for lo, g in ((60, S_T1), (62, S_T0), (64, S_T2)):
        L += ["s_lshl_b32 s%d, %s, 9" % (lo, s(g)),
              "s_lshr_b32 s%d, %s, 23" % (lo + 1, s(g)),
              "s_add_u32 s%d, s%d, %s" % (lo, lo, s(S_RET)),
              "s_addc_u32 s%d, s%d, %s" % (lo + 1, lo + 1, s(S_RET + 1))]
    halves = [0] if img.retk == img.slots else [0, 1]

    def slots_of(half, ragged):
        """The writes for S_PREVG's half `half`: its own slots, then the other half's."""
        out = []
        for own in (True, False):
            h = half if own else 1 - half
            if h not in halves:
                continue
            for i in range(img.retk):
                j = 8 * h + i
                sk = ".Lph_%s%d_%d_%s" % ("r" if ragged else "f", half, j, tag)
                out += ["s_bitcmp1_b32 %s, %d" % (P, j), "s_cbranch_scc0 %s" % sk]
                if not ragged:
                    if own:
                        out += ["s_cmp_ge_u32 %s, %d" % (s(S_T3), i),
                                "s_cselect_b64 s[66:67], s[60:61], s[64:65]"]
                    out.append("global_store_dwordx2 %s, v[%d:%d], s[%d:%d] offset:%d%s" % (
                        v(R[0]), img.v_rb + 2 * j, img.v_rb + 2 * j + 1, 66 if own else 62,
                        67 if own else 63, 512 * i, SETTINGS.st_policy))
                else:
                    if own:
                        out += ["s_cmp_ge_u32 %s, %d" % (s(S_T3), i),
                                "s_cselect_b32 %s, %s, %s" % (s(S_BYTES), s(S_T1), s(S_T2))]
                    else:
                        out.append("s_mov_b32 %s, %s" % (s(S_BYTES), s(S_T0)))
                    out += ["s_add_u32 %s, %s, %d" % (s(S_BYTES), s(S_BYTES), i),   # the group
                            "s_lshl_b32 s66, %s, 6" % s(S_BYTES),
                            "s_sub_u32 s66, %s, s66" % s(S_COUNT),                 # its packets
                            "v_cmp_gt_u32_e64 vcc, s66, %s" % v(R[1]),
                            "s_mov_b64 exec, vcc",
                            "s_lshl_b32 s66, %s, 9" % s(S_BYTES),
                            "s_lshr_b32 s67, %s, 23" % s(S_BYTES),
                            "s_add_u32 s66, s66, %s" % s(S_RET),
                            "s_addc_u32 s67, s67, %s" % s(S_RET + 1),
                            "global_store_dwordx2 %s, v[%d:%d], s[66:67]%s" % (
                                v(R[0]), img.v_rb + 2 * j, img.v_rb + 2 * j + 1, SETTINGS.st_policy),
                            "s_mov_b64 exec, -1"]
                out.append(sk + ":")
        return out

    for ragged in (False, True):
        if ragged:
            L += [".Lph_ragged_%s:" % tag,
                  "v_lshrrev_b32 %s, 4, v%d" % (v(R[1]), V_L16)]            # lane
        if len(halves) > 1:
            L += ["s_bitcmp1_b32 %s, 31" % P,
                  "s_cbranch_scc1 .Lph_%sh1_%s" % ("r" if ragged else "f", tag)]
        L += slots_of(0, ragged) + ["s_branch .Lph_done_%s" % tag]
        if len(halves) > 1:
            L += [".Lph_%sh1_%s:" % ("r" if ragged else "f", tag)] + slots_of(1, ragged) + [
                  "s_branch .Lph_done_%s" % tag]
    L += [".Lph_done_%s:" % tag,
          "s_and_b32 %s, %s, 0x80000000" % (P, P),                  # (keeps the half)
          "s_branch .Lsp_none_%s" % tag,
          ".Lph_off_%s:" % tag]
    return L


def store_prev_results(img, tag, final):
    """Write the result slots of the superblock that group S_PREVG ends (at the start of the
    next superblock, or at the end: `final`) as one burst of RETK x 512 B; clobbers exec.
    (With write phasing on, store_phased decides instead.)"""
    L = store_phased(img, tag, final) if img.phased else []
    L += ["s_cmp_eq_u32 %s, -1" % s(S_PREVG),
         "s_cbranch_scc1 .Lsp_none_%s" % tag]
    if not final and img.retk > 1:
        L += ["s_and_b32 %s, %s, %s" % (s(S_T0), s(S_PREVG), s(S_KMASK)),
              "s_cmp_lg_u32 %s, %s" % (s(S_T0), s(S_KMASK)),
              "s_cbranch_scc1 .Lsp_none_%s" % tag]
    # R0 = byte offset of the superblock's first packet result for this lane; R1 = its index
    # (all lanes: the current group's live mask says nothing about the stored groups)
    L += ["s_mov_b64 exec, -1",
          # (one result slot: the group itself, whatever the superblock size the host chose)
          "s_andn2_b32 %s, %s, %s" % (s(S_T0), s(S_PREVG), s(S_KMASK)) if img.retk > 1 else
          "s_mov_b32 %s, %s" % (s(S_T0), s(S_PREVG)),
          ] + (["v_lshrrev_b32 %s, 4, v%d" % (v(R[1]), V_L16),
                "v_lshl_add_u32 %s, %s, 6, %s" % (v(R[1]), s(S_T0), v(R[1]))] if img.staged else
               ["v_mov_b32 %s, v%d" % (v(R[1]), V_IDX)]) + [
          "v_lshlrev_b32 %s, 3, %s" % (v(R[0]), v(R[1]))]
    for k in range(img.retk):
        if k:
            L += ["s_cmp_lt_u32 %s, %d" % (s(S_KMASK), k),        # past this launch's K'
                  "s_cbranch_scc1 .Lsp_none_%s" % tag,
                  "v_add_u32 %s, 64, %s" % (v(R[1]), v(R[1]))]
        L += ["v_cmp_gt_u32_e64 vcc, %s, %s" % (s(S_COUNT), v(R[1])),
              "s_mov_b64 exec, vcc",
              "global_store_dwordx2 %s, v[%d:%d], %s offset:%d%s" % (
                  v(R[0]), img.v_rb + 2 * k, img.v_rb + 2 * k + 1, sp(S_RET), 512 * k, SETTINGS.st_policy)]
    L.append(".Lsp_none_%s:" % tag)
    return L


def next_group(dst):
    """dst = the group after S_GROUP in this wave's sequence (superblocks of RETK groups;
    S_GSTRIDE holds the jump to the next superblock's first group)."""
    return ["s_and_b32 %s, %s, %s" % (s(dst), s(S_GROUP), s(S_KMASK)),
            "s_cmp_eq_u32 %s, %s" % (s(dst), s(S_KMASK)),
            "s_cselect_b32 %s, %s, 1" % (s(dst), s(S_GSTRIDE)),
            "s_add_u32 %s, %s, %s" % (s(dst), s(dst), s(S_GROUP))]


def common_group_code(img):
    """Shared by all kernels (MODE_STAGED: staged 64-B packets; MODE_JIT: compiled program)."""
    L = [".Lcb:",
         "ebpf_cb:",
         ".Lprologue:"]
    # lane stack bottom = lds_base + (wave*64 + lane) * stride
    L += ["s_lshl_b32 %s, %s, 6" % (s(S_T0), s(S_WAVE)),
          "v_add_u32 %s, %s, %s" % (v(H[1]), s(S_T0), v(H[0])),          # tid
          "v_mul_lo_u32 %s, %s, %s" % (v(H[4]), v(H[1]), s(S_STKSTRIDE)),
          "v_add_u32 v%d, %s, %s" % (V_STK, s(S_LDSBASE), v(H[4]))]
    # zero the LDS verdict histogram (bins 0..255, one per lane of the 4 waves)
    L += ["v_lshlrev_b32 %s, 2, %s" % (v(H[2]), v(H[1])),
          "v_mov_b32 %s, 0" % v(H[3]),
          "ds_write_b32 %s, %s" % (v(H[2]), v(H[3]))]
    # copy the LDS-resident array maps (dp_map.lds_off != ~0) into LDS: 256 lanes x 4 B
    L += ["v_lshlrev_b32 %s, 2, %s" % (v(H[4]), v(H[1])),
          "s_mov_b32 %s, 0" % s(S_T2),
          ".Lmc_loop:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_NMAPS)),
          "s_cbranch_scc1 .Lmc_done",
          "s_lshl_b32 %s, %s, 5" % (s(S_T3), s(S_T2)),
          "s_load_dwordx8 s[%d:%d], %s, %s" % (S_REC, S_REC + 7, sp(S_MAPS), s(S_T3)),
          "s_waitcnt lgkmcnt(0)",
          "s_add_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_cmp_eq_u32 s70, -1",
          "s_cbranch_scc1 .Lmc_loop",
          "s_mul_i32 %s, s68, s69" % s(S_T1),
          "s_mov_b32 %s, 0" % s(S_T0),
          ".Lmc_chunk:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T0), s(S_T1)),
          "s_cbranch_scc1 .Lmc_zero",
          "v_add_u32 %s, %s, %s" % (v(H[5]), s(S_T0), v(H[4])),
          "v_cmp_gt_u32_e64 vcc, %s, %s" % (s(S_T1), v(H[5])),
          "s_mov_b64 exec, vcc",
          "global_load_dword %s, %s, s[66:67]" % (v(H[3]), v(H[5])),
          "s_waitcnt vmcnt(0)",
          "v_add_u32 %s, s70, %s" % (v(H[5]), v(H[5])),
          "ds_write_b32 %s, %s" % (v(H[5]), v(H[3])),
          "s_mov_b64 exec, -1",
          "s_add_u32 %s, %s, 1024" % (s(S_T0), s(S_T0)),
          "s_branch .Lmc_chunk",
          # a DP_MAP_LDSDELTA map: its workgroup sums start at zero
          ".Lmc_zero:",
          "s_bitcmp1_b32 s71, 29",
          "s_cbranch_scc0 .Lmc_loop",
          "s_and_b32 %s, s71, 0xffff" % s(S_T3),
          "v_mov_b32 %s, 0" % v(H[3]),
          "s_mov_b32 %s, 0" % s(S_T0),
          ".Lmc_zchunk:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T0), s(S_T1)),
          "s_cbranch_scc1 .Lmc_loop",
          "v_add_u32 %s, %s, %s" % (v(H[5]), s(S_T0), v(H[4])),
          "v_cmp_gt_u32_e64 vcc, %s, %s" % (s(S_T1), v(H[5])),
          "s_mov_b64 exec, vcc",
          "v_add_u32 %s, %s, %s" % (v(H[5]), s(S_T3), v(H[5])),
          "ds_write_b32 %s, %s" % (v(H[5]), v(H[3])),
          "s_mov_b64 exec, -1",
          "s_add_u32 %s, %s, 1024" % (s(S_T0), s(S_T0)),
          "s_branch .Lmc_zchunk",
          ".Lmc_done:",
          "s_waitcnt lgkmcnt(0)",
          "s_barrier"]
    # groups of 64 packets: group = workgroup*4 + wave, stride = total waves
    L += ["s_add_u32 %s, %s, 63" % (s(S_NGROUPS), s(S_COUNT)),
          "s_lshr_b32 %s, %s, 6" % (s(S_NGROUPS), s(S_NGROUPS)),
          # (an XCD-major logical workgroup order, each XCD one contiguous share of the
          # batch, measured 1-5% slower: profiles/r02/s3/ab_xcd_order.txt)
          "s_lshl_b32 %s, s2, 2" % s(S_GROUP),
          "s_add_u32 %s, %s, %s" % (s(S_GROUP), s(S_GROUP), s(S_WAVE)),
          # K' = superblock size of this launch (total_waves bits 28..29 = log2 K')
          "s_lshr_b32 %s, %s, %d" % (s(S_T1), s(S_GSTRIDE), WAVES_SB_SHIFT),
          "s_and_b32 %s, %s, 0xffff" % (s(S_GSTRIDE), s(S_GSTRIDE)),
          "s_lshl_b32 %s, 1, %s" % (s(S_KMASK), s(S_T1)),
          "s_sub_u32 %s, %s, 1" % (s(S_KMASK), s(S_KMASK)),
          "s_lshl_b32 %s, %s, %s" % (s(S_GROUP), s(S_GROUP), s(S_T1)),
          ] + [
          # superblock jump: (total waves - 1) * K' + 1
          "s_lshl_b32 %s, %s, %s" % (s(S_GSTRIDE), s(S_GSTRIDE), s(S_T1)),
          "s_sub_u32 %s, %s, %s" % (s(S_GSTRIDE), s(S_GSTRIDE), s(S_KMASK)),
          # this wave's packet buffer (staged kernel); first group's prefetch
          "s_lshl_b32 %s, %s, 12" % (s(S_T0), s(S_WAVE)),
          "s_add_u32 %s, %s, %s" % (s(S_PKTLDS), s(S_PKTLDS), s(S_T0)),
          mode_test(MODE_STAGED),
          "s_cbranch_scc0 .Lgroup_check",
          "s_mov_b32 %s, %s" % (s(S_T0), s(S_GROUP))] + call(".Lr_prefetch") + [
          "s_branch .Lgroup_check"]
    L += [".Lgroup_done:"]
    L += slot_commit(img) + next_group(S_T0) + [
          # keep mode (MODE_KEEP and MODE_STAGED: staged kernels): the next group's DMA, now that the
          # program is done with the packet buffer
          "s_and_b32 %s, %s, 0x%x" % (s(S_BYTES), s(S_MODE), 1 << MODE_KEEP | 1 << MODE_STAGED),
          "s_cmp_eq_u32 %s, 0x4001" % s(S_BYTES),
          "s_cbranch_scc0 .Lgd_nokeep"] + call(".Lr_prefetch") + [
          ".Lgd_nokeep:",
          "s_mov_b32 %s, %s" % (s(S_GROUP), s(S_T0)),
          ".Lgroup_check:",
          "s_mov_b64 exec, -1",
          "s_cmp_lt_u32 %s, %s" % (s(S_GROUP), s(S_NGROUPS)),
          "s_cbranch_scc0 .Lfinish",
          ] + (
          # write phasing: the clock read for store_phased, early so that the group's staging
          # waits cover its latency
          ["s_cmp_eq_u32 %s, 0" % s(S_WPHASE),
           "s_cbranch_scc1 .Lgc_noclock",
           "s_memrealtime s[%d:%d]" % (S_CLOCK, S_CLOCK + 1),
           ".Lgc_noclock:"] if img.phased else []) + lane_index(img, H[0]) + [
          "v_lshl_add_u32 v%d, %s, 6, %s" % (V_GIDX, s(S_GROUP), v(H[0])),      # packet index
          "v_cmp_gt_u32_e64 %s, %s, v%d" % (sp(S_ALIVE), s(S_COUNT), V_GIDX),
          ] + [
          mode_test(MODE_STAGED),
          "s_cbranch_scc0 .Lgs_general",
          # staged: this group's packets are (or are being) DMA'd into the packet buffer
          "s_waitcnt vmcnt(0)",
          # lane p's chunk c at 1024 (p >> 4) + 256 c + 16 (p & 15) (dma_lane_offsets):
          # 16 p + 3 x (16 p & 0x300), then 256 c per chunk
          "v_and_b32 %s, 0x300, v%d" % (v(H[1]), V_L16),
          "v_mad_u32_u24 %s, %s, 3, v%d" % (v(H[1]), v(H[1]), V_L16),
          "v_add_u32 %s, %s, %s" % (v(H[1]), s(S_PKTLDS), v(H[1]))]
    for q in range(4):
        L.append("ds_read_b128 v[%d:%d], %s offset:%d" % (PKT0 + 4 * q, PKT0 + 4 * q + 3,
                                                          v(H[1]), 256 * q))
    # next group's DMA: a full group (the common case) inline, with exec = all lanes and the
    # instruction offset stepping both the global and the LDS address (M0 set once); a partial
    # group through the masking routine.  (Keep mode, MODE_KEEP: none here; .Lgroup_done
    # issues it once the program is done with the buffer)
    # (keep mode: the group's packets rewritten transposed for the program's loads at run-time
    # offsets, lds_pkt_dwords, once every lane's staging read has returned)
    L += ["s_waitcnt lgkmcnt(0)",
          mode_test(MODE_KEEP),
          "s_cbranch_scc0 .Lgs_pf_dma",
          "v_lshrrev_b32 %s, 2, v%d" % (v(H[1]), V_L16),
          "v_add_u32 %s, %s, %s" % (v(H[1]), s(S_PKTLDS), v(H[1]))] + lds_pkt_dwords(v(H[1])) + [
          "s_branch .Lgs_pf_done",
          ".Lgs_pf_dma:"] + next_group(S_T0) + [
          "s_lshr_b32 %s, %s, 6" % (s(S_BYTES), s(S_COUNT)),        # full groups
          "s_cmp_lt_u32 %s, %s" % (s(S_T0), s(S_BYTES)),
          "s_cbranch_scc0 .Lgs_pf_slow",
          "s_lshr_b32 s65, %s, 20" % s(S_T0),
          "s_lshl_b32 s64, %s, 12" % s(S_T0),
          "s_add_u32 s64, s64, %s" % s(S_DATA),
          "s_addc_u32 s65, s65, %s" % s(S_DATA + 1),
          "s_mov_b64 exec, -1"] + dma_lane_offsets(v(H[4]), v(H[5])) + [
          "s_mov_b32 m0, %s" % s(S_PKTLDS),
          "s_nop 0"] + [
          "global_load_lds_dwordx4 %s, s[64:65] offset:%d%s" % (v(H[4]), 1024 * qq, SETTINGS.ld_policy)
          for qq in range(4)] + [
          "s_branch .Lgs_pf_done",
          ".Lgs_pf_slow:"] + call(".Lr_prefetch") + [
          ".Lgs_pf_done:",
          # a compiled program computes the packet address itself if it needs it
          mode_test(MODE_JIT),
          "s_cbranch_scc1 .Lgs_init",
          "s_mov_b64 exec, %s" % sp(S_ALIVE),
          "v_mov_b32 %s, 64" % v(H[1]),
          "v_mad_u64_u32 v[%d:%d], %s, v%d, %s, %s" % (V_PKT, V_PKT + 1, sp(S_JUNK), V_GIDX,
                                                       v(H[1]), sp(S_DATA)),
          "v_mov_b32 v%d, 64" % V_LEN,
          "s_branch .Lgs_init",
          ".Lgs_general:",
          "s_mov_b64 exec, %s" % sp(S_ALIVE)] + pkt_setup(V_GIDX, "g") + [
          ".Lgs_init:"] + store_prev_results(img, "g", False) + [
          "s_mov_b32 %s, %s" % (s(S_PREVG), s(S_GROUP))] + ([] if img.staged else [
          # V_IDX: this group's packet indices (after the previous group's store read them)
          "s_mov_b64 exec, -1",
          "v_mov_b32 v%d, v%d" % (V_IDX, V_GIDX)]) + [
          "s_mov_b64 exec, %s" % sp(S_ALIVE),
          # fault code 0 for the whole group up front (a faulting lane overwrites its byte)
          "s_cmp_eq_u64 %s, 0" % sp(S_FAULTS),
          "s_cbranch_scc1 .Lgs_nofz",
          ] + lane_pkt_index(img, R[9]) + [
          "v_mov_b32 %s, 0" % v(R[8]),
          "global_store_byte %s, %s, %s" % (v(R[9]), v(R[8]), sp(S_FAULTS)),
          ".Lgs_nofz:",
          # a compiled program (MODE_JIT) starts at the head of its code area and sets up the
          # registers it reads itself (packet address, r1, r10, zeroes: asm_cc.cpp prologue)
          mode_test(MODE_JIT),
          "s_cbranch_scc0 .Lgs_interp"] + goto("ebpf_jit_area+%d" % JIT_ENTRY_OFF) + [
          ".Lgs_interp:"]
    # r0, r2..r9 start at zero
    for r in range(0, 20, 2):
        if r != 2:
            L.append("v_mov_b64 v[%d:%d], 0" % (r, r + 1))
    L += ["v_mov_b64 v[2:3], v[%d:%d]" % (V_PKT, V_PKT + 1),
          "v_add_u32 v20, %s, v%d" % (s(S_STKSTRIDE), V_STK),
          "v_mov_b32 v21, %s" % s(S_SHARED + 1),
          "s_lshl_b32 %s, %s, 5" % (s(S_T0), s(S_START)),
          "v_mov_b32 v%d, %s" % (V_T, s(S_T0))] + goto(".Lr_schedule")
    # finish: this workgroup's LDS histogram (u32 bins) goes into the launch's u64 partial
    # histograms with device-scope atomics, one replica per (workgroup & 7) so that the adds to
    # a hot bin spread over 8 lines; the workgroup whose ticket add returns nwg - 1 arrived last
    # and moves the 8 replicas (read-and-zero swaps) plus the fault count into the caller's
    # histogram (stored, or added), then re-arms the ticket.  One kernel per launch: no
    # second-stage reduce (hand-off form: 8-B agent atomics on both sides, MI355X_MICROARCH.md
    # "Valid forms")
    HR = HIST_REPLICA_BYTES
    L += [".Lfinish:"] + store_prev_results(img, "f", True)
    L += [".Lfinish_body:",
          "s_mov_b64 exec, -1",
          "s_waitcnt vmcnt(0) lgkmcnt(0)",
          "s_barrier"]
    # DP_MAP_LDSDELTA maps: the workgroup's sums into the delta areas (a global atomic per
    # non-zero word; lane tid takes words tid, tid + 256, ...)
    L += lane_index(img, H[0]) + [
          "s_lshl_b32 %s, %s, 6" % (s(S_T0), s(S_WAVE)),
          "v_add_u32 %s, %s, %s" % (v(H[1]), s(S_T0), v(H[0])),       # tid
          "s_mov_b32 %s, 0" % s(S_T2),
          ".Lfd_loop:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_NMAPS)),
          "s_cbranch_scc1 .Lfd_done",
          "s_lshl_b32 %s, %s, 5" % (s(S_T3), s(S_T2)),
          "s_load_dwordx8 s[%d:%d], %s, %s" % (S_REC, S_REC + 7, sp(S_MAPS), s(S_T3)),
          "s_waitcnt lgkmcnt(0)",
          "s_add_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_bitcmp1_b32 s71, 29",
          "s_cbranch_scc0 .Lfd_loop",
          "s_mul_i32 %s, s68, s69" % s(S_T1),                          # bytes
          "s_add_u32 %s, %s, 63" % (s(S_BYTES), s(S_T1)),
          "s_and_b32 %s, %s, -64" % (s(S_BYTES), s(S_BYTES)),          # dp_delta_off
          "s_add_u32 s66, s66, %s" % s(S_BYTES),
          "s_addc_u32 s67, s67, 0",                                    # the delta area
          "s_and_b32 %s, s71, 0xffff" % s(S_T3),                       # the LDS sums
          "s_bitcmp1_b32 s71, 28",
          "s_cselect_b32 %s, 3, 2" % s(S_CODE),                        # log2 of the word
          "v_lshlrev_b32 %s, %s, %s" % (v(H[2]), s(S_CODE), v(H[1])),  # first byte offset
          "s_lshl_b32 %s, 256, %s" % (s(S_BYTES), s(S_CODE)),          # bytes per round
          ".Lfd_word:",
          "v_cmp_gt_u32_e64 vcc, %s, %s" % (s(S_T1), v(H[2])),
          "s_and_saveexec_b64 %s, vcc" % sp(S_MASK),
          "s_cbranch_execz .Lfd_next",
          "v_add_u32 %s, %s, %s" % (v(H[3]), s(S_T3), v(H[2])),
          "v_mov_b32 %s, 0" % v(R[3]),
          "s_cmp_eq_u32 %s, 3" % s(S_CODE),
          "s_cbranch_scc0 .Lfd_r4",
          "ds_read_b64 %s, %s" % (vp(R[2]), v(H[3])),
          "s_branch .Lfd_r",
          ".Lfd_r4:",
          "ds_read_b32 %s, %s" % (v(R[2]), v(H[3])),
          ".Lfd_r:",
          "s_waitcnt lgkmcnt(0)",
          "v_cmp_ne_u64_e64 vcc, 0, %s" % vp(R[2]),
          "s_and_b64 exec, exec, vcc",
          "s_cbranch_execz .Lfd_next",
          "v_mov_b32 %s, %s" % (v(R[0]), v(H[2])),
          "s_cmp_eq_u32 %s, 3" % s(S_CODE),
          "s_cbranch_scc0 .Lfd_w4",
          "global_atomic_add_x2 %s, %s, s[66:67]" % (v(R[0]), vp(R[2])),
          "s_branch .Lfd_next",
          ".Lfd_w4:",
          "global_atomic_add %s, %s, s[66:67]" % (v(R[0]), v(R[2])),
          ".Lfd_next:",
          "s_mov_b64 exec, %s" % sp(S_MASK),
          "v_add_u32 %s, %s, %s" % (v(H[2]), s(S_BYTES), v(H[2])),
          "v_cmp_gt_u32_e64 vcc, %s, %s" % (s(S_T1), v(H[2])),
          "s_and_b64 vcc, vcc, exec",
          "s_cbranch_scc1 .Lfd_word",
          "s_mov_b64 exec, -1",
          "s_branch .Lfd_loop",
          ".Lfd_done:",
          "s_mov_b64 exec, -1",
          "s_cmp_eq_u64 %s, 0" % sp(S_HIST),
          "s_cbranch_scc1 .Lfin_end",
          ] + lane_index(img, H[0]) + [
          "s_lshl_b32 %s, %s, 6" % (s(S_T0), s(S_WAVE)),
          "v_add_u32 %s, %s, %s" % (v(H[1]), s(S_T0), v(H[0])),       # bin
          "v_lshlrev_b32 %s, 2, %s" % (v(H[2]), v(H[1])),
          "ds_read_b32 %s, %s" % (v(H[3]), v(H[2])),
          "s_load_dwordx2 %s, %s" % (sp(S_REC), karg("hist_rows")),
          "s_load_dwordx4 s[68:71], %s" % karg("hist_user", "hist_flags", "nwg"),
          "s_waitcnt lgkmcnt(0)",
          "s_cmp_eq_u64 %s, 0" % sp(S_REC),
          "s_cbranch_scc1 .Lfin_atomic",
          "s_and_b32 %s, s2, 7" % s(S_T1),
          "s_mul_i32 %s, %s, %d" % (s(S_T1), s(S_T1), HR),
          "v_lshlrev_b32 %s, 3, %s" % (v(R[0]), v(H[1])),
          "v_add_u32 %s, %s, %s" % (v(R[0]), s(S_T1), v(R[0])),
          "v_mov_b32 %s, %s" % (v(R[2]), v(H[3])),
          "v_mov_b32 %s, 0" % v(R[3]),
          "v_cmp_ne_u32_e64 vcc, 0, %s" % v(H[3]),
          "s_and_saveexec_b64 %s, vcc" % sp(S_SAVE),
          "s_cbranch_execz .Lfin_noadd",
          "global_atomic_add_x2 %s, %s, %s" % (v(R[0]), vp(R[2]), sp(S_REC)),
          ".Lfin_noadd:",
          "s_mov_b64 exec, -1",
          "s_waitcnt vmcnt(0)",          # this wave's adds (and its fault counts) performed
          "s_barrier",                   # ... and every wave's
          "s_cmp_eq_u32 %s, 0" % s(S_WAVE),
          "s_cbranch_scc0 .Lfin_flag",
          # two-level ticket (one hot word would serialise every workgroup's arrival): the
          # workgroups of replica r = wg & 7 count on ticket r; the last of them (its add
          # returns n_r - 1, n_r = (nwg - 1 - r) / 8 + 1) re-arms ticket r and counts on the
          # top ticket, whose last arrival (min(nwg, 8) - 1) is the launch's last workgroup
          "s_mov_b64 exec, 1",
          "s_and_b32 %s, s2, 7" % s(S_T1),
          "s_lshl_b32 %s, %s, 6" % (s(S_T0), s(S_T1)),
          "s_add_u32 %s, %s, %d" % (s(S_T0), s(S_T0), HIST_TICKET_OFF),
          "v_mov_b32 %s, %s" % (v(R[4]), s(S_T0)),
          "v_mov_b32 %s, 1" % v(R[5]),
          "global_atomic_add %s, %s, %s, %s sc0" % (v(R[6]), v(R[4]), v(R[5]), sp(S_REC)),
          "s_sub_u32 %s, s71, 1" % s(S_T3),
          "s_sub_u32 %s, %s, %s" % (s(S_T3), s(S_T3), s(S_T1)),
          "s_lshr_b32 %s, %s, 3" % (s(S_T3), s(S_T3)),        # n_r - 1
          "s_waitcnt vmcnt(0)",
          "v_readfirstlane_b32 %s, %s" % (s(S_T2), v(R[6])),
          "s_cmp_eq_u32 %s, %s" % (s(S_T2), s(S_T3)),
          "s_cselect_b32 %s, 1, 0" % s(S_T2),
          "s_cbranch_scc0 .Lfin_setflag",
          "v_mov_b32 %s, 0" % v(R[10]),
          "global_atomic_swap %s, %s, %s, %s sc0" % (v(R[8]), v(R[4]), v(R[10]), sp(S_REC)),
          "v_mov_b32 %s, %d" % (v(R[9]), HIST_TICKET_OFF + 64 * HIST_REPLICAS),
          "global_atomic_add %s, %s, %s, %s sc0" % (v(R[6]), v(R[9]), v(R[5]), sp(S_REC)),
          "s_min_u32 %s, s71, %d" % (s(S_T3), HIST_REPLICAS),
          "s_sub_u32 %s, %s, 1" % (s(S_T3), s(S_T3)),
          "s_waitcnt vmcnt(0)",
          "v_readfirstlane_b32 %s, %s" % (s(S_T2), v(R[6])),
          "s_cmp_eq_u32 %s, %s" % (s(S_T2), s(S_T3)),
          "s_cselect_b32 %s, 1, 0" % s(S_T2),
          ".Lfin_setflag:",
          "v_mov_b32 %s, %s" % (v(R[7]), s(S_T2)),
          "v_mov_b32 %s, 0" % v(R[8]),
          # LDS word 0 (bin 0, read by every wave before the barrier above) tells the others
          "ds_write_b32 %s, %s" % (v(R[8]), v(R[7])),
          "s_mov_b64 exec, -1",
          "s_waitcnt lgkmcnt(0)",
          ".Lfin_flag:",
          "s_barrier",
          "v_mov_b32 %s, 0" % v(R[8]),
          "ds_read_b32 %s, %s" % (v(R[7]), v(R[8])),
          "s_waitcnt lgkmcnt(0)",
          "v_readfirstlane_b32 %s, %s" % (s(S_T2), v(R[7])),
          "s_cmp_eq_u32 %s, 0" % s(S_T2),
          "s_cbranch_scc1 .Lfin_end",
          # the last workgroup: wave w moves bins 64w..64w+63 (v0..v15 results, v16..v23
          # addresses, v[24:25] = 0: the eBPF registers and staged packet are dead here)
          "v_lshlrev_b32 %s, 3, %s" % (v(R[0]), v(H[1])),
          "v_mov_b32 v24, 0",
          "v_mov_b32 v25, 0"]
    for r in range(HIST_REPLICAS):
        L += ["v_add_u32 v%d, %d, %s" % (16 + r, r * HR, v(R[0])),
              "global_atomic_swap_x2 v[%d:%d], v%d, v[24:25], %s sc0" % (2 * r, 2 * r + 1, 16 + r,
                                                                       sp(S_REC))]
    L += ["s_waitcnt vmcnt(0)"]
    for r in range(1, HIST_REPLICAS):
        L += ["v_lshl_add_u64 v[0:1], v[%d:%d], 0, v[0:1]" % (2 * r, 2 * r + 1)]
    L += ["s_bitcmp1_b32 s70, %d" % HIST_STORE,                   # hist_flags: store (overwrite)
          "s_cbranch_scc0 .Lfin_add",
          "global_store_dwordx2 %s, v[0:1], s[68:69]" % v(R[0]),
          "s_branch .Lfin_faults",
          ".Lfin_add:",
          "global_atomic_add_x2 %s, v[0:1], s[68:69]" % v(R[0]),
          ".Lfin_faults:",
          "s_cmp_eq_u32 %s, 0" % s(S_WAVE),
          "s_cbranch_scc0 .Lfin_end",
          "s_mov_b64 exec, 1",                       # bin 256 (replica 0 only) and the ticket
          "v_mov_b32 v16, 2048",
          "global_atomic_swap_x2 v[2:3], v16, v[24:25], %s sc0" % sp(S_REC),
          "v_mov_b32 v17, %d" % (HIST_TICKET_OFF + 64 * HIST_REPLICAS),   # the top ticket
          "global_atomic_swap v18, v17, v24, %s sc0" % sp(S_REC),
          "s_waitcnt vmcnt(0)",
          "s_bitcmp1_b32 s70, %d" % HIST_STORE,
          "s_cbranch_scc0 .Lfin_fadd",
          "global_store_dwordx2 v16, v[2:3], s[68:69]",
          "s_branch .Lfin_end",
          ".Lfin_fadd:",
          "global_atomic_add_x2 v16, v[2:3], s[68:69]",
          "s_branch .Lfin_end",
          # no partial buffer (variant-free fallback used by nothing today): per-bin atomics
          ".Lfin_atomic:",
          "v_cmp_ne_u32_e64 vcc, 0, %s" % v(H[3]),
          "s_and_saveexec_b64 %s, vcc" % sp(S_SAVE),
          "v_lshlrev_b32 %s, 3, %s" % (v(R[0]), v(H[1])),
          "v_mov_b32 %s, %s" % (v(R[2]), v(H[3])),
          "v_mov_b32 %s, 0" % v(R[3]),
          "global_atomic_add_x2 %s, %s, %s" % (v(R[0]), vp(R[2]), sp(S_HIST)),
          ".Lfin_end:",
          "s_waitcnt vmcnt(0)",
          "s_endpgm"]
    return L


def link_kernel():
    """ebpf_asm_link(dp_entry *e, uint32_t n): e[i].handler (= handler id) -> absolute address."""
    return [".globl ebpf_asm_link", ".p2align 8", ".type ebpf_asm_link,@function",
            "ebpf_asm_link:",
            "s_load_dwordx2 s[4:5], %s" % karg("entries", table=LINK_ARGS),
            "s_load_dword s6, %s" % karg("count", table=LINK_ARGS),
            "s_getpc_b64 s[8:9]",
            ".Llink_base:",
            "s_add_u32 s10, s8, .Lhandler_table-.Llink_base",
            "s_addc_u32 s11, s9, 0",
            "v_lshl_add_u32 v1, s2, 6, v0",
            "s_waitcnt lgkmcnt(0)",
            "v_cmp_gt_u32_e64 vcc, s6, v1",
            "s_and_b64 exec, exec, vcc",
            "s_cbranch_execz .Llink_end",
            "v_mov_b32 v2, 32",
            "v_mad_u64_u32 v[2:3], s[12:13], v1, v2, s[4:5]",
            "global_load_dword v4, v[2:3], off",
            "s_waitcnt vmcnt(0)",
            "v_mov_b32 v6, 4",
            "v_mad_u64_u32 v[6:7], s[12:13], v4, v6, s[10:11]",
            "global_load_dword v8, v[6:7], off",
            "s_waitcnt vmcnt(0)",
            "v_ashrrev_i32 v9, 31, v8",
            "v_lshl_add_u64 v[10:11], v[8:9], 0, s[8:9]",
            "global_store_dwordx2 v[2:3], v[10:11], off",
            ".Llink_end:",
            "s_waitcnt vmcnt(0)",
            "s_endpgm"]


class Tables(NamedTuple):
    """Per handler, in handler-id order: asm_handlers.h ah_<field>.  The host uses one set for
    all images, so every image must give the same."""
    reads: list    # entry SGPRs (bit k = s(10+k)) the body reads
    flags: list    # bit 0: conditional jump; bit 1: body leaves an LDS read outstanding
    fam: list      # family (AHF_*)
    dst: list      # dst register, 255 = none
    src: list      # src register (LDXPKC: packet byte offset), 255 = none


def kd(name, lds, vgprs, sgprs, kernarg, wgsize):
    return [".rodata", ".p2align 6", ".amdhsa_kernel %s" % name,
            ".amdhsa_group_segment_fixed_size %d" % lds,
            ".amdhsa_private_segment_fixed_size 0",
            ".amdhsa_kernarg_size %d" % kernarg,
            ".amdhsa_user_sgpr_count 2",
            ".amdhsa_user_sgpr_kernarg_segment_ptr 1",
            ".amdhsa_system_sgpr_workgroup_id_x 1",
            ".amdhsa_system_vgpr_workitem_id 0",
            ".amdhsa_next_free_vgpr %d" % vgprs,
            ".amdhsa_next_free_sgpr %d" % sgprs,
            ".amdhsa_accum_offset %d" % vgprs,
            ".amdhsa_reserve_vcc 1",
            ".amdhsa_reserve_xnack_mask 0",
            ".amdhsa_ieee_mode 0",
            ".amdhsa_dx10_clamp 0",
            ".end_amdhsa_kernel", ".text"]


def metadata(kernels):
    out = [".amdgpu_metadata", "---", "amdhsa.kernels:"]
    for name, kernarg, lds, vgprs, sgprs, wg in kernels:
        out += ["  - .args:",
                "      - .offset: 0",
                "        .size: %d" % kernarg,
                "        .value_kind: by_value",
                "    .group_segment_fixed_size: %d" % lds,
                "    .kernarg_segment_align: 8",
                "    .kernarg_segment_size: %d" % kernarg,
                "    .max_flat_workgroup_size: %d" % wg,
                "    .name: %s" % name,
                "    .private_segment_fixed_size: 0",
                "    .sgpr_count: %d" % sgprs,
                "    .symbol: %s.kd" % name,
                "    .vgpr_count: %d" % vgprs,
                "    .wavefront_size: 64"]
    out += ["amdhsa.target: amdgcn-amd-amdhsa--gfx950:xnack-", "amdhsa.version:", "  - 1", "  - 2",
            "...", ".end_amdgpu_metadata"]
    return out


def top_register(lines, bank):
    """The highest register of `bank` ("v" or "s") the lines name, alone or as a range's end."""
    ref = re.compile(r"\b%s(\d+)\b|\b%s\[(\d+):(\d+)\]" % (bank, bank))
    top = 0
    for ln in lines:
        for a, b, c in ref.findall(ln.split(";")[0].split("//")[0]):
            top = max(top, int(a or c))
    return top


def generate(img):
    """One image: (its assembly text, its handler Tables)."""
    A = ['.amdgcn_target "amdgcn-amd-amdhsa--gfx950:xnack-"', ".amdhsa_code_object_version 5", ".text"]
    A += kernel(img, "ebpf_interp_s64", True) + kernel(img, "ebpf_interp_gen", False)
    A += kernel(img, "ebpf_jit_s64", True, True) + kernel(img, "ebpf_jit_gen", False, True)
    A += common_group_code(img) + routines(img)
    table = []
    meta = []
    t = Tables([], [], [], [], [])
    hid = 0
    for fi, (name, arity, _, _) in enumerate(FAMILIES):
        for d, sr in variants(arity):
            t.fam.append(fi)
            t.dst.append(255 if d is None else d)
            t.src.append(255 if sr is None else sr)
            label = "h_%d" % hid
            uid = "%d" % hid
            body, own = handler_body(img, name, d, sr)
            body = [ln.replace("{uid}", uid) for ln in body]
            A.append(".p2align 2")
            A.append("%s:" % label)
            is_cond = "@CMPEND" in body
            if is_cond:
                k = body.index("@CMPEND")
                copy = body[:k]
                A += copy + [".Lhe_%d:" % hid] + body[k + 1:]
            else:
                copy = body
                k = early_fetch_point(body) if (img.interp and not own) else None
                if k is not None and k < len(body):
                    # (this image never feeds the code generator, which copies label..Lhe_)
                    fetch = dispatch(12)
                    A += body[:k] + [fetch[0]] + body[k:] + [".Lhe_%d:" % hid] + fetch[1:]
                else:
                    A += body + [".Lhe_%d:" % hid]
                    if not own:
                        A += dispatch(12)
            m = entry_reads(copy)
            if name == "LOOKUPGEN":
                m |= 1 << 2      # the routine resumes at s12
            if name == "HLOOKUP":
                m |= 1 << 4      # the routine reads the map record offset from s14
            if name in ("UPDATE", "HDELETE"):
                m |= (1 << 4) | (1 << 5)   # map record offset (s14), entry index (s15)
            t.reads.append(m)
            # an LDS read whose result the interpreter's dispatch wait (lgkmcnt) covered
            last_ds = max([i for i, ln in enumerate(copy) if ln.startswith("ds_read")] or [-1])
            waits = [i for i, ln in enumerate(copy) if ln.startswith("s_waitcnt") and "lgkmcnt" in ln]
            needw = last_ds >= 0 and not any(i > last_ds for i in waits)
            t.flags.append((1 if is_cond else 0) | (2 if needw else 0))
            table.append(label)
            meta.append("  .long %s-.Lcb, .Lhe_%d-%s" % (label, hid, label))
            hid += 1
    A += link_kernel()
    A += [".p2align 2", ".Lhandler_table:"]
    A += ["  .long %s-.Llink_base" % lab for lab in table]
    # compiled-program support: handler body table, glue templates, the patch area
    A += [".p2align 2", "ebpf_jit_meta:"] + meta
    A += jit_templates()
    A += [".p2align 8", "ebpf_jit_area:", "  .fill %d, 4, 0xbf810000" % (JIT_AREA_BYTES // 4)]
    # every VGPR the image's code names lies inside the kernels' allocation (a register past it
    # assembles but reads whatever the hardware holds there)
    vtop, vmax = top_register(A, "v"), max(img.nvgpr, img.nvgpr_wide)
    assert vtop < vmax, "image code uses v%d, the kernels allocate %d VGPRs" % (vtop, vmax)
    if img.interp:
        # the interpreter kernel declares s0..s73 only: check that the image's code uses no more
        top = top_register(A, "s")
        assert top < NSGPR_INTERP, "interpreter image uses s%d" % top
    ka, nv, ns = KERNARG_BYTES, img.nvgpr, img.nsgpr
    ks = [("ebpf_interp_s64", ka, 0, nv, img.nsgpr_interp, 256),
          ("ebpf_interp_gen", ka, 0, nv, ns, 256),
          ("ebpf_jit_s64", ka, 0, nv, ns, 256),
          ("ebpf_jit_gen", ka, 0, nv, ns, 256),
          ("ebpf_asm_link", LINK_KERNARG_BYTES, 0, 16, 16, 64)]
    if img.nvgpr_wide:
        ks.append(("ebpf_jit_s64w", ka, 0, img.nvgpr_wide, ns, 256))
    for name, kernarg, lds, vg, sg, wg in ks:
        A += kd(name, lds, vg, sg, kernarg, wg)
    text = "\n".join(("\t" + x if not (x.endswith(":") or x.startswith(".") or x.startswith(" ")) else x)
                     for x in A) + "\n" + "\n".join(metadata(ks)) + "\n"
    return text, t


def header(tables):
    """asm_handlers.h: the handler ids and tables (the same for every image), the family
    structure, the ABI, and what the host must know of each image."""
    h = ["// generated by gen_interp.py — handler family ids for asm_runtime.cpp",
         "#pragma once", "#include <stdint.h>", "#define AH_NREGS %d" % NREG]
    hid = 0
    for fi, (name, arity, _, _) in enumerate(FAMILIES):
        h.append("#define AH_%s %d" % (name, hid))
        h.append("#define AHF_%s %d" % (name, fi))
        hid += len(variants(arity))
    assert hid == len(tables.reads)
    h.append("#define AH_COUNT %d" % hid)
    h.append("// entry SGPRs (bit k = s(10+k)) each handler body reads")
    h.append("static const uint8_t ah_reads[AH_COUNT] = {%s};" % ",".join(map(str, tables.reads)))
    h.append("// bit 0: conditional jump (copy the compare only); bit 1: body leaves an LDS read "
             "outstanding")
    h.append("static const uint8_t ah_flags[AH_COUNT] = {%s};" % ",".join(map(str, tables.flags)))
    h.append("// per handler: family (AHF_*), dst register, src register (LDXPKC: packet byte offset);")
    h.append("// 255 = none.  Read by the optimising code generator (asm_cc.cpp)")
    h.append("static const uint8_t ah_fam[AH_COUNT] = {%s};" % ",".join(map(str, tables.fam)))
    h.append("static const uint8_t ah_dst[AH_COUNT] = {%s};" % ",".join(map(str, tables.dst)))
    h.append("static const uint8_t ah_src[AH_COUNT] = {%s};" % ",".join(map(str, tables.src)))
    h += header_families()
    h += header_abi()
    h.append("#define AH_JIT_AREA_BYTES %d" % JIT_AREA_BYTES)
    h.append("#define AH_S_JOIN %d  // structured programs: taken-lane masks s[74:75]..  (staged image)" % S_JOIN)
    h.append("#define AH_JOIN_LEVELS %d" % JOIN_LEVELS)
    h.append("#define AH_GEN_JOIN %d  // the general image holds the join SGPRs too" % GEN_JOIN)
    h.append("#define AH_GEN_HOIST_BASE 64  // general image: spare VGPRs for hoisted loads")
    h.append("#define AH_GEN_HOIST_REGS %d" % SETTINGS.gen_hoist_regs)
    h.append("#define AH_S_RUNMASK %d  // general image: s[76:77], a hoisted-load run's lanes" % S_RUNMASK)
    h.append("#define AH_V_IDX %d  // general image: the lane's packet index" % V_IDX)
    m1, m0, m3 = IMAGES
    h += ["#define AH_RET_GROUPS_STAGED %d  // groups per result burst, staged kernels" % m1.retk,
          "#define AH_NVGPR_STAGED %d" % m1.nvgpr,
          "#define AH_RET_GROUPS_GENERAL %d" % m0.retk,
          "#define AH_NVGPR_STAGED_WIDE %d  // ebpf_jit_s64w: 16 result slots "
          "(write phasing), 0 = none" % m1.nvgpr_wide,
          "#define AH_NVGPR_GENERAL %d" % m0.nvgpr,
          "#define AH_NVGPR_INTERP %d  // the interpreter's staged image (m3)" % m3.nvgpr,
          "#define AH_RET_GROUPS_INTERP %d" % m3.retk]
    return "\n".join(h) + "\n"


def main():
    """gen_interp.py <staged.s> <general.s> <staged-interpreter.s> <handlers.h>"""
    *out_s, out_h = sys.argv[1:5]
    tables = None
    for img, path in zip(IMAGES, out_s):
        text, t = generate(img)
        assert tables is None or t == tables, "image %s: its handler tables differ" % img.name
        tables = t
        with open(path, "w") as f:
            f.write(text)
    with open(out_h, "w") as f:
        f.write(header(tables))


if __name__ == "__main__":
    main()
