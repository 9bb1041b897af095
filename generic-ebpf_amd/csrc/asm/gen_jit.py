"""Compiled-program support: which entry SGPRs a copied handler body reads, and the glue
templates the host's copy-and-patch compiler stitches between copied bodies (their order in
ebpf_jit_tmpl is gen_abi.py JT_LABELS)."""
import re

from gen_emit import *  # noqa: F401,F403

ENTRY_SGPR_RE = re.compile(r"(?<![\w\[:])s(1[0-5])(?![\w\]])|s\[(1[0-5]):(1[0-5])\]")


def entry_reads(lines):
    """6-bit mask of the entry SGPRs s10..s15 a handler body reads (compiled programs set
    exactly those before the copied body)."""
    m = 0
    for ln in lines:
        code = ln.split("//")[0]
        for x in ENTRY_SGPR_RE.finditer(code):
            if x.group(1):
                m |= 1 << (int(x.group(1)) - 10)
            else:
                for r in range(int(x.group(2)), int(x.group(3)) + 1):
                    m |= 1 << (r - 10)
    return m


def jit_templates():
    """Glue the host's copy-and-patch compiler stitches between copied handler bodies.  Never
    executed in place.  Literals 0x5eed5eed and branch offsets are patched per use."""
    L = [".p2align 2", "ebpf_jit_templates:"]
    for r in range(10, 16):
        L += [".Ljt_mov_s%d:" % r, "s_mov_b32 s%d, 0x5eed5eed" % r]
    # conditional tail, short form: no lane taken -> fall through (the common uniform case costs
    # two scalar instructions); all taken -> branch; mixed -> park the taken lanes at the taken
    # block (v41 = its code offset), continue with the rest
    L += [".Ljt_cs:",
          "s_and_b64 %s, vcc, exec" % sp(S_MASK),
          "s_cbranch_scc0 .Ljt_cs_end",
          "s_cmp_eq_u64 %s, exec" % sp(S_MASK),
          ".Ljt_cs_br:",
          "s_cbranch_scc1 .Ljt_cs_br",
          "s_mov_b64 %s, exec" % sp(S_SAVE),
          "s_mov_b64 exec, %s" % sp(S_MASK),
          ".Ljt_cs_vt:",
          "v_mov_b32 v%d, 0x5eed5eed" % V_T,
          "s_andn2_b64 exec, %s, %s" % (sp(S_SAVE), sp(S_MASK)),
          ".Ljt_cs_end:"]
    # long form (taken block beyond a 16-bit branch)
    L += [".Ljt_cl:",
          "s_and_b64 %s, vcc, exec" % sp(S_MASK),
          "s_cbranch_scc0 .Ljt_cl_end",
          "s_cmp_eq_u64 %s, exec" % sp(S_MASK),
          "s_cbranch_scc0 .Ljt_cl_skip",
          ".Ljt_cl_lit:",
          "s_add_u32 %s, %s, 0x5eed5eed" % (s(S_JUNK), s(S_CB)),
          "s_addc_u32 %s, %s, 0" % (s(S_JUNK + 1), s(S_CB + 1)),
          "s_setpc_b64 %s" % sp(S_JUNK),
          ".Ljt_cl_skip:",
          "s_mov_b64 %s, exec" % sp(S_SAVE),
          "s_mov_b64 exec, %s" % sp(S_MASK),
          ".Ljt_cl_vt:",
          "v_mov_b32 v%d, 0x5eed5eed" % V_T,
          "s_andn2_b64 exec, %s, %s" % (sp(S_SAVE), sp(S_MASK)),
          ".Ljt_cl_end:"]
    L += [".Ljt_wait:", "s_waitcnt lgkmcnt(0)",
          ".Ljt_br:", "s_branch .Ljt_br",
          ".Ljt_jl:",
          "s_add_u32 %s, %s, 0x5eed5eed" % (s(S_JUNK), s(S_CB)),
          "s_addc_u32 %s, %s, 0" % (s(S_JUNK + 1), s(S_CB + 1)),
          "s_setpc_b64 %s" % sp(S_JUNK),
          ".Ljt_jl_end:"]
    L += [".p2align 2", "ebpf_jit_tmpl:"] + ["  .long %s-.Lcb" % n for n in JT_LABELS]
    L += ["  .long %d" % JIT_AREA_BYTES]
    return L
