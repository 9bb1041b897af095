"""Handler bodies: the lines of each (family, dst, src) specialisation, which the interpreter
dispatches to and the host compiler copies into compiled programs.  handler_body() maps a family
name to its body.  Only the packet loads that read the staged packet registers depend on the
image."""
from gen_emit import *  # noqa: F401,F403


def h_alu64r(op, d, sr):
    D0, D1, S0, S1 = lo(d), hi(d), lo(sr), hi(sr)
    t = H
    if op == "ADD":
        return ["v_lshl_add_u64 %s, %s, 0, %s" % (pair(d), pair(sr), pair(d))]
    if op == "SUB":
        return ["v_sub_co_u32 %s, vcc, %s, %s" % (D0, D0, S0),
                "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (D1, D1, S1)]
    if op == "MUL":
        return ["v_mad_u64_u32 %s, %s, %s, %s, 0" % (vp(t[0]), sp(S_JUNK), D0, S0),
                "v_mul_lo_u32 %s, %s, %s" % (v(t[2]), D0, S1),
                "v_mul_lo_u32 %s, %s, %s" % (v(t[3]), D1, S0),
                "v_add3_u32 %s, %s, %s, %s" % (D1, v(t[1]), v(t[2]), v(t[3])),
                "v_mov_b32 %s, %s" % (D0, v(t[0]))]
    if op in ("OR", "AND", "XOR"):
        m = {"OR": "v_or_b32", "AND": "v_and_b32", "XOR": "v_xor_b32"}[op]
        return ["%s %s, %s, %s" % (m, D0, D0, S0), "%s %s, %s, %s" % (m, D1, D1, S1)]
    if op == "LSH":
        return ["v_lshlrev_b64 %s, %s, %s" % (pair(d), S0, pair(d))]
    if op == "RSH":
        return ["v_lshrrev_b64 %s, %s, %s" % (pair(d), S0, pair(d))]
    if op in ("DIV", "MOD"):
        return divmod_body(d, sr, None, op, 64)
    raise ValueError(op)


def h_alu32r(op, d, sr):
    D0, D1, S0 = lo(d), hi(d), lo(sr)
    body = {
        "ADD": ["v_add_u32 %s, %s, %s" % (D0, D0, S0)],
        "SUB": ["v_sub_u32 %s, %s, %s" % (D0, D0, S0)],
        "MUL": ["v_mul_lo_u32 %s, %s, %s" % (D0, D0, S0)],
        "OR": ["v_or_b32 %s, %s, %s" % (D0, D0, S0)],
        "AND": ["v_and_b32 %s, %s, %s" % (D0, D0, S0)],
        "XOR": ["v_xor_b32 %s, %s, %s" % (D0, D0, S0)],
        "LSH": ["v_lshlrev_b32 %s, %s, %s" % (D0, S0, D0)],
        "RSH": ["v_lshrrev_b32 %s, %s, %s" % (D0, S0, D0)],
        "MOV": ["v_mov_b32 %s, %s" % (D0, S0)],
    }
    if op in ("DIV", "MOD"):
        return divmod_body(d, sr, None, op, 32)
    return body[op] + ["v_mov_b32 %s, 0" % D1]


def h_alu64i(op, d):
    D0, D1 = lo(d), hi(d)
    t = H
    if op == "ADD":
        return ["v_lshl_add_u64 %s, s[10:11], 0, %s" % (pair(d), pair(d))]
    if op == "MUL":
        return ["v_mad_u64_u32 %s, %s, %s, s10, 0" % (vp(t[0]), sp(S_JUNK), D0),
                "v_mul_lo_u32 %s, %s, s11" % (v(t[2]), D0),
                "v_mul_lo_u32 %s, %s, s10" % (v(t[3]), D1),
                "v_add3_u32 %s, %s, %s, %s" % (D1, v(t[1]), v(t[2]), v(t[3])),
                "v_mov_b32 %s, %s" % (D0, v(t[0]))]
    if op in ("OR", "AND", "XOR"):
        m = {"OR": "v_or_b32", "AND": "v_and_b32", "XOR": "v_xor_b32"}[op]
        return ["%s %s, s10, %s" % (m, D0, D0), "%s %s, s11, %s" % (m, D1, D1)]
    if op == "LSH":
        return ["v_lshlrev_b64 %s, s10, %s" % (pair(d), pair(d))]
    if op == "RSH":
        return ["v_lshrrev_b64 %s, s10, %s" % (pair(d), pair(d))]
    if op == "MOV":
        return ["v_mov_b32 %s, s10" % D0, "v_mov_b32 %s, s11" % D1]
    if op in ("DIV", "MOD"):
        return divmod_body(d, None, True, op, 64)
    raise ValueError(op)


def h_alu32i(op, d):
    D0, D1 = lo(d), hi(d)
    body = {
        "ADD": ["v_add_u32 %s, s10, %s" % (D0, D0)],
        "SUB": ["v_subrev_u32 %s, s10, %s" % (D0, D0)],
        "MUL": ["v_mul_lo_u32 %s, %s, s10" % (D0, D0)],
        "OR": ["v_or_b32 %s, s10, %s" % (D0, D0)],
        "AND": ["v_and_b32 %s, s10, %s" % (D0, D0)],
        "XOR": ["v_xor_b32 %s, s10, %s" % (D0, D0)],
        "LSH": ["v_lshlrev_b32 %s, s10, %s" % (D0, D0)],
        "RSH": ["v_lshrrev_b32 %s, s10, %s" % (D0, D0)],
        "MOV": ["v_mov_b32 %s, s10" % D0],
    }
    if op in ("DIV", "MOD"):
        return divmod_body(d, None, True, op, 32)
    return body[op] + ["v_mov_b32 %s, 0" % D1]


def divmod_body(d, sr, imm, op, bits, zero_ok=False):
    """Operands to R[0:1] (n) and R[2:3] (den); lanes with den == 0 fault DIV_ZERO (the
    reference raises SIGFPE), or with zero_ok (standard eBPF) get 0 (DIV) or n (MOD: the
    divider's remainder for a zero divisor is n); quotient / remainder from the shared
    restoring divider."""
    n0, n1, d0, d1 = v(R[0]), v(R[1]), v(R[2]), v(R[3])
    out = ["v_mov_b32 %s, %s" % (n0, lo(d))]
    out.append("v_mov_b32 %s, %s" % (n1, hi(d) if bits == 64 else "0"))
    if imm:
        out += ["v_mov_b32 %s, s10" % d0, "v_mov_b32 %s, %s" % (d1, "s11" if bits == 64 else "0")]
    else:
        out += ["v_mov_b32 %s, %s" % (d0, lo(sr)),
                "v_mov_b32 %s, %s" % (d1, hi(sr) if bits == 64 else "0")]
    if not imm and not zero_ok:  # (immediate zero divisors are resolved by the translator)
        out += ["v_cmp_eq_u64_e64 %s, %s, 0" % (sp(S_MASK), vp(R[2])),
                "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
                "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
                "s_cbranch_scc1 .Ldz_%s" % "{uid}"]
        out += fault_mask(S_MASK, 2)
        out.append(".Ldz_{uid}:")
    out += call(".Lr_udiv")
    q0, q1, r0, r1 = v(R[4]), v(R[5]), v(R[6]), v(R[7])
    if zero_ok and op == "DIV":
        out += ["v_cmp_eq_u64_e64 vcc, 0, %s" % vp(R[2]),
                "v_cndmask_b32_e64 %s, %s, 0, vcc" % (q0, q0),
                "v_cndmask_b32_e64 %s, %s, 0, vcc" % (q1, q1)]
    src = (q0, q1) if op == "DIV" else (r0, r1)
    out += ["v_mov_b32 %s, %s" % (lo(d), src[0]),
            "v_mov_b32 %s, %s" % (hi(d), src[1] if bits == 64 else "0")]
    return out


CMP = {"JEQ": "eq_u64", "JNE": "ne_u64", "JGT": "gt_u64", "JGE": "ge_u64", "JLT": "lt_u64",
       "JLE": "le_u64", "JSGT": "gt_i64", "JSGE": "ge_i64", "JSLT": "lt_i64", "JSLE": "le_i64"}


def h_cond(c, d, sr, imm):
    srcop = "s[10:11]" if imm else pair(sr)
    out = []
    if c == "JSET":
        if imm:
            out += ["v_and_b32 %s, s10, %s" % (v(H[0]), lo(d)),
                    "v_and_b32 %s, s11, %s" % (v(H[1]), hi(d))]
        else:
            out += ["v_and_b32 %s, %s, %s" % (v(H[0]), lo(d), lo(sr)),
                    "v_and_b32 %s, %s, %s" % (v(H[1]), hi(d), hi(sr))]
        out.append("v_cmp_ne_u64_e64 vcc, %s, 0" % vp(H[0]))
    else:
        out.append("v_cmp_%s_e64 vcc, %s, %s" % (CMP[c], pair(d), srcop))
    # (no lane taken, the usual uniform case, costs two scalar instructions: the AND's SCC says
    # whether any lane takes the branch)
    out += ["@CMPEND",
            "s_and_b64 %s, vcc, exec" % sp(S_MASK),
            "s_cbranch_scc0 .Lnt_{uid}",
            "s_cmp_eq_u64 %s, exec" % sp(S_MASK),
            "s_cbranch_scc1 .Ltk_{uid}",
            ] + goto(".Lr_diverge") + [
            ".Ltk_{uid}:"] + dispatch(13) + [".Lnt_{uid}:"] + dispatch(12)
    return out, True   # (body, has own dispatch)


CMP32 = {"JEQ": "eq_u32", "JNE": "ne_u32", "JGT": "gt_u32", "JGE": "ge_u32", "JLT": "lt_u32",
         "JLE": "le_u32", "JSGT": "gt_i32", "JSGE": "ge_i32", "JSLT": "lt_i32", "JSLE": "le_i32"}


def h_cond32(c, d, sr, imm):
    """JMP32: the compare of the low 32 bits (s10 = u32(imm) for the immediate form)."""
    srcop = "s10" if imm else lo(sr)
    if c == "JSET":
        out = ["v_and_b32 %s, %s, %s" % (v(H[0]), srcop, lo(d)),
               "v_cmp_ne_u32_e64 vcc, 0, %s" % v(H[0])]
    else:
        out = ["v_cmp_%s_e64 vcc, %s, %s" % (CMP32[c], lo(d), srcop)]
    body, own = h_cond(c, d, sr, imm)
    return out + body[body.index("@CMPEND"):], own


def h_std(name, d, sr):
    """Standard-eBPF operations (ebpf_gpu.h EBPF_SEM_STANDARD)."""
    D0, D1 = lo(d), hi(d)
    if name == "MOV64R":
        return ["v_mov_b64 %s, %s" % (pair(d), pair(sr))]
    if name == "NEG64":
        return ["v_sub_co_u32 %s, vcc, 0, %s" % (D0, D0),
                "v_subb_co_u32 %s, vcc, 0, %s, vcc" % (D1, D1)]
    if name == "NEG32":
        return ["v_sub_u32 %s, 0, %s" % (D0, D0), "v_mov_b32 %s, 0" % D1]
    if name == "ARSH64I":
        return ["v_ashrrev_i64 %s, s10, %s" % (pair(d), pair(d))]
    if name == "ARSH64R":
        return ["v_ashrrev_i64 %s, %s, %s" % (pair(d), lo(sr), pair(d))]
    if name == "ARSH32I":
        return ["v_ashrrev_i32 %s, s10, %s" % (D0, D0), "v_mov_b32 %s, 0" % D1]
    if name == "ARSH32R":
        return ["v_ashrrev_i32 %s, %s, %s" % (D0, lo(sr), D0), "v_mov_b32 %s, 0" % D1]
    op, bits = name[:3], int(name[3:5])
    return divmod_body(d, sr, None, op, bits, zero_ok=True)


def h_bswap(w, d):
    D0, D1 = lo(d), hi(d)
    if w == 16:
        return ["v_perm_b32 %s, 0, %s, v%d" % (D0, D0, V_SEL),
                "v_lshrrev_b32 %s, 16, %s" % (D0, D0), "v_mov_b32 %s, 0" % D1]
    if w == 32:
        return ["v_perm_b32 %s, 0, %s, v%d" % (D0, D0, V_SEL), "v_mov_b32 %s, 0" % D1]
    return ["v_perm_b32 %s, 0, %s, v%d" % (v(H[0]), D0, V_SEL),
            "v_perm_b32 %s, 0, %s, v%d" % (D0, D1, V_SEL),
            "v_mov_b32 %s, %s" % (D1, v(H[0]))]


def h_ldx_pkt_staged(z, d):
    """s10 = dword index k of the packet byte offset, s11 = byte shift (offset % 4)."""
    t0, t1, t2 = v(H[0]), v(H[1]), v(H[2])
    out = ["s_set_gpr_idx_on s10, gpr_idx(SRC0)",
           "v_mov_b32 %s, v%d" % (t0, PKT0),
           "v_mov_b32 %s, v%d" % (t1, PKT0 + 1)]
    if z == 8:
        out.append("v_mov_b32 %s, v%d" % (t2, PKT0 + 2))
    out.append("s_set_gpr_idx_off")
    D0, D1 = lo(d), hi(d)
    if z == 8:
        out += ["v_alignbyte_b32 %s, %s, %s, s11" % (D0, t1, t0),
                "v_alignbyte_b32 %s, %s, %s, s11" % (D1, t2, t1)]
    elif z == 4:
        out += ["v_alignbyte_b32 %s, %s, %s, s11" % (D0, t1, t0), "v_mov_b32 %s, 0" % D1]
    else:
        out += ["v_alignbyte_b32 %s, %s, %s, s11" % (t0, t1, t0),
                "v_and_b32 %s, %s, %s" % (D0, "0xff" if z == 1 else "0xffff", t0),
                "v_mov_b32 %s, 0" % D1]
    return out


def h_ldx_pkt_const(img, z, d, off):
    """Packet load at a translation-time byte offset from the packet bytes held in v22..v37,
    so 1-2 VALU (bit-field extract / byte align), no indexing.  Staged kernels: every packet is
    exactly 64 bytes.  General kernels (header staging, MODE_HDRSTAGE): lanes whose packet is shorter
    than off + z fault MEM, lanes shorter than 64 bytes (not staged) load from memory."""
    if off + z > 64:
        return []          # never selected: the lowering faults such loads statically
    if not img.staged:
        out = ["v_cmp_gt_u32_e64 %s, %d, v%d" % (sp(S_MASK), off + z, V_LEN),
               "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
               "s_cbranch_scc0 .Lok_{uid}"] + fault_mask(S_MASK, 3) + [".Lok_{uid}:"]
        out += _pkc_extract(z, d, off)
        ld = {1: "global_load_ubyte", 2: "global_load_ushort", 4: "global_load_dword",
              8: "global_load_dwordx2"}[z]
        out += ["v_cmp_gt_u32_e64 %s, 64, v%d" % (sp(S_MASK), V_LEN),
                "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
                "s_cbranch_scc0 .Lst_{uid}",
                "s_mov_b64 %s, exec" % sp(S_JUNK),
                "s_mov_b64 exec, %s" % sp(S_MASK),
                "%s %s, v[%d:%d], off offset:%d" % (ld, pair(d) if z == 8 else lo(d), V_PKT,
                                                    V_PKT + 1, off),
                "s_waitcnt vmcnt(0)"]
        if z < 8:
            out.append("v_mov_b32 %s, 0" % hi(d))
        return out + ["s_mov_b64 exec, %s" % sp(S_JUNK), ".Lst_{uid}:"]
    return _pkc_extract(z, d, off)


def h_ldx_pkt_be(img, w, d, off):
    """LDXH / LDXW at a constant packet offset followed by BE16 / BE32 of the same register
    (ebpf_interpreter.c:327-338 then the byte swap of :164-185): one v_perm_b32 gathers the
    bytes in big-endian order from the staged packet dwords (staged kernels only)."""
    z = w // 8
    if not img.staged or off + z > 64:
        return []          # never selected
    k, sh = off >> 2, off & 3
    lo_ = "v%d" % (PKT0 + k)
    hi_ = "v%d" % (PKT0 + k + 1) if k + 1 < 16 else lo_   # (then no byte of it is selected)
    sel = 0
    for i in range(4):
        sel |= ((sh + z - 1 - i) if i < z else 0x0c) << (8 * i)
    return ["s_mov_b32 %s, 0x%x" % (s(S_JUNK), sel),
            "v_perm_b32 %s, %s, %s, %s" % (lo(d), hi_, lo_, s(S_JUNK)),
            "v_mov_b32 %s, 0" % hi(d)]


def _pkc_extract(z, d, off):
    k, sh = off >> 2, off & 3
    lo_, hi_ = "v%d" % (PKT0 + k), "v%d" % (PKT0 + k + 1) if k + 1 < 16 else None
    D0, D1 = lo(d), hi(d)
    if z == 1:
        return ["v_bfe_u32 %s, %s, %d, 8" % (D0, lo_, 8 * sh), "v_mov_b32 %s, 0" % D1]
    if z == 2:
        if sh <= 2:
            return ["v_bfe_u32 %s, %s, %d, 16" % (D0, lo_, 8 * sh), "v_mov_b32 %s, 0" % D1]
        return ["v_alignbyte_b32 %s, %s, %s, 3" % (D0, hi_, lo_),
                "v_bfe_u32 %s, %s, 0, 16" % (D0, D0), "v_mov_b32 %s, 0" % D1]
    if z == 4:
        if sh == 0:
            return ["v_mov_b32 %s, %s" % (D0, lo_), "v_mov_b32 %s, 0" % D1]
        return ["v_alignbyte_b32 %s, %s, %s, %d" % (D0, hi_, lo_, sh), "v_mov_b32 %s, 0" % D1]
    if sh == 0:
        if (PKT0 + k) % 2 == 0:
            return ["v_mov_b64 %s, v[%d:%d]" % (pair(d), PKT0 + k, PKT0 + k + 1)]
        return ["v_mov_b32 %s, %s" % (D0, lo_), "v_mov_b32 %s, %s" % (D1, hi_)]
    h2 = "v%d" % (PKT0 + k + 2)
    return ["v_alignbyte_b32 %s, %s, %s, %d" % (D0, hi_, lo_, sh),
            "v_alignbyte_b32 %s, %s, %s, %d" % (D1, h2, hi_, sh)]


LOADS = {1: "global_load_ubyte", 2: "global_load_ushort", 4: "global_load_dword",
         8: "global_load_dwordx2"}


def h_ldx_pkt_general(z, d):
    """s[10:11] = packet byte offset (>= 0); per-lane bound check against the packet length."""
    t = H
    out = ["v_mov_b32 %s, s10" % v(t[0]),
           "v_add_u32 %s, %d, %s" % (v(t[0]), z, v(t[0])),
           "v_cmp_gt_u32_e64 %s, %s, %s" % (sp(S_MASK), v(t[0]), v(V_LEN)),
           "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
           "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
           "s_cbranch_scc1 .Lok_{uid}"] + fault_mask(S_MASK, 3) + [".Lok_{uid}:"]
    out.append("v_lshl_add_u64 %s, s[10:11], 0, %s" % (vp(t[0]), vp(V_PKT)))
    if z == 8:
        out.append("%s %s, %s, off" % (LOADS[8], pair(d), vp(t[0])))
    else:
        out += ["%s %s, %s, off" % (LOADS[z], lo(d), vp(t[0])), "v_mov_b32 %s, 0" % hi(d)]
    out.append("s_waitcnt vmcnt(0)")
    return out


DS_R = {1: "ds_read_u8", 2: "ds_read_u16", 4: "ds_read_b32"}
DS_W = {1: "ds_write_b8", 2: "ds_write_b16", 4: "ds_write_b32"}


def h_ldx_stk(z, d):
    """s10 = LDS byte offset from the lane's stack bottom (aligned to min(z, 4))."""
    a = v(H[0])
    out = ["v_add_u32 %s, s10, v%d" % (a, V_STK)]
    if z == 8:
        out.append("ds_read2_b32 %s, %s offset1:1" % (pair(d), a))
    else:
        out += ["%s %s, %s" % (DS_R[z], lo(d), a), "v_mov_b32 %s, 0" % hi(d)]
    return out   # the dispatch's lgkmcnt(0) waits for the LDS read


def h_stx_stk(z, sr):
    a = v(H[0])
    out = ["v_add_u32 %s, s10, v%d" % (a, V_STK)]
    if z == 8:
        out.append("ds_write2_b32 %s, %s, %s offset1:1" % (a, lo(sr), hi(sr)))
    else:
        out.append("%s %s, %s" % (DS_W[z], a, lo(sr)))
    return out


def h_st_stk(z):
    """s[10:11] = value (sign-extended imm), s14 = LDS offset."""
    a, x0, x1 = v(H[0]), v(H[1]), v(H[2])
    out = ["v_add_u32 %s, s14, v%d" % (a, V_STK), "v_mov_b32 %s, s10" % x0]
    if z == 8:
        out += ["v_mov_b32 %s, s11" % x1, "ds_write2_b32 %s, %s, %s offset1:1" % (a, x0, x1)]
    else:
        out.append("%s %s, %s" % (DS_W[z], a, x0))
    return out


FLAT_LOAD = {1: "flat_load_ubyte", 2: "flat_load_ushort", 4: "flat_load_dword", 8: "flat_load_dwordx2"}


def gather(a0, acc, tmp, z, tag=None):
    """acc (two VGPRs) = the z bytes at the flat address v[a0:a0+1], little-endian.  z: an int
    (tmp a list of z VGPRs: when every running lane's address is z-aligned, one flat load of z
    bytes; else z byte loads issued together, one wait), or None for S_T0 bytes (4 or 8 at run
    time, byte by byte; tmp one VGPR, `tag` names the label)."""
    if z is not None:
        t = tmp
        out = []
        if z > 1:
            out += ["v_and_b32 %s, %d, %s" % (v(t[0]), z - 1, v(a0)),
                    "v_cmp_eq_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(t[0])),
                    "s_and_b64 %s, %s, exec" % (sp(S_JUNK), sp(S_JUNK)),
                    "s_cmp_eq_u64 %s, exec" % sp(S_JUNK),
                    "s_cbranch_scc0 .Lg_una_%s" % tag]
        out += ["%s %s, %s" % (FLAT_LOAD[z], vp(acc[0]) if z == 8 else v(acc[0]), vp(a0)),
                "s_waitcnt vmcnt(0) lgkmcnt(0)"]
        if z < 8:
            out.append("v_mov_b32 %s, 0" % v(acc[1]))
        if z == 1:
            return out
        out += ["s_branch .Lg_done_%s" % tag, ".Lg_una_%s:" % tag]
        out += ["flat_load_ubyte %s, %s offset:%d" % (v(t[b]), vp(a0), b) for b in range(z)]
        out += ["s_waitcnt vmcnt(0) lgkmcnt(0)",
                "v_mov_b32 %s, %s" % (v(acc[0]), v(t[0])), "v_mov_b32 %s, 0" % v(acc[1])]
        for b in range(1, z):
            tgt = v(acc[b // 4])
            out.append("v_lshl_or_b32 %s, %s, %d, %s" % (tgt, v(t[b]), 8 * (b % 4), tgt))
        out.append(".Lg_done_%s:" % tag)
        return out
    out = ["v_mov_b32 %s, 0" % v(acc[0]), "v_mov_b32 %s, 0" % v(acc[1])]
    for b in range(z or 8):
        if z is None and b == 4:
            out += ["s_cmp_le_u32 %s, %d" % (s(S_T0), b), "s_cbranch_scc1 .Lg_done_%s" % tag]
        out.append("flat_load_ubyte %s, %s offset:%d" % (v(tmp), vp(a0), b))
        out.append("s_waitcnt vmcnt(0) lgkmcnt(0)")
        tgt = v(acc[b // 4])
        out.append("v_lshl_or_b32 %s, %s, %d, %s" % (tgt, v(tmp), 8 * (b % 4), tgt))
    if z is None:
        out.append(".Lg_done_%s:" % tag)
    return out


def h_ldx_gen(z, d, sr):
    """Generic load: address = r_src + sext(off) (s[10:11]); region check, then byte-wise
    flat loads (packet/map in global memory, stack in LDS via the shared aperture); a program
    that reads its own stores into map values (dp_launch.vflags VF_OVERLAY) then takes the bytes
    it stored from its overlay (.Lr_ovlfix)."""
    a0 = H[0]
    out = ["v_lshl_add_u64 %s, s[10:11], 0, %s" % (vp(a0), pair(sr)),
           "s_mov_b32 %s, %d" % (s(S_T0), z), "s_mov_b32 %s, 0" % s(S_T1)] + call(".Lr_check")
    out += gather(a0, (H[2], H[3]), [H[4]] + R[:7], z, "{uid}")
    out += vflags_test(VF_OVERLAY, ".Lnovl_{uid}") + call(".Lr_ovlfix") + [".Lnovl_{uid}:"]
    out += ["v_mov_b32 %s, %s" % (lo(d), v(H[2])), "v_mov_b32 %s, %s" % (hi(d), v(H[3]))]
    return out


def h_ldx_pktv(img, z, d, sr):
    """LDXPKTV: address = r_src + sext(off); when every running lane's address holds z bytes of
    its own packet ([V_PKT, V_PKT + V_LEN)), one flat load (or z byte loads when unaligned) —
    in the staged kernel's keep mode from the LDS packet buffer instead; otherwise the generic
    load (region check, faults) for all of them."""
    a0 = H[0]
    out = ["v_lshl_add_u64 %s, s[10:11], 0, %s" % (vp(a0), pair(sr)),
           "v_sub_co_u32 %s, vcc, %s, v%d" % (v(H[2]), v(a0), V_PKT),
           "v_subb_co_u32 %s, vcc, %s, v%d, vcc" % (v(H[3]), v(a0 + 1), V_PKT + 1)]
    if img.staged:   # (every packet is 64 bytes: one unsigned 64-bit compare of the offset)
        out += ["v_cmp_ge_u64_e64 %s, %d, v[%d:%d]" % (sp(S_JUNK), 64 - z, H[2], H[3])]
    else:
        out += ["v_cmp_eq_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(H[3])),
                "v_subrev_u32 %s, %d, v%d" % (v(H[4]), z, V_LEN),
                "v_cmp_le_u32_e64 vcc, %s, %s" % (v(H[2]), v(H[4])),
                "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
                "v_cmp_le_u32_e64 vcc, %d, v%d" % (z, V_LEN),
                "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK))]
    out += ["s_and_b64 %s, %s, exec" % (sp(S_JUNK), sp(S_JUNK)),
            "s_cmp_eq_u64 %s, exec" % sp(S_JUNK),
            "s_cbranch_scc0 .Lpv_gen_{uid}"]
    A, B = v(H[4]), v(H[5])
    if img.staged:
        # keep mode (MODE_KEEP): the group's packets stay in the wave's LDS packet buffer while
        # the program runs, transposed (lds_pkt_dwords), so read them there
        out += [mode_test(MODE_KEEP),
                "s_cbranch_scc0 .Lpv_flat_{uid}",
                "v_lshrrev_b32 %s, 2, v%d" % (A, V_L16),
                "v_add_u32 %s, %s, %s" % (A, s(S_PKTLDS), A)]
    else:
        # general kernels with the headers kept in LDS (MODE_KEEP, every lane's first 64 bytes,
        # transposed, when its packet is at least that long): when every running lane's bytes
        # lie in its first 64 and its packet has them staged, read them there
        out += [mode_test(MODE_KEEP),
                "s_cbranch_scc0 .Lpv_flat_{uid}",
                "v_cmp_ge_u32_e64 vcc, %d, %s" % (64 - z, v(H[2])),
                "s_and_b64 %s, vcc, exec" % sp(S_MASK),
                "v_cmp_le_u32_e64 vcc, 64, v%d" % V_LEN,
                "s_and_b64 %s, %s, vcc" % (sp(S_MASK), sp(S_MASK)),
                "s_cmp_eq_u64 %s, exec" % sp(S_MASK),
                "s_cbranch_scc0 .Lpv_flat_{uid}",
                "v_mbcnt_lo_u32_b32 %s, -1, 0" % A,
                "v_mbcnt_hi_u32_b32 %s, -1, %s" % (A, A),
                "v_lshl_add_u32 %s, %s, 2, %s" % (A, A, s(S_PKTLDS))]
    out += lds_pkt_read(z, d, A, B, v(H[2]))
    out += ["s_branch .Lpv_done_{uid}", ".Lpv_flat_{uid}:"]
    out += gather(a0, (H[2], H[3]), [H[4]] + R[:7], z, "{uid}f")
    out += ["v_mov_b32 %s, %s" % (lo(d), v(H[2])), "v_mov_b32 %s, %s" % (hi(d), v(H[3])),
            "s_branch .Lpv_done_{uid}",
            ".Lpv_gen_{uid}:"]
    out += h_ldx_gen(z, d, sr)
    out.append(".Lpv_done_{uid}:")
    return out


def h_ldx_map(z, d, sr):
    """Load from an LDS-resident array-map value: r_src is (by pointer provenance) a lookup
    result of one map, i.e. NULL or dev_base + k*value_size + c.  s[10:11] = dev_base - off,
    s13 = map bytes - z (last valid byte offset), s14 = the map's LDS byte address.  Lanes whose
    address leaves the map (NULL, out of range) fault MEM; the rest read the LDS copy (aligned
    by construction: the host only selects this family when the access is)."""
    u0, u1, t = v(H[0]), v(H[1]), v(H[2])
    out = ["v_sub_co_u32 %s, vcc, %s, s10" % (u0, lo(sr)),
           "v_mov_b32 %s, s11" % t,
           "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (u1, hi(sr), t),
           "v_cmp_ge_u32_e64 %s, s13, %s" % (sp(S_MASK), u0),
           "v_cmp_eq_u32_e64 vcc, 0, %s" % u1,
           "s_and_b64 %s, %s, vcc" % (sp(S_MASK), sp(S_MASK)),
           "s_andn2_b64 %s, exec, %s" % (sp(S_MASK), sp(S_MASK)),
           "s_cbranch_scc0 .Lok_{uid}"] + fault_mask(S_MASK, 3) + [".Lok_{uid}:",
           "v_add_u32 %s, s14, %s" % (u0, u0)]
    if z == 8:
        out.append("ds_read2_b32 %s, %s offset1:1" % (pair(d), u0))
    else:
        out += ["%s %s, %s" % (DS_R[z], lo(d), u0), "v_mov_b32 %s, 0" % hi(d)]
    return out


def h_ldx_hv(z, d, sr):
    """Load from a hashtable value: r_src is (by pointer provenance) a lookup result of a
    hashtable map, i.e. NULL or a slot's value address, and the translator proved
    [off, off + z) inside the value (s14 = off, naturally aligned).  NULL lanes fault MEM;
    the rest do one global load (no region walk)."""
    ld = {1: "global_load_ubyte", 2: "global_load_ushort", 4: "global_load_dword",
          8: "global_load_dwordx2"}[z]
    a = vp(H[0])
    out = ["v_cmp_eq_u64_e64 %s, 0, %s" % (sp(S_MASK), pair(sr)),
           "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
           "s_cbranch_scc0 .Lok_{uid}"] + fault_mask(S_MASK, 3) + [".Lok_{uid}:",
           "v_add_co_u32 %s, vcc, s14, %s" % (v(H[0]), lo(sr)),
           "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(H[1]), hi(sr))]
    if z == 8:
        out += ["%s %s, %s, off" % (ld, pair(d), a)]
    else:
        out += ["%s %s, %s, off" % (ld, lo(d), a), "v_mov_b32 %s, 0" % hi(d)]
    return out + ["s_waitcnt vmcnt(0)"]


def store_bytes(a0, vals, z):
    out = []
    for b in range(z):
        src = vals[b // 4]
        if b % 4:
            out.append("v_lshrrev_b32 %s, %d, %s" % (v(H[4]), 8 * (b % 4), src))
            out.append("flat_store_byte %s, %s offset:%d" % (vp(a0), v(H[4]), b))
        else:
            out.append("flat_store_byte %s, %s offset:%d" % (vp(a0), src, b))
    out.append("s_waitcnt vmcnt(0) lgkmcnt(0)")
    return out


def h_stx_gen(z, d, sr, kind=1):
    """Generic store: the value in H[2:3] before the region check, which hands stores into map
    values to .Lr_vstore (kind 1: plain, 2: a counter update's STX) and points those lanes'
    address at their scratch; then byte-wise flat stores."""
    a0 = H[0]
    out = ["v_lshl_add_u64 %s, s[10:11], 0, %s" % (vp(a0), pair(d)),
           "v_mov_b32 %s, %s" % (v(H[2]), lo(sr)), "v_mov_b32 %s, %s" % (v(H[3]), hi(sr)),
           "s_mov_b32 %s, %d" % (s(S_T0), z), "s_mov_b32 %s, %d" % (s(S_T1), kind)] + call(".Lr_check")
    return out + store_bytes(a0, [v(H[2]), v(H[3])], z)


def h_xadd(z, p, x, fetch):
    """XADD: *(u32 / u64 *)(r_p + off) += r_x (fetch: r_x = the old value).  The check hands a
    map value's lanes to .Lr_vstore (kind 3), which leaves the old value the packet sees in the
    lane's scratch and points the address there; the read-modify-write below then serves every
    lane alike."""
    a0 = H[0]
    old, nv = (R[0], R[1]), (R[2], R[3])
    out = ["v_lshl_add_u64 %s, s[10:11], 0, %s" % (vp(a0), pair(p)),
           "v_mov_b32 %s, %s" % (v(H[2]), lo(x)), "v_mov_b32 %s, %s" % (v(H[3]), hi(x)),
           "s_mov_b32 %s, %d" % (s(S_T0), z), "s_mov_b32 %s, 3" % s(S_T1)] + call(".Lr_check")
    out += gather(a0, old, [H[4]] + R[4:11], z, "{uid}")
    out += ["v_lshl_add_u64 %s, %s, 0, %s" % (vp(nv[0]), vp(old[0]), vp(H[2]))]
    out += store_bytes(a0, [v(nv[0]), v(nv[1])], z)
    if fetch:
        out += ["v_mov_b32 %s, %s" % (lo(x), v(old[0])),
                "v_mov_b32 %s, %s" % (hi(x), v(old[1]) if z == 8 else "0")]
    return out


def h_st_gen(z, d):
    """s[10:11] = the value (sign-extended imm), s15 = the offset (aux1)."""
    a0 = H[0]
    out = ["s_ashr_i32 %s, s15, 31" % s(S_T3),
           "v_mov_b32 %s, s15" % v(H[2]), "v_mov_b32 %s, %s" % (v(H[3]), s(S_T3)),
           "v_lshl_add_u64 %s, %s, 0, %s" % (vp(a0), vp(H[2]), pair(d)),
           "v_mov_b32 %s, s10" % v(H[2]), "v_mov_b32 %s, s11" % v(H[3]),
           "s_mov_b32 %s, %d" % (s(S_T0), z), "s_mov_b32 %s, 1" % s(S_T1)] + call(".Lr_check")
    return out + store_bytes(a0, [v(H[2]), v(H[3])], z)


def h_lookup_stk():
    """r0 = lookup(map, *(u32*)(r10 + c)) with the map resolved at translation time:
    s[10:11] = device base of the map mirror, s13 = max_entries, s14 = key LDS offset,
    s15 = value_size (ebpf_map.c:77-84 -> ebpf_map_array.c:115-124)."""
    k, vs = v(H[0]), v(H[1])
    return ["v_add_u32 %s, s14, v%d" % (k, V_STK),
            "ds_read_b32 %s, %s" % (k, k),
            "v_mov_b32 %s, s15" % vs,
            "s_waitcnt lgkmcnt(0)",
            "v_cmp_gt_u32_e64 vcc, s13, %s" % k,
            "v_mad_u64_u32 %s, %s, %s, %s, s[10:11]" % (vp(H[2]), sp(S_JUNK), k, vs),
            "v_cndmask_b32 v0, 0, %s, vcc" % v(H[2]),
            "v_cndmask_b32 v1, 0, %s, vcc" % v(H[3])]


def handler_body(img, name, d, sr):
    """Returns (lines, has_dispatch)."""
    if name.startswith("A64R_"):
        return h_alu64r(name[5:], d, sr), False
    if name.startswith("A32R_"):
        return h_alu32r(name[5:], d, sr), False
    if name.startswith("A64I_"):
        return h_alu64i(name[5:], d), False
    if name.startswith("A32I_"):
        return h_alu32i(name[5:], d), False
    if name.startswith("BSWAP"):
        return h_bswap(int(name[5:]), d), False
    for c in CONDS:
        if name == c + "_R":
            return h_cond(c, d, sr, False)
        if name == c + "_I":
            return h_cond(c, d, None, True)
    if name.startswith("LDXPKC"):
        return h_ldx_pkt_const(img, int(name[6:]), d, sr), False
    if name.startswith("LDXPKBE"):
        return h_ldx_pkt_be(img, int(name[7:]), d, sr), False
    if name.startswith("LDXPKTG"):
        return h_ldx_pkt_general(int(name[7:]), d), False
    if name.startswith("LDXSTK"):
        return h_ldx_stk(int(name[6:]), d), False
    if name.startswith("STXSTK"):
        return h_stx_stk(int(name[6:]), d), False
    if name.startswith("STSTK"):
        return h_st_stk(int(name[5:])), False
    if name.startswith("LDXGEN"):
        return h_ldx_gen(int(name[6:]), d, sr), False
    if name.startswith("LDXPKTV"):
        return h_ldx_pktv(img, int(name[7:]), d, sr), False
    if name.startswith("LDXMAP"):
        return h_ldx_map(int(name[6:]), d, sr), False
    if name.startswith("LDXHV"):
        return h_ldx_hv(int(name[5:]), d, sr), False
    if name in ("MOV64R", "NEG64", "NEG32", "ARSH64I", "ARSH64R", "ARSH32I", "ARSH32R",
                "DIV64Z", "MOD64Z", "DIV32Z", "MOD32Z"):
        return h_std(name, d, sr), False
    if name.startswith("J32"):
        c = "J" + name[3:-2]
        return h_cond32(c, d, sr, name.endswith("_I"))
    if name.startswith("STXGEN"):
        return h_stx_gen(int(name[6:]), d, sr), False
    if name.startswith("CNTST"):
        return h_stx_gen(int(name[5:]), d, sr, kind=2), False
    if name.startswith("XADDF"):
        return h_xadd(int(name[5:]), sr, d, True), False
    if name.startswith("XADD"):
        return h_xadd(int(name[4:]), d, sr, False), False
    if name.startswith("STGEN"):
        return h_st_gen(int(name[5:]), d), False
    if name == "EXIT":
        return goto(".Lr_exit"), True
    if name == "FAULT":
        return ["s_mov_b32 %s, s14" % s(S_CODE), "s_mov_b64 %s, exec" % sp(S_MASK)] + \
            call(".Lr_fault") + ["s_endpgm"], True
    if name == "NOP":
        return [], False
    if name == "LOOKUPSTK":
        return h_lookup_stk(), False
    if name == "LOOKUPGEN":
        return goto(".Lr_lookup"), True
    if name == "HLOOKUP":
        return call(".Lr_hlookup"), False
    if name == "UPDATE":
        return call(".Lr_update"), False
    if name == "HDELETE":
        return call(".Lr_hdelete"), False
    if name.startswith("CNTAI"):
        z = int(name[5:])
        out = ["v_mov_b32 %s, s14" % v(H[2]), "v_mov_b32 %s, 0" % v(H[3]),
               "v_lshl_add_u64 %s, %s, 0, %s" % (vp(H[0]), vp(H[2]), pair(d)),
               "v_mov_b32 %s, s10" % v(H[2]), "v_mov_b32 %s, s11" % v(H[3])]
        if z == 8:
            return out + ["global_atomic_add_x2 %s, %s, off" % (vp(H[0]), vp(H[2]))], False
        return out + ["global_atomic_add %s, %s, off" % (vp(H[0]), v(H[2]))], False
    if name.startswith("CNTAL"):
        z = int(name[5:])
        out = ["v_subrev_u32 %s, s15, %s" % (v(H[0]), lo(d)),
               "v_add_u32 %s, s14, %s" % (v(H[0]), v(H[0])),
               "v_mov_b32 %s, s10" % v(H[2]), "v_mov_b32 %s, s11" % v(H[3])]
        if z == 8:
            return out + ["ds_add_u64 %s, %s" % (v(H[0]), vp(H[2]))], False
        return out + ["ds_add_u32 %s, %s" % (v(H[0]), v(H[2]))], False
    if name == "OVLINIT":   # the overlay's count and the logged-write count
        return ["v_mov_b32 %s, 0" % v(H[0]), "v_add_u32 %s, %d, v%d" % (v(H[1]), OVL_COUNT, V_STK),
                "ds_write_b32 %s, %s" % (v(H[1]), v(H[0])),
                "ds_write_b32 %s, %s offset:%d" % (v(H[1]), v(H[0]), WCOUNT - OVL_COUNT)], False
    if name == "LOOPINIT":
        return ["v_mov_b32 %s, 0" % v(H[0]), "ds_write_b32 v%d, %s" % (V_STK, v(H[0]))], False
    if name == "LOOPCNT":
        # count the taken backward jump; lanes past the budget fault LOOP (EBPF_FAULT_LOOP = 8)
        # (one LDS add returning the count before it: past the budget when that is >= budget)
        return ["v_mov_b32 %s, 1" % v(H[0]),
                "ds_add_rtn_u32 %s, v%d, %s" % (v(H[0]), V_STK, v(H[0])),
                "s_waitcnt lgkmcnt(0)",
                "v_cmp_le_u32_e32 vcc, %d, %s" % (LOOP_BUDGET, v(H[0])),
                "s_and_b64 %s, vcc, exec" % sp(S_MASK),
                "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
                "s_cbranch_scc1 .Lok_{uid}"] + fault_mask(S_MASK, 8) + [".Lok_{uid}:"], False
    raise ValueError(name)
