"""Map routines: the hashtable probe (HLOOKUP), map_update_elem / map_delete_elem into the
launch's write log (UPDATE, HDELETE), stores into map values (.Lr_vstore) and the per-lane
overlay that lets a program read its own stores back.  The image matters only where a record
names the lane's packet (lane_pkt_index)."""
from gen_emit import *  # noqa: F401,F403
from gen_handlers import gather
from gen_image import SETTINGS


def _hl_word(dst, off, n):
    """dst = the little-endian key word at byte offset s[off] of the key at H[0:1], bytes at or
    past the key size (S_T0) read as 0 (jhash's zero-padded tail; the device table stores keys
    zero-padded the same way).  Clobbers R[8:10], H[3:5], S_BYTES, vcc."""
    t = [v(R[10]), v(H[3]), v(H[4]), v(H[5])]
    out = ["v_add_co_u32 %s, vcc, %s, %s" % (v(R[8]), s(off), v(H[0])),
           "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(R[9]), v(H[1]))]
    for j in range(4):
        out += ["s_add_u32 %s, %s, %d" % (s(S_BYTES), s(off), j + 1),
                "s_cmp_le_u32 %s, %s" % (s(S_BYTES), s(S_T0)),
                "s_cbranch_scc0 .Lhw_z%s_%d" % (n, j),
                "flat_load_ubyte %s, %s offset:%d" % (t[j], vp(R[8]), j),
                "s_branch .Lhw_d%s_%d" % (n, j),
                ".Lhw_z%s_%d:" % (n, j),
                "v_mov_b32 %s, 0" % t[j],
                ".Lhw_d%s_%d:" % (n, j)]
    out += ["s_waitcnt vmcnt(0) lgkmcnt(0)",
            "v_lshl_or_b32 %s, %s, 8, %s" % (dst, t[1], t[0]),
            "v_lshl_or_b32 %s, %s, 16, %s" % (dst, t[2], dst),
            "v_lshl_or_b32 %s, %s, 24, %s" % (dst, t[3], dst)]
    return out


def _rot(d, x, k):
    """d = rotl32(x, k)"""
    return ["v_alignbit_b32 %s, %s, %s, %d" % (d, x, x, 32 - k)]


def probe_wait(tag):
    """Wait for the hashtable probe load just issued."""
    return ["s_waitcnt vmcnt(0)"]


def hlookup_routine():
    """HLOOKUP (called): r0 = hashtable_map_lookup_elem(map, r2) for the map whose dp_map record
    is at byte offset s14 of the map table (ebpf_map.c:77-84 -> ebpf_map_hashtable.c:285-301).
    The key (key_size bytes at r2, anywhere a program may read) is region-checked like a load,
    hashed with jhash (ebpf_jhash.h hashlittle, initval 0) and probed linearly in the device
    table (dprog.h dp_map): a lane stops at its key (r0 = the slot's value) or at an empty slot
    (r0 = NULL).  r2 == 0 gives NULL with no access, as the reference's NULL-key check.
    Uses s[8:9] (return address), s[10:11] (entry exec), R[*], H[*]; compiled programs treat
    s10..s11 as clobbered after it."""
    L = [".Lr_hlookup:",
         "s_mov_b64 s[8:9], %s" % sp(S_LINK),
         "s_mov_b64 s[10:11], exec",
         "v_mov_b32 v0, 0", "v_mov_b32 v1, 0",
         "v_cmp_ne_u64_e64 vcc, 0, v[4:5]",
         "s_and_b64 exec, exec, vcc",              # NULL keys: r0 = NULL, nothing read
         "s_cbranch_execz .Lhl_ret"] + hprobe_body("") + [
         ".Lhl_ret:",
         # every lane that entered and did not fault (S_ALIVE lost the faulted ones)
         "s_and_b64 exec, s[10:11], %s" % sp(S_ALIVE),
         "s_setpc_b64 s[8:9]"]
    return L


def hprobe_body(tag):
    """The probe of HLOOKUP (shared with the hashtable path of UPDATE, whose labels carry `tag`):
    for the lanes in exec, v[0:1] = the value address of the key at r2 in the map at s14, or
    NULL; lanes whose key is not readable fault MEM.  Ends at .Lhl_ret<tag> (defined by the
    caller) with exec arbitrary.  Uses R[*], H[*], S_T*, S_OK, S_JUNK, s[64:71]."""
    a, b, c = v(R[0]), v(R[1]), v(R[2])
    t = v(R[3])
    T = tag
    L = ["s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
         "s_waitcnt lgkmcnt(0)",
         "s_and_b32 %s, s71, 0xffff" % s(S_T0),    # key size
         "s_mov_b32 %s, 0" % s(S_T1),
         "v_mov_b32 %s, v4" % v(H[0]), "v_mov_b32 %s, v5" % v(H[1])] + call(".Lr_check") + [
         # exec = the lanes whose key is readable (the others retired with a fault); a
         # structured compiled program may come back with none
         "s_cbranch_execz .Lhl_ret%s" % T,
         "s_mov_b64 %s, exec" % sp(S_MASK),
         "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
         "s_waitcnt lgkmcnt(0)",
         "s_and_b32 %s, s71, 0xffff" % s(S_T0),             # key size
         "s_bfe_u32 %s, s71, 0x50010" % s(S_T1),            # log2 slot stride (5 bits at 16)
         "s_sub_u32 s69, s69, 1",                            # slot mask
         "s_add_u32 s70, %s, 15" % s(S_T0),
         "s_and_b32 s70, s70, -8",                           # value offset 8 + round8(key size)
         # jhash: a = b = c = 0xdeadbeef + length (+ initval 0)
         "s_add_u32 %s, %s, 0xdeadbeef" % (s(S_JUNK), s(S_T0)),
         "v_mov_b32 %s, %s" % (a, s(S_JUNK)), "v_mov_b32 %s, %s" % (b, s(S_JUNK)),
         "v_mov_b32 %s, %s" % (c, s(S_JUNK)),
         "s_mov_b32 %s, 0" % s(S_T2),                       # byte offset
         "s_mov_b32 %s, %s" % (s(S_T3), s(S_T0)),           # bytes left
         ".Lhh_loop%s:" % T,
         "s_cmp_le_u32 %s, 12" % s(S_T3),
         "s_cbranch_scc1 .Lhh_tail%s" % T]
    n = [0]

    def add_words(keep=False):
        out = []
        for i, x in enumerate((a, b, c)):
            out += _hl_word(t, S_T2, "%s%d" % (T, n[0]))
            n[0] += 1
            out += ["v_add_u32 %s, %s, %s" % (x, x, t), "s_add_u32 %s, %s, 4" % (s(S_T2), s(S_T2))]
            if keep and i < 2:   # keys of <= 8 bytes: the tail's first two words are the key
                out.append("v_mov_b32 %s, %s" % (v(H[2]) if i == 0 else v(R[5]), t))
        return out
    L += add_words()
    for (x, y, z, k) in ((a, c, b, 4), (b, a, c, 6), (c, b, a, 8), (a, c, b, 16), (b, a, c, 19),
                         (c, b, a, 4)):
        # x -= y; x ^= rot(y, k); y += z
        L += ["v_sub_u32 %s, %s, %s" % (x, x, y)] + _rot(t, y, k) + \
             ["v_xor_b32 %s, %s, %s" % (x, x, t), "v_add_u32 %s, %s, %s" % (y, y, z)]
    L += ["s_sub_u32 %s, %s, 12" % (s(S_T3), s(S_T3)),
          "s_branch .Lhh_loop%s" % T,
          ".Lhh_tail%s:" % T]
    L += add_words(keep=True)
    for (x, y, k) in ((c, b, 14), (a, c, 11), (b, a, 25), (c, b, 16), (a, c, 4), (b, a, 14), (c, b, 24)):
        # x ^= y; x -= rot(y, k)
        L += ["v_xor_b32 %s, %s, %s" % (x, x, y)] + _rot(t, y, k) + ["v_sub_u32 %s, %s, %s" % (x, x, t)]
    # probe: slot i = hash & mask, then i + 1, ... until the key or an empty slot
    idx, sa, hd = v(R[3]), vp(R[4]), vp(R[6])
    # keys of up to 8 bytes: one 16-byte load per slot (used, hash, key) compared in registers
    k0, k1 = v(H[2]), v(H[3])
    L += ["s_cmp_le_u32 %s, 8" % s(S_T0),
          "s_cbranch_scc0 .Lhp_general%s" % T,
          "v_mov_b32 %s, %s" % (k1, v(R[5])),
          "v_and_b32 %s, s69, %s" % (idx, c),
          "s_mov_b64 %s, exec" % sp(S_OK),
          ".Lhq_loop%s:" % T,
          "v_mov_b32 %s, %s" % (v(R[4]), idx),
          "v_mov_b32 %s, 0" % v(R[5]),
          "v_lshlrev_b64 %s, %s, %s" % (sa, s(S_T1), sa),
          "v_lshl_add_u64 %s, %s, 0, s[66:67]" % (sa, sa),
          "global_load_dwordx4 v[%d:%d], %s, off%s" % (R[6], R[9], sa, SETTINGS.probe_policy),
          # the slot's first 8 value bytes (value offset 16 for keys of <= 8 bytes), same line:
          # lanes that meet their key here keep them in v[50:51] for the code generator's
          # forwarded value loads (asm_cc.cpp AHF_LDXHV)
          "global_load_dwordx2 %s, %s, off offset:16%s" % (vp(V_HVAL), sa, SETTINGS.probe_policy)] + \
        probe_wait("hq" + T) + [
          "v_cmp_eq_u32_e64 vcc, 0, %s" % v(R[6]),           # empty slot: not found
          "s_andn2_b64 %s, %s, vcc" % (sp(S_OK), sp(S_OK)),
          "v_cmp_eq_u32_e64 %s, %s, %s" % (sp(S_JUNK), v(R[7]), c),
          "v_cmp_eq_u32_e64 vcc, %s, %s" % (v(R[8]), k0),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "v_cmp_eq_u32_e64 vcc, %s, %s" % (v(R[9]), k1),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_and_b64 exec, %s, %s" % (sp(S_JUNK), sp(S_OK)),  # found here
          "v_add_co_u32 v0, vcc, s70, %s" % v(R[4]),
          "v_addc_co_u32 v1, vcc, 0, %s, vcc" % v(R[5]),
          "s_andn2_b64 %s, %s, exec" % (sp(S_OK), sp(S_OK)),
          "s_mov_b64 exec, %s" % sp(S_OK),
          "s_cbranch_execz .Lhl_ret%s" % T,
          "v_add_u32 %s, 1, %s" % (idx, idx),
          "v_and_b32 %s, s69, %s" % (idx, idx),
          "s_branch .Lhq_loop%s" % T,
          ".Lhp_general%s:" % T]
    L += ["v_and_b32 %s, s69, %s" % (idx, c),
          "s_mov_b64 %s, exec" % sp(S_OK),                  # lanes still probing
          ".Lhp_loop%s:" % T,
          "v_mov_b32 %s, %s" % (v(R[4]), idx),
          "v_mov_b32 %s, 0" % v(R[5]),
          "v_lshlrev_b64 %s, %s, %s" % (sa, s(S_T1), sa),
          "v_lshl_add_u64 %s, %s, 0, s[66:67]" % (sa, sa),
          "global_load_dwordx2 %s, %s, off" % (hd, sa)] + probe_wait("hp" + T) + [
          "v_cmp_eq_u32_e64 vcc, 0, %s" % v(R[6]),          # empty slot: not found
          "s_andn2_b64 %s, %s, vcc" % (sp(S_OK), sp(S_OK)),
          "s_and_b64 exec, exec, %s" % sp(S_OK),
          "v_cmp_eq_u32_e64 vcc, %s, %s" % (v(R[7]), c),    # stored hash matches: compare keys
          "s_and_b64 exec, exec, vcc",
          "s_cbranch_execz .Lhp_next%s" % T,
          "s_mov_b32 %s, 0" % s(S_T2),
          ".Lhc_loop%s:" % T,
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_T0)),
          "s_cbranch_scc1 .Lhc_found%s" % T] + _hl_word(v(R[6]), S_T2, T + "99") + [
          "v_add_co_u32 %s, vcc, %s, %s" % (v(R[8]), s(S_T2), v(R[4])),
          "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(R[9]), v(R[5])),
          "global_load_dword %s, %s, off offset:8" % (v(R[7]), vp(R[8])),
          "s_waitcnt vmcnt(0)",
          "v_cmp_ne_u32_e64 vcc, %s, %s" % (v(R[6]), v(R[7])),
          "s_andn2_b64 exec, exec, vcc",
          "s_cbranch_execz .Lhp_next%s" % T,
          "s_add_u32 %s, %s, 4" % (s(S_T2), s(S_T2)),
          "s_branch .Lhc_loop%s" % T,
          ".Lhc_found%s:" % T,
          "v_add_co_u32 v0, vcc, s70, %s" % v(R[4]),
          "v_addc_co_u32 v1, vcc, 0, %s, vcc" % v(R[5]),
          "s_andn2_b64 %s, %s, exec" % (sp(S_OK), sp(S_OK)),
          ".Lhp_next%s:" % T,
          "s_mov_b64 exec, %s" % sp(S_OK),
          "s_cbranch_execz .Lhl_ret%s" % T,
          "v_add_u32 %s, 1, %s" % (idx, idx),
          "v_and_b32 %s, s69, %s" % (idx, idx),
          "s_branch .Lhp_loop%s" % T]
    return L


def log_record(img, T, word, ret):
    """For the lanes in exec: a slot in the launch's write log (one atomic add on its counter per
    wave), R[4:5] = the record's address (log + 64 + slot * stride), its first 16 bytes written:
    {u64 packet index, u32 entry | map << 20, u32 `word`}.  With dp_launch.vflags VF_WCAP
    (DP_VF_WCAP) every lane first counts the write in its stack slice (DP_WCOUNT): a packet's
    write past WRITES_MAX faults it EBPF_FAULT_WRITES instead.  A full log (the host sizes it for
    the program's most writes per path: a library bug) faults MEM, loudly, rather than lose a
    write; exec empty after that branches to `ret`.  Uses R[0:7], S_T0..2, S_MASK, S_JUNK,
    s[64:69]."""
    return [
        "s_load_dword %s, %s" % (s(S_T0), karg("vflags")),
        "s_waitcnt lgkmcnt(0)",
        "s_bitcmp1_b32 %s, %d" % (s(S_T0), VF_WCAP),
        "s_cbranch_scc0 .Lwc_ok%s" % T,
        "v_add_u32 %s, %d, v%d" % (v(R[0]), WCOUNT, V_STK),
        "v_mov_b32 %s, 1" % v(R[1]),
        "ds_add_rtn_u32 %s, %s, %s" % (v(R[2]), v(R[0]), v(R[1])),
        "s_waitcnt lgkmcnt(0)",
        "v_cmp_le_u32_e64 %s, %d, %s" % (sp(S_MASK), WRITES_MAX, v(R[2])),
        "s_and_b64 %s, %s, exec" % (sp(S_MASK), sp(S_MASK)),
        "s_cbranch_scc0 .Lwc_ok%s" % T,
        "s_mov_b32 %s, %d" % (s(S_CODE), FAULT_WRITES)] + call(".Lr_fault") + [
        "s_cbranch_execz %s" % ret,
        ".Lwc_ok%s:" % T,
        # a log slot per lane: one atomic add on the log's counter for the wave
        "s_load_dwordx4 s[64:67], %s" % karg("upd_log", "upd_cap", "upd_stride"),
        "s_load_dwordx2 s[68:69], %s" % karg("pkt_base"),
        "s_waitcnt lgkmcnt(0)",
        "s_bcnt1_i32_b64 %s, exec" % s(S_T0),
        "v_mbcnt_lo_u32_b32 %s, exec_lo, 0" % v(R[0]),
        "v_mbcnt_hi_u32_b32 %s, exec_hi, %s" % (v(R[0]), v(R[0])),
        "s_mov_b64 %s, exec" % sp(S_MASK),
        "s_ff1_i32_b64 %s, exec" % s(S_T1),
        "s_lshl_b64 exec, 1, %s" % s(S_T1),
        "v_mov_b32 %s, %s" % (v(R[1]), s(S_T0)),
        "v_mov_b32 %s, 0" % v(R[2]),
        "global_atomic_add %s, %s, %s, s[64:65] sc0" % (v(R[3]), v(R[2]), v(R[1])),
        "s_waitcnt vmcnt(0)",
        "v_readfirstlane_b32 %s, %s" % (s(S_T2), v(R[3])),
        "s_mov_b64 exec, %s" % sp(S_MASK),
        "v_add_u32 %s, %s, %s" % (v(R[0]), s(S_T2), v(R[0])),      # this lane's slot
        # (the host sizes the log for the program's most updates per path; a full log is a
        # library bug: MEM fault, loudly, rather than a lost write)
        "v_cmp_gt_u32_e64 vcc, s66, %s" % v(R[0]),
        "s_andn2_b64 %s, exec, vcc" % sp(S_MASK),
        "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
        "s_cbranch_scc1 .Lup_room%s" % T,
        "s_mov_b32 %s, 3" % s(S_CODE)] + call(".Lr_fault") + [
        "s_cbranch_execz %s" % ret,
        "s_load_dwordx4 s[64:67], %s" % karg("upd_log", "upd_cap", "upd_stride"),
        "s_load_dwordx2 s[68:69], %s" % karg("pkt_base"),
        "s_waitcnt lgkmcnt(0)",
        ".Lup_room%s:" % T,
        # the record: log + 64 + slot * stride
        "s_add_u32 s64, s64, 64",
        "s_addc_u32 s65, s65, 0",
        "v_mov_b32 %s, s67" % v(R[1]),
        "v_mad_u64_u32 %s, %s, %s, %s, s[64:65]" % (vp(R[4]), sp(S_JUNK), v(R[0]), v(R[1])),
        # packet index (pkt_base = this launch's first packet in its batch)
    ] + lane_pkt_index(img, R[2]) + [
        "v_mov_b32 %s, s69" % v(R[3]),
        "v_add_co_u32 %s, vcc, s68, %s" % (v(R[2]), v(R[2])),
        "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(R[3]), v(R[3])),
        "global_store_dwordx2 %s, %s, off" % (vp(R[4]), vp(R[2])),
        "s_lshr_b32 %s, s14, 5" % s(S_T0),                  # map index
        "s_lshl_b32 %s, %s, 20" % (s(S_T0), s(S_T0)),
        "s_or_b32 %s, %s, s15" % (s(S_T0), s(S_T0)),        # | entry index
        "v_mov_b32 %s, %s" % (v(R[6]), s(S_T0)),
        "v_mov_b32 %s, %s" % (v(R[7]), word),
        "global_store_dwordx2 %s, %s, off offset:8" % (vp(R[4]), vp(R[6]))]


def copy_record(T, src, n, off):
    """Bytes [0, s[n]) at the flat address v[src:src+1] into the record at R[4:5] + s[off]
    (byte by byte: the source may be the stack, the packet or a map value).  Uses S_T0, S_T1,
    H[0], H[1], H[3:5], vcc."""
    return ["s_mov_b32 %s, 0" % s(S_T0),
            ".Lcp%s:" % T,
            "s_cmp_ge_u32 %s, %s" % (s(S_T0), s(n)),
            "s_cbranch_scc1 .Lcpe%s" % T,
            "v_add_co_u32 %s, vcc, %s, v%d" % (v(H[0]), s(S_T0), src),
            "v_addc_co_u32 %s, vcc, 0, v%d, vcc" % (v(H[1]), src + 1),
            "flat_load_ubyte %s, %s" % (v(H[3]), vp(H[0])),
            "s_add_u32 %s, %s, %s" % (s(S_T1), s(S_T0), s(off)),
            "v_add_co_u32 %s, vcc, %s, %s" % (v(H[4]), s(S_T1), v(R[4])),
            "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(H[5]), v(R[5])),
            "s_waitcnt vmcnt(0) lgkmcnt(0)",
            "global_store_byte %s, %s, off" % (vp(H[4]), v(H[3])),
            "s_add_u32 %s, %s, 1" % (s(S_T0), s(S_T0)),
            "s_branch .Lcp%s" % T,
            ".Lcpe%s:" % T]


def ovl_fix(T, acc):
    """The packet's own stores into map values over the z = S_T0 bytes just read at H[0:1] into
    acc (two VGPRs): every byte whose 8-byte word has an overlay entry (dprog.h DP_OVL_*) comes
    from that entry.  For the lanes in exec; clobbers R[6:10], H[4], S_T3, S_BYTES, S_MASK, vcc."""
    E, D0, D1, X, Y, C = R[10], R[6], R[7], R[8], R[9], H[4]   # (pairs start even: gfx950)
    L = ["v_add_u32 %s, %d, v%d" % (v(C), OVL_COUNT, V_STK),
         "ds_read_b32 %s, %s" % (v(C), v(C)),
         "s_mov_b32 %s, 0" % s(S_T3),
         ".Lof%s_loop:" % T,
         "s_waitcnt lgkmcnt(0)",
         "v_cmp_lt_u32_e64 vcc, %s, %s" % (s(S_T3), v(C)),
         "s_and_b64 vcc, vcc, exec",
         "s_cbranch_scc0 .Lof%s_done" % T,
         "s_mov_b64 %s, exec" % sp(S_MASK),
         "s_mov_b64 exec, vcc",
         "s_lshl_b32 %s, %s, 4" % (s(S_BYTES), s(S_T3)),
         "s_add_u32 %s, %s, %d" % (s(S_BYTES), s(S_BYTES), OVL_ENTRIES),
         "v_add_u32 %s, %s, v%d" % (v(E), s(S_BYTES), V_STK),
         "ds_read2_b32 %s, %s offset1:1" % (vp(D0), v(E)),          # the entry's word address
         "v_and_b32 %s, -8, %s" % (v(X), v(H[0])),
         "s_waitcnt lgkmcnt(0)",
         # d = entry word - (address & ~7): 0 or 8 when it is a word of this load
         "v_sub_co_u32 %s, vcc, %s, %s" % (v(D0), v(D0), v(X)),
         "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(D1), v(D1), v(H[1])),
         "v_cmp_ne_u32_e64 vcc, 0, %s" % v(D1),
         "v_cndmask_b32_e64 %s, %s, 16, vcc" % (v(D0), v(D0))]
    for b in range(8):
        if b in (1, 2, 4):
            L += ["s_cmp_le_u32 %s, %d" % (s(S_T0), b), "s_cbranch_scc1 .Lof%s_next" % T]
        k = 8 * (b % 4)
        a = v(acc[b // 4])
        L += ["v_and_b32 %s, 7, %s" % (v(X), v(H[0])),
              "v_add_u32 %s, %d, %s" % (v(X), b, v(X)),               # j = (a & 7) + b
              "v_and_b32 %s, 8, %s" % (v(Y), v(X)),                   # 8 * (j >> 3)
              "v_cmp_eq_u32_e64 vcc, %s, %s" % (v(Y), v(D0)),
              "v_and_b32 %s, 7, %s" % (v(X), v(X)),
              "v_add3_u32 %s, %s, %s, 8" % (v(X), v(X), v(E)),
              "ds_read_u8 %s, %s" % (v(Y), v(X)),
              "s_waitcnt lgkmcnt(0)",
              "v_lshlrev_b32 %s, %d, %s" % (v(Y), k, v(Y)),
              "v_and_b32 %s, 0x%x, %s" % (v(X), 0xffffffff ^ (0xff << k), a),
              "v_or_b32 %s, %s, %s" % (v(X), v(X), v(Y)),
              "v_cndmask_b32 %s, %s, %s, vcc" % (a, a, v(X))]
    L += [".Lof%s_next:" % T,
          "s_mov_b64 exec, %s" % sp(S_MASK),
          "s_add_u32 %s, %s, 1" % (s(S_T3), s(S_T3)),
          "s_branch .Lof%s_loop" % T,
          ".Lof%s_done:" % T]
    return L


def ovl_store(T, nv):
    """Remember, in the lanes' overlays, the z = S_T0 bytes of nv (two VGPRs) stored at H[0:1]:
    for each of the (one or two) 8-byte words the store touches, its entry — made on first use
    with the word's batch-start bytes from the mirror — gets the bytes.  A lane whose overlay is
    full (its entries = dp_launch.vflags from VF_ENTRIES_SHIFT up; only a program with loops that
    reads its counters back fills it, ebpf_gpu.h) when the store needs a new entry gets OVF = 1 and
    stores nothing more.  For the lanes in exec; clobbers R[0:3], R[8:10], H[2:4], S_T3,
    S_BYTES, S_MASK, S_JUNK (saved exec), vcc."""
    W0, W1, CNT, IDX, E, X, Y, OVF = R[0], R[1], R[2], R[3], R[8], H[2], H[3], R[9]
    L = ["s_mov_b64 %s, exec" % sp(S_JUNK),
         "v_mov_b32 %s, 0" % v(OVF),
         "v_add_u32 %s, %d, v%d" % (v(X), OVL_COUNT, V_STK),
         "ds_read_b32 %s, %s" % (v(CNT), v(X)),
         "s_waitcnt lgkmcnt(0)"]
    for wi in (0, 1):
        t = "%s%d" % (T, wi)
        L += ["s_mov_b64 exec, %s" % sp(S_JUNK),
              "v_cmp_eq_u32_e64 vcc, 0, %s" % v(OVF),       # (not the lanes already full)
              "s_and_b64 exec, exec, vcc",
              "s_cbranch_execz .Los%s_end" % t]
        if wi:  # only lanes whose store reaches past its first word
            L += ["v_and_b32 %s, 7, %s" % (v(X), v(H[0])),
                  "v_add_u32 %s, %s, %s" % (v(X), s(S_T0), v(X)),
                  "v_cmp_lt_u32_e64 vcc, 8, %s" % v(X),
                  "s_and_b64 exec, exec, vcc",
                  "s_cbranch_execz .Los%s_end" % t]
        L += ["v_and_b32 %s, -8, %s" % (v(W0), v(H[0])),
              "v_mov_b32 %s, %s" % (v(W1), v(H[1]))]
        if wi:
            L += ["v_add_co_u32 %s, vcc, 8, %s" % (v(W0), v(W0)),
                  "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(W1), v(W1))]
        # the word's entry (IDX), if any
        L += ["v_mov_b32 %s, -1" % v(IDX),
              "s_mov_b32 %s, 0" % s(S_T3),
              ".Los%s_find:" % t,
              "v_cmp_lt_u32_e64 vcc, %s, %s" % (s(S_T3), v(CNT)),
              "s_and_b64 vcc, vcc, exec",
              "s_cbranch_scc0 .Los%s_found" % t,
              "s_mov_b64 %s, exec" % sp(S_MASK),
              "s_mov_b64 exec, vcc",
              "s_lshl_b32 %s, %s, 4" % (s(S_BYTES), s(S_T3)),
              "s_add_u32 %s, %s, %d" % (s(S_BYTES), s(S_BYTES), OVL_ENTRIES),
              "v_add_u32 %s, %s, v%d" % (v(E), s(S_BYTES), V_STK),
              "ds_read2_b32 %s, %s offset1:1" % (vp(X), v(E)),
              "v_mov_b32 %s, %s" % (v(E), s(S_T3)),
              "s_waitcnt lgkmcnt(0)",
              "v_cmp_eq_u64_e64 vcc, %s, %s" % (vp(X), vp(W0)),
              "v_cndmask_b32 %s, %s, %s, vcc" % (v(IDX), v(IDX), v(E)),
              "s_mov_b64 exec, %s" % sp(S_MASK),
              "s_add_u32 %s, %s, 1" % (s(S_T3), s(S_T3)),
              "s_branch .Los%s_find" % t,
              ".Los%s_found:" % t,
              # none: a new entry with the word's batch-start bytes (a full overlay: OVF)
              "v_cmp_eq_u32_e64 vcc, -1, %s" % v(IDX),
              "s_and_saveexec_b64 %s, vcc" % sp(S_MASK),
              "s_cbranch_execz .Los%s_have" % t,
              "s_load_dword %s, %s" % (s(S_T3), karg("vflags")),
              "s_waitcnt lgkmcnt(0)",
              "s_bfe_u32 %s, %s, 0x%x" % (s(S_T3), s(S_T3), VF_ENTRIES_BITS << 16 | VF_ENTRIES_SHIFT),
              "v_cmp_le_u32_e64 vcc, %s, %s" % (s(S_T3), v(CNT)),
              "v_cndmask_b32_e64 %s, %s, 1, vcc" % (v(OVF), v(OVF)),
              "s_andn2_b64 exec, exec, vcc",
              "s_cbranch_execz .Los%s_have" % t,
              "v_mov_b32 %s, %s" % (v(IDX), v(CNT)),
              "v_add_u32 %s, 1, %s" % (v(CNT), v(CNT)),
              "v_lshl_add_u32 %s, %s, 4, v%d" % (v(E), v(IDX), V_STK),
              "v_add_u32 %s, %d, %s" % (v(E), OVL_ENTRIES, v(E)),
              "global_load_dwordx2 %s, %s, off" % (vp(X), vp(W0)),
              "ds_write2_b32 %s, %s, %s offset1:1" % (v(E), v(W0), v(W1)),
              "s_waitcnt vmcnt(0)",
              "ds_write2_b32 %s, %s, %s offset0:2 offset1:3" % (v(E), v(X), v(Y)),
              "v_add_u32 %s, %d, v%d" % (v(X), OVL_COUNT, V_STK),
              "ds_write_b32 %s, %s" % (v(X), v(CNT)),
              ".Los%s_have:" % t,
              "s_or_b64 exec, exec, %s" % sp(S_MASK),
              "v_cmp_eq_u32_e64 vcc, 0, %s" % v(OVF),
              "s_and_b64 exec, exec, vcc",
              "s_cbranch_execz .Los%s_end" % t,
              "v_lshl_add_u32 %s, %s, 4, v%d" % (v(E), v(IDX), V_STK),
              "v_add_u32 %s, %d, %s" % (v(E), OVL_ENTRIES + 8, v(E))]   # the entry's bytes
        # the bytes of the store that fall in this word
        for b in range(8):
            if b in (1, 2, 4):
                L += ["s_cmp_le_u32 %s, %d" % (s(S_T0), b), "s_cbranch_scc1 .Los%s_end" % t]
            L += ["v_and_b32 %s, 7, %s" % (v(X), v(H[0])),
                  "v_add_u32 %s, %d, %s" % (v(X), b, v(X)),          # j = (a & 7) + b
                  "v_and_b32 %s, 8, %s" % (v(Y), v(X)),
                  "v_cmp_eq_u32_e64 vcc, %d, %s" % (8 * wi, v(Y)),
                  "s_and_saveexec_b64 %s, vcc" % sp(S_MASK),
                  "v_and_b32 %s, 7, %s" % (v(X), v(X)),
                  "v_add_u32 %s, %s, %s" % (v(X), v(X), v(E)),
                  "v_lshrrev_b32 %s, %d, %s" % (v(Y), 8 * (b % 4), v(nv[b // 4])),
                  "ds_write_b8 %s, %s" % (v(X), v(Y)),
                  "s_or_b64 exec, exec, %s" % sp(S_MASK)]
        L += [".Los%s_end:" % t]
    L += ["s_mov_b64 exec, %s" % sp(S_JUNK),
          "s_waitcnt lgkmcnt(0)"]
    return L


def vstore_routine(img):
    """VSTORE (called by .Lr_check for the lanes of one map, exec = those lanes): a store into
    that map's values (ebpf_gpu.h "Stores into map values"), S_T1 = kind (1 a plain store of
    H[2:3]; 2 a counter update's STX of H[2:3]; 3 XADD of the addend H[2:3]), S_T0 = bytes,
    H[0:1] = the address, S_T2 = the map's index, s[64:71] its dp_map record.
      * kinds 2 and 3 read the value the packet sees there (L: the mirror's bytes under its
        overlay); kind 3 leaves L in the lane's scratch (the handler's own read-modify-write,
        pointed there, then fetches it); kind 2 adds X - L, kind 3 the addend;
      * the overlay (dp_launch.vflags VF_OVERLAY) remembers the stored value;
      * an addition aligned to its width within the values of a DP_MAP_ATOMIC map goes into its
        delta area (a device atomic); everything else is a record in the batch's log
        {packet, map << 20 | DP_REC_VALUE | add << 16 | size, offset, data, hashtable slot}.
    Returns S_JUNK = the lanes to fault (code S_CODE): the log full, or value stores not provided
    for (vflags VF_VSTORE clear: the translator saw none).  Preserves S_T0..S_T2 and v51 (SPILL);
    clobbers R[*], H[2:4], S_T3, S_BYTES, S_MASK, s[64:71], vcc."""
    L_, NV, OFF, VOFF, SLOT, WORD, ADD = (R[4], R[5]), (R[6], R[7]), R[0], R[2], R[3], R[8], R[10]
    L = [".Lr_vstore:",
         "v_writelane_b32 v%d, %s, 11" % (SPILL, s(S_LINK)),
         "v_writelane_b32 v%d, %s, 12" % (SPILL, s(S_LINK + 1)),
         "s_mov_b64 %s, 0" % sp(S_JUNK),
         "s_load_dword %s, %s" % (s(S_T3), karg("vflags")),
         "s_waitcnt lgkmcnt(0)",
         "s_bitcmp1_b32 %s, %d" % (s(S_T3), VF_VSTORE),
         "s_cbranch_scc1 .Lvs_go",
         "s_mov_b64 %s, exec" % sp(S_JUNK),
         "s_mov_b32 %s, 9" % s(S_CODE),          # EBPF_FAULT_MAP_WRITE
         "s_branch .Lvs_ret",
         ".Lvs_go:",
         "s_cmp_eq_u32 %s, 1" % s(S_T1),
         "s_cbranch_scc1 .Lvs_plain"] + gather(H[0], L_, H[4], None, "vs") + \
        vflags_test(VF_OVERLAY, ".Lvs_noovl") + ovl_fix("vs", L_) + [
         ".Lvs_noovl:",
         "s_cmp_eq_u32 %s, 3" % s(S_T1),
         "s_cbranch_scc0 .Lvs_cnt",
         # XADD: new = L + addend, L to the scratch, delta = the addend
         "v_lshl_add_u64 %s, %s, 0, %s" % (vp(NV[0]), vp(L_[0]), vp(H[2])),
         "v_add_u32 %s, %d, v%d" % (v(R[9]), VST_SCRATCH, V_STK),
         "ds_write2_b32 %s, %s, %s offset1:1" % (v(R[9]), v(L_[0]), v(L_[1])),
         "v_mov_b32 %s, %s" % (v(L_[0]), v(H[2])),
         "v_mov_b32 %s, %s" % (v(L_[1]), v(H[3])),
         "s_branch .Lvs_have",
         ".Lvs_cnt:",                             # a counter's STX: delta = X - L
         "v_mov_b32 %s, %s" % (v(NV[0]), v(H[2])),
         "v_mov_b32 %s, %s" % (v(NV[1]), v(H[3])),
         "v_sub_co_u32 %s, vcc, %s, %s" % (v(L_[0]), v(H[2]), v(L_[0])),
         "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(L_[1]), v(H[3]), v(L_[1])),
         "s_branch .Lvs_have",
         ".Lvs_plain:",
         "v_mov_b32 %s, %s" % (v(NV[0]), v(H[2])),
         "v_mov_b32 %s, %s" % (v(NV[1]), v(H[3])),
         "v_mov_b32 %s, 0" % v(L_[0]),
         "v_mov_b32 %s, 0" % v(L_[1]),
         ".Lvs_have:"] + vflags_test(VF_OVERLAY, ".Lvs_noovl2") + ovl_store("vs", NV) + [
         # (ovl_store kept exec there) lanes whose overlay was full fault WRITES, with nothing
         # of this store done
         "v_cmp_ne_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(R[9])),
         "s_andn2_b64 exec, exec, %s" % sp(S_JUNK),
         "s_mov_b32 %s, %d" % (s(S_CODE), FAULT_WRITES),
         "s_cbranch_execz .Lvs_ret",
         "s_branch .Lvs_ovl_done",
         ".Lvs_noovl2:",
         "s_mov_b64 %s, 0" % sp(S_JUNK),
         ".Lvs_ovl_done:",
         # offsets: OFF = address - the mirror (hashtables: SLOT, VOFF = in the value)
         "v_sub_co_u32 %s, vcc, %s, s66" % (v(OFF), v(H[0])),
         "v_mov_b32 %s, s67" % v(R[9]),
         "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(R[1]), v(H[1]), v(R[9])),
         "v_mov_b32 %s, %s" % (v(VOFF), v(OFF)),
         "v_mov_b32 %s, 0" % v(SLOT),
         "s_bitcmp1_b32 s71, 31",
         "s_cbranch_scc0 .Lvs_arr",
         "s_bfe_u32 %s, s71, 0x50010" % s(S_T3),                    # log2 of the slot stride
         "v_lshrrev_b64 %s, %s, %s" % (vp(R[8]), s(S_T3), vp(OFF)),
         "v_mov_b32 %s, %s" % (v(SLOT), v(R[8])),
         "s_lshl_b32 %s, 1, %s" % (s(S_BYTES), s(S_T3)),
         "s_sub_u32 %s, %s, 1" % (s(S_BYTES), s(S_BYTES)),
         "v_and_b32 %s, %s, %s" % (v(VOFF), s(S_BYTES), v(OFF)),
         "s_and_b32 %s, s71, 0xffff" % s(S_T3),                    # value offset in the slot:
         "s_add_u32 %s, %s, 15" % (s(S_T3), s(S_T3)),               # 8 + round8(key size)
         "s_and_b32 %s, %s, -8" % (s(S_T3), s(S_T3)),
         "v_subrev_u32 %s, %s, %s" % (v(VOFF), s(S_T3), v(VOFF)),
         ".Lvs_arr:",
         # ADD = an addition (kinds 2, 3) aligned to its width within the values
         "s_sub_u32 %s, %s, 1" % (s(S_T3), s(S_T0)),
         "v_and_b32 %s, %s, %s" % (v(ADD), s(S_T3), v(VOFF)),
         "v_cmp_eq_u32_e64 vcc, 0, %s" % v(ADD),
         "s_cmp_eq_u32 %s, 1" % s(S_T1),
         "s_cselect_b64 vcc, 0, vcc",
         "v_cndmask_b32_e64 %s, 0, 1, vcc" % v(ADD),
         # a DP_MAP_ATOMIC map: the additions into its delta area
         "s_bitcmp1_b32 s71, 30",
         "s_cbranch_scc0 .Lvs_rec",
         "s_and_saveexec_b64 %s, vcc" % sp(S_MASK),
         "s_cbranch_execz .Lvs_atom_done",
         # the workgroup's LDS sums (DP_MAP_LDSDELTA: table at s71 & 0xffff)
         "s_bitcmp1_b32 s71, 29",
         "s_cbranch_scc0 .Lvs_atom_g",
         "s_and_b32 %s, s71, 0xffff" % s(S_BYTES),
         "v_add_u32 %s, %s, %s" % (v(R[8]), s(S_BYTES), v(OFF)),
         "s_cmp_eq_u32 %s, 8" % s(S_T0),
         "s_cbranch_scc0 .Lvs_lds4",
         "ds_add_u64 %s, %s" % (v(R[8]), vp(L_[0])),
         "s_branch .Lvs_atom_done",
         ".Lvs_lds4:",
         "ds_add_u32 %s, %s" % (v(R[8]), v(L_[0])),
         "s_branch .Lvs_atom_done",
         ".Lvs_atom_g:",
         "s_mul_i32 %s, s68, s69" % s(S_BYTES),
         "s_add_u32 %s, %s, 63" % (s(S_BYTES), s(S_BYTES)),
         "s_and_b32 %s, %s, -64" % (s(S_BYTES), s(S_BYTES)),      # dprog.h dp_delta_off
         "v_lshl_add_u64 %s, %s, 0, s[66:67]" % (vp(R[8]), vp(OFF)),
         "v_add_co_u32 %s, vcc, %s, %s" % (v(R[8]), s(S_BYTES), v(R[8])),
         "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(R[9]), v(R[9])),
         "s_cmp_eq_u32 %s, 8" % s(S_T0),
         "s_cbranch_scc0 .Lvs_atom4",
         "global_atomic_add_x2 %s, %s, off" % (vp(R[8]), vp(L_[0])),
         "s_branch .Lvs_atom_done",
         ".Lvs_atom4:",
         "global_atomic_add %s, %s, off" % (vp(R[8]), v(L_[0])),
         ".Lvs_atom_done:",
         "s_waitcnt lgkmcnt(0)",
         "s_andn2_b64 exec, %s, exec" % sp(S_MASK),                # the lanes left: records
         ".Lvs_rec:",
         "s_cbranch_execz .Lvs_ret",
         # capped writes (vflags VF_WCAP): every record (the lanes here: a DP_MAP_ATOMIC
         # map's additions went to its delta area above) counts in the lane's slice; the one past
         # WRITES_MAX faults
         "s_load_dword %s, %s" % (s(S_T3), karg("vflags")),
         "s_waitcnt lgkmcnt(0)",
         "s_bitcmp1_b32 %s, %d" % (s(S_T3), VF_WCAP),
         "s_cbranch_scc0 .Lvs_wc_ok",
         "s_mov_b64 %s, exec" % sp(S_MASK),
         "v_add_u32 %s, %d, v%d" % (v(R[1]), WCOUNT, V_STK),
         "v_mov_b32 %s, 1" % v(R[9]),
         "ds_add_rtn_u32 %s, %s, %s" % (v(R[9]), v(R[1]), v(R[9])),
         "s_waitcnt lgkmcnt(0)",
         "v_cmp_le_u32_e64 vcc, %d, %s" % (WRITES_MAX, v(R[9])),
         "s_and_b64 vcc, vcc, exec",              # (vcc = the lanes past the cap)
         "s_mov_b64 exec, %s" % sp(S_MASK),
         "s_andn2_b64 exec, exec, vcc",
         "s_or_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
         "s_mov_b32 %s, %d" % (s(S_CODE), FAULT_WRITES),
         "s_cbranch_execz .Lvs_ret",
         ".Lvs_wc_ok:",
         # the record's word and data (an addition: the addend; else the stored bytes)
         "s_lshl_b32 %s, %s, 20" % (s(S_T3), s(S_T2)),
         "s_or_b32 %s, %s, 0x%x" % (s(S_T3), s(S_T3), 0x80000),
         "s_or_b32 %s, %s, %s" % (s(S_T3), s(S_T3), s(S_T0)),
         "v_mov_b32 %s, %s" % (v(WORD), s(S_T3)),
         "v_cmp_ne_u32_e64 vcc, 0, %s" % v(ADD),
         "v_or_b32 %s, 0x%x, %s" % (v(R[9]), 0x10000, v(WORD)),
         "v_cndmask_b32 %s, %s, %s, vcc" % (v(WORD), v(WORD), v(R[9])),
         "v_cndmask_b32 %s, %s, %s, vcc" % (v(L_[0]), v(NV[0]), v(L_[0])),
         "v_cndmask_b32 %s, %s, %s, vcc" % (v(L_[1]), v(NV[1]), v(L_[1])),
         # a log slot per lane: one atomic add on the log's counter for the wave
         "s_load_dwordx4 s[64:67], %s" % karg("upd_log", "upd_cap", "upd_stride"),
         "s_load_dwordx2 s[68:69], %s" % karg("pkt_base"),
         "s_waitcnt lgkmcnt(0)",
         "s_cmp_eq_u64 s[64:65], 0",
         "s_cbranch_scc0 .Lvs_log",
         "s_or_b64 %s, %s, exec" % (sp(S_JUNK), sp(S_JUNK)),       # (no log: a library bug)
         "s_mov_b32 %s, 3" % s(S_CODE),
         "s_branch .Lvs_ret",
         ".Lvs_log:",
         "s_bcnt1_i32_b64 %s, exec" % s(S_T3),
         "v_mbcnt_lo_u32_b32 %s, exec_lo, 0" % v(OFF),
         "v_mbcnt_hi_u32_b32 %s, exec_hi, %s" % (v(OFF), v(OFF)),
         "s_mov_b64 %s, exec" % sp(S_MASK),
         "s_ff1_i32_b64 %s, exec" % s(S_BYTES),
         "s_lshl_b64 exec, 1, %s" % s(S_BYTES),
         "v_mov_b32 %s, %s" % (v(R[1]), s(S_T3)),
         "v_mov_b32 %s, 0" % v(R[9]),
         "global_atomic_add %s, %s, %s, s[64:65] sc0" % (v(R[6]), v(R[9]), v(R[1])),
         "s_waitcnt vmcnt(0)",
         "v_readfirstlane_b32 %s, %s" % (s(S_T3), v(R[6])),
         "s_mov_b64 exec, %s" % sp(S_MASK),
         "v_add_u32 %s, %s, %s" % (v(OFF), s(S_T3), v(OFF)),      # this lane's slot
         # a full log (the host sizes it for the program's records per path: a library bug)
         # faults MEM, loudly, rather than losing a write
         "v_cmp_gt_u32_e64 vcc, s66, %s" % v(OFF),
         "s_andn2_b64 %s, exec, vcc" % sp(S_MASK),
         "s_or_b64 %s, %s, %s" % (sp(S_JUNK), sp(S_JUNK), sp(S_MASK)),
         "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
         "s_cselect_b32 %s, %s, 3" % (s(S_CODE), s(S_CODE)),
         "s_and_b64 exec, exec, vcc",
         "s_cbranch_execz .Lvs_ret",
         # the record: log + 64 + slot * stride
         "s_add_u32 s64, s64, 64",
         "s_addc_u32 s65, s65, 0",
         "v_mov_b32 %s, s67" % v(R[1]),
         "v_mad_u64_u32 %s, vcc, %s, %s, s[64:65]" % (vp(NV[0]), v(OFF), v(R[1]))] + \
        lane_pkt_index(img, R[0]) + [
         "v_mov_b32 %s, s69" % v(R[1]),
         "v_add_co_u32 %s, vcc, s68, %s" % (v(R[0]), v(R[0])),
         "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(R[1]), v(R[1])),
         "global_store_dwordx2 %s, %s, off" % (vp(NV[0]), vp(R[0])),
         "v_mov_b32 %s, %s" % (v(R[9]), v(VOFF)),
         "global_store_dwordx2 %s, %s, off offset:8" % (vp(NV[0]), vp(WORD)),
         "global_store_dwordx2 %s, %s, off offset:16" % (vp(NV[0]), vp(L_[0])),
         "global_store_dword %s, %s, off offset:24" % (vp(NV[0]), v(SLOT)),
         ".Lvs_ret:",
         "v_readlane_b32 %s, v%d, 11" % (s(S_LINK), SPILL),
         "v_readlane_b32 %s, v%d, 12" % (s(S_LINK + 1), SPILL),
         "s_setpc_b64 %s" % sp(S_LINK)]
    return L


def update_routine(img):
    """UPDATE (called): r0 = map_update_elem(map, r2, r3, r4) for the map whose dp_map record is
    at byte offset s14 of the map table (ebpf_map.c:101-108 -> ebpf_map_array.c:185-211), with
    the device-batch semantics (ebpf_gpu.h "Map writes in a device batch"): the return code is
    the reference's (EINVAL for a NULL key / value or flags > EBPF_EXIST, EEXIST for
    EBPF_NOEXIST, EINVAL for a key >= max_entries, else 0) and the write itself goes to the
    launch's log (dp_launch.upd_log: {u64 packet, u32 entry | map << 20, u32 key, value}),
    applied after the batch in packet order.  Key and value are region-checked like loads.
    A hashtable (.Lup_hash): the return code against the batch-start table (EEXIST / ENOENT by
    the key's presence, ebpf_map_hashtable.c:87-100; EBUSY for a new key when the table was
    full, :371-377) and, for 0, a record {packet, entry | map << 20, flags << 8, key, value}
    replayed on the host after the batch.  Uses s[8:9] (return address), s[10:11] (entry exec),
    R[*], H[*], v63 (restored); compiled programs treat s10..s11 as clobbered after it."""
    key = v(H[2])
    L = [".Lr_update:",
         "s_mov_b64 s[8:9], %s" % sp(S_LINK),
         "s_mov_b64 s[10:11], exec",
         "v_mov_b32 v0, 22", "v_mov_b32 v1, 0",
         # NULL key / value or flags > EBPF_EXIST: EINVAL, nothing read (ebpf_map.c:101-107)
         "v_cmp_ne_u64_e64 %s, 0, v[4:5]" % sp(S_JUNK),
         "v_cmp_ne_u64_e64 vcc, 0, v[6:7]",
         "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
         "v_cmp_ge_u64_e64 vcc, 2, v[8:9]",
         "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
         "s_and_b64 exec, exec, %s" % sp(S_JUNK),
         "s_cbranch_execz .Lup_ret",
         "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
         "s_waitcnt lgkmcnt(0)",
         "s_bitcmp1_b32 s71, 31",
         "s_cbranch_scc1 .Lup_hash",
         # EBPF_NOEXIST: every key of an array exists -> EEXIST (ebpf_map_array.c:188-189)
         "v_and_b32 %s, 1, v8" % v(R[0]),
         "v_cmp_ne_u32_e64 vcc, 0, %s" % v(R[0]),
         "s_mov_b64 %s, exec" % sp(S_MASK),
         "s_and_b64 exec, exec, vcc",
         "v_mov_b32 v0, 17",
         "s_andn2_b64 exec, %s, vcc" % sp(S_MASK),
         "s_cbranch_execz .Lup_ret",
         # the key: 4 bytes at r2, region-checked like a load
         "v_mov_b32 %s, v4" % v(H[0]), "v_mov_b32 %s, v5" % v(H[1]),
         "s_mov_b32 %s, 4" % s(S_T0), "s_mov_b32 %s, 0" % s(S_T1)] + call(".Lr_check") + [
         "s_cbranch_execz .Lup_ret",
         "v_mov_b32 %s, 0" % key]
    for b in range(4):
        L += ["flat_load_ubyte %s, %s offset:%d" % (v(H[3]), vp(H[0]), b),
              "s_waitcnt vmcnt(0) lgkmcnt(0)",
              "v_lshl_or_b32 %s, %s, %d, %s" % (key, v(H[3]), 8 * b, key)]
    L += ["s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "v_cmp_gt_u32_e64 vcc, s69, %s" % key,          # key >= max_entries: EINVAL
          "s_and_b64 exec, exec, vcc",
          "s_cbranch_execz .Lup_ret",
          # the value: value_size bytes at r3, region-checked
          "v_mov_b32 %s, v6" % v(H[0]), "v_mov_b32 %s, v7" % v(H[1]),
          "s_mov_b32 %s, s68" % s(S_T0), "s_mov_b32 %s, 0" % s(S_T1)] + call(".Lr_check") + [
          "s_cbranch_execz .Lup_ret",
          "v_mov_b32 v0, 0"] + log_record(img, "", key, ".Lup_ret") + [
          # the value, byte by byte (r3 may point at the stack, the packet or a map value)
          "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "s_mov_b32 %s, 0" % s(S_T0),
          ".Lup_copy:",
          "s_cmp_ge_u32 %s, s68" % s(S_T0),
          "s_cbranch_scc1 .Lup_ret",
          "v_add_co_u32 %s, vcc, %s, v6" % (v(H[0]), s(S_T0)),
          "v_addc_co_u32 %s, vcc, 0, v7, vcc" % v(H[1]),
          "flat_load_ubyte %s, %s" % (v(H[3]), vp(H[0])),
          "v_add_co_u32 %s, vcc, %s, %s" % (v(H[4]), s(S_T0), v(R[4])),
          "v_addc_co_u32 %s, vcc, 0, %s, vcc" % (v(H[5]), v(R[5])),
          "s_waitcnt vmcnt(0) lgkmcnt(0)",
          "global_store_byte %s, %s, off offset:16" % (vp(H[4]), v(H[3])),
          "s_add_u32 %s, %s, 1" % (s(S_T0), s(S_T0)),
          "s_branch .Lup_copy"]
    # hashtable: the lanes probing are marked in v63 (the probe leaves no mask register alone)
    L += [".Lup_hash:",
          "s_mov_b64 %s, exec" % sp(S_JUNK),
          "s_mov_b64 exec, s[10:11]",
          "v_mov_b32 v%d, 0" % V_SEL,
          "s_mov_b64 exec, %s" % sp(S_JUNK),
          "v_mov_b32 v%d, 1" % V_SEL,
          "v_mov_b32 v0, 0", "v_mov_b32 v1, 0"] + hprobe_body("U") + [
          ".Lhl_retU:",
          "s_and_b64 exec, s[10:11], %s" % sp(S_ALIVE),
          "v_cmp_eq_u32_e64 vcc, 1, v%d" % V_SEL,
          "s_and_b64 exec, exec, vcc",
          "s_cbranch_execz .Lup_hret",
          "v_cmp_ne_u64_e64 %s, 0, v[0:1]" % sp(S_MASK),         # the key is in the table
          "v_mov_b32 v0, 0", "v_mov_b32 v1, 0",
          "v_and_b32 %s, 1, v8" % v(R[0]),                        # EBPF_NOEXIST: EEXIST
          "v_cmp_ne_u32_e64 vcc, 0, %s" % v(R[0]),
          "s_and_b64 vcc, vcc, %s" % sp(S_MASK),
          "v_cndmask_b32_e64 v0, v0, 17, vcc",
          "v_and_b32 %s, 2, v8" % v(R[0]),                        # EBPF_EXIST: ENOENT
          "v_cmp_ne_u32_e64 vcc, 0, %s" % v(R[0]),
          "s_andn2_b64 vcc, vcc, %s" % sp(S_MASK),
          "v_cndmask_b32_e64 v0, v0, 2, vcc",
          # a new key with the table full (the trailer: live entries, max_entries): EBUSY
          "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "s_bfe_u32 %s, s71, 0x50010" % s(S_T1),
          "s_mov_b32 s64, s69",
          "s_mov_b32 s65, 0",
          "s_lshl_b64 s[64:65], s[64:65], %s" % s(S_T1),
          "s_add_u32 s64, s64, s66",
          "s_addc_u32 s65, s65, s67",
          "s_load_dwordx2 s[64:65], s[64:65], 0x0",
          "s_waitcnt lgkmcnt(0)",
          "s_cmp_lt_u32 s64, s65",
          "s_cbranch_scc1 .Lup_hroom",
          "v_cmp_eq_u32_e64 vcc, 0, v0",
          "s_andn2_b64 vcc, vcc, %s" % sp(S_MASK),
          "v_cndmask_b32_e64 v0, v0, 16, vcc",
          ".Lup_hroom:",
          "v_cmp_eq_u32_e64 vcc, 0, v0",
          "s_and_b64 exec, exec, vcc",
          "s_cbranch_execz .Lup_hret",
          # the value is read only by a call that succeeds (ebpf_map_hashtable.c:380-381)
          "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "v_mov_b32 %s, v6" % v(H[0]), "v_mov_b32 %s, v7" % v(H[1]),
          "s_mov_b32 %s, s68" % s(S_T0), "s_mov_b32 %s, 0" % s(S_T1)] + call(".Lr_check") + [
          "s_cbranch_execz .Lup_hret",
          "v_lshlrev_b32 %s, 8, v8" % v(H[2])] + log_record(img, "h", v(H[2]), ".Lup_hret") + [
          "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "s_and_b32 %s, s71, 0xffff" % s(S_T2),                  # key size
          "s_mov_b32 %s, 16" % s(S_T3)] + copy_record("uk", 4, S_T2, S_T3) + [
          "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
          "s_waitcnt lgkmcnt(0)",
          "s_and_b32 %s, s71, 0xffff" % s(S_T3),
          "s_add_u32 %s, %s, 23" % (s(S_T3), s(S_T3)),
          "s_and_b32 %s, %s, -8" % (s(S_T3), s(S_T3)),            # 16 + round8(key size)
          "s_mov_b32 %s, s68" % s(S_T2)] + copy_record("uv", 6, S_T2, S_T3) + [
          ".Lup_hret:",
          "s_mov_b64 exec, s[10:11]",
          "v_mov_b32 v%d, 0x00010203" % V_SEL,
          ".Lup_ret:",
          # every lane that entered and did not fault (S_ALIVE lost the faulted ones)
          "s_and_b64 exec, s[10:11], %s" % sp(S_ALIVE),
          "s_setpc_b64 s[8:9]"]
    return L


def hdelete_routine(img):
    """HDELETE (called): r0 = map_delete_elem(map, r2) on the hashtable whose dp_map record is at
    s14 (ebpf_map.c:126-132 -> ebpf_map_hashtable.c:475-502): EINVAL for a NULL key, else 0 with
    the key region-checked (the reference hashes it) and a record {packet, entry | map << 20, 1,
    key} for the host's replay after the batch."""
    return [".Lr_hdelete:",
            "s_mov_b64 s[8:9], %s" % sp(S_LINK),
            "s_mov_b64 s[10:11], exec",
            "v_mov_b32 v0, 22", "v_mov_b32 v1, 0",
            "v_cmp_ne_u64_e64 vcc, 0, v[4:5]",
            "s_and_b64 exec, exec, vcc",
            "s_cbranch_execz .Lhd_ret",
            "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
            "s_waitcnt lgkmcnt(0)",
            "s_and_b32 %s, s71, 0xffff" % s(S_T0),
            "s_mov_b32 %s, 0" % s(S_T1),
            "v_mov_b32 %s, v4" % v(H[0]), "v_mov_b32 %s, v5" % v(H[1])] + call(".Lr_check") + [
            "s_cbranch_execz .Lhd_ret",
            "v_mov_b32 v0, 0",
            "v_mov_b32 %s, 1" % v(H[2])] + log_record(img, "d", v(H[2]), ".Lhd_ret") + [
            "s_load_dwordx8 s[%d:%d], %s, s14" % (S_REC, S_REC + 7, sp(S_MAPS)),
            "s_waitcnt lgkmcnt(0)",
            "s_and_b32 %s, s71, 0xffff" % s(S_T2),
            "s_mov_b32 %s, 16" % s(S_T3)] + copy_record("dk", 4, S_T2, S_T3) + [
            ".Lhd_ret:",
            "s_and_b64 exec, s[10:11], %s" % sp(S_ALIVE),
            "s_setpc_b64 s[8:9]"]
