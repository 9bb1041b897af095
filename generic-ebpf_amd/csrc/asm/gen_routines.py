"""The routines every kernel of an image shares, reached from handlers and compiled programs
through .Lcb-relative addresses: schedule, diverge, exit, fault, the divider, the region check,
the generic lookup, the map routines (gen_maps.py), the overlay fix and the staged prefetch."""
from gen_emit import *  # noqa: F401,F403
from gen_image import SETTINGS
from gen_maps import hdelete_routine, hlookup_routine, ovl_fix, update_routine, vstore_routine


def routines(img):
    L = []

    # --- schedule: pick the parked group of the first live lane
    L += [".Lr_schedule:",
          "s_mov_b64 exec, %s" % sp(S_ALIVE),
          "s_cbranch_execz .Lgroup_done",
          "s_ff1_i32_b64 %s, exec" % s(S_T0),
          "v_readlane_b32 s6, v%d, %s" % (V_T, s(S_T0)),
          "v_cmp_eq_u32_e64 %s, s6, v%d" % (sp(S_MASK), V_T),
          "s_and_b64 exec, %s, %s" % (sp(S_MASK), sp(S_ALIVE)),
          mode_test(MODE_JIT),
          "s_cbranch_scc1 .Lsched_jit",
          "s_load_dwordx8 s[8:15], s[%d:%d], s6" % (S_PROG, S_PROG + 1),
          "s_waitcnt lgkmcnt(0)",
          "s_setpc_b64 s[8:9]",
          # compiled program: V_T is a code offset from .Lcb
          ".Lsched_jit:",
          "s_add_u32 s8, %s, s6" % s(S_CB),
          "s_addc_u32 s9, %s, 0" % s(S_CB + 1),
          "s_setpc_b64 s[8:9]"]
    # --- diverge: taken lanes (s[mask]) park at the target, the rest continue
    L += [".Lr_diverge:",
          "s_mov_b64 %s, exec" % sp(S_SAVE),
          "s_mov_b64 exec, %s" % sp(S_MASK),
          "v_mov_b32 v%d, s13" % V_T,
          "s_andn2_b64 exec, %s, %s" % (sp(S_SAVE), sp(S_MASK))] + dispatch(12)
    # EXIT: value r0 into V_RET (the group's results are stored together, see group code).
    # (the fault byte of every lane is zeroed when its group starts, and the LDS histogram is
    # kept whether or not the launch asked for one, so an exit does neither check)
    L += [".Lr_exit:"] + ret_slot_write("v0", "v1") + [
          "v_mov_b32 %s, 255" % v(R[8]),
          "v_mov_b32 %s, 0" % v(R[9]),
          "v_cmp_lt_u64_e64 vcc, v[0:1], %s" % vp(R[8]),
          "v_cndmask_b32 %s, %s, v0, vcc" % (v(R[8]), v(R[8])),
          # one LDS atomic per wave when every exiting lane has the same verdict (the usual
          # case); per-lane adds to one address would serialise.  (s_nop: a VALU write, then
          # v_readfirstlane of it, needs one wait state; without it the read can see the
          # previous value and every exit took the per-lane path)
          "s_nop 0",
          "v_readfirstlane_b32 %s, %s" % (s(S_BYTES), v(R[8])),
          "v_cmp_eq_u32_e64 %s, %s, %s" % (sp(S_MASK), s(S_BYTES), v(R[8])),
          "s_cmp_eq_u64 %s, exec" % sp(S_MASK),
          "s_cbranch_scc0 .Lex_lanes",
          # EXIT with r0 known at compile time (compiled programs): v[44:45] = r0 and S_BYTES =
          # its verdict bin are set by the caller, so the verdict needs no per-lane work
          ".Lr_exit_k:",
          ".Lex_uniform:",
          "s_bcnt1_i32_b64 %s, exec" % s(S_CODE),
          "s_lshl_b32 %s, %s, 2" % (s(S_BYTES), s(S_BYTES)),
          "s_mov_b64 %s, exec" % sp(S_SAVE),
          "s_mov_b64 exec, 1",
          "v_mov_b32 %s, %s" % (v(R[8]), s(S_BYTES)),
          "v_mov_b32 %s, %s" % (v(R[9]), s(S_CODE)),
          "ds_add_u32 %s, %s" % (v(R[8]), v(R[9])),
          "s_mov_b64 exec, %s" % sp(S_SAVE),
          "s_branch .Lex_nohist",
          ".Lex_lanes:",
          "v_lshlrev_b32 %s, 2, %s" % (v(R[8]), v(R[8])),
          "v_mov_b32 %s, 1" % v(R[9]),
          "ds_add_u32 %s, %s" % (v(R[8]), v(R[9])),
          ".Lex_nohist:",
          "s_andn2_b64 %s, %s, exec" % (sp(S_ALIVE), sp(S_ALIVE)),
          # structured compiled programs (MODE_STRUCTURED) call the exit and continue themselves
          mode_test(MODE_STRUCTURED),
          "s_cbranch_scc0 .Lex_sched",
          "s_setpc_b64 %s" % sp(S_LINK),
          ".Lex_sched:"] + goto(".Lr_schedule")
    # FAULT: lanes s[mask], code s[S_CODE]; returns via s[link] unless no lane remains
    L += [".Lr_fault:",
          "s_mov_b64 %s, exec" % sp(S_SAVE),
          "s_mov_b64 exec, %s" % sp(S_MASK),
          ] + ret_slot_write("0", "0") + [
          "s_cmp_eq_u64 %s, 0" % sp(S_FAULTS),
          "s_cbranch_scc1 .Lfl_nofault",
          ] + lane_pkt_index(img, R[9]) + [
          "v_mov_b32 %s, %s" % (v(R[8]), s(S_CODE)),
          "global_store_byte %s, %s, %s" % (v(R[9]), v(R[8]), sp(S_FAULTS)),
          ".Lfl_nofault:",
          # a program with map writes: the packet's bit in dp_launch.upd_faulted (its logged
          # writes do not land; map_writes.hip)
          "s_load_dwordx2 %s, %s" % (sp(S_JUNK), karg("upd_faulted")),
          "s_load_dword %s, %s" % (s(S_BYTES), karg("pkt_base")),   # (low word)
          "s_waitcnt lgkmcnt(0)",
          "s_cmp_eq_u64 %s, 0" % sp(S_JUNK),
          "s_cbranch_scc1 .Lfl_nomark"] + lane_pkt_index(img, R[9]) + [
          "v_add_u32 %s, %s, %s" % (v(R[9]), s(S_BYTES), v(R[9])),
          "v_lshrrev_b32 %s, 5, %s" % (v(R[8]), v(R[9])),
          "v_lshlrev_b32 %s, 2, %s" % (v(R[8]), v(R[8])),
          "v_and_b32 %s, 31, %s" % (v(R[10]), v(R[9])),
          "v_lshlrev_b32_e64 %s, %s, 1" % (v(R[10]), v(R[10])),
          "global_atomic_or %s, %s, %s" % (v(R[8]), v(R[10]), sp(S_JUNK)),
          ".Lfl_nomark:",
          # bin 256 (faulted) goes straight to the global histogram: faults are rare, and the
          # LDS histogram then holds exactly 256 bins (1 KB)
          "s_cmp_eq_u64 %s, 0" % sp(S_HIST),
          "s_cbranch_scc1 .Lfl_nohist",
          "s_bcnt1_i32_b64 %s, exec" % s(S_BYTES),
          "s_mov_b64 exec, 1",     # lane 0 only (its operands set below, after the switch)
          "v_mov_b32 %s, %s" % (v(R[8]), s(S_BYTES)),
          "v_mov_b32 %s, 0" % v(R[9]),
          "v_mov_b32 %s, 0" % v(R[10]),
          "global_atomic_add_x2 %s, %s, %s offset:2048" % (v(R[10]), vp(R[8]), sp(S_HIST)),
          ".Lfl_nohist:",
          "s_andn2_b64 %s, %s, %s" % (sp(S_ALIVE), sp(S_ALIVE), sp(S_MASK)),
          "s_andn2_b64 exec, %s, %s" % (sp(S_SAVE), sp(S_MASK)),
          "s_cbranch_execz .Lfl_none",
          "s_setpc_b64 %s" % sp(S_LINK),
          ".Lfl_none:",
          # structured compiled programs continue with no lane (their join restores the rest)
          mode_test(MODE_STRUCTURED),
          "s_cbranch_scc0 .Lfl_sched",
          "s_setpc_b64 %s" % sp(S_LINK),
          ".Lfl_sched:"] + goto(".Lr_schedule")
    # UDIVMOD64: n = R[0:1], d = R[2:3] (non-zero) -> q = R[4:5], r = R[6:7]; clobbers R[8:9]
    n, dd, q, r = vp(R[0]), vp(R[2]), vp(R[4]), vp(R[6])
    L += [".Lr_udiv:",
          "v_mov_b32 %s, 0" % v(R[4]), "v_mov_b32 %s, 0" % v(R[5]),
          "v_mov_b32 %s, 0" % v(R[6]), "v_mov_b32 %s, 0" % v(R[7]),
          "s_mov_b32 %s, 64" % s(S_T2),
          ".Ludiv_loop:",
          "v_lshlrev_b64 %s, 1, %s" % (r, r),
          "v_lshrrev_b32 %s, 31, %s" % (v(R[8]), v(R[1])),
          "v_or_b32 %s, %s, %s" % (v(R[6]), v(R[6]), v(R[8])),
          "v_lshlrev_b64 %s, 1, %s" % (n, n),
          "v_lshlrev_b64 %s, 1, %s" % (q, q),
          "v_cmp_ge_u64_e64 vcc, %s, %s" % (r, dd),
          "v_sub_co_u32 %s, %s, %s, %s" % (v(R[8]), sp(S_JUNK), v(R[6]), v(R[2])),
          "v_subb_co_u32 %s, %s, %s, %s, %s" % (v(R[9]), sp(S_JUNK), v(R[7]), v(R[3]), sp(S_JUNK)),
          "v_cndmask_b32 %s, %s, %s, vcc" % (v(R[6]), v(R[6]), v(R[8])),
          "v_cndmask_b32 %s, %s, %s, vcc" % (v(R[7]), v(R[7]), v(R[9])),
          "v_cndmask_b32 %s, 0, 1, vcc" % v(R[8]),
          "v_or_b32 %s, %s, %s" % (v(R[4]), v(R[4]), v(R[8])),
          "s_sub_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_cmp_lg_u32 %s, 0" % s(S_T2),
          "s_cbranch_scc1 .Ludiv_loop",
          "s_setpc_b64 %s" % sp(S_LINK)]
    # CHECK: address H[0:1], size s[S_T0], write s[S_T1]; lanes outside every region fault
    # (MEM, or MAP_WRITE for a store into a map value); returns with exec = good lanes.
    ok = sp(S_OK)             # accumulated ok mask (the fault routine leaves it alone)
    L += [".Lr_check:",
          "s_mov_b64 %s, 0" % ok,
          # packet: u = a - pkt; u_hi == 0 && len >= size && u_lo <= len - size
          "v_sub_co_u32 %s, vcc, %s, v%d" % (v(R[0]), v(H[0]), V_PKT),
          "v_subb_co_u32 %s, vcc, %s, v%d, vcc" % (v(R[1]), v(H[1]), V_PKT + 1),
          "v_subrev_u32 %s, %s, v%d" % (v(R[2]), s(S_T0), V_LEN),
          "v_cmp_eq_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(R[1])),
          "v_cmp_ge_u32_e64 vcc, v%d, %s" % (V_LEN, s(S_T0)),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "v_cmp_le_u32_e64 vcc, %s, %s" % (v(R[0]), v(R[2])),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_or_b64 %s, %s, %s" % (ok, ok, sp(S_JUNK)),
          # stack: the reference's 512 bytes below r10 (generic accesses force a 516-byte slice,
          # the slice top is r10): u = a - {shared_hi : top - 512}; u_hi == 0 && u_lo <= 512 - size
          "s_sub_u32 %s, %s, 512" % (s(S_T3), s(S_STKSTRIDE)),
          "v_add_u32 %s, %s, v%d" % (v(R[4]), s(S_T3), V_STK),
          "v_sub_co_u32 %s, vcc, %s, %s" % (v(R[0]), v(H[0]), v(R[4])),
          "v_mov_b32 %s, %s" % (v(R[3]), s(S_SHARED + 1)),
          "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(R[1]), v(H[1]), v(R[3])),
          "s_sub_u32 %s, 512, %s" % (s(S_T3), s(S_T0)),
          "v_cmp_eq_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(R[1])),
          "v_cmp_ge_u32_e64 vcc, %s, %s" % (s(S_T3), v(R[0])),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_or_b64 %s, %s, %s" % (ok, ok, sp(S_JUNK)),
          # maps: for m in table (dp_map records of 32 B -> s[64:71])
          "s_mov_b32 %s, 0" % s(S_T2),
          ".Lck_map_loop:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_NMAPS)),
          "s_cbranch_scc1 .Lck_map_done",
          "s_lshl_b32 %s, %s, 5" % (s(S_T3), s(S_T2)),
          "s_load_dwordx8 s[%d:%d], %s, %s" % (S_REC, S_REC + 7, sp(S_MAPS), s(S_T3)),
          "s_waitcnt lgkmcnt(0)",
          "s_bitcmp1_b32 s71, 31",                 # hashtable record: its own rule below
          "s_cbranch_scc1 .Lck_hash",
          # s[66:67] = dev_base, s68 = value_size, s69 = max_entries
          "s_mul_i32 %s, s68, s69" % s(S_BYTES),
          "s_sub_u32 %s, %s, %s" % (s(S_T3), s(S_BYTES), s(S_T0)),
          "v_mov_b32 %s, s67" % v(R[3]),
          "v_sub_co_u32 %s, vcc, %s, s66" % (v(R[0]), v(H[0])),
          "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(R[1]), v(H[1]), v(R[3])),
          "v_cmp_eq_u32_e64 %s, 0, %s" % (sp(S_JUNK), v(R[1])),
          "v_cmp_ge_u32_e64 vcc, %s, %s" % (s(S_T3), v(R[0])),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_cmp_ge_u32 %s, %s" % (s(S_BYTES), s(S_T0)),
          "s_cselect_b64 %s, %s, 0" % (sp(S_JUNK), sp(S_JUNK)),
          ".Lck_map_tail:",
          "s_and_b64 %s, %s, exec" % (sp(S_JUNK), sp(S_JUNK)),
          "s_cmp_eq_u32 %s, 0" % s(S_T1),
          "s_cbranch_scc1 .Lck_map_ok",
          # a store into a map value (ebpf_gpu.h "Stores into map values"): .Lr_vstore for those
          # lanes (SGPRs it clobbers spilled to lanes of v51), whose address then points at the
          # lane's scratch, so the handler's own store leaves the map alone
          "s_cmp_eq_u64 %s, 0" % sp(S_JUNK),
          "s_cbranch_scc1 .Lck_map_next"]
    spill = [(S_LINK, 0), (S_LINK + 1, 1), ("exec_lo", 2), ("exec_hi", 3), (S_T0, 4), (S_T1, 5),
             (S_T2, 6), (S_OK, 7), (S_OK + 1, 8), (S_JUNK, 9), (S_JUNK + 1, 10)]
    L += ["v_writelane_b32 v%d, %s, %d" % (SPILL, r if isinstance(r, str) else s(r), k) for r, k in spill]
    L += ["s_mov_b64 exec, %s" % sp(S_JUNK)] + call(".Lr_vstore") + [
          # the lanes that stored: ok, their address the scratch
          "v_readlane_b32 %s, v%d, 9" % (s(S_MASK), SPILL),
          "v_readlane_b32 %s, v%d, 10" % (s(S_MASK + 1), SPILL),
          "s_andn2_b64 %s, %s, %s" % (sp(S_MASK), sp(S_MASK), sp(S_JUNK)),
          "v_readlane_b32 %s, v%d, 7" % (s(S_OK), SPILL),
          "v_readlane_b32 %s, v%d, 8" % (s(S_OK + 1), SPILL),
          "s_or_b64 %s, %s, %s" % (sp(S_OK), sp(S_OK), sp(S_MASK)),
          "s_mov_b64 exec, %s" % sp(S_MASK),
          "v_add_u32 %s, %d, v%d" % (v(H[0]), VST_SCRATCH, V_STK),
          "v_mov_b32 %s, %s" % (v(H[1]), s(S_SHARED + 1)),
          "v_readlane_b32 %s, v%d, 4" % (s(S_T0), SPILL),
          "v_readlane_b32 %s, v%d, 5" % (s(S_T1), SPILL),
          "v_readlane_b32 %s, v%d, 6" % (s(S_T2), SPILL),
          "v_readlane_b32 exec_lo, v%d, 2" % SPILL,
          "v_readlane_b32 exec_hi, v%d, 3" % SPILL,
          # the lanes .Lr_vstore could not serve fault (S_CODE)
          "s_cmp_eq_u64 %s, 0" % sp(S_JUNK),
          "s_cbranch_scc1 .Lck_vs_ok",
          "s_mov_b64 %s, %s" % (sp(S_MASK), sp(S_JUNK))] + call(".Lr_fault") + [
          ".Lck_vs_ok:",
          "v_readlane_b32 %s, v%d, 0" % (s(S_LINK), SPILL),
          "v_readlane_b32 %s, v%d, 1" % (s(S_LINK + 1), SPILL),
          "s_branch .Lck_map_next",
          ".Lck_map_ok:",
          "s_or_b64 %s, %s, %s" % (ok, ok, sp(S_JUNK)),
          ".Lck_map_next:",
          "s_add_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_branch .Lck_map_loop",
          # hashtable table (dprog.h dp_map): only [value, value + value_size) of a slot:
          # u = a - base < slots << lg, and (u mod stride) - value_off <= value_size - size
          ".Lck_hash:",
          "s_mov_b32 s64, s69",
          "s_mov_b32 s65, 0",
          "s_bfe_u32 s70, s71, 0x50010",
          "s_lshl_b64 s[64:65], s[64:65], s70",
          "v_mov_b32 %s, s67" % v(R[3]),
          "v_sub_co_u32 %s, vcc, %s, s66" % (v(R[0]), v(H[0])),
          "v_subb_co_u32 %s, vcc, %s, %s, vcc" % (v(R[1]), v(H[1]), v(R[3])),
          "v_cmp_gt_u64_e64 %s, s[64:65], %s" % (sp(S_JUNK), vp(R[0])),
          "s_lshl_b32 %s, 1, s70" % s(S_BYTES),
          "s_sub_u32 %s, %s, 1" % (s(S_BYTES), s(S_BYTES)),
          "v_and_b32 %s, %s, %s" % (v(R[2]), s(S_BYTES), v(R[0])),
          "s_and_b32 %s, s71, 0xffff" % s(S_T3),
          "s_add_u32 %s, %s, 15" % (s(S_T3), s(S_T3)),
          "s_and_b32 %s, %s, -8" % (s(S_T3), s(S_T3)),
          "v_subrev_u32 %s, %s, %s" % (v(R[2]), s(S_T3), v(R[2])),
          "s_sub_u32 %s, s68, %s" % (s(S_BYTES), s(S_T0)),
          "s_cselect_b64 %s, 0, %s" % (sp(S_JUNK), sp(S_JUNK)),  # (scc: size > value_size)
          "v_cmp_ge_u32_e64 vcc, %s, %s" % (s(S_BYTES), v(R[2])),
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_branch .Lck_map_tail",
          ".Lck_map_done:",
          "s_andn2_b64 %s, exec, %s" % (sp(S_MASK), ok),
          "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
          "s_cbranch_scc1 .Lck_ret",
          "s_mov_b32 %s, 3" % s(S_CODE)] + goto(".Lr_fault") + [   # tail call: returns to our caller
          ".Lck_ret:",
          "s_setpc_b64 %s" % sp(S_LINK)]
    # LOOKUP (generic, entered by goto, leaves by dispatch): r0 = lookup(r1, r2) for any r1/r2
    # (NULL -> NULL, unknown map -> BAD_MAP).  Lanes with r1 == 0 or r2 == 0 get r0 = NULL and
    # are parked at the next entry (the scheduler resumes them after the running lanes).
    L += [".Lr_lookup:",
          "v_mov_b32 v0, 0", "v_mov_b32 v1, 0",
          "v_mov_b32 v%d, s12" % V_T,
          "v_cmp_ne_u64_e64 %s, v[2:3], 0" % sp(S_JUNK),
          "v_cmp_ne_u64_e64 vcc, v[4:5], 0",
          "s_and_b64 %s, %s, vcc" % (sp(S_JUNK), sp(S_JUNK)),
          "s_and_b64 exec, %s, exec" % sp(S_JUNK),
          "s_cbranch_execz .Llk_sched",
          # which lanes name a known map
          "s_mov_b64 %s, 0" % sp(S_OK),
          "s_mov_b32 %s, 0" % s(S_T2),
          ".Llk_scan:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_NMAPS)),
          "s_cbranch_scc1 .Llk_scan_done",
          "s_lshl_b32 %s, %s, 5" % (s(S_T3), s(S_T2)),
          "s_load_dwordx2 s[%d:%d], %s, %s" % (S_REC, S_REC + 1, sp(S_MAPS), s(S_T3)),
          "s_waitcnt lgkmcnt(0)",
          "v_cmp_eq_u64_e64 vcc, v[2:3], s[%d:%d]" % (S_REC, S_REC + 1),
          "s_or_b64 %s, %s, vcc" % (sp(S_OK), sp(S_OK)),
          "s_add_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_branch .Llk_scan",
          ".Llk_scan_done:",
          "s_andn2_b64 %s, exec, %s" % (sp(S_MASK), sp(S_OK)),
          "s_cmp_eq_u64 %s, 0" % sp(S_MASK),
          "s_cbranch_scc1 .Llk_known",
          "s_mov_b32 %s, 10" % s(S_CODE)] + call(".Lr_fault") + [
          ".Llk_known:",
          # key = *(u32*)r2, region checked
          "v_mov_b32 %s, v4" % v(H[0]), "v_mov_b32 %s, v5" % v(H[1]),
          "s_mov_b32 %s, 4" % s(S_T0), "s_mov_b32 %s, 0" % s(S_T1)] + call(".Lr_check")
    key = v(H[2])
    L += ["v_mov_b32 %s, 0" % key]
    for b in range(4):
        L += ["flat_load_ubyte %s, %s offset:%d" % (v(H[3]), vp(H[0]), b),
              "s_waitcnt vmcnt(0) lgkmcnt(0)",
              "v_lshl_or_b32 %s, %s, %d, %s" % (key, v(H[3]), 8 * b, key)]
    L += ["s_mov_b32 %s, 0" % s(S_T2),
          ".Llk_map:",
          "s_cmp_ge_u32 %s, %s" % (s(S_T2), s(S_NMAPS)),
          "s_cbranch_scc1 .Llk_done",
          "s_lshl_b32 %s, %s, 5" % (s(S_T3), s(S_T2)),
          "s_load_dwordx8 s[%d:%d], %s, %s" % (S_REC, S_REC + 7, sp(S_MAPS), s(S_T3)),
          "s_waitcnt lgkmcnt(0)",
          "v_cmp_eq_u64_e64 %s, v[2:3], s[64:65]" % sp(S_JUNK),
          "v_cmp_gt_u32_e64 vcc, s69, %s" % key,
          "s_and_b64 vcc, vcc, %s" % sp(S_JUNK),
          "v_mov_b32 %s, s68" % v(H[3]),
          "v_mad_u64_u32 %s, %s, %s, %s, s[66:67]" % (vp(H[4]), sp(S_JUNK), key, v(H[3])),
          "v_cndmask_b32 v0, v0, %s, vcc" % v(H[4]),
          "v_cndmask_b32 v1, v1, %s, vcc" % v(H[5]),
          "s_add_u32 %s, %s, 1" % (s(S_T2), s(S_T2)),
          "s_branch .Llk_map",
          ".Llk_done:",
          mode_test(MODE_JIT),
          "s_cbranch_scc1 .Llk_jit"] + dispatch(12) + [
          ".Llk_jit:",     # compiled program: s12 = code offset of the next block
          "s_add_u32 %s, %s, s12" % (s(S_JUNK), s(S_CB)),
          "s_addc_u32 %s, %s, 0" % (s(S_JUNK + 1), s(S_CB + 1)),
          "s_setpc_b64 %s" % sp(S_JUNK)] + [
          ".Llk_sched:"] + goto(".Lr_schedule")
    L += hlookup_routine()
    L += update_routine(img)
    L += hdelete_routine(img)
    L += vstore_routine(img)
    # OVLFIX (called by generic loads when dp_launch.vflags VF_OVERLAY): the packet's own stores over
    # the S_T0 bytes at H[0:1] just read into H[2:3]
    L += [".Lr_ovlfix:"] + ovl_fix("L", (H[2], H[3])) + ["s_setpc_b64 %s" % sp(S_LINK)]
    # PREFETCH (staged kernel): LDS-DMA the 4 KB of 64-B packets of group s[S_T0] into this
    # wave's packet buffer, coalesced (DMA q covers bytes q*1024 .. +1023, its lanes permuted:
    # dma_lane_offsets), lanes past the batch end masked off.  Clobbers s[64:68], m0, exec,
    # H[4:5].
    # The lane mask is a VALU compare, so it is computed under exec = all lanes, whatever exec
    # the caller arrives with (a compare under exec = 0 would DMA no chunk)
    L += [".Lr_prefetch:",
          "s_mov_b64 exec, -1",
          "s_cmp_ge_u32 %s, %s" % (s(S_T0), s(S_NGROUPS)),
          "s_cbranch_scc1 .Lpf_ret",
          "s_lshl_b32 s66, %s, 6" % s(S_T0),
          "s_sub_u32 s66, %s, s66" % s(S_COUNT),           # packets left from this group on
          "s_mov_b32 s64, %s" % s(S_T0),
          "s_mov_b32 s65, 0",
          "s_lshl_b64 s[64:65], s[64:65], 12",
          "s_add_u32 s64, s64, %s" % s(S_DATA),
          "s_addc_u32 s65, s65, %s" % s(S_DATA + 1),
          "s_mov_b32 s67, %s" % s(S_PKTLDS)] + dma_lane_offsets(v(H[4]), v(H[5]))
    for qq in range(4):
        # (lane l's bytes belong to packet 16 qq + (l & 15): inside the batch iff its offset,
        # 64 (l & 15) + 16 (l >> 4), is below 64 x the block's packets left)
        L += ["s_sub_i32 s68, s66, %d" % (16 * qq),
              "s_max_i32 s68, s68, 0",
              "s_min_u32 s68, s68, 16",
              "s_lshl_b32 s68, s68, 6",
              "v_cmp_gt_u32_e64 vcc, s68, %s" % v(H[4]),
              "s_mov_b64 exec, vcc",   # (a VALU write of EXEC would need 5 wait states here)
              "s_mov_b32 m0, s67",
              "s_nop 0",
              "global_load_lds_dwordx4 %s, s[64:65]%s" % (v(H[4]), SETTINGS.ld_policy)]
        if qq < 3:
            L += ["s_add_u32 s64, s64, 1024", "s_addc_u32 s65, s65, 0",
                  "s_add_u32 s67, s67, 1024"]
    L += [".Lpf_ret:",
          "s_setpc_b64 %s" % sp(S_LINK)]
    return L
