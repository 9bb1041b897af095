"""The register plan, the handler families and the ABI shared with the host: what the kernels,
the host that launches them and the host compiler agree on, stated once, and the asm_handlers.h
lines that export it (header_abi, header_families).  Data and header text only: no instruction
is emitted here.
"""
import re

NREG = 11

# VGPRs
PKT0 = 22            # v22..v37 staged packet dwords (staged kernel)
V_PKT = 38           # v[38:39] packet base address
V_LEN = 40           # packet length (bytes)
V_T = 41             # parked entry byte offset
V_STK = 42           # lane stack bottom (LDS byte address)
V_L16 = 43           # staged image: lane * 16 (LDS-DMA staging offset)
V_IDX = 43           # general image: the lane's packet index in the launch
V_RES = 44           # v[44:45]: r0 of the lanes that retired in the running group
# v[44:45] (RETK == 1) or v[64:64+2*RETK]: r0 of the lanes that retired, per group of the
# current superblock (stored together at the start of the next superblock)
H = [46, 47, 48, 49, 50, 51]         # handler temporaries
R = list(range(52, 63))              # routine temporaries
V_GIDX = H[3]        # at a group's start: the lanes' packet indices in the launch (the start
                     # block of a compiled program reads them, asm_cc.cpp cc_prologue)
V_HVAL = H[4]        # v[50:51] after .Lr_hlookup: the found slot's first 8 value bytes
V_SEL = 63                           # v_perm selector 0x00010203 (byte swap)


# Launch-private verdict partials (dp_launch.hist_rows, shared with asm_runtime.cpp): 8 replicas
# of EBPF_HIST_BINS u64 (bin 256 of replica 0 = the fault count), then the u32 arrival tickets:
# one per replica and a top one, each on a 64-B line of its own.
HIST_REPLICAS = 8
HIST_REPLICA_BYTES = 257 * 8
HIST_TICKET_OFF = HIST_REPLICAS * HIST_REPLICA_BYTES

# SGPRs (next_free_sgpr 80 -> 8 waves per SIMD)
S_CB = 4             # s[4:5] code base (.Lcb): routines are reached at S_CB + (label - .Lcb)
S_ENT = 8            # s[8:15] current entry: s[8:9] handler, s[10:11] imm, s12 next, s13 target,
                     # s14 aux0, s15 aux1
S_ALIVE = 16         # s[16:17]
S_SAVE = 18          # s[18:19]
S_PROG, S_MAPS, S_DATA, S_OFFS, S_OFFBASE, S_RET, S_FAULTS, S_HIST = 20, 22, 24, 26, 28, 30, 32, 34
S_COUNT, S_STRIDE, S_START, S_NMAPS, S_NENT = 36, 38, 39, 40, 41
S_STKSTRIDE, S_LDSBASE = 42, 43      # dp_launch.stack_stride, .lds_stack_base
S_GROUP, S_GSTRIDE, S_NGROUPS, S_PKTLDS = 44, 45, 46, 47
S_MASK = 48          # s[48:49] temp mask
S_LINK = 50          # s[50:51] subroutine return address
S_CODE = 52          # fault code argument
S_T0, S_T1, S_T2, S_T3 = 53, 54, 55, 56
S_BYTES = 57         # check routine scratch
S_SHARED = 58        # s[58:59] src_shared_base
S_JUNK = 60          # s[60:61] scratch sdst
S_OK = 62            # s[62:63] check: accumulated ok lanes
S_REC = 64           # s[64:71] map record {handle, dev_base, value_size, max_entries, lds_off, pad}
S_PREVG = 72         # group whose results are still in V_RET (-1: none)
S_KMASK = 73         # superblock size - 1 of this launch (K' <= RETK, a power of two; host-chosen,
                     # dp_launch.total_waves from WAVES_SB_SHIFT up = log2 K'): small batches use
                     # shorter superblocks so that every wave gets work
S_WAVE = 3
S_SHORT = 74         # s[74:75], general image: compiled programs' short-lane mask (asm_cc.cpp
                     # ldxpkc_general)
NSGPR = 76           # + VCC, XNACK, FLAT_SCRATCH
# general image: s[76:77] = the run mask of a compiled program's hoisted packet loads (asm_cc.cpp
# runmask: the running lanes whose packet holds every load of the run)
S_RUNMASK = 76
NSGPR_GEN = 88
# staged image: s[74:75] .. s[96:97] hold the taken-lane masks of a structured compiled program's
# pending branches (asm_jit.cpp; 12 levels); 98 SGPRs still allow the image's 6 waves per SIMD
S_JOIN = 74
JOIN_LEVELS = 12
# staged image with result bursts (RETK > 1): s98 = the result slots holding unwritten groups
# (bit k = slot k), s99 = dp_launch.wphase (store_phased)
S_PEND = S_JOIN + 2 * JOIN_LEVELS
S_WPHASE = S_PEND + 1
S_CLOCK = S_WPHASE + 1   # s[100:101]: the constant clock, read at the group's start
NSGPR_STAGED = S_CLOCK + 2
# (no join SGPRs in the general image: s74..s97 would overlap the run mask and the short-lane
# mask, and structured exits address the LDS histogram through lane 0 of v43, which the general
# image uses for V_IDX; AH_GEN_JOIN stays 0)
GEN_JOIN = 0


ALU64R = ["ADD", "SUB", "MUL", "OR", "AND", "XOR", "LSH", "RSH", "DIV", "MOD"]
ALU32R = ["ADD", "SUB", "MUL", "OR", "AND", "XOR", "LSH", "RSH", "MOV", "DIV", "MOD"]
ALU64I = ["ADD", "MUL", "OR", "AND", "XOR", "LSH", "RSH", "DIV", "MOD", "MOV"]   # MOV = LDDW
ALU32I = ["ADD", "SUB", "MUL", "OR", "AND", "XOR", "LSH", "RSH", "MOV", "DIV", "MOD"]
CONDS = ["JEQ", "JNE", "JGT", "JGE", "JLT", "JLE", "JSGT", "JSGE", "JSLT", "JSLE", "JSET"]
SIZES = [1, 2, 4, 8]

# (name, arity, class, index) arity: 2 = (dst, src), 1 = (reg), 0.  The class groups the families
# the host compiler treats alike (asm_cc.cpp reads ah_fam_class / ah_fam_idx, never the order of
# the registrations below); the index within it is the ALU operation's position in its list, the
# condition's position in CONDS, or log2 of the access size in bytes.  A family registered
# without a class is a class of its own.
FAMILIES = []


def fam(name, arity, cls=None, idx=0):
    FAMILIES.append((name, arity, cls or name, idx))


def lg2(z):
    return z.bit_length() - 1


for i, o in enumerate(ALU64R):
    fam("A64R_" + o, 2, "A64R", i)
for i, o in enumerate(ALU32R):
    fam("A32R_" + o, 2, "A32R", i)
for i, c in enumerate(CONDS):
    fam(c + "_R", 2, "JR", i)
for z in SIZES:
    fam("LDXGEN%d" % z, 2, "LDXGEN", lg2(z))
for z in SIZES:
    fam("STXGEN%d" % z, 2, "STXGEN", lg2(z))
for z in SIZES:
    fam("LDXMAP%d" % z, 2, "LDXMAP", lg2(z))
for i, o in enumerate(ALU64I):
    fam("A64I_" + o, 1, "A64I", i)
for i, o in enumerate(ALU32I):
    fam("A32I_" + o, 1, "A32I", i)
for w in (16, 32, 64):
    fam("BSWAP%d" % w, 1, "BSWAP", lg2(w // 8))
for i, c in enumerate(CONDS):
    fam(c + "_I", 1, "JI", i)
for z in SIZES:
    fam("LDXPKTG%d" % z, 1, "LDXPKTG", lg2(z))
for z in SIZES:
    fam("LDXSTK%d" % z, 1, "LDXSTK", lg2(z))
for z in SIZES:
    fam("STXSTK%d" % z, 1, "STXSTK", lg2(z))
for z in SIZES:
    fam("STGEN%d" % z, 1, "STGEN", lg2(z))
for z in SIZES:
    fam("STSTK%d" % z, 0, "STSTK", lg2(z))
for n in ("EXIT", "FAULT", "NOP", "LOOKUPSTK", "LOOKUPGEN"):
    fam(n, 0)
for z in SIZES:                # staged packet load at a constant byte offset: (dst, offset)
    fam("LDXPKC%d" % z, 3, "LDXPKC", lg2(z))
fam("HLOOKUP", 0)              # hashtable lookup, map known at translation time (s14 = record offset)
fam("UPDATE", 0)               # map_update_elem, map known (s14 = record offset, s15 = entry index)
for z in SIZES:                # load from a hashtable value (lookup result), in range by provenance
    fam("LDXHV%d" % z, 2, "LDXHV", lg2(z))
# standard-eBPF semantics (ebpf_prog_set_semantics): the operations whose meaning differs from
# the reference's, and the JMP32 class
fam("MOV64R", 2)
fam("NEG64", 1)
fam("NEG32", 1)
fam("ARSH64I", 1)
fam("ARSH64R", 2)
fam("ARSH32I", 1)
fam("ARSH32R", 2)
for o in ("DIV64Z", "MOD64Z", "DIV32Z", "MOD32Z"):
    fam(o, 2)                  # register divisor; zero gives 0 (DIV) or dst (MOD)
for i, c in enumerate(CONDS):
    fam("J32" + c[1:] + "_R", 2, "J32R", i)
for i, c in enumerate(CONDS):
    fam("J32" + c[1:] + "_I", 1, "J32I", i)
# loops under standard semantics (dprog.h DK_LOOPINIT / DK_LOOPCNT): the lane's count of taken
# backward jumps in the first 4 bytes of its stack slice (below the frame the program addresses)
fam("LOOPINIT", 0)
fam("LOOPCNT", 0)
fam("HDELETE", 0)              # map_delete_elem on a hashtable known at translation time (s14, s15)
# interpreter superinstructions (asm_runtime.cpp asm_fuse_interp; staged kernels): a packet load at
# a constant offset fused with the BE16 / BE32 of its destination (dst, offset)
fam("LDXPKBE16", 3, "LDXPKBE", 1)
fam("LDXPKBE32", 3, "LDXPKBE", 2)
# stores into map values (ebpf_gpu.h "Stores into map values"; dprog.h DK_CNT_STORE / DK_XADD):
# the STX of a counter update (d = the pointer, s = the value), XADD (d = the pointer, s = the
# addend) and XADD | FETCH (d = the addend, which receives the old value; s = the pointer)
for z in (4, 8):
    fam("CNTST%d" % z, 2, "CNTST", lg2(z))
for z in (4, 8):
    fam("XADD%d" % z, 2, "XADD", lg2(z))
for z in (4, 8):
    fam("XADDF%d" % z, 2, "XADDF", lg2(z))
fam("OVLINIT", 0)              # dprog.h DK_OVLINIT: the lane's overlay and write counts = 0
# a counter update the translator resolved completely (asm_runtime.cpp): an immediate addend
# (s[10:11]) into a DP_MAP_ATOMIC map's delta area at r_d + s14 (d = the value pointer, a
# non-NULL lookup result; s14 = the offset + the map's delta-area offset)
for z in (4, 8):
    fam("CNTAI%d" % z, 1, "CNTAI", lg2(z))
# ... into the workgroup's LDS sums of a DP_MAP_LDSDELTA map: at (r_d - s15) + s14 (s15 = the
# mirror's address, low word; s14 = the offset + the table's LDS address)
for z in (4, 8):
    fam("CNTAL%d" % z, 1, "CNTAL", lg2(z))
# a load through a packet pointer at an offset only known at run time (translate.cpp AV_CTXV:
# a cursor advanced in a loop): one bounds check against the lane's packet, one load; lanes whose
# address leaves the packet take the generic path (s[10:11] = the offset)
for z in SIZES:
    fam("LDXPKTV%d" % z, 2, "LDXPKTV", lg2(z))
del i, o, c, z, w, n            # (the loops' variables: not part of what `import *` hands out)
SPILL = 51                     # v51 (H[5]): .Lr_check's SGPR spill lanes around .Lr_vstore


# The ABI shared with the host.
# The kernels, the host that launches them (asm_runtime.cpp, gpu_runtime.cpp) and the host
# compiler that encodes machine words running inside them (asm_cc.cpp, asm_jit.cpp) agree on the
# kernel-argument layout, on registers, on flag bits and on a few constants.  This file states all
# of them once and header_abi() writes them into asm_handlers.h:
#   * registers (AH_S_*, AH_V_*), the mode bits (AH_MODE_*) and the template table's order
#     (AH_JT_*) are this file's to choose: the host names them and holds no copy;
#   * layouts and values that dprog.h / ebpf_gpu.h declare for all the device code (dp_launch,
#     dp_map, dp_entry, DP_*, EBPF_FAULT_WRITES) are copied here, exported (AH_L_*, AH_M_*,
#     AH_E_*, AH_DP_*, AH_EBPF_FAULT_WRITES) and asserted equal to the declarations in
#     asm_runtime.cpp, entry by entry through the lists AH_LAUNCH_FIELDS / AH_SHARED_VALUES
#     (dprog.h cannot include a generated header: the HIP sources include it).  A copy that
#     drifts stops the build there.

# dp_launch fields the kernels load: name -> (byte offset, bytes), and the kernarg size
LAUNCH = {
    "prog": (0x00, 8), "maps": (0x08, 8), "data": (0x10, 8), "offsets": (0x18, 8),
    "off_base": (0x20, 8), "ret": (0x28, 8), "faults": (0x30, 8), "hist": (0x38, 8),
    "count": (0x40, 8), "stride": (0x48, 4), "start": (0x4c, 4), "nmaps": (0x50, 4),
    "nentries": (0x54, 4), "stack_stride": (0x58, 4), "lds_stack_base": (0x5c, 4),
    "total_waves": (0x60, 4), "lds_pkt_base": (0x64, 4), "hist_rows": (0x68, 8),
    "hist_user": (0x70, 8), "hist_flags": (0x78, 4), "nwg": (0x7c, 4),
    "upd_log": (0x80, 8), "upd_cap": (0x88, 4), "upd_stride": (0x8c, 4), "pkt_base": (0x90, 8),
    "upd_faulted": (0xa8, 8), "vflags": (0xcc, 4), "wphase": (0xd0, 4),
}
KERNARG_BYTES = 232
# ebpf_asm_link's arguments (asm_runtime.cpp asm_link_args)
LINK_ARGS = {"entries": (0x0, 8), "count": (0x8, 4)}
LINK_KERNARG_BYTES = 16


# dp_map (a record is loaded whole into s[S_REC:S_REC+7]) and the lowered dp_entry (into
# s[S_ENT:S_ENT+7]; aux0 / aux1 are the two operand words asm_runtime.cpp set_aux writes)
MAP_REC = {"handle": 0, "dev_base": 8, "value_size": 16, "max_entries": 20, "lds_off": 24, "flags": 28}
MAP_REC_BYTES = 32
ENTRY = {"handler": 0, "imm": 8, "next": 16, "target": 20, "aux0": 24, "aux1": 28}
ENTRY_BYTES = 32

# the mode word s7: what kind of kernel and launch this is, set once at kernel start
S_MODE = 7
MODE_STAGED = 0        # staged 64-B packets (else the general kernels)
MODE_JIT = 1           # a compiled program: V_T holds code offsets, not entry offsets
MODE_STRUCTURED = 2    # ... with structured control flow (set by its prologue, asm_cc.cpp)
MODE_HDRSTAGE = 3      # general kernels: header staging (PKTLDS_HDRSTAGE)
MODE_OVERLAY = 13      # VF_OVERLAY
MODE_KEEP = 14         # keep mode (VF_KEEP), general kernels: PKTLDS_HDRKEEP
MODE_EXTENTS = 15      # VF_EXTENTS


# dp_launch.vflags bits (dprog.h DP_VF_*)
VF_OVERLAY = 0         # the program reads its own stores into map values
VF_VSTORE = 1          # it has value-store sites
VF_EXTENTS = 2         # offsets holds (start, end) pairs
VF_KEEP = 3            # staged kernels keep the group's packets in LDS (LDXPKTV)
VF_WCAP = 4            # count each packet's logged writes
VF_ENTRIES_SHIFT, VF_ENTRIES_BITS = 8, 8     # the overlay's entries per lane
# dp_launch.lds_pkt_base bits above the LDS offset (general kernels)
PKTLDS_HDRSTAGE = 31   # stage packet headers into v22..v37
PKTLDS_HDRKEEP = 30    # ... and keep them in the wave's LDS packet buffer
# dp_launch.total_waves: log2 of the superblock size above the wave count
WAVES_SB_SHIFT = 28
# dp_launch.hist_flags
HIST_STORE = 0         # the last workgroup stores the reduced histogram instead of adding it
# dp_launch.wphase (store_phased): window | log2(period) << 16, bit 31 = the wide kernel's 16 slots
WPHASE_PERIOD_SHIFT = 16
WPHASE_WIDE = 31

LOOP_BUDGET = 1 << 20          # DP_LOOP_BUDGET
# the lane's stack slice below the frame (DP_OVL_*, DP_WCOUNT): loop count, overlay count, the
# scratch a store into a map value is redirected to, the write count, the overlay entries
OVL_COUNT, VST_SCRATCH, WCOUNT, OVL_ENTRIES = 4, 8, 16, 24
WRITES_MAX = 16                # DP_WRITES_MAX (VF_WCAP)
FAULT_WRITES = 11              # EBPF_FAULT_WRITES


def variants(arity):
    if arity == 3:
        return [(d, o) for o in range(64) for d in range(NREG)]
    if arity == 2:
        return [(d, s) for d in range(NREG) for s in range(NREG)]
    if arity == 1:
        return [(d, None) for d in range(NREG)]
    return [(None, None)]


JIT_AREA_BYTES = 512 * 1024
JIT_ENTRY_OFF = 16     # a compiled program starts here in the area (the bytes before: never executed)


# ebpf_jit_tmpl: offsets from .Lcb of the glue (gen_jit.py) and of the routines compiled programs reach,
# then the area's size.  asm_jit.cpp indexes it by AH_JT_<label without its .Ljt_ / .Lr_ / .L /
# ebpf_ prefix, in capitals> (header_abi), so the order here is the only order there is.
JT_LABELS = [".Ljt_mov_s%d" % r for r in range(10, 16)] + [
    ".Ljt_cs", ".Ljt_cs_br", ".Ljt_cs_vt", ".Ljt_cs_end",
    ".Ljt_cl", ".Ljt_cl_lit", ".Ljt_cl_vt", ".Ljt_cl_end",
    ".Ljt_br", ".Ljt_jl", ".Ljt_jl_end", ".Ljt_wait", ".Lr_exit_k", ".Lr_exit", ".Lr_fault",
    ".Lr_hlookup", ".Lgroup_done",
    ".Lr_schedule",
    "ebpf_jit_area"]


def header_abi():
    """The asm_handlers.h lines of the ABI section above (the same for every image)."""
    out = ["// dp_launch fields the kernels load (byte offsets) and the kernarg size; "
           "asm_runtime.cpp asserts them"]
    out += ["#define AH_L_%s 0x%x" % (f.upper(), off) for f, (off, _) in LAUNCH.items()]
    out += ["#define AH_KERNARG_BYTES %d" % KERNARG_BYTES,
            "#define AH_LAUNCH_FIELDS(X) " + " ".join("X(%s, AH_L_%s)" % (f, f.upper()) for f in LAUNCH)]
    out += ["#define AH_LINK_%s 0x%x" % (f.upper(), off) for f, (off, _) in LINK_ARGS.items()]
    out += ["#define AH_LINK_KERNARG_BYTES %d" % LINK_KERNARG_BYTES]
    out += ["#define AH_M_%s %d" % (f.upper(), off) for f, off in MAP_REC.items()]
    out += ["#define AH_MAP_REC_BYTES %d" % MAP_REC_BYTES]
    out += ["#define AH_E_%s %d" % (f.upper(), off) for f, off in ENTRY.items()]
    out += ["#define AH_ENTRY_BYTES %d" % ENTRY_BYTES]
    out += ["// registers the host compiler's encoders name (gen_interp.py register plan)"]
    # (AH_S_OPND: s10..s15, the entry's operand words imm .. aux1; bit k of ah_reads = s(10 + k))
    sregs = [("MODE", S_MODE), ("CB", S_CB), ("ENT", S_ENT), ("OPND", S_ENT + ENTRY["imm"] // 4),
             ("SAVE", S_SAVE), ("DATA", S_DATA),
             ("STKSTRIDE", S_STKSTRIDE), ("PKTLDS", S_PKTLDS), ("MASK", S_MASK), ("LINK", S_LINK),
             ("CODE", S_CODE), ("BYTES", S_BYTES), ("SHARED", S_SHARED), ("JUNK", S_JUNK),
             ("SHORT", S_SHORT)]
    vregs = [("PKT0", PKT0), ("PKT", V_PKT), ("LEN", V_LEN), ("T", V_T), ("STK", V_STK),
             ("L16", V_L16), ("RES", V_RES), ("GIDX", V_GIDX), ("HVAL", V_HVAL), ("SEL", V_SEL)]
    vregs += [("H%d" % i, r) for i, r in enumerate(H)] + [("R%d" % i, r) for i, r in enumerate(R)]
    out += ["#define AH_S_%s %d" % x for x in sregs] + ["#define AH_V_%s %d" % x for x in vregs]
    out += ["// bits of the mode word s[AH_S_MODE]"]
    out += ["#define AH_MODE_%s %d" % x for x in (
        ("STAGED", MODE_STAGED), ("JIT", MODE_JIT), ("STRUCTURED", MODE_STRUCTURED),
        ("HDRSTAGE", MODE_HDRSTAGE), ("OVERLAY", MODE_OVERLAY), ("KEEP", MODE_KEEP),
        ("EXTENTS", MODE_EXTENTS))]
    out += ["// dprog.h / ebpf_gpu.h values the kernels were generated with; asm_runtime.cpp asserts them"]
    values = (
        ("DP_VF_OVERLAY", 1 << VF_OVERLAY), ("DP_VF_VSTORE", 1 << VF_VSTORE),
        ("DP_VF_EXTENTS", 1 << VF_EXTENTS), ("DP_VF_KEEP", 1 << VF_KEEP), ("DP_VF_WCAP", 1 << VF_WCAP),
        ("DP_VF_ENTRIES_SHIFT", VF_ENTRIES_SHIFT), ("DP_VF_ENTRIES_MAX", (1 << VF_ENTRIES_BITS) - 1),
        ("DP_PKTLDS_HDRSTAGE", 1 << PKTLDS_HDRSTAGE), ("DP_PKTLDS_HDRKEEP", 1 << PKTLDS_HDRKEEP),
        ("DP_WAVES_SB_SHIFT", WAVES_SB_SHIFT), ("DP_HIST_STORE", 1 << HIST_STORE),
        ("DP_WPHASE_PERIOD_SHIFT", WPHASE_PERIOD_SHIFT), ("DP_WPHASE_WIDE", 1 << WPHASE_WIDE),
        ("DP_LOOP_BUDGET", LOOP_BUDGET), ("DP_OVL_COUNT", OVL_COUNT), ("DP_OVL_SCRATCH", VST_SCRATCH),
        ("DP_WCOUNT", WCOUNT), ("DP_OVL_ENTRIES", OVL_ENTRIES), ("DP_WRITES_MAX", WRITES_MAX),
        ("EBPF_FAULT_WRITES", FAULT_WRITES), ("DP_HIST_REPLICAS", HIST_REPLICAS),
        ("DP_HIST_REPLICA_BYTES", HIST_REPLICA_BYTES), ("DP_HIST_TICKET_OFF", HIST_TICKET_OFF),
        ("DP_HIST_PARTIAL_BYTES", HIST_TICKET_OFF + 64 * (HIST_REPLICAS + 1)))
    out += ["#define AH_%s %du" % x for x in values]
    out += ["#define AH_SHARED_VALUES(X) " + " ".join("X(%s)" % n for n, _ in values)]
    out += ["// ebpf_jit_tmpl's entries, in the table's order"]
    jt = [re.sub(r"^(\.Ljt_|\.Lr_|\.L|ebpf_)", "", n).upper() for n in JT_LABELS] + ["AREA_BYTES"]
    out += ["enum {"] + ["\tAH_JT_%s," % n for n in jt] + ["\tAH_JT_COUNT", "};"]
    out += ["#define AH_JIT_ENTRY_OFF %d  // a compiled program's start block in ebpf_jit_area" % JIT_ENTRY_OFF]
    return out


# The staged image the assembly interpreter (variant 2) launches from (m3): one result group per
# burst (64 VGPRs) and an interpreter kernel that declares only the SGPRs the image's own code
# touches (s0..s73; compiled programs' join masks start at s74), so that 8 workgroups of 256
# lanes fit a CU (MI355X_MICROARCH.md "Residency": .sgpr_count <= 80 -> 8; 98 -> 6).  The
# interpreter is bound by its dependent dispatch chain (s_load -> s_waitcnt -> s_setpc per
# entry) and scales with resident waves (C4: 2 workgroups per CU 3.19 ms ... 6: 1.25 ms).
NSGPR_INTERP = S_JOIN


def header_families():
    """The family structure the host compiler reads: per family its class (AHC_*) and its index
    within the class, and the names of the condition indices."""
    classes = []
    for _, _, cls, _ in FAMILIES:
        if cls not in classes:
            classes.append(cls)
    for cls in classes:   # an index names one family of its class
        idx = [i for _, _, c, i in FAMILIES if c == cls]
        assert len(set(idx)) == len(idx), "class %s: index used twice" % cls
    h = ["#define AHF_COUNT %d" % len(FAMILIES),
         "// family classes: the families the code generator treats alike (asm_cc.cpp)",
         "enum { %s, AHC_COUNT };" % ", ".join("AHC_" + c for c in classes),
         "// per family: class (AHC_*), index within the class (the ALU operation, the condition",
         "// AH_CC_*, log2 of the access size in bytes)",
         "static const uint8_t ah_fam_class[AHF_COUNT] = {%s};" % ",".join(
             str(classes.index(c)) for _, _, c, _ in FAMILIES),
         "static const uint8_t ah_fam_idx[AHF_COUNT] = {%s};" % ",".join(
             str(i) for _, _, _, i in FAMILIES),
         "// condition indices of the conditional-jump classes (JR, JI, J32R, J32I)"]
    h += ["#define AH_CC_%s %d" % (c, i) for i, c in enumerate(CONDS)]
    return h
