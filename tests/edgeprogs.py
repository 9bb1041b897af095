"""Every opcode at edge operands ("an opcode-semantics fixture: 90 opcodes × edge
operands, covering Appendix A quirks"): the programs, their packets, and a plain big-int model
of one ALU op, one jump and one endian / neg op under both instruction semantics.

The operands travel in the packet: `a` at byte 0, `b` at byte 8 (bytes 16..23 hold 0xa5 for the
store cases), one packet per operand pair, so that a batch over E×E has 784 packets (a ragged
last wave) and one over E has 28.  A program is a node list (isa.Insn, layout.LdDw,
layout.Branch) that both semantics run: layout.assemble lays it out for the reference's
cumulative stepping, assemble_std one slot after the other.  Results reach r0 through
`mov_imm r0, 0; mov64_reg r0, rX` (the reference's MOV64 adds, the standard one moves) and
constants through `mov_imm` / LDDW, so the same nodes mean the same thing under both.

Groups (build(sem)):
  single      one op per program: the 12 binary ALU ops × {32, 64} `_reg` over E×E and `_imm`
              per IMM value over E, the 11 conditional jumps likewise (r0 = 1 taken, 2 not),
              neg / neg64 per IMM value, le / be at widths 16, 32, 64, 8, 0, 48; standard
              semantics adds the JMP32 class.  For the CPU checks and for naming a failure.
  folded      one program per (op, width) with all its IMM forms, each result folded into r0 as
              r0 = (r0 ^ result) * 0x2545F491, a bijection of r0 at every step; a jump's
              outcomes go into r0 as one bit each (five jumps a program: a tree of 32 leaves,
              since the reference's stepping never joins two paths again).
  const_src   `_reg` forms with dst from the packet and src a compile-time constant.
  const_both  both operands constants (equal pairs among them).
  same_reg    `op r2, r2` and `jXX r2, r2` over E.
  narrow      the `_reg` forms over E×E with the operands' low 1, 2 or 4 bytes, loaded with
              ldxb / ldxh / ldxw (upper bits known to be zero), four load pairs folded; and the
              shift pairs and masks that extend a narrower value, over E.
  stores      stx{b,h,w,dw} of `a` and st{b,h,w,dw} of every IMM value into packet bytes 16..23
              and into the stack, read back with ldxdw; and each store once as the program's
              last access to the packet.
DIV and MOD leave out the operands whose divisor is zero (the reference crashes on them; for a
32-bit op the divisor is its low 32 bits); build_div0(sem) holds those programs over the full
operand sets.

The model is written from include/ebpf_gpu.h's description of EBPF_SEM_* and SURVEY.md
Appendix A, not from any of the implementations it is compared with."""
import functools

import numpy as np

import stdprogs
from generic_ebpf_amd import isa, layout

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
SEM_REFERENCE, SEM_STANDARD = 0, 1
FAULT_DIV_ZERO = 2     # include/ebpf_gpu.h EBPF_FAULT_DIV_ZERO
FOLD_MUL = 0x2545F491  # odd: r0 -> (r0 ^ v) * FOLD_MUL is a bijection for every v

# the 64-bit operands
E = [0, 1, 2, 0x7f, 0x80, 0xff, 0x7fff, 0x8000, 0xffff, 31, 32, 33, 63, 64, 65,
     0x7fffffff, 0x80000000, 0xffffffff, 0x1_0000_0000, 0x1_0000_0001,
     2**63 - 1, 2**63, 2**64 - 1, 0xffffffff_80000000, 0xffffffff_7fffffff,
     0xffffffff_00000000, 0x0123456789abcdef, 0xfedcba9876543210]
IMM = [0, 1, -1, 2, 31, 32, 33, 63, 64, 65, 0x7fffffff, -0x80000000, 0xff, -256, 0x10000]
# compile-time constants for a src register
CONSTS = [0, 1, 2, 31, 32, 33, 63, 64, 0x7fffffff, 0x80000000, 0xffffffff, 2**32, 2**63,
          2**64 - 1]
# constant (dst, src) pairs, all from E
PAIRS = [(0, 0), (1, 1), (2**63, 2**63), (2**64 - 1, 2**64 - 1), (0x80000000, 0x80000000),
         (2**63 - 1, 2**63), (2**63, 2**63 - 1), (0xffffffff, 0x1_0000_0000),
         (0x1_0000_0001, 1), (0x7fffffff, 0x80000000), (0xffffffff_80000000, 0x80000000),
         (0x0123456789abcdef, 0xfedcba9876543210), (0xfedcba9876543210, 63), (1, 64),
         (2**64 - 1, 32), (0xffffffff_7fffffff, 33), (0, 2**64 - 1),
         (0xffffffff_00000000, 0xffffffff), (65, 31)]
assert len(E) == 28 and len(set(E)) == 28 and len(IMM) == 15
assert all(x in E and y in E for x, y in PAIRS)

ALU_OPS = ["add", "sub", "mul", "div", "or", "and", "lsh", "rsh", "mod", "xor", "mov", "arsh"]
JUMPS = ["jeq", "jgt", "jge", "jset", "jne", "jsgt", "jsge", "jlt", "jle", "jslt", "jsle"]
ENDIAN_WIDTHS = [16, 32, 64, 8, 0, 48]
STORE_SIZES = {"b": 1, "h": 2, "w": 4, "dw": 8}
JUMPS_PER_PROGRAM = 5
GROUPS = ["single", "folded", "const_src", "const_both", "same_reg", "narrow", "stores"]

EE = [(a, b) for a in E for b in E]
E1 = [(a, 0) for a in E]
EA = [(a, a) for a in E]

R0, R1, R2, R3, R4, R10 = 0, 1, 2, 3, 4, 10
I = isa.Insn
LdDw, Branch = layout.LdDw, layout.Branch


# ------------------------------------------------------------------------------ the model

def sx(imm):
    """An s32 immediate sign-extended to 64 bits."""
    return imm & M64


def _signed(x, bits):
    return x - (1 << bits) if x >> (bits - 1) else x


def divisor_is_zero(width, s):
    return (s & M32 if width == 32 else s) == 0


def model_alu(sem, name, width, d, s):
    """One binary ALU op on the u64 register values d and s (an immediate arrives as sx(imm)).
    Returns (dst after, fault code).  32-bit ops work on the low words and zero-extend."""
    mask = M32 if width == 32 else M64
    d, s = d & mask, s & mask
    sh = s & (width - 1)        # the shift count is masked to 5 or 6 bits
    if name == "add":
        v = d + s
    elif name == "sub":
        v = d - s
    elif name == "mul":
        v = d * s
    elif name in ("div", "mod"):   # unsigned
        if s == 0:
            if sem == SEM_REFERENCE:
                return 0, FAULT_DIV_ZERO
            v = 0 if name == "div" else d      # (mod: dst, truncated for a 32-bit op)
        else:
            v = d // s if name == "div" else d % s
    elif name == "or":
        v = d | s
    elif name == "and":
        v = d & s
    elif name == "xor":
        v = d ^ s
    elif name == "lsh":
        v = d << sh
    elif name == "rsh":
        v = d >> sh
    elif name == "arsh":           # the reference's is logical
        v = d >> sh if sem == SEM_REFERENCE else _signed(d, width) >> sh
    elif name == "mov":            # the reference's MOV64 adds; MOV32 moves under both
        v = d + s if sem == SEM_REFERENCE and width == 64 else s
    else:
        raise ValueError(name)
    return v & mask, 0


def model_jump(sem, name, width, d, s):
    """Is the conditional jump taken?  width 64, or 32 for the JMP32 class (standard only)."""
    if width == 32 and sem == SEM_REFERENCE:
        raise ValueError("the reference has no JMP32 class")
    mask = M32 if width == 32 else M64
    d, s = d & mask, s & mask
    sd, ss = _signed(d, width), _signed(s, width)
    return {"jeq": d == s, "jne": d != s, "jgt": d > s, "jge": d >= s, "jlt": d < s,
            "jle": d <= s, "jset": (d & s) != 0, "jsgt": sd > ss, "jsge": sd >= ss,
            "jslt": sd < ss, "jsle": sd <= ss}[name]


def model_unary(sem, name, d, imm):
    """neg / neg64 / le / be with immediate imm on the u64 register value d."""
    if name == "neg":      # the reference negates the immediate and ignores dst
        return (-(imm if sem == SEM_REFERENCE else d)) & M32
    if name == "neg64":    # the reference subtracts the immediate
        return (d - sx(imm)) & M64 if sem == SEM_REFERENCE else (-d) & M64
    if imm not in (16, 32, 64):
        return d           # any other width leaves dst as it is
    if name == "le":
        return d & ((1 << imm) - 1)
    if name == "be":
        return int.from_bytes((d & ((1 << imm) - 1)).to_bytes(imm // 8, "little"), "big")
    raise ValueError(name)


def model_store(size, value, old):
    """8 bytes at the store's address after `size` bytes of value went in."""
    return (value & M64).to_bytes(8, "little")[:size] + bytes(old[size:])


def fold(r0, v):
    return ((r0 ^ v) * FOLD_MUL) & M64


# ------------------------------------------------------------------------------ assembling

def assemble_std(nodes):
    """The node list one slot after the other; the taken side of a Branch goes after everything
    placed so far (a taken jump goes to pc + 1 + off)."""
    slots, pending = [], []

    def place(ns):
        for n in ns:
            if isinstance(n, LdDw):
                v = n.value & M64
                slots.append(isa.encode(isa.OPS["lddw"], n.dst, 0, 0, isa.s32(v)))
                slots.append(isa.encode(0, 0, 0, 0, isa.s32(v >> 32)))
            elif isinstance(n, Branch):
                pending.append((len(slots), n))
                slots.append(None)
            else:
                slots.append(n.encode())

    place(nodes)
    while pending:
        at, br = pending.pop(0)
        ins = br.insn
        slots[at] = isa.encode(ins.op, ins.dst, ins.src, len(slots) - (at + 1), ins.imm)
        place(br.taken)
    return b"".join(slots)


def assemble(sem, nodes):
    return layout.assemble(nodes).code if sem == SEM_REFERENCE else assemble_std(nodes)


def const(reg, v):
    """reg = the constant v: MOV32 (zero-extends) where it fits 32 bits, LDDW else."""
    return I("mov_imm", reg, imm=isa.s32(v)) if v <= M32 else LdDw(reg, v)


def alu_name(name, width, form):
    return name + ("64" if width == 64 else "") + "_" + form


def jump_insn(name, width, form, dst, src=0, imm=0):
    op = (stdprogs.JMP64 if width == 64 else stdprogs.JMP32)[name] | (8 if form == "reg" else 0)
    return I(op, dst, src, 0, imm)


LOAD_A = [I("ldxdw", R2, R1, 0)]
LOAD_AB = [I("ldxdw", R2, R1, 0), I("ldxdw", R3, R1, 8)]
FOLD_R2 = [I("xor64_reg", R0, R2), I("mul64_imm", R0, imm=FOLD_MUL)]


def ret(reg):
    return [I("mov_imm", R0, imm=0), I("mov64_reg", R0, reg), I("exit")]


def taken_or_not(insn):
    return [Branch(insn, [I("mov_imm", R0, imm=1), I("exit")]), I("mov_imm", R0, imm=2),
            I("exit")]


def jump_tree(tests, k=0):
    """tests: [(nodes that set the operands up, jump)]: bit k of r0 (zero before) is set when
    jump k is taken.  Both arms carry the rest of the tree."""
    if not tests:
        return [I("exit")]
    pre, ins = tests[0]
    rest = jump_tree(tests[1:], k + 1)
    return list(pre) + [Branch(ins, [I("or_imm", R0, imm=1 << k)] + rest)] + rest


def chunks(items, most):
    n = -(-len(items) // most)
    return [items[len(items) * k // n: len(items) * (k + 1) // n] for k in range(n)]


# ------------------------------------------------------------------------------ cases

class EdgeCase:
    """name = group/what; operands: the (a, b) of each packet; want(a, b) -> (r0, fault, the 8
    packet bytes at 16 after or None for unchanged), from the model."""

    def __init__(self, sem, name, nodes, operands, want, hint="", general_only=False):
        self.sem, self.name, self.group = sem, name, name.split("/")[0]
        # a program that reads the packet after storing into it reads it from memory: the
        # device runs it in the general kernel layout even over 64-B packets
        self.general_only = general_only
        self.code = assemble(sem, nodes)
        self.operands, self.want, self.hint = operands, want, hint
        self.count = len(operands)

    def packets(self, stride=64):
        """(count, stride) bytes: a, b, 8 × 0xa5, zeros to 64, 0x5a beyond."""
        pk = np.zeros((self.count, stride), dtype=np.uint8)
        ab = np.array(self.operands, dtype=np.uint64).reshape(-1, 2)
        pk[:, :16] = ab.view(np.uint8).reshape(-1, 16)
        pk[:, 16:24] = 0xa5
        pk[:, 64:] = 0x5a
        return pk

    def expect(self, stride=64):
        """The model's (r0, faults, packets after)."""
        after = self.packets(stride)
        r0 = np.zeros(self.count, dtype=np.uint64)
        faults = np.zeros(self.count, dtype=np.uint8)
        for i, (a, b) in enumerate(self.operands):
            v, f, stored = self.want(a, b)
            r0[i], faults[i] = (0 if f else v), f     # a faulted packet's result is 0
            if stored is not None and not f:
                after[i, 16:24] = np.frombuffer(stored, dtype=np.uint8)
        return r0, faults, after


def _plain(v_f):
    return v_f[0], v_f[1], None


def _alu_cases(sem, out, div0):
    """ALU ops into `out`; the zero-divisor operands of DIV and MOD into `div0` instead."""
    for name in ALU_OPS:
        for width in (32, 64):
            dm = name in ("div", "mod")
            nz = (lambda s, w=width: not divisor_is_zero(w, s)) if dm else (lambda s: True)
            alu = functools.partial(model_alu, sem, name, width)
            reg, imm_op = alu_name(name, width, "reg"), alu_name(name, width, "imm")
            op_reg = LOAD_AB + [I(reg, R2, R3)] + ret(R2)
            want_reg = lambda a, b, alu=alu: _plain(alu(a, b))
            out.append(EdgeCase(sem, "single/" + reg, op_reg,
                                [(a, b) for a, b in EE if nz(b)], want_reg))
            for imm in IMM:
                c = EdgeCase(sem, "single/%s[%d]" % (imm_op, imm),
                             LOAD_A + [I(imm_op, R2, imm=imm)] + ret(R2), E1,
                             lambda a, b, alu=alu, imm=imm: _plain(alu(a, sx(imm))))
                (out if nz(sx(imm)) else div0).append(c)
            # folded: every immediate in one program
            imms = [i for i in IMM if nz(sx(i))]
            nodes = [I("mov_imm", R0, imm=0)]
            for imm in imms:
                nodes += LOAD_A + [I(imm_op, R2, imm=imm)] + FOLD_R2
            out.append(EdgeCase(
                sem, "folded/" + imm_op, nodes + [I("exit")], E1,
                lambda a, b, alu=alu, imms=imms: (functools.reduce(
                    lambda r, i: fold(r, alu(a, sx(i))[0]), imms, 0), 0, None),
                hint="single/%s[IMM] for IMM in %s" % (imm_op, imms)))
            # const_src: dst from the packet, src a constant
            cs = [c for c in CONSTS if nz(c)]
            nodes = [I("mov_imm", R0, imm=0)]
            for c in cs:
                nodes += LOAD_A + [const(R3, c), I(reg, R2, R3)] + FOLD_R2
            out.append(EdgeCase(
                sem, "const_src/" + reg, nodes + [I("exit")], E1,
                lambda a, b, alu=alu, cs=cs: (functools.reduce(
                    lambda r, c: fold(r, alu(a, c)[0]), cs, 0), 0, None),
                hint="single/%s with b in %s" % (reg, [hex(c) for c in cs])))
            # const_both: every pair a constant, and `a` folded in last so that lanes differ
            ps = [p for p in PAIRS if nz(p[1])]
            nodes = [I("mov_imm", R0, imm=0)]
            for x, y in ps:
                nodes += [const(R2, x), const(R3, y), I(reg, R2, R3)] + FOLD_R2
            out.append(EdgeCase(
                sem, "const_both/" + reg, nodes + LOAD_A + FOLD_R2 + [I("exit")], E1,
                lambda a, b, alu=alu, ps=ps: (fold(functools.reduce(
                    lambda r, p: fold(r, alu(*p)[0]), ps, 0), a), 0, None),
                hint="single/%s with (a, b) in %s" % (reg, [(hex(x), hex(y)) for x, y in ps])))
            same = LOAD_A + [I(reg, R2, R2)] + ret(R2)
            want_same = lambda a, b, alu=alu: _plain(alu(a, a))
            out.append(EdgeCase(sem, "same_reg/" + reg, same, [p for p in EA if nz(p[0])],
                                want_same))
            if dm:
                div0.append(EdgeCase(sem, "div0/" + reg, op_reg, EE, want_reg))
                div0.append(EdgeCase(sem, "div0/%s_same_reg" % reg, same, EA, want_same))
                for c in [c for c in CONSTS if not nz(c)]:
                    div0.append(EdgeCase(
                        sem, "div0/%s_const[%#x]" % (reg, c),
                        LOAD_A + [const(R3, c), I(reg, R2, R3)] + ret(R2), E1,
                        lambda a, b, alu=alu, c=c: _plain(alu(a, c))))
    for name in ("neg", "neg64"):
        for imm in IMM:
            out.append(EdgeCase(sem, "single/%s[%d]" % (name, imm),
                                LOAD_A + [I(name, R2, imm=imm)] + ret(R2), E1,
                                lambda a, b, name=name, imm=imm:
                                (model_unary(sem, name, a, imm), 0, None)))
    for name in ("le", "be"):
        for w in ENDIAN_WIDTHS:
            out.append(EdgeCase(sem, "single/%s[%d]" % (name, w),
                                LOAD_A + [I(name, R2, imm=w)] + ret(R2), E1,
                                lambda a, b, name=name, w=w:
                                (model_unary(sem, name, a, w), 0, None)))


def _jump_cases(sem, out):
    for width in (64, 32) if sem == SEM_STANDARD else (64,):
        for name in JUMPS:
            tag = ("jmp32_" if width == 32 else "") + name
            jmp = functools.partial(model_jump, sem, name, width)
            bits = lambda outcomes: sum(1 << k for k, t in enumerate(outcomes) if t)
            out.append(EdgeCase(sem, "single/%s_reg" % tag,
                                LOAD_AB + taken_or_not(jump_insn(name, width, "reg", R2, R3)), EE,
                                lambda a, b, jmp=jmp: (1 if jmp(a, b) else 2, 0, None)))
            for imm in IMM:
                out.append(EdgeCase(
                    sem, "single/%s_imm[%d]" % (tag, imm),
                    LOAD_A + taken_or_not(jump_insn(name, width, "imm", R2, imm=imm)), E1,
                    lambda a, b, jmp=jmp, imm=imm: (1 if jmp(a, sx(imm)) else 2, 0, None)))
            for k, imms in enumerate(chunks(IMM, JUMPS_PER_PROGRAM)):
                tests = [([], jump_insn(name, width, "imm", R2, imm=i)) for i in imms]
                out.append(EdgeCase(
                    sem, "folded/%s_imm.%d" % (tag, k),
                    [I("mov_imm", R0, imm=0)] + LOAD_A + jump_tree(tests), E1,
                    lambda a, b, jmp=jmp, imms=imms: (bits(jmp(a, sx(i)) for i in imms), 0, None),
                    hint="single/%s_imm[IMM] for IMM in %s (bit k of r0: the k-th)" % (tag, imms)))
            for k, cs in enumerate(chunks(CONSTS, JUMPS_PER_PROGRAM)):
                tests = [([const(R3, c)], jump_insn(name, width, "reg", R2, R3)) for c in cs]
                out.append(EdgeCase(
                    sem, "const_src/%s_reg.%d" % (tag, k),
                    [I("mov_imm", R0, imm=0)] + LOAD_A + jump_tree(tests), E1,
                    lambda a, b, jmp=jmp, cs=cs: (bits(jmp(a, c) for c in cs), 0, None),
                    hint="single/%s_reg with b in %s (bit k of r0: the k-th)" % (
                        tag, [hex(c) for c in cs])))
            for k, ps in enumerate(chunks(PAIRS, JUMPS_PER_PROGRAM)):
                tests = [([const(R2, x), const(R3, y)], jump_insn(name, width, "reg", R2, R3))
                         for x, y in ps]
                out.append(EdgeCase(
                    sem, "const_both/%s_reg.%d" % (tag, k),
                    [I("mov_imm", R0, imm=0)] + jump_tree(tests), E1,
                    lambda a, b, jmp=jmp, ps=ps: (bits(jmp(x, y) for x, y in ps), 0, None),
                    hint="single/%s_reg with (a, b) in %s (bit k of r0: the k-th)" % (
                        tag, [(hex(x), hex(y)) for x, y in ps])))
            out.append(EdgeCase(sem, "same_reg/%s_reg" % tag,
                                LOAD_A + taken_or_not(jump_insn(name, width, "reg", R2, R2)), EA,
                                lambda a, b, jmp=jmp: (1 if jmp(a, a) else 2, 0, None)))


# (load of a, load of b): the operands' low bytes, zero-extended by the load
NARROW_LOADS = [("w", "b"), ("w", "w"), ("h", "h"), ("b", "w")]


def _narrow_cases(sem, out):
    """Operands that reach their registers through narrower loads, so that whatever the compiled
    code knows about their upper bits is in play, and the shift pairs and masks compilers emit
    for extensions."""
    def lo(sz, v):
        return v & ((1 << 8 * STORE_SIZES[sz]) - 1)
    for name in ALU_OPS:
        for width in (32, 64):
            reg = alu_name(name, width, "reg")
            alu = functools.partial(model_alu, sem, name, width)
            nodes = [I("mov_imm", R0, imm=0)]
            for la, lb in NARROW_LOADS:
                nodes += [I("ldx" + la, R2, R1, 0), I("ldx" + lb, R3, R1, 8), I(reg, R2, R3)]
                nodes += FOLD_R2
            ops = [p for p in EE if p[1] & 0xff] if name in ("div", "mod") else EE
            out.append(EdgeCase(
                sem, "narrow/" + reg, nodes + [I("exit")], ops,
                lambda a, b, alu=alu: (functools.reduce(
                    lambda r, l: fold(r, alu(lo(l[0], a), lo(l[1], b))[0]), NARROW_LOADS, 0),
                    0, None),
                hint="single/%s with the low bytes of a and b, loads %s" % (reg, NARROW_LOADS)))
    for width in (64, 32) if sem == SEM_STANDARD else (64,):
        for name in JUMPS:
            tag = ("jmp32_" if width == 32 else "") + name
            jmp = functools.partial(model_jump, sem, name, width)
            tests = [([I("ldx" + la, R2, R1, 0), I("ldx" + lb, R3, R1, 8)],
                      jump_insn(name, width, "reg", R2, R3)) for la, lb in NARROW_LOADS]
            out.append(EdgeCase(
                sem, "narrow/%s_reg" % tag, [I("mov_imm", R0, imm=0)] + jump_tree(tests), EE,
                lambda a, b, jmp=jmp: (sum(1 << k for k, (la, lb) in enumerate(NARROW_LOADS)
                                           if jmp(lo(la, a), lo(lb, b))), 0, None),
                hint="single/%s_reg with the low bytes of a and b, loads %s (bit k of r0: the "
                     "k-th)" % (tag, NARROW_LOADS)))
    # extension idioms on a: (what, nodes after r2 = a, the value they leave in r2)
    alu = functools.partial(model_alu, sem)

    def pair(first, second, width, count):
        w = "64" if width == 64 else ""
        return ("%s%s_%s%s_%d" % (first, w, second, w, count),
                [I("%s%s_imm" % (first, w), R2, imm=count), I("%s%s_imm" % (second, w), R2, imm=count)],
                lambda a: alu(second, width, alu(first, width, a, count)[0], count)[0])
    idioms = [pair("lsh", "arsh", 64, 32), pair("lsh", "rsh", 64, 32), pair("lsh", "arsh", 64, 48),
              pair("lsh", "arsh", 64, 56), pair("lsh", "arsh", 32, 24), pair("lsh", "arsh", 32, 16),
              pair("rsh", "lsh", 64, 32),
              ("and64_ff_sub64_1", [I("and64_imm", R2, imm=0xff), I("sub64_imm", R2, imm=1)],
               lambda a: alu("sub", 64, alu("and", 64, a, 0xff)[0], 1)[0]),
              ("mov32_self", [I("mov_reg", R2, R2)], lambda a: alu("mov", 32, a, a)[0]),
              ("and_m1_arsh64_31", [I("and_imm", R2, imm=-1), I("arsh64_imm", R2, imm=31)],
               lambda a: alu("arsh", 64, alu("and", 32, a, sx(-1))[0], 31)[0])]
    nodes = [I("mov_imm", R0, imm=0)]
    for _, ns, _ in idioms:
        nodes += LOAD_A + ns + FOLD_R2
    for sz, w in (("h", 16), ("w", 32), ("w", 64), ("b", 16)):
        nodes += [I("ldx" + sz, R2, R1, 0), I("be", R2, imm=w)] + FOLD_R2
        idioms.append(("ldx%s_be%d" % (sz, w), None,
                       lambda a, sz=sz, w=w: model_unary(sem, "be", lo(sz, a), w)))
    out.append(EdgeCase(
        sem, "narrow/idioms", nodes + [I("exit")], E1,
        lambda a, b: (functools.reduce(lambda r, i: fold(r, i[2](a)), idioms, 0), 0, None),
        hint="folded in order: %s" % [i[0] for i in idioms]))


STACK_FILL_IMM = isa.s32(0xa5a5a5a5)                       # stdw: sign-extended to 8 bytes
STACK_FILL = sx(STACK_FILL_IMM).to_bytes(8, "little")
PKT_FILL = bytes([0xa5] * 8)


def _store_cases(sem, out):
    for k, (sz, size) in enumerate(STORE_SIZES.items()):
        for where, base, off, prep, old in (("pkt", R1, 16, [], PKT_FILL),
                                            ("stack", R10, -8,
                                             [I("stdw", R10, 0, -8, STACK_FILL_IMM)], STACK_FILL)):
            pkt = where == "pkt"

            def want_stx(a, b, size=size, old=old, pkt=pkt):
                new = model_store(size, a, old)
                return int.from_bytes(new, "little"), 0, new if pkt else None
            out.append(EdgeCase(sem, "stores/stx%s_%s" % (sz, where),
                                LOAD_A + prep + [I("stx" + sz, base, R2, off),
                                                 I("ldxdw", R4, base, off)] + ret(R4),
                                E1, want_stx, general_only=pkt))
            if pkt:   # the store last (the staged layout keeps such a program): a from r2
                out.append(EdgeCase(sem, "stores/stx%s_pkt_last" % sz,
                                    LOAD_A + [I("mov_imm", R0, imm=0), I("mov64_reg", R0, R2),
                                              I("stx" + sz, R1, R2, 16), I("exit")], E1,
                                    lambda a, b, size=size: (a, 0, model_store(size, a, PKT_FILL))))
                out.append(EdgeCase(sem, "stores/st%s_pkt_last" % sz,
                                    LOAD_A + [I("mov_imm", R0, imm=0), I("mov64_reg", R0, R2),
                                              I("st" + sz, R1, 0, 16, -256), I("exit")], E1,
                                    lambda a, b, size=size: (a, 0, model_store(size, sx(-256),
                                                                               PKT_FILL))))
            # every immediate in turn into the same 8 bytes (they keep the earlier stores'
            # upper bytes), each read back and folded; the last one differs by size
            imms = IMM[3 * k:] + IMM[:3 * k]
            nodes = [I("mov_imm", R0, imm=0)] + prep
            for imm in imms:
                nodes += [I("st" + sz, base, 0, off, imm), I("ldxdw", R2, base, off)] + FOLD_R2

            def want_st(a, b, size=size, old=old, pkt=pkt, imms=imms):
                r0, cur = 0, old
                for imm in imms:
                    cur = model_store(size, sx(imm), cur)
                    r0 = fold(r0, int.from_bytes(cur, "little"))
                return r0, 0, cur if pkt else None
            out.append(EdgeCase(sem, "stores/st%s_%s" % (sz, where), nodes + [I("exit")], E1,
                                want_st, hint="immediates in order: %s" % imms,
                                general_only=pkt))


@functools.lru_cache(maxsize=None)
def _all(sem):
    out, div0 = [], []
    _alu_cases(sem, out, div0)
    _jump_cases(sem, out)
    _narrow_cases(sem, out)
    _store_cases(sem, out)
    for c in div0:
        c.name = "div0/" + c.name.split("/", 1)[1]
        c.group = "div0"
    out.sort(key=lambda c: GROUPS.index(c.group))   # (stable: by group, else as built)
    names = [c.name for c in out + div0]
    assert len(set(names)) == len(names)
    return tuple(out), tuple(div0)


def build(sem):
    """The cases of GROUPS under `sem`; none divides by zero."""
    return list(_all(sem)[0])


def build_div0(sem):
    """The `div0` group: the DIV and MOD programs over their full operand sets, the `_imm` forms
    with immediate 0 and a constant zero divisor included.  name -> the case of build(sem) with
    the same program and operands where the divisor is not zero: div0_twin(name)."""
    return list(_all(sem)[1])


def div0_twin(name):
    what = name.split("/", 1)[1]
    if what.endswith("_same_reg"):
        return "same_reg/" + what[:-len("_same_reg")]
    if what.endswith("_reg"):
        return "single/" + what
    return None   # an immediate 0 or a constant zero divisor: every packet divides by zero


def div0_divisor(name, a, b):
    """The operand the program of div0 case `name` divides by, and the op's width."""
    what = name.split("/", 1)[1]
    width = 64 if what[3:5] == "64" else 32
    if what.endswith("_same_reg"):
        return a, width
    if what.endswith("_reg"):
        return b, width
    return int(what[what.index("[") + 1:-1], 0), width
