#!/usr/bin/env python3
"""Digests of the compiled device code (ebpf_prog_device_code) of a fixed corpus of programs,
under every A/B knob of the host compiler (asm_cc.cpp cc_options) and both packet layouts.  Needs
no GPU.  Two trees whose outputs are equal line for line emit the same code: the check a change
to the compiler that means to change no emitted byte runs before and after.

One line per (program, knob setting, layout): name, knobs, layout, code length, sha256 of the
code — or the error string where the program does not compile for that layout.

Map handles are heap addresses and appear in the code as literals, so before hashing every
aligned 32-bit word equal to the low or the high half of one of the program's map handles
becomes a fixed placeholder per map; two processes then agree.

The corpus: workloads.CONFIGS, the programs of tests/golden/rand.npz, randprog.random_program
over --seeds seeds in three forms (plain; writes and value stores; many writes), and the
programs of tests/stdprogs.py, hashprogs.py, loopwrites.py, manywrites.py, and edges(): one small
program per translator path the rest does not reach (tools/translation_digest.py hashes the
same corpus's translations).  --groups picks a subset.  A knob whose digests equal the default's
on the whole corpus is unexercised: the tool fails (not checked when --groups leaves part of the
corpus out)."""
import argparse
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pkgload  # noqa: E402

pkgload.load()
from generic_ebpf_amd import native, randprog, workloads  # noqa: E402

# every knob setting: the default, each EBPF_CC_OFF bit, each switch of its own
KNOBS = [{}] + [{"EBPF_CC_OFF": str(1 << b)} for b in range(6)] + \
    [{"EBPF_CC_" + k: "1"} for k in ("NORUNMASK", "NOHOIST", "NOSHORT", "EXITCALL", "NOPKTV",
                                     "NOHFWD", "KEEPSTORES")] + \
    [{"EBPF_JIT_" + k: "1"} for k in ("NOCC", "NOSTRUCT", "NOREVLOOP")]
GROUPS = ("workloads", "golden", "random", "tests", "edges")
STD = 1   # native.SEM_STANDARD


def arr(max_entries, value_size):
    return ("array", max_entries, value_size)


def hsh(key_size, value_size, max_entries):
    return ("hash", key_size, value_size, max_entries)


def corpus(groups, seeds):
    """[(name, code, relocs, map specs, semantics)]"""
    out = []

    def add(name, code, relocs=(), maps=(), sem=0):
        out.append((name, bytes(code), list(relocs), list(maps), sem))

    if "workloads" in groups:
        for cfg, c in workloads.CONFIGS.items():
            lay = c["prog"]()
            maps = {"c4": [arr(256, 8)], "c4c": [arr(256, 8), arr(256, 8)], "c4h": [hsh(4, 8, 64)],
                    "c5ms": [arr(16, 4 * workloads.c5meldsim_table().shape[1])]}.get(cfg, [])
            add("wl/" + cfg, lay.code, lay.relocs, maps, c.get("semantics", 0))
    if "golden" in groups:
        import goldens
        for c in goldens.load(os.path.join(goldens.GOLDEN_DIR, "rand.npz")):
            add("golden/" + c.name, c.code, c.relocs, [arr(me, vs) for vs, me, _ in c.maps])
    if "random" in groups:
        forms = (("plain", {}), ("writes", dict(writes=True, vstores=True)),
                 ("many", dict(many_writes=True)))
        for seed in range(seeds):
            for form, kw in forms:
                lay = randprog.random_program(seed, **kw)
                add("rand/%d/%s" % (seed, form), lay.code, lay.relocs, [arr(256, 8)])
    if "tests" in groups:
        import hashprogs
        import loopwrites
        import manywrites
        import stdprogs
        for name, items, _ in stdprogs.KATS:
            code, rel = stdprogs.asm(items)
            add("std/kat/" + name, code, rel, [], STD)
        for s in range(8):
            add("std/gen/%d" % s, *stdprogs.gen_program(1000 + s, length=30 + 5 * s, with_map=s % 2 == 1),
                [arr(16, 8)] if s % 2 else [], STD)
            add("std/loop/%d" % s, *stdprogs.gen_loop_program(7000 + s), [], STD)
            add("std/cursor/%d" % s, *stdprogs.gen_cursor_program(7000 + s), [], STD)
            add("std/loopwrite/%d" % s, *stdprogs.gen_loop_write_program(800 + s, counters=s % 3 == 2),
                [arr(16, 16), arr(16, 8)], STD)
            add("std/loopwrite_fetched/%d" % s, *stdprogs.gen_loop_write_program(1000 + s, fetched=True),
                [arr(16, 32), arr(16, 8)], STD)
            add("std/loopwrite_mixed/%d" % s, *stdprogs.gen_loop_write_program(1200 + s, mixed=True),
                [hsh(4, 16, 16), arr(16, 8)], STD)
        add("std/countdown", *stdprogs.countdown(100), [], STD)
        for ks, src, off, read, store, second in (
                (4, "stack", 0, (8, 0), False, None), (4, "stack", 0, (8, 0), True, None),
                (6, "packet", 10, (8, 0), False, None), (8, "packet", 16, (4, 4), False, None),
                (1, "stack", 3, (1, 0), False, None), (16, "stack", 8, (2, 6), False, None),
                (4, "null", 0, (8, 0), False, None), (4, "stack", 0, (8, 8), False, (8, 20))):
            lay = hashprogs.lookup_program(ks, src, off, read=read, store=store, second=second)
            maps = [hsh(ks, 16, 32)] + ([hsh(second[0], 8, 32)] if second else [])
            add("hash/%d_%s_%d_%d_%d%s%s" % (ks, src, off, read[0], read[1], "_store" if store else "",
                                             "_second" if second else ""), lay.code, lay.relocs, maps)
        for kind, fn in loopwrites.PROGS.items():
            add("loopwrites/" + kind, *fn(),
                [arr(loopwrites.MAP_KEYS.get(kind, loopwrites.NKEYS), loopwrites.VALUE_SIZE[kind])], STD)
        for kind, fn in loopwrites.HASH_PROGS.items():
            add("loopwrites/hash_" + kind, *fn(), [hsh(4, loopwrites.VALUE_SIZE[kind], 16)], STD)
        add("loopwrites/idiom_live", *loopwrites.prog_idiom_counters(live=True), [arr(16, 8)], STD)
        add("loopwrites/mixed_counter_store", *loopwrites.prog_mixed_counter_store(), [arr(16, 8)], STD)
        for name, (fn, vs, me) in list(manywrites.CASES.items()) + list(manywrites.READBACK.items()):
            lay = fn()
            add("manywrites/" + name, lay.code, lay.relocs, [arr(me, vs)])
    if "edges" in groups:
        for name, code, relocs, maps, sem in edges():
            add("edges/" + name, code, relocs, maps, sem)
    return out


def edges():
    """One small program per translator path that nothing else in the corpus reaches: every
    translation-time fault, the zero-immediate DIV / MOD rewrites, the JA corner cases, the
    run-time-map compare chains, delete on either kind of map, and counter idioms at a merge
    point.  [(name, code, relocs, map specs, semantics)]; tests/test_translate_and_layout.py
    names the entry each one is there for."""
    import stdprogs
    import test_map_writes
    from generic_ebpf_amd import isa, layout
    E, I, ops = isa.encode, stdprogs.I, isa.OPS
    exit_ = E(ops["exit"])
    out = []

    def raw(name, code, sems=(0,), maps=()):
        for sem in sems:
            out.append((name + ("_std" if sem else ""), code, [], list(maps), sem))

    # (reference stepping runs slot 0, then slot 1: two slots are a program)
    raw("bad_opcode", E(0x8d) + exit_)
    raw("bad_dst", E(ops["mov_imm"], 11) + exit_)
    raw("bad_src", E(ops["mov_reg"], 0, 12) + exit_)
    raw("jmp32_bad_src", E(stdprogs.JMP32["jeq"] | 8, 0, 12, 1) + exit_ + exit_, (STD,))
    for op in ("div_imm", "mod_imm", "div64_imm", "mod64_imm"):
        raw(op + "_zero", E(ops["mov_imm"], 0, imm=9) + E(ops[op], 0, imm=0) + exit_ + exit_, (0, STD))
    raw("lddw_last_slot", E(ops["mov_imm"], 0, imm=1) + E(ops["lddw"], 0, imm=1))
    raw("helper_out_of_range", E(ops["call"], imm=64) + exit_)
    raw("helper_unset", E(ops["call"], imm=5) + exit_)
    raw("helper_unsupported", E(ops["call"], imm=3) + exit_)
    raw("jump_to_own_state", E(ops["jeq_imm"], 0, off=-1) + exit_, (0, STD))
    raw("jump_past_end", E(ops["jeq_imm"], 0, off=100) + exit_, (0, STD))
    raw("jump_pc_wraps", E(ops["jeq_imm"], 0, off=-2) + exit_)            # pc 1 - 2: 2^32 - 1 slots on
    raw("ja_to_itself", E(ops["ja"], off=-1) + exit_, (0, STD))
    raw("ja_before_slot_0", E(ops["ja"], off=-5) + exit_, (STD,))
    # (a JA chain cannot outgrow the program: every hop moves forward.  This one's second hop
    # wraps the u32 pc and lands 2^32 slots on)
    raw("ja_chain_pc_wraps", E(ops["ja"], off=0) + E(ops["ja"], off=-3))
    raw("jmp32_invalid", E(0x06) + exit_, (STD,))
    raw("xadd_imm_2", E(0xdb, 10, 0, -8, 2) + exit_, (STD,))
    raw("falls_off_the_end", E(ops["mov_imm"], 0, imm=1) + E(ops["mov_imm"], 0, imm=1))

    # (the map pointer goes through the stack, as in prog_runtime_map: the translator no longer
    # knows which map it is.  No arithmetic on handles: their difference would be in the dump)
    N, look = isa.Insn, lambda k: [
        layout.LdDw(1, layout.MapRef(k)), N("stxdw", 10, 1, -24), N("ldxdw", 1, 10, -24),
        N("mov_imm", 2, imm=0), N("mov64_reg", 2, 10), N("add64_imm", 2, imm=-4), N("call", imm=0),
        layout.Branch(N("jeq_imm", 0, imm=0), [N("mov_imm", 0, imm=0xdead), N("exit")]),
        N("ldxdw", 0, 0, 0), N("exit")]
    lay = layout.assemble([N("ldxw", 6, 1, 0), N("stxw", 10, 6, -4), N("ldxb", 7, 1, 5),
                           N("and_imm", 7, imm=1), layout.Branch(N("jeq_imm", 7, imm=0), look(0))] + look(1))
    out.append(("runtime_map_lookup", lay.code, lay.relocs, [hsh(4, 8, 16), arr(16, 8)], 0))
    lay = test_map_writes.prog_runtime_map()
    out.append(("runtime_map_update_delete", lay.code, lay.relocs, [hsh(4, 8, 16), arr(16, 8)], 0))
    key = [I("stw", 10, 0, -4, 0), I("mov64_reg", 2, 10), I("add64_imm", 2, imm=-4)]
    value = [I("stdw", 10, 0, -16, 7), I("mov64_reg", 3, 10), I("add64_imm", 3, imm=-16),
             I("mov64_imm", 4, imm=0)]
    for name, items, maps in (
            ("update_constant_not_a_map", [("lddw", 1, 0x1234)] + key + value + [I("call", imm=1)], []),
            ("delete_hashtable", [("lddw_map", 1, 0)] + key + [I("call", imm=2)], [hsh(4, 8, 16)]),
            ("delete_array", [("lddw_map", 1, 0)] + key + [I("call", imm=2)], [arr(16, 8)])):
        out.append((name,) + stdprogs.asm(items + [I("exit")]) + (maps, STD))
    # a counter idiom (LDX, ADD, STX on a lookup result) that another path enters at its ADD / STX
    for name, at_alu in (("counter_alu_is_target", True), ("counter_stx_is_target", False)):
        items = [I("ldxb", 6, 1, 0), ("lddw_map", 1, 0)] + key + [
            I("call", imm=0), I("jne_imm", 0, off="hit", imm=0), I("exit"), ("label", "hit"),
            I("mov64_imm", 7, imm=5), I("jeq_imm", 6, off="alu" if at_alu else "stx", imm=0),
            I("ldxdw", 7, 0, 0), ("label", "alu"), I("add64_imm", 7, imm=1),
            ("label", "stx"), I("stxdw", 0, 7, 0), I("mov64_imm", 0, imm=0), I("exit")]
        out.append((name,) + stdprogs.asm(items) + ([arr(16, 8)], STD))
    out += loop_edges()
    return out


def loop_edges():
    """edges(), continued: what keeps a loop's count (xlate_loops.cpp), the interval rules that
    drop it, the slot-graph restatement's corners (xlate_slots.cpp) and the two refusals of
    xlate_writes.cpp that need a program of some size.  Standard semantics but for the last."""
    import loopwrites
    import stdprogs
    import test_write_rules
    I, out = stdprogs.I, []

    def std(name, items, maps=()):
        out.append((name,) + stdprogs.asm(items) + (list(maps), STD))

    def countdown(reg, n, label, body=()):
        return [I("mov64_imm", reg, imm=n), ("label", label), I("sub64_imm", reg, imm=1)] + list(body) + \
            [I("jne_imm", reg, off=label, imm=0)]

    std("two_loops", countdown(2, 3, "A") + countdown(3, 3, "B") + [I("exit")])
    # the backward jump's target is an invalid JMP32 slot: the loop head is a fault entry
    std("loop_head_faults", [I("ja", off="S"), ("label", "B"), I(0x06), ("label", "S"),
                             I("mov64_imm", 2, imm=1), I("jne_imm", 2, off="B", imm=0), I("exit")])
    # the backward JA is reached by falling into it and by a jump: its count has two predecessors
    std("loop_count_two_predecessors", [
        I("mov64_imm", 2, imm=3), ("label", "H"), I("sub64_imm", 2, imm=1),
        I("jeq_imm", 2, off="X", imm=0), I("jgt_imm", 2, off="J", imm=1), I("mov64_imm", 3, imm=0),
        ("label", "J"), I("ja", off="H"), ("label", "X"), I("exit")])
    # a backward jump whose target never comes back to it
    std("loop_head_leaves", [I("ja", off="S"), ("label", "H"), I("mov64_imm", 0, imm=0), I("exit"),
                             ("label", "S"), I("mov64_imm", 2, imm=1), I("jne_imm", 2, off="H", imm=0),
                             I("exit")])
    std("loop_two_decrements", countdown(2, 4, "H", [I("sub64_imm", 2, imm=1)]) + [I("exit")])
    std("loop_decrement_on_one_arm", [I("ldxb", 4, 1, 0)] + countdown(
        2, 4, "H", [I("jeq_imm", 4, off="S", imm=0), I("sub64_imm", 2, imm=1), ("label", "S")]) + [I("exit")])
    std("loop_counter_overwritten", countdown(2, 4, "H", [I("and64_imm", 2, imm=7)]) + [I("exit")])
    # every interval rule on the way to a counter in [1, 5]: the count goes
    std("loop_intervals", [
        I("stdw", 10, 0, -8, 0), (0xdb, 10, 4, -8, 0),                     # XADD: nothing known after
        I("ldxb", 3, 1, 0), I("mov_imm", 4, imm=7), I("and_imm", 3, imm=15), I("mod64_imm", 3, imm=5),
        I("add64_imm", 3, imm=1), I("add64_imm", 4, imm=-3), I("add64_imm", 4, imm=-100),
        I("sub64_imm", 5, imm=1),
        I("jge_imm", 3, off="X", imm=9), I("jgt_imm", 3, off="X", imm=-1),
        I(stdprogs.JMP32["jeq"], 4, off="X", imm=99),
        ("label", "H"), I("sub64_imm", 3, imm=1), I("jne_imm", 3, off="H", imm=0),
        ("label", "X"), I("exit")])
    # counter idioms on the stack, in a loop, none read back: with a JA inside, 32-bit ALU forms,
    # an ALU that is none, a STX elsewhere; then a JA -1 after an LDX, an XADD with fetch that
    # nothing reaches, and an idiom cut off by the program's end
    std("loop_slot_shapes", [
        I("mov64_imm", 2, imm=3), I("stdw", 10, 0, -8, 0), I("stdw", 10, 0, -16, 0), ("label", "H"),
        I("ldxw", 5, 10, -8), I("ja", off=0), I("add_imm", 5, imm=1), I("stxw", 10, 5, -8),
        I("ldxw", 5, 10, -16), I("add_reg", 5, 2), I("stxw", 10, 5, -16),
        I("ldxw", 5, 10, -8), I("mov64_reg", 5, 2),
        I("ldxw", 5, 10, -8), I("add_imm", 5, imm=1), I("stxw", 10, 5, -12),
        I("neg64", 5), I("be", 5, imm=16),
        I("sub64_imm", 2, imm=1), I("jne_imm", 2, off="H", imm=0),
        I("jeq_imm", 2, off="W", imm=1), I("jeq_imm", 2, off="T", imm=2), I("exit"),
        ("label", "W"), I("ldxw", 5, 10, -8), I("ja", off=-1), (0xdb, 10, 5, -8, 1),
        ("label", "T"), I("ldxw", 5, 10, -8), I("add_imm", 5, imm=1)])
    # refused: a loop that loads a word its XADD (device atomics: an array) changed
    out.append(("loop_xadd_then_load",) + loopwrites.prog_xadd_then_load() + ([arr(16, 8)], STD))
    # refused: more stores read back on one path than the spilled overlay holds
    lay = test_write_rules._readback_stores(2049)
    out.append(("readback_2049_stores", lay.code, lay.relocs, [arr(16, 8)], 0))
    return out


def normalised(code, handles):
    """the code with every aligned word equal to half a map handle replaced by a placeholder"""
    w = np.frombuffer(code, dtype="<u4").copy()
    for k, h in enumerate(handles):
        for half, v in enumerate((h & 0xffffffff, (h >> 32) & 0xffffffff)):
            w[w == v] = 0x4d415000 | (k << 1) | half   # "MAP", map number, low / high
    return w.tobytes()


def digests(progs, out):
    """write every program's lines; returns per knob setting the list of its digests"""
    L = native.lib()
    cap = 1 << 20
    buf = (ctypes.c_uint8 * cap)()
    per_knob = [[] for _ in KNOBS]
    env = native.Env()
    def create(specs):
        return [native.HashMap(env, s[1], s[2], s[3]) if s[0] == "hash" else native.Map(env, s[1], s[2])
                for s in specs]

    for name, code, relocs, specs, sem in progs:
        # The code's shape depends on one property of the handles: a register or operand that
        # holds the high half of one handle is not set again for the next (mov64, the operand
        # preloads).  A heap that crosses a 4 GiB boundary between two maps would change it, so
        # such a set of maps is put aside and made again.
        maps, aside = create(specs), []
        while len({m.handle >> 32 for m in maps}) > 1:
            aside += maps
            assert len(aside) < 8 * len(specs), "map handles keep differing in their high halves"
            maps = create(specs)
        handles = [m.handle for m in maps]
        p = native.Prog(env, native.patch_relocs(code, relocs, handles))
        if sem:
            p.set_semantics(native.SEM_STANDARD)
        for ki, knobs in enumerate(KNOBS):
            os.environ.update(knobs)
            try:
                for layout in (0, 1):
                    n = ctypes.c_size_t(cap)
                    err = L.ebpf_prog_device_code(p.ptr, layout, buf, ctypes.byref(n))
                    if err:
                        res = "error %d: %s" % (err, native.last_error())
                    else:
                        dc = normalised(bytes(buf[:n.value]), handles)
                        res = "%d %s" % (len(dc), hashlib.sha256(dc).hexdigest())
                    per_knob[ki].append(res)
                    out.write("%s %s %d %s\n" % (
                        name, ",".join("%s=%s" % kv for kv in knobs.items()) or "-", layout, res))
            finally:
                for k in knobs:
                    os.environ.pop(k, None)
        p.destroy()
        for m in maps + aside:
            m.destroy()
    assert env.destroy() == 0
    return per_knob


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--groups", default=",".join(GROUPS), help="of " + ", ".join(GROUPS))
    ap.add_argument("--seeds", type=int, default=300, help="randprog seeds (group random)")
    ap.add_argument("-o", "--output", help="file to write (default: standard output)")
    a = ap.parse_args()
    groups = [g for g in a.groups.split(",") if g]
    assert all(g in GROUPS for g in groups), groups
    for k in list(os.environ):
        if k.startswith("EBPF_CC_") or k.startswith("EBPF_JIT_"):
            del os.environ[k]
    out = open(a.output, "w") if a.output else sys.stdout
    per_knob = digests(corpus(groups, a.seeds), out)
    if a.output:
        out.close()
    if set(groups) == set(GROUPS):
        idle = [KNOBS[k] for k in range(1, len(KNOBS)) if per_knob[k] == per_knob[0]]
        if idle:
            sys.exit("knobs the corpus does not exercise: %s" % idle)


if __name__ == "__main__":
    main()
