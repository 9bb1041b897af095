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
programs of tests/stdprogs.py, hashprogs.py, loopwrites.py, manywrites.py.  --groups picks a
subset.  A knob whose digests equal the default's on the whole corpus is unexercised: the tool
fails (not checked when --groups leaves part of the corpus out)."""
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
GROUPS = ("workloads", "golden", "random", "tests")
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
