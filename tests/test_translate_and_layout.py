"""Host-side translation (reference stepping → device program) and the stepping-aware
assembler.  No GPU needed: ebpf_prog_device_info only translates."""
import os
import sys

import numpy as np

import goldens
from generic_ebpf_amd import isa, layout, workloads


def test_assembler_triangular_stepping():
    slots, how = layout.simulate_slots(workloads.prog_c2().code)
    assert how == "exit" and slots == [0, 1, 3, 6, 10, 15, 21, 28]


def test_assembler_main_path_counts():
    assert workloads.prog_c2().main_path_steps == 8
    assert workloads.prog_c3().main_path_steps == 64
    assert workloads.prog_c4().main_path_steps >= 64
    assert workloads.prog_c5().main_path_steps == 256


def _info(native, env, code):
    p = native.Prog(env, code)
    try:
        return p.info()
    finally:
        p.destroy()


def test_translation_sizes(native, env):
    i = _info(native, env, workloads.prog_c2().code)
    assert (i.nslots, i.nentries) == (29, 8)
    lay = workloads.prog_c3()
    i = _info(native, env, lay.code)
    assert i.nslots == lay.nslots
    # JA stride resets are folded away: fewer entries than executed-path instructions+resets
    assert 60 <= i.nentries < 200


def test_translation_faults_are_entries(native, env):
    O = isa.OPS
    e = isa.encode
    # falls off the end, self-loop, invalid opcode: each becomes a (shared) FAULT entry
    for code in (e(O["mov_imm"], 0, imm=1) + e(O["mov_imm"], 0, imm=1),
                 e(O["ja"], off=-1) + e(O["exit"]),
                 e(0x06) + e(O["exit"])):
        assert _info(native, env, code).nentries >= 1


def test_translation_resolves_maps(native, env):
    lay = workloads.prog_c4()
    m = native.Map(env, 256, 8)
    try:
        p = native.Prog(env, native.patch_relocs(lay.code, lay.relocs, [m.handle]))
        i = p.info()
        assert i.nmaps == 1 and i.max_stack == 4
        p.destroy()
    finally:
        m.destroy()


def test_all_goldens_translate(native, env):
    for f in goldens.all_golden_files():
        for c in goldens.load(f):
            assert _info(native, env, c.code).nentries >= 1


def test_literal_slot_programs_execute_the_stepped_slots():
    """SURVEY.md §8(d) literal N-slot variants: 64 slots execute 11, 256 execute 23 (slots
    0, 1, 3, 6, ... under cumulative stepping), ending in EXIT."""
    from generic_ebpf_amd import layout, workloads
    for n, k in ((64, 11), (256, 23)):
        lay = workloads.prog_literal(n)
        seq, how = layout.simulate_slots(lay.code)
        assert len(lay.code) == 8 * n and how == "exit" and len(seq) == k == lay.main_path_steps
        assert seq == [i * (i + 1) // 2 for i in range(k)]


# ---- the translation's dump (EBPF_XLATE_DUMP, csrc/host/xlate_dump.cpp) of the corpus's edges
# group (tools/device_code_digest.py edges()): the entry each program is there for

FAULT, LOOKUP, UPDATE, LOOPCNT, HDELETE, CNT_STORE = 0x100, 0x101, 0x10d, 0x10f, 0x110, 0x111
BAD_OPCODE, DIV_ZERO, SLOT, HELPER, UNSUPPORTED, BAD_REG, LOOP, BAD_MAP = 1, 2, 4, 5, 6, 7, 8, 10
JEQ_IMM, JGT_IMM, LDDW, ADD64_IMM, MOV_IMM, MOV_REG, STXDW = 0x15, 0x25, 0x18, 0x07, 0xb4, 0xbc, 0x7b
EINVAL, EOPNOTSUPP = "0x16", 95


class _Dump:
    """err, the header's fields (lists of words) and the entries of one dump; an entry is a dict
    of its fields (imm as written: hex, or MAP<k>) plus `reached`"""

    def __init__(self, err, text):
        self.err, self.head, self.entries = err, {}, []
        for ln in text.splitlines():
            w = ln.split()
            if not w[0].isdigit():
                self.head[w[0]] = w[1:]
                continue
            e = dict(zip(w[1:17:2], w[2:18:2]))
            e = {k: v if k == "imm" else int(v, 0) for k, v in e.items()}
            e["reached"] = "in" in w[17:18]
            self.entries.append(e)
        self.start = int(self.head["start"][0])

    def find(self, kind, **fields):
        """the reached entries of a kind whose fields are as given"""
        return [e for e in self.entries if e["reached"] and e["kind"] == kind and
                all(e[k] == v for k, v in fields.items())]

    def fault(self, code):
        return self.find(FAULT, aux=code)

    def is_fault(self, index, code):
        e = self.entries[index]
        return e["reached"] and e["kind"] == FAULT and e["aux"] == code

    def rungs(self, handle):
        """kinds the reached "JEQ r1, handle" compares of a chain are taken into"""
        return {self.entries[j["target"]]["kind"] for j in self.find(JEQ_IMM, dst=1, imm=handle)}


def _jump_into(code):
    return lambda d: any(d.is_fault(j["target"], code) for j in d.find(JEQ_IMM))


def _loop_kept(count=1):
    return lambda d: len(d.find(LOOPCNT)) == count and d.head["has_loops"] == ["1"]


def _update_delete_chains(d):
    upd = {e["aux"] for e in d.find(UPDATE)}
    return (d.rungs("MAP0") == {UPDATE, HDELETE} and d.rungs("MAP1") == {UPDATE, LDDW} and
            upd == {0, 1} and d.find(LDDW, dst=0, imm=EINVAL) and d.fault(BAD_MAP) and
            d.find(JGT_IMM, dst=4, imm="0x2") and d.head["hupd_maps"] == ["0"] and
            d.head["upd_maps"] == ["1"])


EDGES = {
    "bad_opcode": lambda d: d.is_fault(d.start, BAD_OPCODE),
    "bad_dst": lambda d: d.is_fault(d.start, BAD_REG),
    "bad_src": lambda d: d.is_fault(d.start, BAD_REG),
    "jmp32_bad_src_std": lambda d: d.is_fault(d.start, BAD_REG),
    "div_imm_zero": lambda d: d.fault(DIV_ZERO),
    "mod_imm_zero": lambda d: d.fault(DIV_ZERO),
    "div64_imm_zero": lambda d: d.fault(DIV_ZERO),
    "mod64_imm_zero": lambda d: d.fault(DIV_ZERO),
    "div_imm_zero_std": lambda d: d.find(MOV_IMM, dst=0, imm="0") and not d.fault(DIV_ZERO),
    "mod_imm_zero_std": lambda d: d.find(MOV_REG, dst=0, src=0) and not d.fault(DIV_ZERO),
    "div64_imm_zero_std": lambda d: d.find(LDDW, dst=0, imm="0") and not d.fault(DIV_ZERO),
    "mod64_imm_zero_std": lambda d: d.find(ADD64_IMM, dst=0, imm="0", aux=1) and not d.fault(DIV_ZERO),
    "lddw_last_slot": lambda d: d.fault(SLOT),
    "helper_out_of_range": lambda d: d.is_fault(d.start, HELPER),
    "helper_unset": lambda d: d.is_fault(d.start, HELPER),
    "helper_unsupported": lambda d: d.is_fault(d.start, UNSUPPORTED),
    "jump_to_own_state": _jump_into(LOOP),
    "jump_to_own_state_std": _jump_into(LOOP),
    "jump_past_end": _jump_into(SLOT),
    "jump_past_end_std": _jump_into(SLOT),
    "jump_pc_wraps": _jump_into(SLOT),
    "ja_to_itself": lambda d: d.is_fault(d.start, LOOP),
    "ja_to_itself_std": lambda d: d.is_fault(d.start, LOOP),
    "ja_before_slot_0_std": lambda d: d.is_fault(d.start, SLOT) and d.head["has_loops"] == ["0"],
    "ja_chain_pc_wraps": lambda d: d.is_fault(d.start, SLOT),
    "jmp32_invalid_std": lambda d: d.is_fault(d.start, BAD_OPCODE),
    "xadd_imm_2_std": lambda d: d.is_fault(d.start, BAD_OPCODE),
    "falls_off_the_end": lambda d: d.fault(SLOT),
    # one rung per hashtable (map 0), taken into a lookup that knows its map; the array (map 1)
    # is left to the generic lookup at the chain's end
    "runtime_map_lookup": lambda d: d.rungs("MAP0") == {LOOKUP} and d.rungs("MAP1") == set() and all(
        d.entries[j["next"]]["kind"] == LOOKUP for j in d.find(JEQ_IMM, dst=1, imm="MAP0")),
    "runtime_map_update_delete": _update_delete_chains,
    "update_constant_not_a_map": lambda d: d.fault(BAD_MAP) and not d.find(UPDATE),
    "delete_hashtable": lambda d: d.find(HDELETE, aux=0) and d.head["hupd_maps"] == ["0"],
    "delete_array": lambda d: d.find(LDDW, dst=0, imm=EINVAL) and not d.find(HDELETE) and not d.find(UPDATE),
    # the idiom's path has copies of its own (entries after the enumerated ones); the path that
    # joins it keeps the plain STX
    "counter_alu_is_target": lambda d: d.find(CNT_STORE, aux=0x208, imm="0x1") and d.find(STXDW) and
    len(d.find(ADD64_IMM, dst=7, imm="0x1")) == 2,
    "counter_stx_is_target": lambda d: d.find(CNT_STORE, aux=0x208, imm="0x1") and d.find(STXDW) and
    len(d.find(ADD64_IMM, dst=7, imm="0x1")) == 1,
    "two_loops": _loop_kept(2),
    "loop_head_faults": lambda d: _loop_kept()(d) and d.is_fault(d.find(LOOPCNT)[0]["next"], BAD_OPCODE),
    "loop_count_two_predecessors": lambda d: _loop_kept()(d) and len(
        [e for e in d.entries if e["reached"] and d.entries[e["next"]]["kind"] == LOOPCNT or
         e["kind"] == 0x25 and d.entries[e["target"]]["kind"] == LOOPCNT]) == 2,
    "loop_head_leaves": _loop_kept(),
    "loop_two_decrements": _loop_kept(),
    "loop_decrement_on_one_arm": _loop_kept(),
    "loop_counter_overwritten": _loop_kept(),
    # the count is dropped: its entry is still there, and nothing reaches it
    "loop_intervals": lambda d: _loop_kept(0)(d) and [e for e in d.entries if e["kind"] == LOOPCNT],
    # (a countdown from 3 as well: no count)
    "loop_slot_shapes": lambda d: _loop_kept(0)(d) and len(d.find(CNT_STORE)) == 2 and
    d.head["reads_counters"] == ["0"],
    "loop_xadd_then_load": lambda d: d.err == EOPNOTSUPP and d.head["maps"] == [],
    "readback_2049_stores": lambda d: d.err == EOPNOTSUPP and d.head["ovl_entries"] == ["4098"],
}


def test_edge_programs_translate_to_the_entries_they_are_named_for(native):
    """Every program of the corpus's edges group: its dump holds, reached, the entry the shape is
    there for — the fault codes, DK_CALL_HDELETE, the compare chains' JEQ r1 ladders, the copied
    DK_CNT_STORE, the loop counts kept or dropped — and the refused ones their errno."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import device_code_digest
    import translation_digest
    seen = set()
    for name, err, text in translation_digest.dumps(device_code_digest.corpus(["edges"], 0)):
        name = name[len("edges/"):]
        seen.add(name)
        d = _Dump(err, text)
        assert d.head["err"][0] == str(err) and (err == 0 or err == EOPNOTSUPP), name
        assert EDGES[name](d), "%s:\n%s" % (name, text)
    assert seen == set(EDGES)
