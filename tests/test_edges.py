"""Every opcode at edge operands, on the CPU (tests/edgeprogs.py; the device runs the same
programs in tests/test_gpu_edges.py).

Ground truth under reference semantics is tests/golden/edges/edges.npz: the GENUINE reference's
r0 and packet bytes for every case of edgeprogs.build(SEM_REFERENCE) (tools/gen_golden.py --only
edges).  The oracle, ebpf_prog_run (the CPU path) and edgeprogs' big-int model are each compared
with it; that proves the model where truth exists.  Standard semantics has no reference: there
the model, written from the description of EBPF_SEM_STANDARD, is the expectation for the oracle
(semantics=1) and the CPU path.  All comparisons are exact integer equality.

Division by zero: the reference crashes, so the fixture's DIV and MOD cases leave those operands
out and edgeprogs.build_div0 holds the programs over the full operand sets.  The rule checked
here: a packet faults with EBPF_FAULT_DIV_ZERO exactly when its divisor (the low 32 bits for a
32-bit op) is zero, and every other packet gives the fixture's value for the same operands;
under standard semantics DIV by zero gives 0 and MOD by zero dst (truncated for a 32-bit op)."""
import os

import numpy as np
import pytest

import edgeprogs
import goldens
import pyoracle

REF, STD = edgeprogs.SEM_REFERENCE, edgeprogs.SEM_STANDARD
EDGES = os.path.join(goldens.GOLDEN_DIR, "edges", "edges.npz")
GROUPS = edgeprogs.GROUPS
# what the device tests run has to compile (variant 0 must not fall back to the interpreter)
COMPILED_GROUPS = ["folded", "const_src", "const_both", "same_reg", "narrow", "stores",
                   "single_reg", "div0"]

_cache = {}


def fixture():
    """name -> goldens.Case of the committed fixture (loaded once, never modified)."""
    if "fx" not in _cache:
        _cache["fx"] = {c.name: c for c in goldens.load(EDGES)}
    return _cache["fx"]


def cases(sem, group):
    if group == "div0":
        return edgeprogs.build_div0(sem)
    if group == "single_reg":   # the `_reg` forms over E×E
        return [c for c in edgeprogs.build(sem) if c.group == "single" and c.count > 28]
    return [c for c in edgeprogs.build(sem) if c.group == group]


def describe(case, i, got, want, what="r0"):
    a, b = case.operands[i]
    return "%s: packet %d (a=%#x b=%#x) %s got %#x want %#x" % (case.name, i, a, b, what,
                                                                 int(got), int(want))


def first_mismatch(case, got, want, what="r0"):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    return describe(case, bad[0], got[bad[0]], want[bad[0]], what) if len(bad) else None


def div0_reference_expectation(case):
    """(r0, faults) of a div0 case under reference semantics, from the rule in this module's
    docstring and the fixture; nothing here comes from an implementation."""
    twin = edgeprogs.div0_twin(case.name)
    known = {}
    if twin is not None:
        t = next(c for c in edgeprogs.build(REF) if c.name == twin)
        known = dict(zip(t.operands, fixture()[twin].expect_r0))
    r0 = np.zeros(case.count, dtype=np.uint64)
    faults = np.zeros(case.count, dtype=np.uint8)
    for i, (a, b) in enumerate(case.operands):
        s, width = edgeprogs.div0_divisor(case.name, a, b)
        if (s & 0xffffffff if width == 32 else s) == 0:
            faults[i] = 2        # EBPF_FAULT_DIV_ZERO; a faulted packet's result is 0
        else:
            r0[i] = known[(a, b)]
    return r0, faults


def cpu_path(native, env, case):
    """ebpf_prog_run over the case's packets, one call each: (r0, packets after)."""
    p = native.Prog(env, case.code)
    try:
        if case.sem == STD:
            p.set_semantics(native.SEM_STANDARD)
        pk = case.packets(64)
        r0 = np.zeros(case.count, dtype=np.uint64)
        for i in range(case.count):
            r, raw = p.run_cpu(pk[i].tobytes())
            r0[i] = r
            pk[i] = np.frombuffer(raw, dtype=np.uint8)
        return r0, pk
    finally:
        p.destroy()


# ------------------------------------------------------------------------- fixture = generator

def test_fixture_is_what_edgeprogs_builds():
    """Names, code bytes and packets of the fixture equal the module's today, case for case, and
    so does the case count of every group: generator and fixture cannot drift apart."""
    built = edgeprogs.build(REF)
    fx = fixture()
    assert [c.name for c in built] == list(fx)
    for c in built:
        f = fx[c.name]
        assert f.code == c.code, c.name
        assert f.count == c.count and f.stride == 64, c.name
        assert np.array_equal(f.data, c.packets(64).reshape(-1)), c.name
        assert len(f.expect_r0) == c.count and len(f.expect_data) == 64 * c.count, c.name
    for g in GROUPS:
        n = sum(1 for name in fx if name.split("/")[0] == g)
        assert n == len(cases(REF, g)) > 0, g
    assert os.path.getsize(EDGES) < 1 << 20
    assert EDGES not in goldens.all_golden_files()


def test_operand_sets_are_complete():
    """The sets the issue fixed: 28 operands (784 pairs), 15 immediates; 28 resp. 112 pairs with
    a zero divisor left out of the 64- resp. 32-bit DIV and MOD cases."""
    assert len(edgeprogs.E) == 28 and len(edgeprogs.EE) == 784 and len(edgeprogs.IMM) == 15
    by = {c.name: c for c in edgeprogs.build(REF)}
    for op in ("div", "mod"):
        assert by["single/%s64_reg" % op].count == 784 - 28
        assert by["single/%s_reg" % op].count == 784 - 112
    assert by["single/add_reg"].count == by["single/jsgt_reg"].count == 784
    for c in edgeprogs.build_div0(REF):
        assert c.count in (28, 784)


# ------------------------------------------------------------------------- reference semantics

@pytest.mark.parametrize("group", GROUPS)
def test_oracle_against_fixture(group):
    for c in cases(REF, group):
        f = fixture()[c.name]
        r0, faults, after, _ = pyoracle.OracleProgram(c.code).run(f.data, c.count, 64)
        assert not faults.any(), (c.name, int(np.flatnonzero(faults)[0]))
        assert first_mismatch(c, r0, f.expect_r0) is None, first_mismatch(c, r0, f.expect_r0)
        assert np.array_equal(after, f.expect_data), c.name


@pytest.mark.parametrize("group", GROUPS)
def test_cpu_path_against_fixture(native, env, group):
    for c in cases(REF, group):
        f = fixture()[c.name]
        r0, after = cpu_path(native, env, c)
        assert first_mismatch(c, r0, f.expect_r0) is None, first_mismatch(c, r0, f.expect_r0)
        assert np.array_equal(after.reshape(-1), f.expect_data), c.name


@pytest.mark.parametrize("group", GROUPS)
def test_reference_model_against_fixture(group):
    """The big-int model on the semantics that have ground truth (`single` is the group that
    proves it op by op; the others prove the folds built from it)."""
    for c in cases(REF, group):
        f = fixture()[c.name]
        r0, faults, after = c.expect(64)
        assert not faults.any(), c.name
        assert first_mismatch(c, r0, f.expect_r0) is None, first_mismatch(c, r0, f.expect_r0)
        assert np.array_equal(after.reshape(-1), f.expect_data), c.name


def test_oracle_faults_on_division_by_zero():
    for c in edgeprogs.build_div0(REF):
        want, wf = div0_reference_expectation(c)
        r0, faults, after, _ = pyoracle.OracleProgram(c.code).run(c.packets(64).reshape(-1),
                                                                  c.count, 64)
        assert first_mismatch(c, faults, wf, "fault") is None, first_mismatch(c, faults, wf, "fault")
        assert first_mismatch(c, r0, want) is None, first_mismatch(c, r0, want)
        assert np.array_equal(after, c.packets(64).reshape(-1)), c.name
        # (and the model states the same rule)
        mr, mf, _ = c.expect(64)
        assert np.array_equal(mr, want) and np.array_equal(mf, wf), c.name


# ------------------------------------------------------------------------- standard semantics

@pytest.mark.parametrize("group", GROUPS + ["div0"])
def test_standard_model_against_oracle_and_cpu_path(native, env, group):
    cs = cases(STD, group)
    if group == "single":
        assert sum(1 for c in cs if "jmp32_" in c.name) == 11 * (1 + 15)
    for c in cs:
        want, wf, wafter = c.expect(64)
        assert not wf.any(), c.name      # standard semantics defines division by zero
        r0, faults, after, _ = pyoracle.OracleProgram(c.code, semantics=1).run(
            c.packets(64).reshape(-1), c.count, 64)
        assert not faults.any(), c.name
        assert first_mismatch(c, r0, want) is None, "oracle " + first_mismatch(c, r0, want)
        assert np.array_equal(after, wafter.reshape(-1)), c.name
        r0, after = cpu_path(native, env, c)
        assert first_mismatch(c, r0, want) is None, "cpu path " + first_mismatch(c, r0, want)
        assert np.array_equal(after, wafter), c.name


def test_standard_division_by_zero_values():
    """DIV by zero gives 0 and MOD by zero dst, truncated for the 32-bit ops: spelt out on two
    operands, so that the rule stands here and not only in the model."""
    a = 0xfedcba9876543210
    assert edgeprogs.model_alu(STD, "div", 64, a, 0) == (0, 0)
    assert edgeprogs.model_alu(STD, "mod", 64, a, 0) == (a, 0)
    assert edgeprogs.model_alu(STD, "div", 32, a, 1 << 32) == (0, 0)
    assert edgeprogs.model_alu(STD, "mod", 32, a, 1 << 32) == (0x76543210, 0)
    assert edgeprogs.model_alu(REF, "mod", 32, a, 1 << 32) == (0, 2)


# ------------------------------------------------------------------------- the compiled path

@pytest.mark.parametrize("sem", [REF, STD], ids=["reference", "standard"])
@pytest.mark.parametrize("group", COMPILED_GROUPS)
def test_programs_compile_for_both_layouts(native, env, group, sem):
    """No GPU needed: ebpf_prog_device_code gives the gfx950 code of either packet layout, or
    E2BIG for a program variant 0 would hand to the interpreter."""
    for c in cases(sem, group):
        p = native.Prog(env, c.code)
        try:
            if sem == STD:
                p.set_semantics(native.SEM_STANDARD)
            for lay in (0, 1):
                assert len(p.device_code(lay)) > 0, (c.name, lay)
        finally:
            p.destroy()
