"""Every opcode at edge operands on the device: the compiled code (variant 0), the portable HIP
interpreter (1) and the assembly interpreter (2), each in the staged layout (64-B packets) and
the general one (72-B stride, the same 16 operand bytes in front), under both instruction
semantics.  The programs are tests/edgeprogs.py's `folded`, `const_src`, `const_both`,
`same_reg`, `narrow`, `stores` and `div0` groups and the `_reg` forms of `single`, over batches
of 28 and 784 packets (a ragged last wave).

r0, fault codes and the packet bytes after the batch are compared for exact equality with the
committed fixture of the GENUINE reference (tests/golden/edges/edges.npz) under reference
semantics, and with edgeprogs' big-int model under standard semantics (tests/test_edges.py
proves that model against the fixture where the semantics agree, and against the oracle and
the CPU path).  Division by zero under reference semantics follows the rule stated in
tests/test_edges.py: EBPF_FAULT_DIV_ZERO exactly where the divisor is zero, the fixture's value
on every other packet of the same waves."""
import numpy as np
import pytest

import edgeprogs
import test_edges as cpu

pytestmark = pytest.mark.gpu

REF, STD = edgeprogs.SEM_REFERENCE, edgeprogs.SEM_STANDARD
_want = {}


def expectation(case, stride):
    """(r0, faults, packets after as (count, stride)), computed once per case and stride."""
    key = (case.sem, case.name, stride)
    if key not in _want:
        if case.sem == STD:
            w = case.expect(stride)
        else:
            after = case.packets(stride)
            if case.group == "div0":     # (no program of that group stores)
                r0, faults = cpu.div0_reference_expectation(case)
            else:
                f = cpu.fixture()[case.name]
                r0, faults = f.expect_r0, np.zeros(case.count, dtype=np.uint8)
                after[:, :64] = f.expect_data.reshape(case.count, 64)
            w = (r0, faults, after)
        for x in w:
            x.setflags(write=False)
        _want[key] = w
    return _want[key]


def run(native, env, case, stride, variant):
    p = native.Prog(env, case.code)
    try:
        if case.sem == STD:
            p.set_semantics(native.SEM_STANDARD)
        native.set_variant(variant)
        data = np.ascontiguousarray(case.packets(stride).reshape(-1))
        ret, faults, _ = p.run_batch(data, case.count, stride)
        return ret, faults, data.reshape(case.count, stride), p.exec_info(0)
    finally:
        native.set_variant(0)
        p.destroy()


@pytest.mark.parametrize("sem", [REF, STD], ids=["reference", "standard"])
@pytest.mark.parametrize("stride", [64, 72], ids=["staged", "general"])
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_edges_on_device(gpu, env, variant, stride, sem):
    """332 (reference) or 475 (standard) programs a test: 1.3 to 2.3 s on an MI355X for
    variant 0, which compiles each of them, under 0.1 s for the interpreters."""
    bad = []
    for c in [c for group in cpu.COMPILED_GROUPS for c in cpu.cases(sem, group)]:
        want, wf, wafter = expectation(c, stride)
        got, gf, after, (ran, lay, _, _) = run(gpu, env, c, stride, variant)
        # what the launch ran, or the path under test was not what got tested (variant 0 hands
        # a program too large to compile to the interpreter); the HIP interpreter has one
        # kernel for every batch, which reports layout 0
        staged = variant != 1 and stride == 64 and not c.general_only
        assert (ran, lay) == (("compiled", "hip", "interpreter")[variant], 1 if staged else 0), \
            (c.name, ran, lay)
        msg = cpu.first_mismatch(c, gf, wf, "fault") or cpu.first_mismatch(c, got, want)
        if msg is None and not np.array_equal(after, wafter):
            i = int(np.flatnonzero((after != wafter).any(axis=1))[0])
            msg = cpu.describe(c, i, int.from_bytes(after[i, 16:24].tobytes(), "little"),
                               int.from_bytes(wafter[i, 16:24].tobytes(), "little"),
                               "packet bytes 16..23 (or others) after")
        if msg is not None:
            bad.append(msg + (" -- to find the operand run: " + c.hint if c.hint else ""))
    assert not bad, "%d programs differ:\n%s" % (len(bad), "\n".join(bad[:20]))
