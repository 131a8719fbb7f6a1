"""A changed second call never replays a stale captured step (tests/call_sequences.py holds the table).

Per family x mutation x capture mode (HIP graph, launch plan): call A captures the step; the mutation changes one thing of the
pipeline or of the call; call B must be, bit for bit, what a freshly built pipeline in the same state computes EAGERLY -- zero
tolerance is the project's own standard (test_every_pipeline_replays_its_step_as_a_plan: graph == plan == eager on a first call).
A mutation that only changes the contents of static buffers must not cost a capture; undoing the mutation gives call A's result
again.  A stale replay fails an assert here, it does not fault: a wrongly replayed step reads buffers that are still alive (the
packed tensors of before a reload are held until the asserts are done; a scheduler's buffers can only be mistaken for the old ones
where they sit at the old -- live -- addresses)."""
import pytest
import torch

import call_sequences as CS

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("mode", [True, "plan"], ids=["graph", "plan"])
@pytest.mark.parametrize("family,mut", CS.CASES, ids=CS.CASE_IDS)
def test_second_call_after_a_change(family, mut, mode):
    fam = CS.FAMILIES[family]
    A = mut.base(fam.kwargs)
    pipe = fam.build(DEV)
    mut.setup(pipe)
    a = CS.run(pipe, A, mode)
    g = pipe._graph
    keep = CS.hold_packed(pipe)                 # alive until the end of the test
    B = mut(pipe, A)
    b = CS.run(pipe, B, mode)

    oracle = fam.build(DEV)
    mut.setup(oracle)
    want = CS.run(oracle, mut(oracle, A), False)
    assert torch.isfinite(want.float()).all()
    assert not torch.equal(want, a), "the mutation changed nothing: the case cannot tell a stale replay from a fresh capture"
    assert torch.equal(b, want), f"{family} / {mut.name}: the second call is not what a fresh pipeline computes eagerly"
    if mut.expect == "replay":
        assert pipe._graph is g, f"{family} / {mut.name}: a change of buffer contents only must replay the captured step"
    mut.undo(pipe)
    assert torch.equal(CS.run(pipe, A, mode), a), f"{family} / {mut.name}: undone, the first call's result must come back"
    del keep
