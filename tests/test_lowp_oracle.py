"""The twelve 16-bit vectors on the CPU: the reference itself (where its build is present) and our restatement
run_csegment -- the checker that stands in for the reference on the GPU box -- against the stored results."""
import pytest

import lowp_util


@pytest.mark.parametrize("name", lowp_util.names())
def test_reference_reproduces_the_stored_result(oracle, name):
    if not oracle.have_reference():
        pytest.skip("oracle/_ref is absent: the reference tree is not on this machine")
    v = lowp_util.load(name)
    ref = oracle.run_reference(v["class_probs"], v["sameness_probs"], v["spec"]["C"], v["offsets"], *v["opts"])
    assert oracle.masks_equivalent(ref.mask, ref.object_class, v["mask"], v["object_class"])


@pytest.mark.parametrize("name", lowp_util.names())
def test_restatement_equals_the_stored_result(oracle, name):
    v = lowp_util.load(name)
    got = oracle.run_csegment(v["class_probs"], v["sameness_probs"], v["spec"]["C"], v["offsets"], *v["opts"])
    assert oracle.masks_equivalent(got.mask, got.object_class, v["mask"], v["object_class"])
