"""What the models ask of their engine handles, on an MI355X: tests/_binding_trace_child.py drives Siren (bound, re-bound,
masked, re-made for another scratch format / other Adam hyper-parameters / another image size, copied, detached), a padded
Siren, FourierNet, WaveletSiren and FeatherNet in one fresh process and logs every call on every handle plus bool / int
observations of the binding after each step.  tests/golden/binding_trace.json was written by the same child on the binding
as it stood BEFORE models/binding.py (each family with its own copy of the protocol), on an MI355X, so it pins the order and
arguments of the calls that merge had to keep.  No float computed on the device is in the trace: the comparison is exact.
The second half holds the two ways a step runs against each other (the child's step_paths case): train_steps(n) and n
train_epoch calls, live and padded, without and with masks."""
import json
import os

import pytest

from _gpu_child import ROOT, run_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_trace.json")


def test_binding_call_trace_equals_the_recorded_one(tmp_path):
    got = run_case("_binding_trace_child.py", "binding_trace", tmp_path=tmp_path, timeout=120)
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want) == ["A", "B", "C", "D", "E"]
    for name in sorted(want):
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (name, i, g, w)
        assert len(got[name]) == len(want[name]), (name, len(got[name]), len(want[name]))
    assert got == want


STEP_CASES = [f"{hidden}_{mask}" for hidden in (32, 20) for mask in ("none", "dense", "sparse")]


@pytest.fixture(scope="module")
def step_paths(tmp_path_factory):
    """train_steps(n = 4) against four train_epoch calls on a deep copy, all six cases from one child: Siren depth 3 on 16 x 16,
    lr 3e-4 halved after every second step; live (32) and padded (20 -> 32) state; no mask, RigL at density 0.5 with dense
    gradients and with sparse ones"""
    got = run_case("_binding_trace_child.py", "step_paths", tmp_path=tmp_path_factory.mktemp("step_paths"), timeout=120)
    assert sorted(got) == sorted(STEP_CASES)
    return got


@pytest.mark.parametrize("case", STEP_CASES)
def test_train_steps_leaves_what_train_epochs_leave_on_the_path_the_case_must_take(step_paths, case):
    """The two ways a step runs - train_epoch n times, train_steps(n) as one sf_step call - leave the same behind, compared
    exactly: every parameter, the optimiser's step counts, the learning rate, the scheduler's epoch, the mask's step count and
    prune rate.  One sf_step call must serve exactly the live cases whose mask needs no host work between two steps; every
    other case must run step by step."""
    r, (hidden, tag) = step_paths[case], case.split("_")
    one, many = r["train_steps"], r["train_epochs"]
    print(case, r)
    assert r["live"] is (hidden == "32")
    assert all(r["params_equal"]) and len(r["params_equal"]) == 6, r["params_equal"]
    assert one["optim_step"] == many["optim_step"] == [4.0] * 6
    assert one["lr"] == many["lr"] == 3e-4 * 0.5 * 0.5 and one["last_epoch"] == many["last_epoch"] == 4
    assert one["mask_step"] == many["mask_step"] == (None if tag == "none" else 4)
    assert one["prune_rate"] == many["prune_rate"] and (one["prune_rate"] is None) == (tag == "none")
    assert r["masks_equal"] and (tag == "none" or r["density"] < 0.9)
    bulk = r["live"] and tag != "sparse"
    assert r["calls"][0] == ({"step": 1, "forward_backward": 0} if bulk else {"step": 0, "forward_backward": 4}), r["calls"]
    assert r["calls"][1] == {"step": 0, "forward_backward": 4}, r["calls"]


@pytest.mark.parametrize("case", STEP_CASES)
def test_train_steps_returns_the_losses_of_train_epochs(step_paths, case):
    """... and the four losses they return are the same numbers (==): a loss is a float's value on both paths, sf_step's
    `(float)(sse / n)` in the C ABI and train_epoch's own rounding of the same quotient (before train_epoch rounded, the two
    sf_step cases differed from it by up to 2.48e-9, a third of the float spacing at 0.064)."""
    one, many = step_paths[case]["train_steps"]["losses"], step_paths[case]["train_epochs"]["losses"]
    print(case, one, many)
    assert len(one) == 4 and one == many, (one, many)
