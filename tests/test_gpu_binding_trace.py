"""What the models ask of their engine handles, on an MI355X: tests/_binding_trace_child.py drives Siren (bound, re-bound,
masked, re-made for another scratch format / other Adam hyper-parameters / another image size, copied, detached), a padded
Siren, FourierNet, WaveletSiren and FeatherNet in one fresh process and logs every call on every handle plus bool / int
observations of the binding after each step.  tests/golden/binding_trace.json was written by the same child on the binding
as it stood BEFORE models/binding.py (each family with its own copy of the protocol), on an MI355X, so it pins the order and
arguments of the calls that merge had to keep.  No float computed on the device is in the trace: the comparison is exact."""
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
