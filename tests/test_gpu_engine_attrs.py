"""What each of the six engine classes shows a caller, on an MI355X: every public plain attribute and the shapes / dtypes
(or the refusal) of render for each want_u8 / want_pred combination, against tests/golden/engine_attrs.json.  The golden
was written by the same child (tests/_engine_attrs_child.py) on the binding as it stood before its constructors and
prototype tables were merged into one path, so it pins what that merge had to keep."""
import json
import os

import pytest

from _gpu_child import ROOT, run_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_attrs.json")
CLASSES = ["SirenEngine", "RenderEngine", "FourierEngine", "FourierRenderEngine", "WaveletEngine", "WaveletRenderEngine"]


def test_engine_attributes_and_render_outputs(tmp_path):
    got = run_case("_engine_attrs_child.py", "engine_attrs", tmp_path=tmp_path, timeout=60)
    want = json.load(open(GOLDEN))
    assert sorted(got) == sorted(want) == sorted(CLASSES)
    for name in CLASSES:
        g, w = got[name], want[name]
        assert g["class"] == w["class"] and g["bases"] == w["bases"], name
        assert g["attrs"] == w["attrs"], (name, g["attrs"], w["attrs"])
        calls = [k for k in w if k.startswith("render")]
        assert calls and sorted(k for k in g if k.startswith("render")) == sorted(calls), name
        for call in calls:
            assert g[call] == w[call], (name, call, g[call], w[call])
            assert g[call]["u8=0,pred=0"]["raises"] == "ValueError", (name, call)      # asking for neither is refused
    assert got == want
