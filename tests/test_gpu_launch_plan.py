"""The launch plan of the engine is pinned: which kernels a pass launches, how often, and the flops / bytes each launch is
charged, for every launch path.  The cases of tests/_launch_plan_child.py run in one child process and are compared with
tests/golden/launch_plan.json, which was recorded by the same child against the library of the commit before the launch
layer was folded into one launcher (SIREN_FIT_LIB=<that build> python tests/_launch_plan_child.py launch_plan OUT.json; the
"cases" -> name -> "plan" part of OUT.json is the golden).

Cases (all eager, profiling on, one sf_forward + one sf_forward_backward, render handles one sf_render):
  SIREN on 40 x 52 (2080 pixels, chunk_pixels 1024: two full chunks and a ragged one): hidden 32 / 64 / 128 / 256, depth
    2 / 3 / 4, scratch formats 16, 12 and 8 at f16 and format 16 at bf16
  SIREN 256x4 on 300 x 300, formats 8 and 16, default chunk (352 pixel groups: the persistent-grid clamps bind)
  wide path 512x3 at formats 16, 12, 8 and 1024x3 at format 12, on 40 x 52, chunk_pixels 1024
  FourierNet hidden 32 and 256, three Linear layers, map_size 64 and 128 on 40 x 52, chunk_pixels 1024.  The creator takes
    map_size 64 .. 512, so k_ff_dw's NI = 2 and 4 come from layer 0 at map_size 64 / 128 (and 4 from the 256-wide layers);
    NI = 1 comes from the 32-wide layers of the hidden-32 cases
  WaveletSiren 64x3 at H = 2 (the smallest image the creator accepts; its 9 coefficients are one chunk whatever
    chunk_pixels is) and, for the two-pass path (k_wv_inject), at H = 30 with chunk_pixels 256: the smallest even H whose
    17 x 17 coefficient grid passes the smallest chunk of 256
  render handles: sf_render_create 64x3 and 256x4, sf_fourier_render_create 64, sf_wavelet_render_create 64x3 (H = 30);
    at 16 bits per sample sf_render16 on the 64x3 handle and sf_wavelet_render16 of a pixel window whose coefficient
    window starts inside the grid and is narrower than it (golden: the library before the passes shared one chunk loop)
  wide render handles (sf_wide_render_create) on 40 x 52, chunk_pixels 1024: 512x3 at 8 bits per sample and 1024x4 at 16,
    where the two activation planes wrap (golden: the library before the wide forward and the render loop shared one walk)
  Feathermap: an attached 64x3 handle, with one sf_adam_step after the two passes

One more case runs with profiling off: sf_step with three learning rates and want_loss on a WaveletSiren 64x3 handle at
H = 2, eagerly and with set_graph_replay(True), from the same parameters.  The sub-handles launch through the handle's own
launch context, so a captured step puts their kernels on the capturing stream.  The three losses and the sha256 of the
parameters of both runs equal, exactly, what the library of the commit before the host split recorded (golden key
"wavelet_step_64x3_H2", through the same child and SIREN_FIT_LIB)."""
import json
import os

import pytest

from _gpu_child import ROOT, run_case

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan.json")
REL = 1e-12      # flops / bytes are host doubles: only the order of a sum may move them


STEP_KEY = "wavelet_step_64x3_H2"


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    """the one run of the child that both tests read"""
    return run_case("_launch_plan_child.py", "launch_plan", tmp_path=tmp_path_factory.mktemp("launch_plan"), timeout=60)


def test_launch_plan_matches_golden(child):
    got = {name: c["plan"] for name, c in child["cases"].items()}
    want = json.load(open(GOLDEN))
    del want[STEP_KEY]
    assert sorted(got) == sorted(want)
    bad = []
    for name in sorted(want):
        if sorted(got[name]) != sorted(want[name]):
            bad.append((name, "kernels", sorted(got[name]), sorted(want[name])))
            continue
        for k, w in want[name].items():
            g = got[name][k]
            if g["launches"] != w["launches"]:
                bad.append((name, k, "launches", g["launches"], w["launches"]))
            for f in ("flops_per_launch", "bytes_per_launch"):
                if abs(g[f] - w[f]) > REL * abs(w[f]):
                    bad.append((name, k, f, g[f], w[f]))
    assert not bad, bad[:20]


def test_wavelet_step_replay_equals_eager_and_golden(child):
    want = json.load(open(GOLDEN))[STEP_KEY]
    got = child["wavelet_step"]
    print("eager", got["eager"], "replay", got["replay"], "golden", want)
    assert len(want["losses"]) == 3
    assert got["replay"] == got["eager"]
    assert got["eager"] == want
