"""sf_eval on the GPU (tests/_eval_child.py, one case per process): eval_epoch's three figures from one pass that stores no
prediction.  Exactness of the integer sum and bit-equality of the SSE against the handle's own forward() on every kernel
family at its smallest edge shapes; nothing else moves; refusals; the Python route (eval_metrics, fit.py)."""
import math

import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_eval_child.py"


def assert_exact(res, outside):
    """eval_sums()[1] == S, eval_sums()[0] is forward()'s double bit for bit, sse8_view() holds S, eval_sums(sync=False)
    leaves the same words.  outside: "both" - some prediction below 0 and some above 1 somewhere in the family (truncation
    toward zero, no clamp); "any" - at least one side (the composed WaveletSiren picture); "none" - the sigmoid of
    FourierNet stays inside (0, 1); "free" - whatever the materialised Feathermap weights give"""
    assert res
    for name, r in res.items():
        print(name, r)
        assert r["sse8"] == r["S"], name
        assert r["eval_sse"] == r["sse"], name
        assert r["view8"] == r["S"], name
        assert r["async8"] == r["S"] and r["async_sse"] == r["sse"] and r["async_returns"] == [None, None], name
        assert r["S"] > 0, name
    below, above = sum(r["below"] for r in res.values()), sum(r["above"] for r in res.values())
    if outside == "both":
        assert below > 0 and above > 0, (below, above)
    elif outside == "any":
        assert below + above > 0
    elif outside == "none":
        assert below == 0 and above == 0


@pytest.mark.parametrize("family,outside,n_shapes", [("k_fwd", "both", 36), ("k_fwd_pipe", "both", 6), ("wide", "both", 4),
                                                     ("fourier", "none", 4), ("wavelet", "any", 3), ("feather", "free", 1)])
def test_sums_are_exact_on_every_kernel_family(tmp_path, family, outside, n_shapes):
    res = run_case(CHILD, family, tmp_path=tmp_path, timeout=120)
    assert len(res) == n_shapes
    assert_exact(res, outside)
    if family == "wavelet":
        assert [r["two_pass"] for r in res.values()] == [False, False, True]


def test_pixel_split_sums_add_up(tmp_path):
    res = run_case(CHILD, "split", tmp_path=tmp_path, timeout=120)
    assert_exact(res, "both")
    assert res["top"]["npix"] == 27 and res["bottom"]["npix"] == 36 and res["whole"]["npix"] == 63
    assert res["top"]["S"] + res["bottom"]["S"] == res["whole"]["S"]
    assert res["top"]["sse8"] + res["bottom"]["sse8"] == res["whole"]["sse8"]


def test_nothing_else_moves(tmp_path):
    """4 sf_step steps with an sf_eval between every two against 4 without: losses, parameters, moments and scratch bytes are
    bitwise equal, and forward() after sf_eval gives the same prediction and SSE"""
    res = run_case(CHILD, "state", tmp_path=tmp_path, timeout=120)
    assert res["plain"]["step"] == 4 and len(res["plain"]["losses"]) == 4
    assert res["with_eval"] == res["plain"]


def test_eval_metrics_figures_and_no_torch_memory(tmp_path):
    r = run_case(CHILD, "metrics", tmp_path=tmp_path, timeout=120)
    print(r)
    assert r["loss"][0] == r["loss"][1] and r["psnr"][0] == r["psnr"][1]
    assert r["psnr8_bits"] == r["psnr8_exact"]
    assert r["psnr8"] == 10 * math.log10(65025 / (r["S"] / r["n"]))
    # an fp32 tree mean over at most 2^26 values and fp32 log10 are off by about 1e-5 dB from the exact figure; ten times that
    assert abs(r["psnr8"] - r["psnr8_epoch"]) <= 1e-4
    assert r["allocated"][1] == r["allocated"][0] and r["peak"][1] == r["peak"][0]


def test_refusals_launch_nothing(tmp_path):
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    print(r)
    INVALID, STATE = -1, -4
    for name in ("render_siren", "render_wide", "render_fourier", "render_wavelet", "render_feather"):
        assert r[name]["rc"] == INVALID and "sf_eval" in r[name]["msg"] and "render handle" in r[name]["msg"], (name, r[name])
        assert r["launches_" + name] == 0
    for name, what in (("no_coords", "sf_set_coords"), ("no_target", "sf_set_target"), ("no_encoding", "sf_set_encoding"),
                       ("wavelet_no_coords", "sf_set_coords"), ("wavelet_no_target", "sf_set_target")):
        assert r[name]["rc"] == STATE and "sf_eval" in r[name]["msg"] and what in r[name]["msg"], (name, r[name])
    assert r["launches_siren"] == 0 and r["launches_fourier"] == 0 and r["launches_wavelet"] == 0
    assert r["ok_siren"]["rc"] == 0


def assert_fit_routes_agree(res, n_evals):
    auto, off = res["auto"], res["off"]
    eight = [k for k in off["result"] if "8bit" in k]
    assert eight and auto["result"].keys() == off["result"].keys()
    for k in off["result"]:
        if k not in eight:
            assert auto["result"][k] == off["result"][k], k
    for k in eight:
        print(k, auto["values"][k], off["values"][k])
        assert abs(auto["values"][k] - off["values"][k]) <= 1e-4, k
    assert auto["model"] == off["model"] and auto.get("container") == off.get("container")
    assert auto["returned_equal_saved"] and off["returned_equal_saved"]
    assert auto["calls"] == {"forward_pred": 0, "eval_sums": n_evals}
    assert off["calls"] == {"forward_pred": n_evals, "eval_sums": 0}


def test_fit_with_quantise_phase_is_the_same_on_both_routes(tmp_path):
    """masking=none quant=kmeans at 32^2, 40 + 20 steps: 2 training evaluations, 2 in the quantise phase, 1 after it"""
    res = run_case(CHILD, "fit_quant", tmp_path=tmp_path, timeout=180)
    assert "container" in res["off"] and "Quant PSNR 8bit" in res["off"]["result"] and "PSNR_8bit" in res["off"]["result"]
    assert_fit_routes_agree(res, 5)


def test_masked_fit_is_the_same_on_both_routes(tmp_path):
    """masking=RigL quant=none, 40 steps: 2 evaluations"""
    res = run_case(CHILD, "fit_masked", tmp_path=tmp_path, timeout=180)
    assert_fit_routes_agree(res, 2)
