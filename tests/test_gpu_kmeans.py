"""sf_kmeans_fit on an MI355X (csrc/siren_kmeans.hip): the k-means quantiser as five kernels without a host read.  One case of
tests/_kmeans_child.py per child process; the contract the kernels are held to is tests/_kmeans_ref.py, which
tests/test_kmeans_host.py holds against float64, the torch mirror and the reference's fixtures on the CPU.  Every comparison
with the restatement here is bit equality: nothing has a tolerance."""
import json
import math

import pytest

import _kmeans_child as child  # (the row groups only: nothing touches the device at import)
from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_kmeans_child.py"
NO_DIFF = {"centroids": 0, "new_weight": 0, "centres": 0, "labels": 0, "n_centroids": 0}


@pytest.mark.parametrize("group", range(len(child.GROUPS)), ids=["small_rows", "bits9_limit", "large_rows"])
def test_abi_against_the_restatement(group, tmp_path):
    """The rows of the case table (tests/_kmeans_ref.py: TABLE, make_input, row_condition) through SirenEngine.kmeans_fit with
    the torch.linspace guess of find_centroids_native: all five Lloyd iterations on a ragged last block, a stop at the third,
    empty bins at K = 255, K = 511 above the 256 threads that load the centres, n < K, a constant layer, a +c / -c pair,
    exact float32 distance ties, values down to subnormals, -0.0 weights, the second sweep of the grid-stride loop, one
    non-zero weight; then a layer without any.  Labels, centroids, new weights and the Lloyd centres left in centers_dev
    (floats as int32 views: -0.0 counts), the centroid count and the zero padding equal the restatement's bit for bit, a
    second call gives the same bits, and each row's condition holds on the input the device saw."""
    r = run_case(CHILD, "abi", str(group), tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert list(r["rows"]) == child.GROUPS[group]
    for name, c in r["rows"].items():
        assert c["diff"] == NO_DIFF, (name, c["diff"])
        assert c["repeat"] and c["padding_zero"], name
        assert c["condition"] is None, c["condition"]
        assert c["guess_as_on_the_cpu"], name                      # torch.linspace gives the bits of the mirror's guess
        assert c["n_centroids"] == c["ref_n_centroids"] <= c["K"] + 1
        assert c["minus_zero_out"] == 0, name                      # a zero weight of either sign gets the centroid +0.0
    rows = r["rows"]
    if "stops_at_three" in rows:
        assert rows["stops_at_three"]["iterations"] == 3
        assert rows["stops_at_three"]["same_at_3"] and not rows["stops_at_three"]["same_at_2"]
        assert rows["five_iterations"]["iterations"] == 5 and rows["five_iterations"]["n"] % 256 == 1
    if "grid_stride" in rows:
        assert rows["grid_stride"]["n"] == 4 * r["cus"] * 256 + 257
        assert rows["pruned_minus_zero"]["minus_zero_in"] >= 1000
    z = r["all_zero"]
    assert z["empty"] and not z["guess_finite"]
    assert z["diff"] == NO_DIFF and z["n_centroids"] == 1 and z["labels_nonzero"] == 0, z
    assert not z["new_weight_bits_set"] and not z["centroid_bits_set"], z


def test_raw_abi_iteration_limits_tolerances_and_optional_outputs(tmp_path):
    """lib.sf_kmeans_fit on the five_iterations input: iter_limit 0 finishes on the guess itself, iter_limit 1, tol 0 never
    stops (also on the input that would stop at three), tol 1e30 stops after one iteration; with labels_dev, new_weight_dev
    and n_centroids_dev NULL in turn and all three NULL the outputs that remain equal the full call's and the restatement's,
    and the buffers that were not passed keep their sentinel; a centroids_cap above K + 1 is zero padded to the cap.  A layer
    without a non-zero weight at iter_limit 0: the NaN guess reaches k_km_finish as it is (with an iteration, k_km_update
    has written 0 for every empty bin before), and the one centroid +0.0 still comes out."""
    r = run_case(CHILD, "abi_raw", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    for name, c in r.items():
        assert c["rc"] == 0, (name, c)
        assert set(c["diff"].values()) == {0}, (name, c["diff"])
    assert r["full"]["iterations"] == 5 and r["tol_0"]["iterations"] == 5 and r["tol_0_where_it_would_stop"]["iterations"] == 5
    assert r["iter_limit_0"]["iterations"] == 0 and r["iter_limit_0"]["centres_are_the_guess"]
    assert r["iter_limit_1"]["iterations"] == 1 and r["tol_1e30"]["iterations"] == 1
    assert not r["full"]["centres_are_the_guess"]
    assert r["all_zero_iter_limit_0"]["empty"] and r["all_zero_iter_limit_0"]["n_centroids"] == 1
    for name, missing in (("no_labels", {"labels"}), ("no_new_weight", {"new_weight"}), ("no_n_centroids", {"n_centroids"}),
                          ("centroids_only", {"labels", "new_weight", "n_centroids"})):
        assert set(r[name]["outputs"]) == set(NO_DIFF) - missing and set(r[name]["diff"]) == set(NO_DIFF) - missing
        assert r[name]["as_full"] and r[name]["null_outputs_untouched"], name
    assert r["cap_larger"]["diff"]["centroids"] == 0 and r["cap_larger"]["null_outputs_untouched"]


def test_used_workspace_gives_the_bits_of_a_fresh_one(tmp_path):
    """one handle, in this order: K = 511 on 70 001 weights, one non-zero weight at K = 3, a layer without a non-zero weight,
    five iterations at K = 31.  Each result equals the same call on a fresh handle and the restatement bit for bit: no stale
    sums, counts, sorted list, centroid count or done / empty flag"""
    r = run_case(CHILD, "reuse", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert list(r) == ["bits9_limit", "single_weight", "all_zero", "five_iterations"]
    for name, c in r.items():
        assert c["as_fresh"] and c["diff"] == NO_DIFF, (name, c)
    assert r["all_zero"]["n_centroids"] == 1 and r["single_weight"]["n_centroids"] == 2


def test_refusals_launch_nothing(tmp_path):
    """K = 0, K = 1 (one centre does not bracket the weights: the fixed-point unit rests on that), K = 512, n <= 0,
    centroids_cap = K, iter_limit = -1 and a null w_dev / centers_dev / centroids_dev / handle return SF_ERR_INVALID with a
    message, a render handle its refusal; the profile counters stay at zero and no buffer is written.  K = 2 and K = 511 run."""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=120)
    print(json.dumps(r, indent=1))
    for name in ("K_0", "K_1", "K_512", "n_0", "n_negative", "cap_K", "iter_limit_negative", "null_w", "null_centers",
                 "null_centroids", "null_handle", "render"):
        assert r[name]["rc"] == -1 and r[name]["msg"], (name, r[name])
    for name in ("K_0", "K_1", "K_512", "n_0", "cap_K", "iter_limit_negative", "render"):
        assert "sf_kmeans_fit" in r[name]["msg"], (name, r[name])
    assert "render handle" in r["render"]["msg"]
    assert r["launches_after_refusals"] == {"train": 0, "render": 0}
    assert r["outputs_untouched"] and r["guess_untouched"]
    assert r["ok_K_2"]["rc"] == 0 and r["ok_K_511"]["rc"] == 0 and r["ok_wrote"]


def test_quantise_phase_over_a_layer_without_a_non_zero_weight(tmp_path):
    """fit_one, masking=none quant=kmeans, 64x4 on a 32x32 synthetic image, 20 steps and 3 of the quantise phase, with all of
    layers.1.linear.weight zero before the phase and before each of its passes (what a mask that pruned the layer away
    keeps): the run finishes, every label of the layer is 0, its saved codebook is [0.], the PSNR in result.json is finite"""
    r = run_case(CHILD, "phase", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["codebook"] == [0.0] and r["codebook_sign_bits"] == 0
    assert r["labels_nonzero"] == 0 and r["labels_shape"] == [64, 64]
    assert math.isfinite(r["PSNR"]) and math.isfinite(r["quant_PSNR"])
    assert 1 < r["other_layer_codebook"] <= 256 and r["other_layer_finite"]
