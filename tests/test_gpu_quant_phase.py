"""The quantise phase on an MI355X (csrc/siren_quant.hip, quant_host.hip): sf_quant_pass / sf_quant_nudge / sf_quant_step.  One
case of tests/_quant_phase_child.py per child process.  The contract is tests/_kmeans_ref.py (the Lloyd iterations, the
centroids, the labels) with tests/_quant_phase_ref.py (the guess, the nudge), which tests/test_quant_phase_host.py holds
against exact arithmetic on the CPU.  Every comparison here is bit equality unless a bound is named."""
import json

import pytest

import _quant_phase_child as child  # (the shape table only: nothing touches the device at import)
from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_quant_phase_child.py"
NO_DIFF = {"centroids": 0, "new_weight": 0, "centres": 0, "labels": 0, "n_centroids": 0}
ITER_LIMIT = 5
PASS_LAUNCHES = 3 + 2 * ITER_LIMIT


def test_guess_gives_the_bits_of_torch_linspace(tmp_path):
    """k_kmq_guess against torch.linspace on the device at K = 3, 15, 31, 255, 511: the end pairs of the k-means case table
    plus 1 000 seeded pairs (min == max, ends of opposite sign, subnormal spans among them), 16 layers per launch.  No entry
    differs - ATen's multiply-add is contracted, the kernel's form is fma - and the kernel equals the numpy restatement.  A layer without a
    non-zero weight gets non-finite ends, as torch.linspace(inf, -inf) has, and with them the empty call."""
    r = run_case(CHILD, "guess", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["pairs"] >= 1000 and sorted(r["K"], key=int) == ["3", "15", "31", "255", "511"]
    for K, c in r["K"].items():
        assert c["entries"] == r["pairs"] * int(K)
        assert c["kernel_vs_torch"] == 0, (K, c)
        assert c["kernel_vs_restatement"] == 0, (K, c)
    e = r["empty"]
    assert not e["ends_finite"] and not e["torch_ends_finite"]
    assert e["n_centroids"] == 1 and e["labels_nonzero"] == 0 and not e["weight_bits_set"] and not e["centroid_bits_set"], e


@pytest.mark.parametrize("name", sorted(child.pass_shapes()))
def test_pass_against_the_restatement(name, tmp_path):
    """sf_quant_pass on one handle, every listed layer in the same launches, against the restatement layer by layer: labels,
    centroids with their zero padding, counts, the Lloyd centres and the codebook weights written into params; what is not a
    listed weight stays; a second call on the same handle gives the same bits; the per-layer sf_kmeans_fit gives them too.
    64x4 with every layer at bits 4 and 8 (128, 4 096, 4 096 and 192 weights, n < K at bits 8), 32x3 at bits 9 (K = 511), a layer
    of zeros between two others (its empty flag is its own), a 40 % pruned layer with -0.0 entries, 512x3 at bits 8 (262 144
    weights: the grid-stride walk), and a layer that stops at the third iteration beside one that runs all five."""
    r = run_case(CHILD, "pass", name, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    hidden, depth, bits, layers, special = child.pass_shapes()[name]
    assert [int(l) for l in r["layers"]] == layers and r["other_params_untouched"]
    for l, c in r["layers"].items():
        assert c["diff"] == NO_DIFF, (l, c["diff"])
        assert c["repeat"] and c["padding_zero"] and c["as_single_call"], (l, c)
        assert c["minus_zero_out"] == 0, l
    if name == "64x4_bits8":
        assert r["n"] == [128, 4096, 4096, 192] and r["K"] == 255
    if name == "32x3_bits9":
        assert r["K"] == 511 and 1024 in r["n"]
    if special == "zero":
        z = r["layers"]["1"]
        assert z["empty"] and z["n_centroids"] == 1
        assert not r["layers"]["0"]["empty"] and not r["layers"]["2"]["empty"] and r["layers"]["2"]["n_centroids"] > 1
    if special == "pruned":
        assert r["layers"]["1"]["minus_zero_in"] >= 100
    if special == "stops":
        assert r["layers"]["1"]["iterations"] == 3 and r["layers"]["2"]["iterations"] == 5
    if name == "512x3_bits8":
        assert 262144 in r["n"]


def test_nudge_is_the_restatement_and_within_the_bound_of_the_host_path(tmp_path):
    """sf_quant_nudge on four layers at once - one of them empty (one centroid), one with all gradients zero (a -0.0 among
    them), one with gradients far below the unit of the sums - equals the restatement bit for bit and is the same on a second
    run; it and the host path's scatter_add_ both lie within lr * (n_k * 2^-24 * sum|g_i| + two float roundings) of the
    exact float64 result (tests/_quant_phase_ref.nudge_bound, derived there)."""
    r = run_case(CHILD, "nudge", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert sorted(r["layers"]) == ["0", "1", "2", "3"]
    for l, c in r["layers"].items():
        assert c["diff"] == 0 and c["repeat"], (l, c)
        assert c["device_over_bound"] <= 0 and c["host_over_bound"] <= 0, (l, c)
    assert r["layers"]["3"]["moved"] == 0 and r["layers"]["1"]["moved"] > 100


@pytest.mark.parametrize("masked", ["dense", "masked"])
def test_step_equals_the_step_by_step_path(masked, tmp_path):
    """64x4 on 32x32 at bits 8, 12 steps with an eval pass after steps 4, 8 and 12, both routes from one state: train_epoch
    with quant.device_phase off against train_steps in chunks of 4, which is sf_quant_step.  All 12 losses, the three eval
    losses, params, exp_avg, exp_avg_sq, the labels and the centroids after the last eval are equal bit for bit; with a mask
    of density 0.5 on the copy's engine every pruned weight is still exactly 0."""
    r = run_case(CHILD, "step", masked, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["plan"] and not r["host_plan"]
    assert len(r["losses"]["host"]) == len(r["losses"]["device"]) == 12
    assert r["losses_equal"] and r["evals_equal"]
    assert all(v == 0 for v in r["diff"].values()), r["diff"]
    assert {"params", "exp_avg", "exp_avg_sq", "labels0", "labels1", "centroids0", "centroids1"} <= set(r["diff"])
    assert r["adam_steps"] == [12, 12] and r["opt_steps"] == [12.0, 12.0] and r["lr"][0] == r["lr"][1]
    if masked == "masked":
        assert r["pruned"] > 3000 and r["pruned_nonzero"] == 0


def test_state_right_after_a_train_step(tmp_path):
    """No eval after the step: the labels equal the step-by-step path's, labels and Lloyd centres equal the restatement on
    the weights the pass saw, the nudged centroids equal the restatement bit for bit and - like the host path's, whose
    scatter_add_ sums with float atomics - lie within the derived bound of the exact result."""
    r = run_case(CHILD, "step_no_eval", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert sorted(r["layers"]) == ["1", "2"]
    for l, c in r["layers"].items():
        assert c["labels"] == 0 and c["labels_vs_ref"] == 0 and c["centres_vs_ref"] == 0 and c["nudged_vs_ref"] == 0, (l, c)
        assert c["host_over_bound"] <= 0 and c["device_over_bound"] <= 0, (l, c)
        assert c["nudge_moved"] > 10, (l, c)


def test_refusals_launch_and_write_nothing(tmp_path):
    """Every refusal of include/siren_fit.h returns its code and a message that names the entry point, for each of the three
    entry points; afterwards the launch counters of all five handles are 0 and no buffer and no parameter was written."""
    r = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    words = {"abi": "abi_version", "K_1": "K", "K_512": "K", "iter_limit_negative": "iter_limit", "layer_out_of_range": "ascending",
             "layer_negative": "ascending", "not_ascending": "ascending", "repeated": "ascending", "n_layers_0": "n_layers",
             "n_layers_5": "n_layers", "null_centroids": "null", "null_args": "null", "null_layers": "null", "null_handle": "null",
             "render": "render handle", "fourier": "FourierNet", "wavelet": "WaveletSiren", "feather": "Feathermap"}
    for fn in ("sf_quant_pass", "sf_quant_nudge", "sf_quant_step"):
        for name, word in words.items():
            c = r[f"{fn}/{name}"]
            assert c["rc"] == -1 and fn in c["msg"] and word in c["msg"], (fn, name, c)
    for name in ("null_lr", "n_negative"):
        c = r[f"sf_quant_step/{name}"]
        assert c["rc"] == -1 and "sf_quant_step" in c["msg"], c
    assert r["sf_quant_step/no_coords"]["rc"] == -4 and "sf_quant_step: sf_set_coords" in r["sf_quant_step/no_coords"]["msg"]
    assert r["sf_quant_step/no_target"]["rc"] == -4 and "sf_quant_step: sf_set_target" in r["sf_quant_step/no_target"]["msg"]
    assert set(r["launches_after_refusals"].values()) == {0}, r["launches_after_refusals"]
    assert r["buffers_untouched"] and r["params_untouched"]
    assert r["ok_pass"]["rc"] == 0 and r["ok_nudge"]["rc"] == 0 and r["ok_wrote"]


def test_launch_counts(tmp_path):
    """Through sf_profile_get, one record per launch: a pass over six layers is 3 + 2 * iter_limit launches, the nudge one;
    quant_step(n) adds n times (the pass, a training pass, the nudge, Adam, the image refresh) and nothing else."""
    r = run_case(CHILD, "launches", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["pass"] == {"k_kmq_guess": 1, "k_kmq_assign": ITER_LIMIT, "k_kmq_update": ITER_LIMIT, "k_kmq_finish": 1, "k_kmq_predict": 1}
    assert sum(r["pass"].values()) <= PASS_LAUNCHES
    assert r["nudge"] == {"k_kmq_nudge": 1}
    for key, n in (("quant_step_3", 3), ("quant_step_2_no_loss", 2)):
        want = {k: n * v for k, v in r["plain_step"].items()}
        want.update({k: n * v for k, v in r["pass"].items()})
        want["k_kmq_nudge"] = n
        assert r[key] == want, (key, r[key], want)
    assert r["losses_finite"]


def test_make_fit_at_bits_9_and_decode(tmp_path):
    """fit_one with masking=none quant=kmeans quant.bits=9 on 64x4, 32x32, 20 + 6 steps finishes with Compressed Bytes, the
    two quantised layers carry uint16 labels, and `make decode` of the run directory draws on the render kernel from the
    container: its bytes are those of the engine's forward on the container's weights.  (The container holds fp16 values,
    the fit's last eval ran on their fp32 originals: the 8-bit PSNR of the two agrees to the 0.5 dB the bits-8 decode test
    allows, when no sample leaves [0, 1].)"""
    r = run_case(CHILD, "fit_bits9", tmp_path=tmp_path, timeout=300)
    print(json.dumps({k: v for k, v in r.items()}, indent=1))
    assert r["saved"]["Compressed Bytes"] == r["container_bytes"] > 0 and "Quant PSNR" in r["saved"]
    wide = [n for n, d in r["dtypes"].items() if d == "uint16"]
    assert wide and all(n.endswith("labeled_weight") for n in wide), r["dtypes"]
    assert r["path"] == "kernel" and r["source"] == "container" and r["ppm_equal"]
    if r["outside_01"] == 0:
        assert abs(r["psnr8_decode"] - r["psnr8_fit"]) < 0.5


def test_make_fit_is_the_same_on_both_routes(tmp_path):
    """The same fit at bits 8 with quant.device_phase=off and =auto: result.json equal to the last bit (the seconds aside),
    the same container bytes and meta data."""
    r = run_case(CHILD, "fit_routes", tmp_path=tmp_path, timeout=300)
    print(json.dumps({p: c["result"] for p, c in r.items()}, indent=1))
    assert r["off"]["returned_equal_saved"] and r["auto"]["returned_equal_saved"]
    assert r["off"]["result"] == r["auto"]["result"] and "Compressed Bytes" in r["auto"]["result"]
    assert r["off"]["container"] == r["auto"]["container"] and r["off"]["meta"] == r["auto"]["meta"]
