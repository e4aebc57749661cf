"""FourierNet (mlp=fourier) on the gfx950 engine against reference-minted fixtures (tests/golden/make_golden_fourier.py).
One case of tests/_fourier_child.py per child process."""
import json

import numpy as np
import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_fourier_child.py"


def test_forward_and_gradients_match_the_reference(tmp_path):
    """seed-0 models, ragged 48x40 grid.  Tolerances are literal: measured on an MI355X (fp16 MFMA operands against the
    reference's fp32) and rounded up about 2x.  Measured: prediction 3.3e-5 (64x4) / 5.5e-6 (yaml) max abs; loss 1.4e-6 /
    1.3e-7 relative; 64x4 gradients max |err| / max |ref| 0.0146 (layers.2.weight, the fp16 operands of g and h);
    yaml per-tensor gradient norms 0.0028 relative."""
    r = run_case(CHILD, "parity", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["small_pred_maxabs"] < 1e-4 and r["yaml_pred_maxabs"] < 1e-4
    assert r["small_loss_rel"] < 1e-5 and r["yaml_loss_rel"] < 1e-5
    for k, v in r.items():
        if k.startswith("small_grad_rel/"):
            assert v < 3e-2, (k, v)
        if k.startswith("yaml_gradnorm_rel/"):
            assert v < 6e-3, (k, v)


def test_train_steps_eager_replay_and_reruns_are_bit_identical(tmp_path):
    r = run_case(CHILD, "steps", tmp_path=tmp_path, timeout=300)
    assert r["eager_vs_bulk"] == [True, True]
    assert r["bulk_rerun"] == [True, True]
    assert r["replay_vs_eager"] == [True, True]
    assert r["loss_first_last"][1] < r["loss_first_last"][0]


def test_small_dense_width_runs_zero_padded(tmp_path):
    r = run_case(CHILD, "padded", tmp_path=tmp_path, timeout=300)
    assert r["hidden"] == 90 and r["width"] == 128
    print(json.dumps(r, indent=1))
    # measured: prediction 1.5e-5 max abs, loss 3.4e-7 relative, gradients max |err| / max |ref| 0.054 (fp16 operands of
    # g and h against the fp32 mirror, depth 5 / map 128)
    assert r["pred_maxabs"] < 1e-4 and r["loss_rel"] < 1e-5 and r["grad_rel"] < 0.1
    assert r["padding_max"] == 0.0


def test_engine_masks_hold_pruned_weights_at_zero(tmp_path):
    r = run_case(CHILD, "masks", tmp_path=tmp_path, timeout=300)
    assert r["n_pruned"] > 1000 and r["pruned_nonzero"] == 0 and r["kept_nonzero"] > 0
    assert r["losses"][-1] < r["losses"][0]


def test_plateau_psnr_within_0p05_db_of_the_reference(tmp_path, golden):
    """yaml model (128x8, map 256, scale 16), 300 steps at lr 3e-4, 256x256.  Reference PSNR with 8 / 2 torch threads:
    synthetic 27.880 / 27.891 dB (spread 0.011), non-smooth 18.819 / 18.783 dB (spread 0.036): inside the 0.05 dB bound.
    Engine measured on an MI355X: 27.890 (+0.010) and 18.816 (-0.003)."""
    g = golden("fourier_plateau")
    r = run_case(CHILD, "plateau", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    for name in ("synthetic", "nonsmooth"):
        ref = float(g[f"{name}/t8/psnr"])
        assert abs(r[name]["psnr"] - ref) <= 0.05, (name, r[name]["psnr"], ref, float(g[f"{name}/t2/psnr"]))


def test_make_fit_fourier_with_kmeans_and_plain_container(tmp_path):
    r = run_case(CHILD, "fit", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    assert r["keys"][0] == "encoding.B" and r["keys"][1:3] == ["layers.0.weight", "layers.0.bias"]
    assert r["keys"][-1] == "layers.4.bias"   # depth 4: three Linear layers at Sequential indices 0, 2, 4
    # (the container writes a quantised layer's centroids / labels after its bias: linear_state_dict)
    assert r["dec_keys"][0] == "encoding.B" and sorted(r["dec_keys"]) == sorted(r["keys"])
    assert r["B_equal"]
    assert r["res"]["PSNR"] > 15.0 and r["res"]["Quant PSNR"] > 15.0
    # every Linear is quantised (kmeans.yaml's layers.first/last.linear names match no FourierNet module): 8 bits
    assert all(n <= 256 for n in r["uniq"].values()), r["uniq"]
