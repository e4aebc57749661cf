"""Feathermap (masking=Feathermap) on the gfx950 engine against reference-minted fixtures
(tests/golden/make_golden_feather.py) and fp64 products.  One case of tests/_feather_child.py per child process."""
import json

import numpy as np
import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_feather_child.py"


def test_materialise_adjoint_forward_and_gradients(tmp_path):
    r = run_case(CHILD, "parity", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    for tag in ("small", "padded96", "yaml"):
        assert r[f"fp64_{tag}/mat_rel"] <= 1e-6, tag
        assert r[f"fp64_{tag}/padding_max"] == 0.0, tag
        for k in ("dV1_rel", "dV2_rel", "dscaler_rel"):
            assert r[f"fp64_{tag}/{k}"] <= 1e-5, (tag, k)
    # against the reference (fp32): the engine's fp16 operands.  Bars are the measured values on an MI355X rounded up
    # about 2x.  Measured: prediction 1.1e-4 (64x4) / 1.05e-3 (128x8: the product weights carry no low-magnitude structure
    # for the fp16 images to keep, so the SIREN bar of 3e-4 holds at 64x4 only); loss 3.1e-8 / 3.5e-5 relative; V1 / V2
    # gradients 0.011 / 0.011 (64x4) max |err| / max |ref|, norms 0.004 / 0.001 (128x8); wide 512x4 against the mirror
    # 0.0061 (largest tensor).
    assert r["small_pred_maxabs"] <= 3e-4 and r["yaml_pred_maxabs"] <= 2e-3
    assert r["small_loss_rel"] < 1e-6 and r["yaml_loss_rel"] < 1e-4
    assert r["small_grad_rel/_V1"] < 2.5e-2 and r["small_grad_rel/_V2"] < 2.5e-2
    assert r["yaml_gradnorm_rel/_V1"] < 1e-2 and r["yaml_gradnorm_rel/_V2"] < 5e-3
    assert r["small_scalers_rel"] < 0.1 and r["yaml_scalers_rel"] < 0.1
    assert max(r["wide_grad_rel"]) < 1.5e-2


def test_twenty_step_trajectory_follows_the_reference(tmp_path):
    r = run_case(CHILD, "traj", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["max_rel"] < 5e-3


def test_train_steps_eager_replay_and_reruns_are_bit_identical(tmp_path):
    r = run_case(CHILD, "steps", tmp_path=tmp_path, timeout=300)
    assert r["eager_vs_bulk"] == [True, True]
    assert r["bulk_rerun"] == [True, True]
    assert r["replay_vs_eager"] == [True, True]
    assert r["loss_first_last"][1] < r["loss_first_last"][0]


def test_host_edits_and_a_rebuilt_handle_keep_the_state(tmp_path):
    r = run_case(CHILD, "state", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["edit_pred_maxabs"] < 3e-4
    assert r["rebuilt"] and r["carried"] == [True, True, True, True] and r["optim_bound_to_new"]


def test_plateau_psnr_within_0p05_db_of_the_reference(tmp_path, golden):
    """SIREN 64x4 at density 0.2, 300 steps at lr 3e-4, 256x256, at scratch format 16 and as `make fit` builds the model
    (scratch format left at auto, which a FeatherNet turns into 16).  Reference PSNR with 8 / 2 torch threads: synthetic
    13.0826 / 13.0827, non-smooth 12.9625 / 12.9626 dB.  Measured on an MI355X at format 16: 13.0997 (+0.017) and 12.9671
    (+0.005); the engine's auto format (12 at this size) measured -0.064 and -0.267 dB, hence the default."""
    g = golden("feather_plateau")
    r = run_case(CHILD, "plateau", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    for name in ("synthetic", "nonsmooth"):
        ref = float(g[f"{name}/t8/psnr"])
        for fmt in (16, 0):
            got = r[f"{name}/fmt{fmt}"]["psnr"]
            assert r[f"{name}/fmt{fmt}"]["format"] == 16
            assert abs(got - ref) <= 0.05, (name, fmt, got, ref, float(g[f"{name}/t2/psnr"]))


def test_make_fit_feathermap_saves_the_reference_keys(tmp_path, golden):
    r = run_case(CHILD, "fit", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    assert r["keys"] == [k[len("small/"):] for k in golden("feather_init").files if k.startswith("small/") and k != "small/nm"]
    assert r["log_has_psnr"]
    assert r["res"]["Stored Params"] == 1888 and r["res"]["Dense Params"] == 8707
    assert abs(r["reload_psnr"] - r["res"]["PSNR"]) < 1e-9
