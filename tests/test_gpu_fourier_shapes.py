"""FourierNet kernels at the shapes test_gpu_fourier.py leaves out, against fp64 and a rounding model.

Every fourier_kernels.hip path is run here: widths 32 and 256 (k_ff_fwd / k_ff_bwd<32 | 256>, the WD-256 backward is
the one Fourier kernel that spills), layer 0 staged in several LDS slices with a partial last one (map 512 at WD 128 /
256, map 256 at WD 256), map 64 (k_ff_dw<2, true>, one partial slice at WD 256), k_ff_dw<1, false> (WD 32), 2 and 12
Linear layers, Small_Dense widths zero-padded to 64 and 256, multi-chunk passes and grids of 1, 300 x 1 and 1 x 300
pixels.  One case of tests/_fourier_shapes_child.py per child process.

Three references: the rounding model (_fourier_ref.engine_model_loss_and_grads: the kernels' fp16 rounding points,
fp64 elsewhere) is the tight one; the fp64 mirror bounds the whole fp16 error; fourier_shapes.npz is the reference's
own fp32 output.  Bars are literal: measured on an MI355X and rounded up about 2x.  Gradient errors are per tensor,
max |err| / max |ref|."""
import json

import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_fourier_shapes_child.py"
TAGS = ["h32_m64_d3", "h45p_m512_d13", "h128_m512_d4", "h256_m256_d4", "h256_m512_d8", "h198p_m64_d5"]

# Measured on an MI355X (worst tensor of the 24x20 seed-0 pass), engine vs fp64 mirror / engine vs rounding model:
#   h32_m64_d3 2.4e-2 / 3.3e-6, h45p_m512_d13 5.0e-2 / 1.2e-4 (2.4e-4 with an fp64-accumulating model),
#   h128_m512_d4 3.4e-2 / 3.4e-2, h256_m256_d4 0.101 / 9.1e-5, h256_m512_d8 6.5e-2 / 1.1e-4, h198p_m64_d5 7.9e-2 / 7.6e-5.
# The model is 200-7000x closer than fp64 except at h128_m512_d4.  There the error is consistent with one ReLU decision
# that differs: the layer-1 pre-activation closest to zero is 2.9e-6 (model), less than one fp16 step of an upstream h
# moves it (w * ulp16(h) ~ 5e-5).  The engine's h values differ from the model's by such single fp16 steps wherever
# v_sin / v_cos or the MFMA's internal summation order put an fp32 value on the other side of an fp16 rounding boundary
# (neither is reproducible on the CPU), and a flipped ReLU adds or drops that pixel's whole g term in the layer's dW.
# The fp64 comparison sees the same event, so this shape gets no 10x separation.  It is not a missing rounding point:
# modelling the fp32 accumulator per MFMA k-step (_fourier_ref._acc32) did not move it.
FP64_GRAD = {"h32_m64_d3": 5e-2, "h45p_m512_d13": 0.1, "h128_m512_d4": 7e-2, "h256_m256_d4": 0.2, "h256_m512_d8": 0.13,
             "h198p_m64_d5": 0.16}
MODEL_GRAD = {"h32_m64_d3": 1e-5, "h45p_m512_d13": 5e-4, "h128_m512_d4": 7e-2, "h256_m256_d4": 2e-4,
              "h256_m512_d8": 3e-4, "h198p_m64_d5": 2e-4}
MASK_FLIP = {"h128_m512_d4"}


@pytest.mark.parametrize("tag", TAGS)
def test_shape_against_rounding_model_fp64_and_reference(tag, tmp_path):
    """seed-0 model, ragged 24x20 grid (480 pixels: two workgroups, the second partial)."""
    r = run_case(CHILD, "shape", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    if tag not in MASK_FLIP:
        assert MODEL_GRAD[tag] * 10 <= FP64_GRAD[tag]
    # the tight check.  Prediction: measured <= 1.4e-5 max abs against the model (one fp16 step of an h near 1, through
    # the output layer) vs <= 7.0e-5 against fp64; SSE <= 3.8e-7 relative vs the fp64 loss's <= 8.0e-6.
    assert r["model_pred_maxabs"] < 3e-5 and r["model_sse_rel"] < 1e-6
    for n, v in r["model_grad_rel"].items():
        assert v < MODEL_GRAD[tag], (n, v)
    # the whole fp16 error
    assert r["fp64_pred_maxabs"] < 1.5e-4 and r["fp64_loss_rel"] < 2e-5
    for n, v in r["fp64_grad_rel"].items():
        assert v < FP64_GRAD[tag], (n, v)
    # the reference itself (fp32): measured prediction <= 7.0e-5, loss <= 8.1e-6, gradient norms <= 8.5e-3 relative
    assert r["fixture_pred_maxabs"] < 1.5e-4 and r["fixture_loss_rel"] < 2e-5
    for n, v in r["fixture_gradnorm_rel"].items():
        assert v < 2e-2, (n, v)
    # k_ff_fwd<WD, false> (eval) and <WD, true> (training) form the same SSE: measured bit-identical at every shape
    assert r["sse_eval_eq_train"], r["sse_eval_train"]
    if r["padded"]:   # padded weights, biases and their gradients: exactly zero, also after 10 Adam steps
        assert r["pad_grad_max"] == 0.0 and r["pad_param_max_after_10"] == 0.0
        assert r["losses_first_last"][1] < r["losses_first_last"][0]


@pytest.mark.parametrize("tag", ["h32_m64_d3", "h256_m512_d8"])
def test_chunked_passes_match_the_unchunked_handle(tag, tmp_path):
    """37x29 = 1073 pixels at chunk_pixels 256 (five chunks, the last of 49 pixels) and 768 (768 + 305): the chunk's
    pix0 in the forward and in k_ff_dw<*, true>'s recomputed encoding, gradients accumulated over chunks, sse_off."""
    r = run_case(CHILD, "chunks", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    # measured: prediction and SSE bit-identical to the unchunked handle, gradients within 1.4e-7 (768: the slab split
    # over pixels differs); against the model 1.1e-5 / 8.1e-8 / 8.4e-6 (h32) and 7.7e-3 (h256_m512_d8: a ReLU flip as
    # at h128_m512_d4, vs 4.5e-2 against fp64 on this grid)
    model_grad = {"h32_m64_d3": 2e-5, "h256_m512_d8": 1.5e-2}[tag]
    for cp in ("0", "256", "768"):
        c = r[cp]
        assert c["params_equal"] and c["pred_bit_equal"] and c["sse_eval_eq_train"], (cp, c)
        assert c["sse_rel_vs_unchunked"] < 1e-6 and c["grad_rel_vs_unchunked"] < 1e-6, (cp, c)
        assert c["model_pred_maxabs"] < 3e-5 and c["model_sse_rel"] < 2e-7 and c["model_grad_rel"] < model_grad, (cp, c)
        assert c["fp64_grad_rel"] < FP64_GRAD[tag], (cp, c)


@pytest.mark.parametrize("tag", ["h32_m64_d3", "h256_m256_d4"])
def test_tiny_grids(tag, tmp_path):
    """1x1, 1x300 and 300x1: one partial workgroup, a single row or column of coordinates"""
    r = run_case(CHILD, "tiny", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    # measured against the model: prediction <= 1.4e-5, SSE <= 5.2e-7, gradients <= 3.5e-5; against fp64: prediction
    # <= 6.1e-5, loss <= 7.2e-5 (1x1: three values), gradients <= 2.5e-2
    for k, c in r.items():
        assert c["sse_eval_eq_train"], k
        assert c["model_pred_maxabs"] < 3e-5 and c["model_sse_rel"] < 1e-6 and c["model_grad_rel"] < 1e-4, (k, c)
        assert c["fp64_pred_maxabs"] < 1.5e-4 and c["fp64_loss_rel"] < 1.5e-4 and c["fp64_grad_rel"] < FP64_GRAD[tag], (k, c)


def test_twenty_step_trajectory_follows_fp64_adam(tmp_path):
    """256x8 / map 512 / scale 16, 24x20: 20 train_epoch steps at lr 3e-4 against torch.optim.Adam on the fp64 mirror.
    Measured 3.7e-5 worst loss-relative difference.  (At lr 1e-3 this fit is chaotic by step 15: the reference's own
    fp32 run leaves the fp64 one by 23 % at step 20, so that lr tests nothing.)"""
    r = run_case(CHILD, "traj", "h256_m512_d8", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["losses"][-1] < r["losses"][0]
    assert r["max_rel"] < 1e-4
