"""WaveletSiren at the shapes test_gpu_wavelet.py leaves out, against fp64, a rounding model and the reference.

Every sub-network kernel path a WaveletSiren reaches runs here with its dL/dout injected from outside (k_wv_adjoint): widths
32 (k_fwd<32>, one partial tile), 64 at depth 2 (layer 1 is both the last layer and the layer-0 re-derivation layer), 128
and 256 with a sine output layer (outermost_linear=False), 256 at depth 2 (k_fwd<256>) and at depth >= 3 (k_fwd_pipe),
Small_Dense 181 zero-padded to 256, depth 16, first / hidden omega 30 / 50, images of 2 x 2 (n = 3 > H: Cb / Cr
down-sampled), 4 x 4 (bilinear scale exactly 1) and 6 x 6, the two-pass path at 11 chunks, on the pipe and with a sine
output, and 4096 x 4096 with default chunking.  One case of tests/_wavelet_shapes_child.py per child process.

Three references: the rounding model (_wavelet_ref.engine_model_loss_and_grads: the engine's fp16 rounding points,
oracle/engine_model.py's scratch-16 chain per sub-network); the fp64 mirror, which bounds the whole fp16 error;
wavelet_shapes.npz, the reference's own fp32 output.  Bars are literal: measured on an MI355X and rounded up about 2x.
Gradient errors are per tensor, max |err| / max |ref|.

The rounding model is not 10x closer than fp64 on gradients, except at depth 2.  A sine network's fp16 roundings of
hidden activations, phases and deltas are not reproducible on the CPU: v_sin / v_cos against libm and the MFMA's
summation order move fp32 values by an ulp, and a value that crosses an fp16 rounding boundary moves by a whole fp16
step, which omega (30 / 50) amplifies downstream.  The model's own floor shows this.  Scaling its parameters by
(1 + 1.2e-7 N(0, 1)), one fp32 ulp, changes its gradients by 2.7e-4 (32x3), 6.2e-4 (256x6), 6.3e-4 (128x5 sine) and
4.2e-4 (64x3 at 2 x 2), but the fp64 mirror's by <= 1.4e-5.  The engine sits at that floor: 3.4e-4 / 4.5e-4 / 6.4e-4 /
7.7e-4.  At depth 2 there is no hidden layer, and the model is 120x closer (4.1e-6 vs 5.0e-4).  At 64x3 on a 2 x 2 image
it is no closer than fp64 (7.7e-4 vs 6.1e-4), because the floor dominates a 27-value loss.  The model still earns its
place.  It takes the same dfac and pre-scale as the engine, so a missing or wrong factor is off by 0.4 .. 1.0 in every
tensor against it and against fp64 alike."""
import json

import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_wavelet_shapes_child.py"
TAGS = ["h32_d3_s24", "h64_d2_s10", "h128_d5_sin_s40", "h256_d2_s30", "h256_d6_s64", "h256_d4_sin_om_s48",
        "h181p_d4_s48", "h32_d16_s20"]
TINY = ["h64_d3_s2", "h64_d3_s4", "h64_d3_s6"]
SINE = {"h128_d5_sin_s40", "h256_d4_sin_om_s48"}

# Measured on an MI355X (worst tensor), engine vs rounding model / vs fp64 mirror:
#   h32_d3_s24 3.4e-4 / 1.3e-3, h64_d2_s10 3.9e-5 / 3.3e-4, h128_d5_sin_s40 6.4e-4 / 1.1e-3, h256_d2_s30 4.1e-6 / 5.0e-4,
#   h256_d6_s64 4.5e-4 / 9.1e-4, h256_d4_sin_om_s48 3.7e-4 / 8.5e-4, h181p_d4_s48 3.9e-4 / 8.8e-4,
#   h32_d16_s20 1.5e-3 / 3.7e-3, h64_d3_s2 7.7e-4 / 6.1e-4, h64_d3_s4 3.3e-4 / 5.6e-4, h64_d3_s6 3.5e-4 / 6.8e-4.
# Before the sine-output fix (no d sin(omega z)/dz on dL/dout) the two sine shapes were 1.0 / 1.1 off against both.
MODEL_GRAD = {"h32_d3_s24": 7e-4, "h64_d2_s10": 8e-5, "h128_d5_sin_s40": 1.3e-3, "h256_d2_s30": 1e-5,
              "h256_d6_s64": 1e-3, "h256_d4_sin_om_s48": 8e-4, "h181p_d4_s48": 8e-4, "h32_d16_s20": 3e-3,
              "h64_d3_s2": 1.5e-3, "h64_d3_s4": 7e-4, "h64_d3_s6": 7e-4}
FP64_GRAD = {"h32_d3_s24": 3e-3, "h64_d2_s10": 7e-4, "h128_d5_sin_s40": 2.5e-3, "h256_d2_s30": 1e-3,
             "h256_d6_s64": 2e-3, "h256_d4_sin_om_s48": 1.7e-3, "h181p_d4_s48": 1.8e-3, "h32_d16_s20": 8e-3,
             "h64_d3_s2": 1.3e-3, "h64_d3_s4": 1.2e-3, "h64_d3_s6": 1.4e-3}
# (10x separation: only where no hidden layer holds an fp16 rounding that can flip)
SEPARATED = {"h256_d2_s30", "h64_d2_s10"}


def check_shape(tag, r):
    sine = tag in SINE
    if tag in SEPARATED:
        assert MODEL_GRAD[tag] * 8 <= FP64_GRAD[tag]
    # the tight check.  Measured against the model: prediction <= 3.6e-5 max abs with a linear output, <= 4.8e-4 with a
    # sine output (omega 30 / 50 on the output layer, at the floor above); SSE <= 1.5e-6 / 5.6e-6 relative
    assert r["model_pred_maxabs"] < (1e-3 if sine else 8e-5), r["model_pred_maxabs"]
    assert r["model_sse_rel"] < (1.2e-5 if sine else 3e-6), r["model_sse_rel"]
    for n, v in r["model_grad_rel"].items():
        assert v < MODEL_GRAD[tag], (n, v)
    # the whole fp16 error.  Measured: prediction <= 6.1e-5 (linear) / 1.25e-3 (sine); loss <= 1.4e-5 / 6.9e-5 relative
    assert r["fp64_pred_maxabs"] < (2.5e-3 if sine else 1.5e-4), r["fp64_pred_maxabs"]
    assert r["fp64_loss_rel"] < (1.5e-4 if sine else 3e-5), r["fp64_loss_rel"]
    for n, v in r["fp64_grad_rel"].items():
        assert v < FP64_GRAD[tag], (n, v)
    # the reference itself (fp32).  Measured: as against fp64; gradient norms <= 2.4e-4 relative (depth 16: 1.1e-3)
    assert r["fixture_pred_maxabs"] < (2.5e-3 if sine else 1.5e-4) and r["fixture_loss_rel"] < (1.5e-4 if sine else 3e-5)
    for n, v in r["fixture_gradnorm_rel"].items():
        assert v < (2.5e-3 if tag == "h32_d16_s20" else 5e-4), (n, v)
    # the inference kernels (eval forward) and the training forward form the same SSE: measured bit-identical everywhere
    assert r["sse_eval_eq_train"], r["sse_eval_train"]


@pytest.mark.parametrize("tag", TAGS)
def test_shape_against_rounding_model_fp64_and_reference(tag, tmp_path):
    """seed-0 model on synthetic_image(H, H, seed 5)"""
    r = run_case(CHILD, "shape", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    check_shape(tag, r)
    if r["padded"]:
        # padded parameters stay exactly 0 through 5 Adam steps (the mask); their gradients are not exactly 0: measured
        # 3.2e-6 at most, which the per-tensor gradient checks above include
        assert r["pad_param_max_after_5"] == 0.0 and r["pad_grad_max"] < 1e-5
        assert r["losses_first_last"][1] < r["losses_first_last"][0]


@pytest.mark.parametrize("tag", TINY)
def test_tiny_images(tag, tmp_path):
    """64x3 at H = 2 (n = 3: Cb / Cr down-sampled), 4 (scale 1) and 6"""
    r = run_case(CHILD, "shape", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    check_shape(tag, r)


def test_compose_and_adjoint_kernels_at_tiny_images(tmp_path):
    """k_wv_compose / k_wv_adjoint at H = 2, 4, 6 on random inputs against the fp64 mirror, and <A x, y> = <x, A^T y>.
    Measured: <= 1.1e-7 relative, dot identity <= 1.5e-8."""
    r = run_case(CHILD, "kernels", "x", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    for H, v in r.items():
        assert v["pred_rel"] < 1e-6 and v["g_rel"] < 1e-6, (H, v)
        assert v["adj_lf_rel"] < 1e-6 and v["adj_hf_rel"] < 1e-6, (H, v)
        assert v["dot_rel"] < 1e-7, (H, v)


@pytest.mark.parametrize("tag", ["h64_d4_s100_c256", "h256_d4_s64_c1024", "h256_d4_sin_om_s48_c256"])
def test_two_pass_path_against_fp64_and_the_model(tag, tmp_path):
    """64x4 at 100 x 100, chunk 256 (2704 coefficients, 11 chunks, the last of 144); 256x4 at 64 x 64, chunk 1024 (the
    pipe's inference and training kernels both feed the pass); the sine-output 256x4 at 48 x 48, chunk 256 (dfac written by
    each chunk's training forward, applied by k_wv_inject)"""
    r = run_case(CHILD, "twopass", tag, tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    sine = "sin" in tag
    # against the one-chunk handle: measured prediction, SSE and eval SSE bit-identical, gradients <= 2.8e-7
    assert r["params_equal"] and r["pred_bit_equal"] and r["sse_equal_one_chunk"] and r["sse_eval_eq_train"], r
    assert r["grad_rel_vs_one_chunk"] < 1e-6
    # measured against the model: gradients 1.2e-4 / 2.3e-4 / 3.4e-4, prediction <= 1.7e-5 (linear) / 4.7e-4 (sine);
    # against fp64: gradients 5.1e-4 / 1.1e-3 / 8.5e-4, loss <= 7.0e-6 / 9.2e-6
    assert r["model_grad_rel"] < {"h64_d4_s100_c256": 3e-4, "h256_d4_s64_c1024": 5e-4, "h256_d4_sin_om_s48_c256": 8e-4}[tag]
    assert r["fp64_grad_rel"] < {"h64_d4_s100_c256": 1e-3, "h256_d4_s64_c1024": 2e-3, "h256_d4_sin_om_s48_c256": 1.7e-3}[tag]
    assert r["model_pred_maxabs"] < (1e-3 if sine else 4e-5) and r["model_sse_rel"] < (5e-6 if sine else 1e-6)
    assert r["fp64_pred_maxabs"] < (2.5e-3 if sine else 1.5e-4) and r["fp64_loss_rel"] < 2e-5


def test_natural_two_pass_size_4096(tmp_path):
    """32x3 at 4096 x 4096 with default chunking (4 202 500 coefficients: 4 Mi + 8196).  Measured: gradients 1.9e-3
    against the fp64 mirror run on the device (worst tensor), loss 4.1e-6 relative; the engine's SSE (65 536 partials
    through k_sse_reduce, eval and training alike) 2.0e-11 from the fp64 sum over its own prediction."""
    r = run_case(CHILD, "natural", "x", tmp_path=tmp_path, timeout=600)
    print(json.dumps(r, indent=1))
    assert r["n2"] == 4202500
    assert r["sse_eval_eq_train"]
    assert r["sse_rel_own"] < 1e-9 and r["sse_eval_rel_own"] < 1e-9
    assert r["fp64_loss_rel"] < 1e-5
    for n, v in r["fp64_grad_rel"].items():
        assert v < 4e-3, (n, v)


def test_graph_replay_on_a_multi_chunk_fit_is_the_eager_path(tmp_path):
    """set_graph_replay(True) with 1156 coefficients in chunks of 256: train_steps falls back to eager launches; losses
    and parameters after 10 steps are bit-identical to the run without replay"""
    r = run_case(CHILD, "replay", "x", tmp_path=tmp_path, timeout=300)
    print(json.dumps(r, indent=1))
    assert r["losses_equal"] and r["params_equal"]
    assert r["losses"][-1] < r["losses"][0]
