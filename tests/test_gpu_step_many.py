"""sf_step_many on the GPU (tests/_step_many_child.py, one case per process): n_steps training steps of B fits of one shape,
one launch per kernel.  The oracle is always fresh handles in the same initial state, stepped by sf_step one handle after
the other; every comparison is bit identity (int32 views in the child, words that differ here), with no tolerance."""
import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu
CHILD = "_step_many_child.py"


def assert_identical(members, n_losses, steps):
    """per member: no word of parameters, gradient or either moment differs, the step counters are `steps`, sf_eval's two
    sums afterwards and every reported loss are the oracle's"""
    assert len(members) == len(steps)
    for b, (r, step) in enumerate(zip(members, steps)):
        print(b, r["diff"], r["got"], r["want"])
        assert r["diff"] == {"params": 0, "grads": 0, "exp_avg": 0, "exp_avg_sq": 0}, (b, r["diff"])
        assert r["got"] == r["want"], (b, r["got"], r["want"])
        assert r["got"]["step"] == step, (b, r["got"]["step"])
        assert r["loss_got"] == r["loss_want"] and len(r["loss_got"]) == n_losses, (b, r["loss_got"], r["loss_want"])
        assert r["nonzero"] > 0
    if len(members) > 1:                          # the members are different fits: different losses from the first step on
        assert len({r["loss_got"][0] for r in members}) == len(members)


@pytest.mark.parametrize("shape,B", [("32x2", 2), ("64x3", 3), ("64x4", 5), ("128x4", 2), ("128x8", 4)])
def test_identity(tmp_path, shape, B):
    """6 steps as calls of 1 + 2 + 3: 32x2 on 8x8 (less than one 256-pixel group; LAST with P0), 64x3 on 24x20 (one group and
    a tail; one hidden layer, P0), 64x4 on 32x32, 128x4 on 40x24, 128x8 on 32x32"""
    res = run_case(CHILD, "identity", shape, tmp_path=tmp_path, timeout=120)
    assert res["formats"] == [16] * B
    assert_identical(res["members"], 6, [6] * B)


def test_masks(tmp_path):
    """two members masked at density 0.5 through set_masks from the auto format, the third unmasked at explicit format 16"""
    res = run_case(CHILD, "masks", tmp_path=tmp_path, timeout=120)
    assert res["formats_before"] == [12, 12, 16] and res["formats"] == [16, 16, 16]
    assert_identical(res["members"], 6, [6, 6, 6])
    assert res["pruned_nonzero"] == [0, 0] and min(res["pruned"]) > 1000      # pruned weights are exactly 0


def test_history(tmp_path):
    """member 0 has taken 3 sf_step steps before the call, member 1 none: each gets the Adam scalars of its own count"""
    res = run_case(CHILD, "history", tmp_path=tmp_path, timeout=120)
    assert_identical(res["members"], 4, [7, 4])


def test_interleave(tmp_path):
    """sf_step_many(3); sf_step(2) with replay on member 0; forward_backward + adam_step on member 1; sf_step_many(2) - against
    the same history with sf_step in place of the batched calls"""
    res = run_case(CHILD, "interleave", tmp_path=tmp_path, timeout=120)
    assert_identical(res["members"][:1], 7, [7])
    assert_identical(res["members"][1:], 5, [6])


def test_bounds(tmp_path):
    res = run_case(CHILD, "bounds", tmp_path=tmp_path, timeout=180)
    assert res["refused"]["rc"] == -1 and "sf_step_many" in res["refused"]["msg"] and "65" in res["refused"]["msg"]
    assert res["refused"]["steps"] == [0] * 65
    assert_identical(res["B1"], 3, [3])
    assert_identical(res["B64"], 3, [3] * 64)


INVALID = ["null_handles", "null_lr", "null_member", "n_fits_0", "n_fits_65", "n_steps_negative", "twice", "render", "fourier",
           "wavelet", "feather", "hidden_256", "bf16", "format_12", "format_8", "chunks", "rows", "height", "width", "hidden",
           "depth", "out_features", "first_omega", "hidden_omega", "outermost_linear", "betas", "eps", "stream"]
STATE = ["no_coords", "no_target"]
NO_INDEX = ["null_handles", "null_lr", "n_fits_0", "n_fits_65", "n_steps_negative"]      # no member to name


def test_refusals(tmp_path):
    """every refusal once: the return code, "sf_step_many" and the offending member's index in the message; afterwards no
    launch on any handle, parameters and step counters untouched; then one accepted call that does change them"""
    res = run_case(CHILD, "refuse", tmp_path=tmp_path, timeout=180)
    ref = res["refusals"]
    assert sorted(ref) == sorted(INVALID + STATE)
    for name, r in ref.items():
        print(name, r)
        assert r["rc"] == (-4 if name in STATE else -1), (name, r)
        assert "sf_step_many" in r["msg"], (name, r)
        if name not in NO_INDEX:
            assert "member 1" in r["msg"], (name, r)
    assert res["launches"]["good"] == [0, 0] and set(res["launches"]["bad"]) == {0}
    assert res["untouched"] == [0, 0] and res["steps"] == res["steps_before"] == [0, 0]
    assert min(res["changed"]) > 0 and res["steps_after"] == [1, 1] and res["launches_after"] > 0


def test_launches_do_not_depend_on_the_batch(tmp_path):
    """the launches the first handle's profile records for a 3-step call: the same for B = 1 and B = 4, and 3 x the kernels of
    one sf_step step (64x4: forward, three layer kernels and k_dw0, their four reductions, the SSE sum, Adam, the images)"""
    res = run_case(CHILD, "launches", tmp_path=tmp_path, timeout=120)
    assert res["B1"] == res["B4"] == res["single"]
    assert res["B4"] == {"k_fwd": 3, "k_bwd_hidden": 3, "k_bwd_last": 3, "k_dw_first": 3, "k_reduce": 12, "k_sse": 3,
                         "k_adam": 3, "k_images": 3, "k_bwd_layer1": 3}


def test_fit_batch_jobs_writes_what_a_sequential_sweep_writes(tmp_path):
    """fit.main on a 3-seed sweep (64x4 on 32x32, 40 steps, RigL updates every 10, 4 quantise steps) with train.batch_jobs=3
    and with 1: per job result.json apart from `seconds`, model.pth, the container and its metadata are equal byte for byte,
    and the batched run's steps went through sf_step_many"""
    res = run_case(CHILD, "fit", tmp_path=tmp_path, timeout=300)
    print(res["counters"], res["equal"])
    assert len(res["jobs"]) == 3 and res["jobs_batched"] == res["jobs"]
    for job, files in res["equal"].items():
        assert set(files) == {"result.json", "model.pth", "compressed_weights.data", "meta_data.json"}, (job, files)
        assert all(files.values()), (job, files)
    assert len(set(res["results"].values())) == 3                       # three different fits
    assert res["counters"]["1"] == {"calls": 0, "steps": 0, "fallbacks": 0}
    many = res["counters"]["3"]
    assert many["calls"] >= 4 and many["fallbacks"] <= 4 and many["steps"] + many["fallbacks"] == 40, many
