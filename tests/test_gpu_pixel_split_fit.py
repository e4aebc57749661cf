"""`make fit` with train.pixel_split on an MI355X (tests/_pixel_split_fit_child.py, fresh processes): one fit across ranks by
image rows.  The ranks share cuda:0 here, so the collectives run over gloo (RCCL refuses two ranks on one device): what is
tested is the product path - row-range handles, the reduced step and evaluation, topology updates and the quantise phase on
reduced gradients, who writes -, not the interconnect.

Bounds.  Replicas: bit-identical (the same reduced buffers through the same kernels).  Split against one process: 1e-5
relative on the losses, the project's shard-composition bound (fp32 summation order of the row blocks,
test_pixel_split_two_real_engines).  A world of one against the ordinary fit: bit-identical, derived - it runs the
step-by-step loop that the bulk calls are documented to equal bit for bit."""
import json
import os
import sys

import numpy as np
import pytest

from _gpu_child import TESTS, run_case, run_ranks

pytestmark = pytest.mark.gpu
CHILD = "_pixel_split_fit_child.py"
SAME_ON_EVERY_RANK = ("losses", "evals", "updates", "result", "dead_nonzero", "codebooks", "codebook_sizes")


def run_split(spec, world, tmp_path, timeout=240):
    """`world` ranks of the fit of SPEC on one device -> their records, rank order"""
    port = 29600 + (os.getpid() % 1000)
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    for k in ("LOCAL_WORLD_SIZE",):
        env.pop(k, None)
    run_ranks([sys.executable, os.path.join(TESTS, CHILD), "ranks", str(tmp_path), spec],
              [dict(env, RANK=str(r)) for r in range(world)], timeout=timeout)
    return [json.load(open(tmp_path / f"r{r}.json")) for r in range(world)]


def assert_replicas(recs):
    """what every rank must report alike, bit for bit; rank 0 alone wrote"""
    first = recs[0]
    for r in recs[1:]:
        for key in SAME_ON_EVERY_RANK:
            assert r.get(key) == first.get(key), (key, r["rank"])
        for key in ("params", "exp_avg", "exp_avg_sq", "adam_steps"):
            assert r["state"][key] == first["state"][key], (key, r["rank"])
        assert r["wrote"] == [], r["wrote"]
    assert {"model.pth", "result.json", "decode.json"} <= set(first["wrote"]), first["wrote"]


def flat(losses):
    return [x for run in losses for x in run]


def assert_losses_compose(rec, single, n):
    a, b = flat(rec["losses"])[:n], flat(single["losses"])[:n]
    print("split ", a, "\nsingle", b)
    assert len(a) == len(b) == n and np.allclose(a, b, rtol=1e-5, atol=0), (a, b)


def test_world_of_one_is_the_ordinary_fit(tmp_path):
    """64x4 on 32x32, RigL + k-means bits 8 + plain container, 20 steps (an update every 10) + 6 quantise steps:
    train.pixel_split=true without WORLD_SIZE against the ordinary fit"""
    r = run_case(CHILD, "identity", tmp_path=tmp_path, timeout=240)
    a, b = r["split"], r["plain"]
    assert a["state"]["rows"] == b["state"]["rows"] == [0, 32]
    assert a["artefacts"]["pth"] == b["artefacts"]["pth"]
    assert a["artefacts"]["container"] == b["artefacts"]["container"] and a["artefacts"]["meta"] == b["artefacts"]["meta"]
    assert a["artefacts"]["result"] == b["artefacts"]["result"] and a["result"] == b["result"]
    assert a["losses"] == b["losses"] and a["evals"] == b["evals"] and a["updates"] == b["updates"]
    assert a["state"] == b["state"] and a["codebooks"] == b["codebooks"]
    assert len(a["updates"]) == 2 and sum(len(x) for x in a["losses"]) == 26


def test_two_ranks_dense(tmp_path):
    """64x4 on 64x48, dense: 12 steps as train_steps runs of 5 / 5 / 2 with an evaluation after each"""
    recs = run_split("dense", 2, tmp_path)
    assert [r["state"]["rows"] for r in recs] == [[0, 32], [32, 64]]
    assert_replicas(recs)
    assert [len(x) for x in recs[0]["losses"]] == [5, 5, 2] and len(recs[0]["evals"]) == 3
    single = run_case(CHILD, "single", "dense", tmp_path=tmp_path, timeout=120)
    assert_losses_compose(recs[0], single, 5)
    assert recs[0]["state"]["adam_steps"] == 12


def test_three_ranks_uneven_tiny_shards(tmp_path):
    """32x3 on 10x12 over three ranks: 4 / 3 / 3 rows, every shard below one kernel tile"""
    recs = run_split("tiny", 3, tmp_path)
    assert [r["state"]["rows"] for r in recs] == [[0, 4], [4, 7], [7, 10]]
    assert_replicas(recs)
    single = run_case(CHILD, "single", "tiny", tmp_path=tmp_path, timeout=120)
    assert_losses_compose(recs[0], single, 4)


def test_two_ranks_wide_path(tmp_path):
    """hidden 512, depth 3, 16x16: the layer-at-a-time kernels under a row range"""
    recs = run_split("wide", 2, tmp_path)
    assert_replicas(recs)
    single = run_case(CHILD, "single", "wide", tmp_path=tmp_path, timeout=120)
    assert_losses_compose(recs[0], single, 3)


@pytest.mark.parametrize("mode,route", [("RigL", "k_mask_update"), ("Pruning", "k_mask_prune_global"), ("SNFS", "k_mask_snfs"),
                                        ("SET", None)])
def test_two_ranks_masked(tmp_path, mode, route):
    """64x4 on 64x48, 40 steps, an update every 10, on reduced gradients and replicated Adam state: the same masks on both
    ranks after every update with no second collective.  SET (RigL with random growth) draws from the device generator: the
    same seed and the same draws on every rank.  Masks are not compared with the one-process run's: a near-tie in a ranking
    may fall either way under another summation order."""
    recs = run_split(mode, 2, tmp_path)
    assert_replicas(recs)
    ups = recs[0]["updates"]
    assert len(ups) == 4 and recs[0]["dead_nonzero"] == recs[1]["dead_nonzero"] == 0
    for r in recs:
        ran = sum(u["launches"].get(route, 0) for u in r["updates"]) if route else 0
        print(mode, "rank", r["rank"], [u["launches"] for u in r["updates"]], [u["nonzero"] for u in r["updates"]])
        assert (ran > 0) if route else all(not u["launches"] for u in r["updates"])
    if mode == "RigL":                          # the budgets depend on counts only
        single = run_case(CHILD, "single", "RigL", tmp_path=tmp_path, timeout=120)
        assert [u["nonzero"] for u in ups] == [u["nonzero"] for u in single["updates"]]


@pytest.mark.parametrize("bits", [8, 9])
def test_two_ranks_quantise_phase(tmp_path, bits):
    """64x4 on 32x32, dense, 10 + 6 steps: sf_quant_pass, forward/backward, all-reduce, sf_quant_nudge, Adam per step; the
    codebooks stay identical, rank 0's container decodes through `make decode`"""
    recs = run_split(f"quant{bits}", 2, tmp_path)
    assert_replicas(recs)
    r = recs[0]
    assert r["codebooks"] and len(r["codebooks"]) == 2 * len(r["codebook_sizes"]) == 4
    assert all(1 < n <= 2 ** bits for n in r["codebook_sizes"].values()), r["codebook_sizes"]
    assert "model_quantized" in r["wrote"] and [len(x) for x in r["losses"]] == [10, 3, 3]
    d = r["decode"]
    print(d, r["result"]["Quant PSNR 8bit"])
    assert d["path"] == "kernel" and d["source"] == "container"
    if d["outside_01"] == 0:
        assert abs(d["psnr8_decode"] - float(r["result"]["Quant PSNR 8bit"])) < 0.5
