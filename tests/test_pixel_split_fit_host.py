"""CPU tests of `make fit` with train.pixel_split: the two keys, what is refused before any GPU work, the backend rule as a
pure function, and PixelSplitFit.steps over gloo world-2 with the oracle standing in for the engine."""
import os

import numpy as np
import pytest
import torch

from implicit_image import fit
from implicit_image.config import load_config
from implicit_image.parallel import PixelSplitFit, RowSplit, shard_rows, split_backend
from oracle import siren_oracle as so
from test_host_cpu import _OracleShard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf")
SMALL = ["img.height=16", "img.width=16", "mlp.hidden_size=64", "mlp.depth=4", "train.num_steps=2", "train.log_steps=2"]


def test_keys_parse_and_bad_values_raise():
    c = load_config(CONF, [])
    assert fit.pixel_split_wanted(c) is False and fit.split_backend_setting(c) == "auto"
    for text, want in (("true", True), ("True", True), ("false", False), ("on", True), ("off", False)):
        assert fit.pixel_split_wanted(load_config(CONF, [f"train.pixel_split={text}"])) is want, text
    for name in ("auto", "nccl", "gloo"):
        assert fit.split_backend_setting(load_config(CONF, [f"train.split_backend={name}"])) == name
    for bad in ("mpi", "rccl", "1"):
        with pytest.raises(ValueError, match="split_backend"):
            fit.split_backend_setting(load_config(CONF, [f"train.split_backend={bad}"]))
        with pytest.raises(ValueError, match="split_backend"):
            split_backend(bad, 0, 1, 1)
    with pytest.raises(ValueError, match="pixel_split"):
        fit.pixel_split_wanted(load_config(CONF, ["train.pixel_split=maybe"]))
    with pytest.raises(ValueError, match="split_backend"):          # a bad backend is refused with the rest, before the GPU
        fit.fit_one(load_config(CONF, SMALL + ["train.pixel_split=true", "train.split_backend=mpi"]), torch.device("cpu"))


@pytest.mark.parametrize("overrides,world,reason", [
    (["mlp=fourier", "masking=none", "quant=none"], 1, "FourierNet"),
    (["mlp=wavelet_siren", "masking=none", "quant=none"], 1, "WaveletSiren"),
    (["masking=Feathermap", "quant=none"], 1, "Feathermap"),
    (["mlp.hidden_size=100", "masking=none"], 1, "padded"),
    (["masking=Small_Dense", "masking.density=0.5"], 1, "padded"),          # 64 * sqrt(0.5) = 45: runs padded to 64
    (["img.height=3", "masking=none"], 4, "rows"),
    (["train.device_eval=off"], 1, "device_eval"),
])
def test_refused_compositions_raise_before_any_gpu_work(monkeypatch, overrides, world, reason):
    """fit_one on the CPU device: a refusal comes from the configuration and WORLD_SIZE alone (a fit that got as far as the
    engine would fail with another error, "runs on the gfx950 engine only"), and check_pixel_split is what main runs on
    every rank before the process group exists"""
    monkeypatch.setenv("WORLD_SIZE", str(world))
    monkeypatch.setenv("RANK", "0")
    cfg = load_config(CONF, SMALL + overrides + ["train.pixel_split=true"])
    with pytest.raises(NotImplementedError, match=reason):
        fit.fit_one(cfg, torch.device("cpu"))
    with pytest.raises(NotImplementedError, match=reason):
        fit.check_pixel_split(cfg, world)
    assert not torch.distributed.is_initialized()


def test_accepted_composition_passes_the_check():
    fit.check_pixel_split(load_config(CONF, SMALL + ["train.pixel_split=true"]), 8)
    fit.check_pixel_split(load_config(CONF, SMALL + ["train.pixel_split=true", "masking=SNFS", "mlp.hidden_size=512"]), 16)


def test_backend_rule_of_auto_is_a_pure_function():
    # (setting, LOCAL_RANK, LOCAL_WORLD_SIZE, device count) -> (backend, the ranks share a device)
    assert split_backend("auto", 0, 1, 1) == ("nccl", False)
    assert split_backend("auto", 3, 8, 8) == ("nccl", False)
    assert split_backend("auto", 7, 8, 8) == ("nccl", False)
    assert split_backend("auto", 0, 2, 1) == ("gloo", True)               # two ranks, one device
    assert split_backend("auto", 1, 2, 1) == ("gloo", True)
    assert split_backend("auto", 0, 9, 8) == ("gloo", True)               # one rank too many
    assert split_backend("auto", 0, 1, 0) == ("gloo", True)               # no device at all
    assert split_backend("gloo", 0, 8, 8) == ("gloo", False)              # an explicit setting is taken as it is
    assert split_backend("nccl", 1, 2, 1) == ("nccl", True)


def test_row_split_shares_out_rows_and_a_world_of_one_reduces_nothing():
    assert [(s.row_begin, s.row_end) for s in (RowSplit(10, r, 3) for r in range(3))] == [shard_rows(10, 3, r) for r in range(3)]
    one = RowSplit(7)
    assert (one.row_begin, one.row_end, one.full_height, one.world) == (0, 7, 7, 1)
    t = torch.tensor([1.5, 2.5])
    one.all_reduce(t)                                                      # no process group exists: nothing is called
    assert t.tolist() == [1.5, 2.5] and one.n_values(torch.zeros(3, 5, 3)) == 7 * 5 * 3
    with pytest.raises(NotImplementedError, match="rows"):
        RowSplit(2, 0, 3)


def _steps_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    H, W, n = 12, 9, 5
    grid, img = so.get_grid(H, W), so.synthetic_image(H, W, seed=5)
    r0, r1 = shard_rows(H, world, rank)
    reads, plain_item = [0], torch.Tensor.item

    def counted(self):
        reads[0] += 1
        return plain_item(self)
    torch.Tensor.item = counted                 # the stub: every `.item()` of this process is counted
    out = {}
    for how in ("step", "steps"):
        p = so.siren_init(32, 3, seed=0)
        split_fit = PixelSplitFit(_OracleShard(p, grid, img, r0, r1), 3 * H * W)
        reads[0] = 0
        out[how] = [split_fit.step(3e-4) for _ in range(n)] if how == "step" else split_fit.steps([3e-4] * n)
        out[how + "_reads"], out[how + "_params"] = reads[0], so.flatten(p)
    torch.Tensor.item = plain_item
    out["empty"] = split_fit.steps([])
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_steps_over_gloo_world2_equals_step_and_reads_once():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 1000)
    procs = [ctx.Process(target=_steps_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    out = [o for _, o in sorted([q.get(timeout=120) for _ in procs], key=lambda t: t[0])]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    for o in out:
        assert len(o["steps"]) == 5 and o["steps"] == o["step"]              # the same doubles
        assert np.array_equal(o["steps_params"], o["step_params"])
        assert o["step_reads"] == 5 and o["steps_reads"] == 0                 # one table read at the end, no .item() per step
        assert o["empty"] == []
    assert out[0]["steps"] == out[1]["steps"] and np.array_equal(out[0]["steps_params"], out[1]["steps_params"])
