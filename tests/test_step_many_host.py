"""sf_step_many without a GPU: the ABI as declared and exported, the null refusal, how a sweep is grouped (fit.group_jobs),
the train.batch_jobs key and its refusals, and which route train_steps_many takes without the entry point."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest

from _step_fakes import FakeModel, FakeOptim
from implicit_image import _engine, fit
from implicit_image.config import expand_sweeps, load_config
from implicit_image.utils import train_helper as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "conf")
PROTO = "int sf_step_many(sf_handle* const* h, int32_t n_fits, const float* lr, int32_t n_steps, float* loss_out);"


def cfgs_of(*overrides):
    return [load_config(CONF, ov) for ov in expand_sweeps(list(overrides))]


def test_abi_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    assert PROTO in hdr and "#define SF_STEP_MANY_MAX 64" in hdr
    assert "sf_step_many" in re.findall(r"^int (sf_\w+)\(", hdr, flags=re.M) and "sf_step_many" in _engine.exported_symbols()
    assert "#define SF_ABI_VERSION 3 " in hdr                      # detected by presence: the version stays
    lib = C.CDLL(_engine._LIB_PATH)
    assert hasattr(lib, "sf_step_many")
    group, args, restype = _engine.PROTOTYPES["sf_step_many"]
    assert group == "core" and len(args) == 5 and restype is C.c_int
    assert _engine.has_step_many(lib) and not _engine.has_step_many(SimpleNamespace(sf_step=None))
    assert _engine.STEP_MANY_MAX == 64 == fit.BATCH_JOBS_MAX
    assert callable(_engine.step_many) and callable(_engine.step_many_refusal)


def test_the_kernels_are_one_source_for_both_forms():
    """every batched kernel calls the device function its single-fit kernel calls, and nothing else computes"""
    csrc = os.path.join(ROOT, "implicit-image-compression_amd", "csrc")
    many = open(os.path.join(csrc, "siren_many.hip")).read()
    single = open(os.path.join(csrc, "siren_kernels.hip")).read()
    for body in ("fwd_body", "bwd_body", "dw0_body", "reduce_body", "reduce_vec_body", "sse_reduce_body", "adam_body",
                 "images_body"):
        assert re.search(rf"^DEV void {body}\(", single, flags=re.M), body             # defined once, beside its kernel
        assert len(re.findall(rf"\b{body}[<(]", single)) >= 2, body                       # ... which calls it
        assert len(re.findall(rf"^\s+{body}[<(]", many, flags=re.M)) + many.count(f"{{ {body}(") == 1, body
    fit_hip = open(os.path.join(csrc, "siren_fit.hip")).read()
    assert '#include "siren_many.hip"' in fit_hip and '#include "many_host.hip"' in fit_hip


def test_null_arguments_are_refused_without_a_gpu():
    lib = _engine.load_library()
    lr = (C.c_float * 1)(1e-3)
    hs = (C.c_void_p * 1)(None)
    assert lib.sf_step_many(None, 1, lr, 1, None) == -1 and lib.sf_last_error().decode() == "sf_step_many: null argument"
    assert lib.sf_step_many(hs, 1, None, 1, None) == -1 and lib.sf_last_error().decode() == "sf_step_many: null argument"
    assert lib.sf_step_many(hs, 1, lr, 1, None) == -1 and lib.sf_last_error().decode() == "sf_step_many: member 0: null handle"
    for n in (0, 65):
        assert lib.sf_step_many(hs, n, lr, 1, None) == -1 and "sf_step_many: n_fits must be 1..64" in lib.sf_last_error().decode()
    assert lib.sf_step_many(hs, 1, lr, -1, None) == -1 and lib.sf_last_error().decode() == "sf_step_many: n_steps < 0"


def test_default_configuration_keeps_every_path():
    cfg = load_config(CONF, [])
    assert cfg.train.batch_jobs == 1 and fit.batch_jobs_setting(cfg) == 1
    many = cfgs_of("seed=0,1,2,3")
    assert fit.group_jobs(many, 1) == [[0], [1], [2], [3]]


@pytest.mark.parametrize("value", ["0", "65", "many", "true", "2.5", "-1"])
def test_batch_jobs_is_validated(value):
    cfg = load_config(CONF, [f"train.batch_jobs={value}"])
    with pytest.raises(ValueError, match="train.batch_jobs"):
        fit.batch_jobs_setting(cfg)


@pytest.mark.parametrize("value", [1, 2, 64])
def test_batch_jobs_takes_1_to_64(value):
    assert fit.batch_jobs_setting(load_config(CONF, [f"train.batch_jobs={value}"])) == value


def test_group_jobs_allow_list():
    """jobs that differ in the free keys alone share a group; any other key keeps them apart"""
    base = ["mlp.hidden_size=64", "mlp.depth=4"]
    for free in ("seed=0,1", "img.seed=1,2", "optim.lr=3e-4,1e-3", "masking.density=0.5,0.25", "masking.prune_rate=0.3,0.5",
                 "masking.sparse_init=ERK,random", "img.name=a,b", "exp_name=x,y", "img.path=/p/a.png,/p/b.png"):
        assert fit.group_jobs(cfgs_of(*base, free), 8) == [[0, 1]], free
    for bound in ("mlp.depth=3,4", "mlp.hidden_size=32,64", "img.height=32,64", "img.width=32,64", "train.num_steps=10,20",
                  "masking.interval=10,20", "masking=RigL,SNFS", "optim.eps=1e-8,1e-6", "mlp.first_omega_0=30,50",
                  "engine.compute_dtype=f16,bf16", "quant.num_steps=4,8", "train.log_steps=5,10"):
        assert fit.group_jobs(cfgs_of(*base, bound), 8) == [[0], [1]], bound
    assert set(fit.GROUP_FREE_KEYS) == {"seed", "exp_name", "img.name", "img.path", "img.seed", "optim.lr", "masking.density",
                                        "masking.prune_rate", "masking.sparse_init"}


def test_group_jobs_cap_order_and_loners():
    cfgs = cfgs_of("seed=0,1,2,3,4", "mlp.hidden_size=64")
    assert fit.group_jobs(cfgs, 2) == [[0, 1], [2, 3], [4]]                      # the cap, in job order
    assert fit.group_jobs(cfgs, 64) == [[0, 1, 2, 3, 4]]
    mixed = cfgs_of("seed=0,1,2", "mlp.hidden_size=64,256")                     # jobs 0 2 4: 64, jobs 1 3 5: 256 (no batched kernels)
    assert fit.group_jobs(mixed, 8) == [[0, 2, 4], [1], [3], [5]]
    assert fit.group_jobs(mixed, 2) == [[0, 2], [1], [3], [4], [5]]
    flat = sorted(j for g in fit.group_jobs(mixed, 2) for j in g)
    assert flat == list(range(6))                                               # every job exactly once
    assert fit.group_jobs([], 4) == []
    # a job that joins no group: another model, Feathermap, a zero-padded width, a width above 128
    for loner in (["mlp=fourier", "masking=none", "quant=none"], ["masking=Feathermap", "quant=none", "mlp.hidden_size=64"],
                  ["mlp.hidden_size=48"], ["mlp.hidden_size=256"]):
        assert fit.group_key(load_config(CONF, loner)) is None, loner
        assert fit.group_jobs(cfgs_of("seed=0,1", *loner), 8) == [[0], [1]], loner
    assert fit.group_key(load_config(CONF, ["mlp.hidden_size=128"])) is not None
    for bad in (0, 65, True, "2"):
        with pytest.raises(ValueError):
            fit.group_jobs(cfgs, bad)


def test_group_jobs_is_pure():
    cfgs = cfgs_of("seed=0,1", "mlp.hidden_size=64")
    before = [repr(c) for c in cfgs]
    assert fit.group_jobs(cfgs, 2) == fit.group_jobs(cfgs, 2) == [[0, 1]]
    assert [repr(c) for c in cfgs] == before


def test_pixel_split_with_batch_jobs_is_refused_before_the_gpu(monkeypatch):
    for name in ("fit_one", "fit_group", "init_split_group", "get_device"):
        monkeypatch.setattr(fit, name, lambda *a, **k: pytest.fail(f"{name} ran before the refusal"))
    with pytest.raises(ValueError, match="train.batch_jobs > 1 with train.pixel_split=true"):
        fit.main(["train.batch_jobs=2", "train.pixel_split=true", "seed=0,1"])
    with pytest.raises(ValueError, match="train.batch_jobs"):
        fit.main(["train.batch_jobs=0"])


def test_without_the_entry_point_train_steps_many_is_train_steps_per_member(monkeypatch):
    old = SimpleNamespace(sf_step=None)                                         # a library built before sf_step_many
    models = [FakeModel(SimpleNamespace(lib=old, h=1)) for _ in range(3)]
    optims = [FakeOptim(m) for m in models]
    seen = []

    def train_steps(model, optim, grid, img, n, **kw):
        seen.append((models.index(model), optims.index(optim), grid, img, n, kw["lr_scheduler"], kw["mask"]))
        return [float(models.index(model))] * n
    monkeypatch.setattr(th, "train_steps", train_steps)
    monkeypatch.setattr(th, "_bulk", lambda *a, **k: True)
    monkeypatch.setattr(_engine, "step_many", lambda *a, **k: pytest.fail("sf_step_many without the symbol"))
    monkeypatch.setattr(_engine, "step_many_refusal", lambda *a, **k: pytest.fail("sf_step_many without the symbol"))
    before = dict(th.MANY_STATS)
    got = th.train_steps_many(models, optims, "grid", ["a", "b", "c"], 4, lr_schedulers=["s0", "s1", "s2"], masks=None)
    assert got == [[0.0] * 4, [1.0] * 4, [2.0] * 4]
    assert seen == [(0, 0, "grid", "a", 4, "s0", None), (1, 1, "grid", "b", 4, "s1", None), (2, 2, "grid", "c", 4, "s2", None)]
    assert all(("count_steps", 4) not in o.calls for o in optims)               # train_steps does its own bookkeeping
    assert th.MANY_STATS["calls"] == before["calls"] and th.MANY_STATS["fallbacks"] == before["fallbacks"] + 1


def test_members_that_are_not_bulk_go_one_by_one(monkeypatch):
    models = [FakeModel(SimpleNamespace(lib=SimpleNamespace(sf_step_many=None), h=1)) for _ in range(2)]
    optims = [FakeOptim(m) for m in models]
    monkeypatch.setattr(th, "train_steps", lambda model, optim, grid, img, n, **kw: [0.5] * n)
    monkeypatch.setattr(_engine, "step_many", lambda *a, **k: pytest.fail("not every member is bulk"))
    assert th.train_steps_many(models, optims, None, [None, None], 1) == [[0.5], [0.5]]      # n = 1: train_steps' own rule
    assert all(m.calls == [] for m in models)
    with pytest.raises(ValueError):
        th.train_steps_many(models, optims[:1], None, [None, None], 2)


def test_with_the_entry_point_one_call_and_the_bookkeeping(monkeypatch):
    lib = SimpleNamespace(sf_step_many=None)
    models = [FakeModel(SimpleNamespace(lib=lib, h=1)) for _ in range(2)]
    optims = [FakeOptim(m) for m in models]
    for o, lr in zip(optims, (1e-3, 2e-3)):
        o.param_groups = [{"lr": lr}]
    calls = []
    monkeypatch.setattr(th, "_bulk", lambda *a, **k: True)
    monkeypatch.setattr(th, "train_steps", lambda *a, **k: pytest.fail("the members qualify"))
    monkeypatch.setattr(_engine, "step_many_refusal", lambda engines: None)
    monkeypatch.setattr(_engine, "step_many", lambda engines, lrs, want_loss: calls.append((len(engines), lrs, want_loss)) or [[1.0] * 3, [2.0] * 3])
    before = dict(th.MANY_STATS)
    assert th.train_steps_many(models, optims, None, [None, None], 3) == [[1.0] * 3, [2.0] * 3]
    assert calls == [(2, [[1e-3, 2e-3]] * 3, True)]
    assert all(m.calls == ["train", "engine"] for m in models) and all(o.calls == ["prepare", ("count_steps", 3)] for o in optims)
    assert th.MANY_STATS["calls"] == before["calls"] + 1 and th.MANY_STATS["steps"] == before["steps"] + 3
    # what the library refuses (a scratch format other than 16, ...) goes member by member, with the reason logged once
    monkeypatch.setattr(_engine, "step_many_refusal", lambda engines: "sf_step_many: member 0: scratch format 12")
    monkeypatch.setattr(th, "train_steps", lambda model, optim, grid, img, n, **kw: [0.25] * n)
    assert th.train_steps_many(models, optims, None, [None, None], 3) == [[0.25] * 3] * 2
