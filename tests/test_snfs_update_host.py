"""sf_mask_update_snfs without a GPU: the ABI as declared, the restatement of its contract (tests/_snfs_ref.py) against the
real reference's captured updates (tests/golden/masking_snfs.npz) and against Masking.truncate_weights() over a small CPU
fit, and the routing of Masking.update_connections() with an engine whose mask_update_snfs is that restatement."""
import ctypes as C
import os
from collections import defaultdict

import numpy as np
import pytest
import torch

import _mask_fixtures
from _mask_fixtures import Cfg
from _mask_update_ref import mask_update_ref
from _snfs_ref import WORDS, bits_d, snfs_update_ref
from implicit_image import _engine
from implicit_image.models import registry
from implicit_image.pipeline.masking.core import SNFS_ROUTE
from implicit_image.utils.train_helper import setup_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# conf/masking/SNFS.yaml on a schedule of twelve updates in sixty steps
SNFS = Cfg(name="SNFS", density=0.3, sparse_init="erdos-renyi-kernel", dense_gradients=True, growth_mode="momentum",
           prune_mode="magnitude", redistribution_mode="momentum", dense=False, prune_rate=0.1, decay_schedule="cosine",
           end_when=60, interval=5)


def test_abi_is_declared():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    assert "int sf_mask_update_snfs(sf_handle* h, const sf_mask_update_snfs_args* a);" in hdr
    assert [f[0] for f in _engine.sf_mask_update_snfs_args._fields_] == [
        "abi_version", "n_layers", "layers", "prune_rate", "adjusted_growth", "growth", "statistic", "dense_gradients", "stats_dev"]
    assert [f[0] for f in _engine.sf_mask_snfs_stats._fields_] == [
        "live_before", "dead_before", "nnz_before", "removed", "live_after", "dead_after", "nnz_after", "prune_rate",
        "stat_before", "budget", "grown", "stat_after"]
    assert _engine.MASK_SNFS_STATS_WORDS == WORDS == 12 and C.sizeof(_engine.sf_mask_update_snfs_args) == 56
    assert _engine.PROTOTYPES["sf_mask_update_snfs"][0] == "core"
    assert _engine.MASK_GROWTH["momentum"] == 2 and _engine.MASK_STATISTIC == {"none": 0, "nonzero": 0, "momentum": 1}
    assert _engine.FourierEngine.mask_update_snfs is None and _engine.WaveletEngine.mask_update_snfs is None
    assert _engine.has_mask_update_snfs(C.CDLL(_engine._LIB_PATH))


# ---- the restatement against the real reference ------------------------------------------------------------------------
def masked_slices(model, names):
    out, off = [], 0
    for n, p in model.named_parameters():
        if n in names:
            out.append((off, p.numel()))
        off += p.numel()
    return out


@pytest.mark.parametrize("upd", [5, 10])
def test_restatement_equals_the_captured_reference(golden, upd):
    """tests/golden/masking_snfs.npz: the real reference's SNFS run on the 64x4 model.  The restatement on its state before
    the update at step `upd` gives its masks, weights and exp_avg after it, bit for bit; the margins of the rounding and
    the truncation are far from the 1e-4 the device tests allow."""
    d = golden("masking_snfs")
    m = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    names = [str(n) for n in d["mask_names"]]
    slices = masked_slices(m, names)
    pre, post = f"u{upd}_", f"a{upd}_"
    w, g, mm, v = (torch.tensor(d[pre + key]).clone() for key in "wgmv")
    k = torch.ones_like(w)
    mb, off = np.unpackbits(d[pre + "mask"]), 0
    for o, n in slices:
        k[o:o + n] = torch.tensor(mb[off:off + n].astype(np.float32))
        off += n
    rows, info = snfs_update_ref(w, g, mm, v, k, slices, float(d[pre + "rate"]), float(d[pre + "adjusted_growth"]), 2, 1, True)
    assert int(rows[-1, 0]) == 0 and not any(any(t) for t in info["tied"])
    assert info["half"] > 0.02 and info["whole"] > 0.01
    got = np.packbits(np.concatenate([k[o:o + n].numpy().astype(np.uint8) for o, n in slices]))
    assert np.array_equal(got, d[post + "mask"])
    assert np.array_equal(w.numpy().view(np.int32), d[post + "w"].view(np.int32))
    assert np.array_equal(mm.numpy().view(np.int32), d[post + "m"].view(np.int32))
    assert rows[:-1, 4].tolist() == d[post + "nnz"].tolist()


# ---- the restatement against the host path over a small fit ------------------------------------------------------------
def forward(model, coords):
    """the SIREN of `model`'s parameters, written out (the model's own forward runs on the engine)"""
    params, x = model._param_list(), coords
    for l in range(0, len(params), 2):
        x = x @ params[l].t() + params[l + 1]
        if l + 2 < len(params):
            x = torch.sin((50.0 if l == 0 else 30.0) * x)
    return x


def host_state(model, optim, mask):
    params = model._param_list()
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).clone()
    return [flat(params), flat([p.grad for p in params]), flat([optim.state[p]["exp_avg"] for p in params]),
            flat([optim.state[p]["exp_avg_sq"] for p in params]), mask.flat_mask().clone()]


def test_restatement_equals_truncate_weights_over_a_dozen_updates():
    """A seeded 64x4 SIREN fitted on the CPU for sixty steps under SNFS's configuration, an update every five.  Every update
    whose selection boundaries are neither tied nor within 4 ulp of a tie gives the host path's masks, weights, moments and
    bookkeeping bit for bit; the step-0 update, where every momentum key lies within a few ulp of sqrt(10), is flagged - and
    it is the only one."""
    torch.manual_seed(0)
    model = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    optim = torch.optim.Adam(model._param_list(), lr=3e-4)
    mask = setup_mask(model, optim, SNFS)
    names = [n for n, _ in model.named_parameters() if n in mask.mask_dict]
    slices = masked_slices(model, names)
    gen = torch.Generator().manual_seed(1)
    coords, target = torch.rand(256, 2, generator=gen) * 2 - 1, torch.rand(256, 3, generator=gen)
    flagged, rounds = [], []
    for step in range(60):
        optim.zero_grad()
        ((forward(model, coords) - target) ** 2).mean().backward()
        mask.step()
        if step % 5:
            continue
        state = host_state(model, optim, mask)
        rate, growth = mask.prune_rate, float(mask.adjusted_growth)
        assert growth >= 0
        rows, info = snfs_update_ref(*state, slices, rate, growth, 2, 1, True)
        mask.update_connections()
        rounds.append(int(rows[-1, 1]))
        if any(any(t) for t in info["tied"]) or any(info["near"]):     # (near: the boundary's two keys fewer than 4 ulp apart -
            flagged.append(step)                                        # torch's vectorised sqrt and divide may differ from
            continue                                                    # the contract's by an ulp on some CPUs)
        assert info["half"] > 1e-4 and info["whole"] > 1e-4, (step, info)
        after = host_state(model, optim, mask)
        for key, a, b in zip("wgmvk", state, after):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (step, key)
        assert [mask.name2prune_rate[n] for n in names] == [bits_d(r[7]) for r in rows[:-1]], step
        assert [mask.stats.nonzeros_dict[n] for n in names] == rows[:-1, 4].tolist(), step
        assert mask.adjustments[-1] == mask.baseline_nonzero - int(rows[:-1, 4].sum()), step
        for n, r in zip(names, rows[:-1]):                      # torch's fp32 mean against the exact sum
            assert mask.stats.variance_dict[n] == pytest.approx(bits_d(r[11]) / bits_d(rows[-1, 11]), rel=1e-5)
    assert flagged == [0], flagged
    assert len(rounds) == 12 and max(rounds) >= 2


# ---- routing -----------------------------------------------------------------------------------------------------------
class SnfsEngine(_mask_fixtures.FakeEngine):
    """an engine with all three routes; mask_update_snfs is the restatement on the optimiser's moments"""
    status = 0

    def __init__(self, model, optim=None):
        super().__init__(model)
        self.lib.sf_mask_update_snfs = None
        self.model, self.optim, self.calls = model, optim, []

    def mask_update(self, layers, prune_rate, growth, dense_gradients, stats):
        state, slices = self.state_and_slices(layers)
        stats.copy_(mask_update_ref(*state, slices, prune_rate, growth, dense_gradients)[0])
        self.updates += 1

    def mask_prune_global(self, *a):
        raise AssertionError("a plan calls nothing")

    def mask_update_snfs(self, layers, prune_rate, adjusted_growth, growth, statistic, dense_gradients, stats):
        self.quiet = True
        off = 0
        for p in self.model._param_list():                      # (dense gradients: the moments are read, never written)
            st = self.optim.state.get(p, {})
            for key in ("exp_avg", "exp_avg_sq"):
                if key in st:
                    self.vecs[key][off:off + p.numel()] = st[key].reshape(-1)
            off += p.numel()
        state, slices = self.state_and_slices(layers)
        if self.status == 1:
            state[2].zero_()
        if self.status == 3:
            state[2][slices[0][0]] = float("nan")
        rows, _ = snfs_update_ref(*state, slices, prune_rate, adjusted_growth, growth, statistic, dense_gradients)
        stats.copy_(rows)
        self.calls.append((adjusted_growth, growth, statistic))
        self.updates += 1
        self.quiet = False


def snfs_model(bind=True, **over):
    torch.manual_seed(0)
    m = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    optim = torch.optim.Adam(m._param_list(), lr=3e-4)
    mask = setup_mask(m, optim, Cfg(SNFS, **over))
    eng = None
    if bind:
        eng = SnfsEngine(m, optim)
        m._engine = eng
        m._bind_params(eng)
    return m, optim, mask, eng


def train_a_little(model, optim, mask, seed, steps=3):
    """a few seeded Adam steps: gradients everywhere, moments that differ from weight to weight, live weights moved"""
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        with torch.no_grad():
            for p in model._param_list():
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
                p.grad.copy_(torch.randn(p.shape, generator=gen) * 1e-3)
        mask.step()


# prune_mode, growth_mode -> the route under redistribution_mode grad, momentum, none, nonzero, for an engine with all three
ROUTE_TABLE = {
    ("global-magnitude", "absolute-gradient"): (None, None, None, None),
    ("global-magnitude", "momentum"): (None, None, None, None),
    ("global-magnitude", "none"): (None, None, "global", "global"),
    ("global-magnitude", "random"): (None, None, None, None),
    ("magnitude", "absolute-gradient"): (None, "snfs", "rigl", "rigl"),
    ("magnitude", "momentum"): (None, "snfs", "snfs", "snfs"),
    ("magnitude", "none"): (None, None, "rigl", "rigl"),
    ("magnitude", "random"): (None, None, None, None),
}


def test_route_table_over_every_registered_mode(monkeypatch):
    from implicit_image.pipeline.masking import grow_registry, prune_registry, redistribute_registry
    assert sorted(redistribute_registry) == ["grad", "momentum", "none", "nonzero"]
    assert sorted(ROUTE_TABLE) == sorted((p, g) for p in prune_registry for g in set(grow_registry) | {"none"})
    for (prune, growth), row in ROUTE_TABLE.items():
        for redistribution, want in zip(sorted(redistribute_registry), row):
            _, _, mask, _ = snfs_model(prune_mode=prune, growth_mode=growth, redistribution_mode=redistribution)
            plan = mask._device_plan()
            assert (plan and plan.route.name) == want, (prune, growth, redistribution)
            for how in ("knob", "off"):                         # the knob and device_update="off" keep the host path
                if how == "knob":
                    monkeypatch.setenv("SIREN_FIT_DEVICE_MASK", "0")
                else:
                    mask.device_update = "off"
                assert mask._device_plan() is None
                monkeypatch.delenv("SIREN_FIT_DEVICE_MASK", raising=False)


def test_an_engine_without_the_method_or_the_symbol_takes_the_host_path():
    m, optim, mask, eng = snfs_model()
    assert mask._device_plan().route is SNFS_ROUTE
    del eng.lib.sf_mask_update_snfs
    assert mask._device_plan() is None
    eng.lib.sf_mask_update_snfs = None
    type(eng).mask_update_snfs, plain = None, type(eng).mask_update_snfs
    try:
        assert mask._device_plan() is None
    finally:
        type(eng).mask_update_snfs = plain


def test_negative_adjusted_growth_runs_that_update_on_the_host():
    m, optim, mask, eng = snfs_model()
    train_a_little(m, optim, mask, 3)
    mask.adjusted_growth = -2.0
    mask.update_connections()
    assert eng.updates == 0 and not mask._pending and len(mask.adjustments) == 1 and mask.mask_step == 4
    mask.adjusted_growth = 1.5
    mask.update_connections()
    assert eng.updates == 1 and eng.calls == [(1.5, 2, 1)] and len(mask._pending) == 1 and mask.mask_step == 5


def test_redistribution_none_passes_no_pool_and_reads_nothing():
    m, optim, mask, eng = snfs_model(redistribution_mode="none")
    train_a_little(m, optim, mask, 3)
    mask.update_connections()
    mask.update_connections()
    assert eng.calls == [(0.0, 2, 0)] * 2 and len(mask._pending) == 2


def test_lazy_completion_equals_the_host_path():
    """two models from one seed, one on the route (the restatement under it), one on the host path: four updates, three
    seeded steps before each.  Masks, weights and the completed bookkeeping are equal; variance_dict to the distance of
    torch's fp32 mean from the exact sum."""
    ma, oa, ka, eng = snfs_model()
    mb, ob, kb, _ = snfs_model(bind=False)
    for u in range(4):
        train_a_little(ma, oa, ka, 50 + u, steps=5)
        train_a_little(mb, ob, kb, 50 + u, steps=5)
        ka.update_connections()
        kb.update_connections()
        assert eng.updates == u + 1 and len(ka._pending) == 1
        assert list(ka.mask_dict) == list(kb.mask_dict)
        for n in kb.mask_dict:
            assert torch.equal(ka.mask_dict[n], kb.mask_dict[n]), (u, n)
        for pa, pb in zip(ma._param_list(), mb._param_list()):
            assert torch.equal(pa.data.view(torch.int32), pb.data.view(torch.int32)), u
        assert ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth and not ka._pending
        assert ka.name2prune_rate == kb.name2prune_rate and ka.mask_step == kb.mask_step
        sa, sb = ka.stats, kb.stats
        assert sa.nonzeros_dict == sb.nonzeros_dict and sa.zeros_dict == sb.zeros_dict
        assert (sa.total_nonzero, sa.total_zero) == (sb.total_nonzero, sb.total_zero)
        assert sa.total_variance == pytest.approx(sb.total_variance, rel=1e-5)
        assert list(sa.variance_dict) == list(sb.variance_dict)
        for n in sb.variance_dict:
            assert sa.variance_dict[n] == pytest.approx(sb.variance_dict[n], rel=1e-5)


@pytest.mark.parametrize("status, error", [(1, AssertionError), (3, RuntimeError)])
def test_a_status_raises_on_the_first_read(status, error):
    m, optim, mask, eng = snfs_model()
    train_a_little(m, optim, mask, 3)
    eng.status = status
    mask.update_connections()
    with pytest.raises(error, match="Total variance is zero" if status == 1 else "sf_mask_update_snfs.*statistic"):
        mask.stats


def test_nothing_is_read_back_when_nothing_is_pending(monkeypatch):
    """the argument step reads adjusted_growth: with no update pending that is no transfer; with one pending it is exactly
    one (Tensor.cpu of its rows), and nothing else inside update_connections() reads the device"""
    m, optim, mask, eng = snfs_model()
    train_a_little(m, optim, mask, 1)
    counts = defaultdict(int)

    def counted(name):
        plain = getattr(torch.Tensor, name)

        def wrapper(self, *a, **kw):
            if not eng.quiet:
                counts[name] += 1
            return plain(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    for name in ("item", "tolist", "cpu", "numpy", "__bool__"):
        counted(name)
    mask.update_connections()
    assert dict(counts) == {} and eng.updates == 1 and len(mask._pending) == 1
    mask.update_connections()
    assert counts["cpu"] == 1 and counts["item"] == 0 and counts["numpy"] == 0 and len(mask._pending) == 1
    assert eng.updates == 2 and len(mask._adjustments) == 1       # (the public attribute would complete the second one)
    mask.stats
    assert counts["cpu"] == 2 and len(mask.adjustments) == 2 and not mask._pending
