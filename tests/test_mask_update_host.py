"""sf_mask_update without a GPU: the entry point is declared, exported and bound; tests/_mask_update_ref.py (the contract as
torch code) equals the host path's own functions; Masking routes to an engine's mask_update exactly when the configuration
is the one RigL ships with, reads nothing back while it does, and completes its bookkeeping on the first read."""
import os
from collections import defaultdict
from types import SimpleNamespace

import pytest
import torch
from torch import nn

import _mask_fixtures
from _mask_fixtures import RIGL, Cfg
from _mask_update_ref import WORDS, bits_rate, mask_update_ref
from implicit_image import _engine
from implicit_image.models import registry
from implicit_image.pipeline.masking import CosineDecay, Masking
from implicit_image.utils.train_helper import setup_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (64, 96, 192, 1000, 4096)
DENSITY = (0.5, 0.3, 0.6, 0.5, 0.9)            # the last layer: under 20 % sparse with the largest share - the rate cap


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    assert "int sf_mask_update(sf_handle* h, const sf_mask_update_args* a);" in hdr
    assert "sf_mask_update" in _engine.exported_symbols() and "sf_mask_update" in _engine.PROTOTYPES
    lib = _engine.load_library()
    assert hasattr(lib, "sf_mask_update") and _engine.has_mask_update(lib)
    assert not _engine.has_mask_update(SimpleNamespace(sf_render=None))
    assert callable(_engine.SirenEngine.mask_update)
    assert _engine.WaveletEngine.mask_update is None and _engine.FourierEngine.mask_update is None
    assert _engine.MASK_STATS_WORDS == WORDS
    fields = [f[0] for f in _engine.sf_mask_layer_stats._fields_]
    assert fields == ["live_before", "dead_before", "nnz_before", "removed", "live_after", "dead_after", "nnz_after", "prune_rate"]
    assert all(f"{name}" in hdr for name in fields)
    assert lib.sf_mask_update(None, None) == -1                  # refused before any device is touched


# ---- the restatement against the host path's functions -------------------------------------------------------------
class Layers(nn.Module):
    bound_engine = None                         # what Masking asks of every module it wraps

    def __init__(self, tensors):
        super().__init__()
        self.w = nn.ParameterList([nn.Parameter(t.clone()) for t in tensors])


def seeded_layers(seed, quantised):
    gen = torch.Generator().manual_seed(seed)
    ws, gs, ks = [], [], []
    for n, dens in zip(SIZES, DENSITY):
        k = (torch.rand(n, generator=gen) < dens).float()
        w, g = torch.randn(n, generator=gen) * 0.1, torch.randn(n, generator=gen) * 1e-3
        if quantised:                           # multiples of 0.5: heavy ties, live zeros, more zeros than dead + drop
            w, g = torch.round(w * 20) * 0.5, torch.round(g * 2000) * 0.5
        ws.append(w * k)
        gs.append(g)
        ks.append(k)
    return ws, gs, ks


def host_masking(ws, gs, ks, rate, growth, dense_gradients):
    """a Masking on the host path over plain parameters, ready for update_connections()"""
    mod = Layers(ws)
    for p, g in zip(mod.w, gs):
        p.grad = g.clone()
    mk = Masking(SimpleNamespace(state=defaultdict(dict)), CosineDecay(prune_rate=rate, T_max=100),
                 dense_gradients=dense_gradients, prune_mode="magnitude", growth_mode=growth, redistribution_mode="none")
    mk.module = mod
    mk.mask_dict = {n: k.clone() for (n, _), k in zip(mod.named_parameters(), ks)}
    mk.baseline_nonzero = int(sum(k.sum() for k in ks))
    return mk, mod


@pytest.mark.parametrize("quantised", [False, True], ids=["continuous", "quantised"])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.3])
@pytest.mark.parametrize("growth", ["absolute-gradient", "none"])
@pytest.mark.parametrize("dense_gradients", [True, False])
def test_restatement_equals_the_host_functions(monkeypatch, quantised, rate, growth, dense_gradients):
    """funcs.magnitude_prune + funcs.abs_grad_growth + adjust_prune_rate through truncate_weights() on five seeded layers
    (64 .. 4096 elements) against the restatement: continuous values, where every boundary is unique (asserted), with torch's
    own sorts; values quantised to 0.5 with the sorts made stable."""
    ws, gs, ks = seeded_layers(7, quantised)
    if quantised:
        plain = torch.sort
        monkeypatch.setattr(torch, "sort", lambda x, *a, **kw: plain(x, *a, **{**kw, "stable": True}))
    mk, mod = host_masking(ws, gs, ks, rate, growth, dense_gradients)
    mk.update_connections()
    w, g, k = torch.cat(ws), torch.cat(gs), torch.cat(ks)
    m, v = torch.ones_like(w), torch.ones_like(w)
    slices, off = [], 0
    for n in SIZES:
        slices.append((off, n))
        off += n
    rows, tied = mask_update_ref(w, g, m, v, k, slices, rate, _engine.MASK_GROWTH[growth], dense_gradients)
    if not quantised:
        assert not any(any(t) for t in tied)
    else:
        assert rate == 0.0 or any(any(t) for t in tied)          # the quantised layers do split groups of ties
    names = [n for n, _ in mod.named_parameters()]
    assert torch.equal(torch.cat([mk.mask_dict[n] for n in names]), k)
    assert torch.equal(torch.cat([p.data for p in mod.w]).view(torch.int32), w.view(torch.int32))
    assert torch.equal(torch.cat([p.grad for p in mod.w]).view(torch.int32), g.view(torch.int32))
    assert torch.equal(m, k if not dense_gradients else torch.ones_like(k)) and torch.equal(m, v)
    assert [mk.name2prune_rate[n] for n in names] == [bits_rate(r[7]) for r in rows[:-1]]
    if rate:
        assert mk.name2prune_rate[names[-1]] < rate              # the cap applied to the 90 % live layer
    assert [mk.stats.nonzeros_dict[n] for n in names] == rows[:-1, 4].tolist()
    assert [mk.stats.zeros_dict[n] for n in names] == rows[:-1, 5].tolist()
    assert mk.adjustments == [mk.baseline_nonzero - int(rows[:-1, 4].sum())]
    assert int(rows[-1, 0]) == 0


def test_restatement_reports_an_all_zero_network():
    w = torch.zeros(96)
    before = [w.clone(), torch.ones(96), torch.ones(96), torch.ones(96), torch.ones(96)]
    state = [t.clone() for t in before]
    rows, _ = mask_update_ref(*state, [(0, 64), (64, 32)], 0.3, 1, False)
    assert int(rows[2, 0]) == 1 and all(torch.equal(a, b) for a, b in zip(state, before))


# ---- routing -----------------------------------------------------------------------------------------------------------
class FakeEngine(_mask_fixtures.FakeEngine):
    """mask_update is the restatement"""

    def mask_update(self, layers, prune_rate, growth, dense_gradients, stats):
        self.quiet = True
        state, slices = self.state_and_slices(layers)
        rows, _ = mask_update_ref(*state, slices, prune_rate, growth, dense_gradients)
        stats.copy_(rows)
        self.updates += 1
        self.quiet = False


class NoUpdateEngine(FakeEngine):
    mask_update = None


def rigl_model(bind=FakeEngine, **over):
    torch.manual_seed(0)
    m = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    optim = torch.optim.Adam(m._param_list(), lr=3e-4)
    mask = setup_mask(m, optim, Cfg(RIGL, **over))
    eng = None
    if bind is not None:
        eng = bind(m)
        m._engine = eng
        m._bind_params(eng)
    return m, optim, mask, eng


def train_a_little(model, mask, seed):
    """what a few steps do to the state an update reads: a gradient everywhere, every live weight moved off zero"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            g, d = torch.randn(p.shape, generator=gen) * 1e-3, torch.randn(p.shape, generator=gen) * 1e-2
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(g)
            p.data.add_(d * mask.mask_dict.get(name, torch.ones_like(p)))
    for _ in range(3):
        mask.prune_rate_decay.step(mask.mask_step)
        mask.mask_step += 1


def test_device_route_equals_the_host_path_over_five_updates():
    ma, _, ka, eng = rigl_model()
    mb, _, kb, _ = rigl_model(bind=None)
    for u in range(5):
        train_a_little(ma, ka, 100 + u)
        train_a_little(mb, kb, 100 + u)
        ka.update_connections()
        kb.update_connections()
        assert eng.updates == u + 1
        assert list(ka.mask_dict) == list(kb.mask_dict)
        for n in kb.mask_dict:
            assert torch.equal(ka.mask_dict[n], kb.mask_dict[n]), (u, n)
            assert ka.mask_dict[n].data_ptr() != eng.vecs["masks"].data_ptr()      # its own tensors, not views
        for pa, pb in zip(ma._param_list(), mb._param_list()):
            assert torch.equal(pa.data.view(torch.int32), pb.data.view(torch.int32)), u
        assert ka.stats == kb.stats and ka.name2prune_rate == kb.name2prune_rate
        assert ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth
        assert ka.mask_step == kb.mask_step
    assert ka.stats.total_nonzero == kb.baseline_nonzero


@pytest.mark.parametrize("why", ["momentum_growth", "random_growth", "global_prune", "momentum_redistribution", "padded",
                                 "knob", "no_method", "off", "foreign_gradient"])
def test_ineligible_configurations_take_the_host_path(monkeypatch, why):
    over = {"momentum_growth": dict(growth_mode="momentum"), "random_growth": dict(growth_mode="random"),
            "global_prune": dict(prune_mode="global-magnitude", growth_mode="none"),      # (as masking=Pruning pairs them)
            "momentum_redistribution": dict(redistribution_mode="momentum")}.get(why, {})
    m, optim, mask, eng = rigl_model(bind=NoUpdateEngine if why == "no_method" else FakeEngine, **over)
    if why == "padded":
        m._padded = True
    if why == "knob":
        monkeypatch.setenv("SIREN_FIT_DEVICE_MASK", "0")
    if why == "off":
        mask.device_update = "off"
    train_a_little(m, mask, 5)
    optim.step()                                # the moments the momentum modes read
    if why == "foreign_gradient":               # a gradient that is not the engine's own vector
        p = m._param_list()[2]
        p.grad = p.grad.clone()
    assert mask._device_plan() is None
    before = {n: k.clone() for n, k in mask.mask_dict.items()}
    mask.update_connections()
    assert eng.updates == 0 and mask.mask_step == 4 and len(mask.adjustments) == 1
    assert any(not torch.equal(before[n], mask.mask_dict[n]) for n in before)
    if why == "knob":
        monkeypatch.setenv("SIREN_FIT_DEVICE_MASK", "1")
        assert mask._device_plan() is not None


class BothRoutesEngine(FakeEngine):
    def mask_prune_global(self, *a):
        raise AssertionError("a plan calls nothing")


# prune_mode, growth_mode -> the route under redistribution_mode grad, momentum, none, nonzero.  Worked out once from the two
# conditions this table replaced (a plan method per route), before they were folded into one.
ROUTE_TABLE = {
    ("global-magnitude", "absolute-gradient"): (None, None, None, None),
    ("global-magnitude", "momentum"): (None, None, None, None),
    ("global-magnitude", "none"): (None, None, "global", "global"),
    ("global-magnitude", "random"): (None, None, None, None),
    ("magnitude", "absolute-gradient"): (None, None, "rigl", "rigl"),
    ("magnitude", "momentum"): (None, None, None, None),
    ("magnitude", "none"): (None, None, "rigl", "rigl"),
    ("magnitude", "random"): (None, None, None, None),
}


def test_route_table_over_every_registered_mode():
    from implicit_image.pipeline.masking import grow_registry, prune_registry, redistribute_registry
    assert sorted(redistribute_registry) == ["grad", "momentum", "none", "nonzero"]
    assert sorted(ROUTE_TABLE) == sorted((p, g) for p in prune_registry for g in set(grow_registry) | {"none"})
    for (prune, growth), row in ROUTE_TABLE.items():
        for redistribution, want in zip(sorted(redistribute_registry), row):
            _, _, mask, _ = rigl_model(bind=BothRoutesEngine, prune_mode=prune, growth_mode=growth,
                                       redistribution_mode=redistribution)
            plan = mask._device_plan()
            assert (plan and plan.route.name) == want, (prune, growth, redistribution)


def test_device_route_reads_nothing_back(monkeypatch):
    """no Tensor.item / tolist / cpu / numpy / bool(tensor) inside update_connections() on the device route; the first read of
    the statistics makes one transfer per pending update"""
    m, _, mask, eng = rigl_model()
    counts = defaultdict(int)

    def counted(name):
        plain = getattr(torch.Tensor, name)

        def wrapper(self, *a, **kw):
            if not eng.quiet:
                counts[name] += 1
            return plain(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    train_a_little(m, mask, 1)
    for name in ("item", "tolist", "cpu", "numpy", "__bool__"):
        counted(name)
    mask.update_connections()
    mask.update_connections()
    assert dict(counts) == {} and eng.updates == 2 and len(mask._pending) == 2 and mask.mask_step == 5
    total = mask.stats.total_nonzero
    assert counts["cpu"] == 2 and counts["item"] == 0 and counts["numpy"] == 0 and not mask._pending
    assert len(mask.adjustments) == 2 and total == mask.baseline_nonzero
    mask.name2prune_rate, mask.adjusted_growth
    assert counts["cpu"] == 2
