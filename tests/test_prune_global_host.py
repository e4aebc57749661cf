"""sf_mask_prune_global without a GPU: the entry point is declared, exported and bound; tests/_prune_global_ref.py (the contract
as torch code) equals the host path's truncate_weights() and the real reference's captured updates; its edge cases; Masking
routes to an engine's mask_prune_global exactly when the configuration is the one Pruning ships with, reads nothing back
unless an update is pending, and completes its bookkeeping - prune_threshold included - on the first read."""
import math
import os
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _mask_fixtures
from _mask_fixtures import PRUNING, Cfg
from _prune_global_ref import ALIVE, REMOVED, STATUS, TRIAL_CAP, TRIALS, prune_global_ref, threshold_bits, threshold_of
from implicit_image import _engine
from implicit_image.models import registry
from implicit_image.pipeline.masking.core import GLOBAL_ROUTE
from implicit_image.utils.train_helper import setup_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "siren_fit.h")).read()
    assert "int sf_mask_prune_global(sf_handle* h, const sf_mask_prune_global_args* a);" in hdr
    assert "sf_mask_prune_global" in _engine.exported_symbols() and "sf_mask_prune_global" in _engine.PROTOTYPES
    assert _engine.PROTOTYPES["sf_mask_prune_global"][0] == "core"
    assert sorted(_engine.PROTOTYPES) == list(_engine.exported_symbols())
    lib = _engine.load_library()
    assert hasattr(lib, "sf_mask_prune_global") and _engine.has_mask_prune_global(lib)
    assert not _engine.has_mask_prune_global(SimpleNamespace(sf_mask_update=None))
    assert callable(_engine.SirenEngine.mask_prune_global)
    assert _engine.WaveletEngine.mask_prune_global is None and _engine.FourierEngine.mask_prune_global is None
    fields = [f[0] for f in _engine.sf_mask_prune_global_args._fields_]
    assert fields == ["abi_version", "n_layers", "layers", "target", "prune_rate", "threshold", "increment", "tolerance",
                      "dense_gradients", "stats_dev"]
    assert all(name in hdr for name in fields) and "kPruneTrialCap" in hdr and str(TRIAL_CAP) in hdr
    assert lib.sf_mask_prune_global(None, None) == -1             # refused before any device is touched
    assert lib.sf_abi_version() == 3


# ---- the restatement against the host path ---------------------------------------------------------------------------------
def pruning_model(hidden=64, depth=4, bind=None, device_update="off", **over):
    torch.manual_seed(0)
    m = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30)
    optim = torch.optim.Adam(m._param_list(), lr=3e-4)
    mask = setup_mask(m, optim, Cfg(PRUNING, **over))
    mask.device_update = device_update
    eng = None
    if bind is not None:
        eng = bind(m)
        m._engine = eng
        m._bind_params(eng)
    return m, optim, mask, eng


def train_a_little(model, optim, mask, seed):
    """what a few steps do to the state an update reads: a gradient and moments everywhere, every live weight moved, three
    steps of the cumulative decay (which reads the density: a pending device update is completed there)"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in model.named_parameters():
            g, d = torch.randn(p.shape, generator=gen) * 1e-3, torch.randn(p.shape, generator=gen) * 1e-2
            if p.grad is None:
                p.grad = torch.zeros_like(p)
            p.grad.copy_(g)
            p.data.add_(d * mask.mask_dict.get(name, torch.ones_like(p)))
            st = optim.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                if key not in st:
                    st[key] = torch.zeros_like(p)
                st[key].copy_(torch.rand(p.shape, generator=gen) * 1e-3 + 1e-4)
    mask.count_steps(3)


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).clone()


def i32(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("hidden,depth", [(64, 4), (32, 3)])
@pytest.mark.parametrize("dense_gradients", [True, False])
def test_restatement_equals_the_host_path(hidden, depth, dense_gradients):
    """truncate_weights() (device_update="off") under the Pruning configuration against the restatement on a copy of the
    same state: six consecutive updates with perturbed weights in between."""
    m, optim, mask, _ = pruning_model(hidden, depth, dense_gradients=dense_gradients)
    params = m._param_list()
    names = [n for n, _ in m.named_parameters()]
    masked = [n for n in names if n in mask.mask_dict]
    slices, off = [], 0
    for n, p in zip(names, params):
        if n in mask.mask_dict:
            slices.append((off, p.numel()))
        off += p.numel()
    seen_trials = []
    for u in range(6):
        train_a_little(m, optim, mask, 40 + u)
        w, g = flat(p.data for p in params), flat(p.grad for p in params)
        mm, vv = flat(optim.state[p]["exp_avg"] for p in params), flat(optim.state[p]["exp_avg_sq"] for p in params)
        k = flat(mask.mask_dict.get(n, torch.ones_like(p)) for n, p in zip(names, params))
        target = math.ceil(mask.prune_rate * mask.baseline_nonzero)
        assert target > 0, u
        before_growth, before_adj = mask.adjusted_growth, list(mask.adjustments)
        rows = prune_global_ref(w, g, mm, vv, k, slices, target, mask.prune_rate, mask.prune_threshold, mask.increment,
                                mask.tolerance, dense_gradients)
        mask.update_connections()
        assert int(rows[-1, STATUS]) == 0 and 0 < int(rows[-1, TRIALS]) < TRIAL_CAP
        seen_trials.append(int(rows[-1, TRIALS]))
        assert torch.equal(i32(flat(mask.mask_dict.get(n, torch.ones_like(p)) for n, p in zip(names, params))), i32(k)), u
        assert torch.equal(i32(flat(p.data for p in params)), i32(w)), u
        assert torch.equal(i32(flat(p.grad for p in params)), i32(g)), u
        assert torch.equal(i32(flat(optim.state[p]["exp_avg"] for p in params)), i32(mm)), u
        assert torch.equal(i32(flat(optim.state[p]["exp_avg_sq"] for p in params)), i32(vv)), u
        assert threshold_bits(mask.prune_threshold) == threshold_bits(threshold_of(rows.tolist())), u
        assert [mask.stats.nonzeros_dict[n] for n in masked] == rows[:-1, 4].tolist()
        assert [mask.stats.zeros_dict[n] for n in masked] == rows[:-1, 5].tolist()
        nnz = rows[:-1, 6].tolist()
        norm = 0.0
        for x in nnz:
            norm += x
        assert [mask.stats.variance_dict[n] for n in masked] == [x / norm for x in nnz]
        assert [threshold_bits(mask.name2prune_rate[n]) for n in masked] == [threshold_bits(threshold_of([r])) for r in rows[:-1].tolist()]
        adj = mask.baseline_nonzero - (int(rows[-1, ALIVE]) - int(rows[-1, REMOVED]))
        assert mask.adjustments == before_adj + [adj]
        assert mask.adjusted_growth == 0.25 * before_growth + 0.75 * adj + np.mean(before_adj + [adj])
        assert [int(r[0] - r[4]) for r in rows[:-1].tolist()] == rows[:-1, 3].tolist()
    assert mask.stats.total_density < 0.95
    print("trials per update:", seen_trials)


# ---- the restatement against the real reference --------------------------------------------------------------------------
@pytest.mark.parametrize("upd", [5, 10])
def test_restatement_against_the_reference(golden, upd):
    """tests/golden/masking_pruning.npz (the real reference's Pruning run on the 64x4 model): the state before the update at
    step `upd` goes through the restatement and gives the state after it."""
    d = golden("masking_pruning")
    torch.manual_seed(0)
    m = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30)
    names = [n for n, _ in m.named_parameters()]
    masked = [str(n) for n in d["mask_names"]]
    sizes = [p.numel() for p in m._param_list()]
    pre, post = f"u{upd}_", f"a{upd}_"
    w, g, mm, vv = (torch.tensor(d[pre + key]).clone() for key in "wgmv")
    k, slices, off, moff = torch.ones_like(w), [], 0, 0
    mb = np.unpackbits(d[pre + "mask"])
    for n, size in zip(names, sizes):
        if n in masked:
            k[off:off + size] = torch.tensor(mb[moff:moff + size].astype(np.float32))
            slices.append((off, size))
            moff += size
        off += size
    baseline = sum(n for _, n in slices)                         # density 1.0: every masked weight starts live
    rate = float(d[pre + "rate"])
    rows = prune_global_ref(w, g, mm, vv, k, slices, math.ceil(rate * baseline), rate, float(d[pre + "prune_threshold"]), 0.2,
                            1e-6, True)
    assert int(rows[-1, STATUS]) == 0 and int(rows[-1, TRIALS]) < TRIAL_CAP
    got_mask = np.packbits(np.concatenate([k[o:o + n].numpy().astype(np.uint8) for o, n in slices]))
    assert np.array_equal(got_mask, d[post + "mask"])
    assert np.array_equal(w.numpy().view(np.int32), d[post + "w"].view(np.int32))
    assert np.array_equal(mm.numpy().view(np.int32), d[post + "m"].view(np.int32))
    assert rows[:-1, 4].tolist() == d[post + "nnz"].tolist()
    assert threshold_of(rows.tolist()) == pytest.approx(float(d[post + "prune_threshold"]), rel=1e-12)
    adjustments = list(d[pre + "adjustments"]) + [baseline - (int(rows[-1, ALIVE]) - int(rows[-1, REMOVED]))]
    growth = 0.25 * float(d[pre + "adjusted_growth"]) + 0.75 * adjustments[-1] + np.mean(adjustments)
    assert growth == pytest.approx(float(d[post + "adjusted_growth"]), rel=1e-12, abs=1e-12)
    live, dead = int(rows[:-1, 4].sum()), int(rows[:-1, 5].sum())
    assert live / (live + dead) == pytest.approx(float(d[post + "density"]), rel=0, abs=1e-15)
    assert int(d[post + "mask_step"]) == int(d[pre + "mask_step"]) + 1


# ---- edge cases of the restatement -------------------------------------------------------------------------------------------
def edge_state(seed=3, n=(96, 1000, 4096), density=0.8):
    gen = torch.Generator().manual_seed(seed)
    N = sum(n)
    w = torch.randn(N, generator=gen) * 0.05
    k = (torch.rand(N, generator=gen) < density).float()
    w = w * k
    g, m, v = torch.randn(N, generator=gen) * 1e-3, torch.randn(N, generator=gen) * 1e-3, torch.rand(N, generator=gen) * 1e-6
    slices, off = [], 0
    for x in n:
        slices.append((off, x))
        off += x
    return [w, g, m, v, k], slices


def run_edge(state, slices, target, threshold=0.001, dense=False, rate=0.1):
    before = [t.clone() for t in state]
    rows = prune_global_ref(*state, slices, target, rate, threshold, 0.2, 1e-6, dense)
    assert int(rows[-1, TRIALS]) < TRIAL_CAP
    return rows, before


def test_edge_target_zero_keeps_the_masks():
    state, slices = edge_state()
    state[4][5] = 1.0                                             # a live weight that is zero stays live: no search ran
    rows, before = run_edge(state, slices, 0)
    assert rows[-1].tolist()[:5] == [0, 0, int(before[4].sum()), 0, 0] and threshold_of(rows.tolist()) == 0.001
    assert torch.equal(state[4], before[4]) and torch.equal(i32(state[0]), i32(before[0] * before[4]))
    assert torch.equal(state[2], before[2] * before[4]) and rows[:-1, 3].tolist() == [0, 0, 0]


def test_edge_target_above_alive_stalls():
    state, slices = edge_state()
    alive = int(state[4].sum())
    rows, _ = run_edge(state, slices, alive + 50)
    assert int(rows[-1, STATUS]) == 0 and int(rows[-1, REMOVED]) == alive and int(state[4].sum()) == 0
    assert 10 <= int(rows[-1, TRIALS]) < TRIAL_CAP


def test_edge_quantised_weights_end_by_stalling():
    state, slices = edge_state()
    state[0].copy_(torch.round(state[0] * 128) / 128)             # multiples of 2^-7: the count jumps over the target
    alive = int(state[4].sum())
    target = alive // 3
    rows, _ = run_edge(state, slices, target)
    removed = int(rows[-1, REMOVED])
    assert abs(removed - target) > target * 1e-6 and 10 < int(rows[-1, TRIALS]) < TRIAL_CAP
    assert int(rows[:-1, 3].sum()) == removed                    # (every live weight here is above zero or pruned)


def test_edge_threshold_equal_to_a_weight_is_strict():
    state, slices = edge_state()
    mags = state[0].abs()
    t = float(mags[mags > 0].sort().values[200])
    alive = int(state[4].sum())
    zero_live = int(((state[0] == 0) & (state[4] == 1)).sum())
    expect = alive - int((mags > t).sum())
    rows, _ = run_edge(state, slices, expect, threshold=t)       # the first count hits the target: one trial
    assert int(rows[-1, TRIALS]) == 1 and int(rows[-1, REMOVED]) == expect == 201 + zero_live
    assert float(state[0].abs()[state[4] == 1].min()) > t and threshold_of(rows.tolist()) == t


def test_edge_threshold_three_decades_off():
    """from far above, the search walks down until the count moves and then converges; from far below, the count (nothing
    removed) does not move for ten trials and the stall break ends the search, as it does on the host"""
    for threshold in (1.0, 1e-6):
        state, slices = edge_state()
        alive = int(state[4].sum())
        target = alive // 10
        rows, before = run_edge(state, slices, target, threshold=threshold)
        final = threshold_of(rows.tolist())
        survivors = int((before[0].abs() > torch.tensor(final, dtype=torch.float64).float()).sum())
        assert int(rows[-1, STATUS]) == 0 and int(rows[-1, REMOVED]) == alive - survivors and int(state[4].sum()) == survivors
        if threshold == 1.0:
            assert int(rows[-1, REMOVED]) == target and 20 < int(rows[-1, TRIALS]) < TRIAL_CAP and final < 0.05
        else:
            assert int(rows[-1, REMOVED]) == 0 and int(rows[-1, TRIALS]) == 10 and threshold < final < 1e-5


def test_edge_all_zero_network_is_left_alone():
    state, slices = edge_state()
    state[0].zero_()
    rows, before = run_edge(state, slices, 100)
    assert int(rows[-1, STATUS]) == 1 and all(torch.equal(i32(a), i32(b)) for a, b in zip(state, before))
    assert threshold_of(rows.tolist()) == 0.001 and int(rows[-1, TRIALS]) == 0


def test_edge_pruned_negative_weights_become_minus_zero():
    state, slices = edge_state()
    rows, before = run_edge(state, slices, int(state[4].sum()) // 2)
    gone = (before[4] == 1) & (state[4] == 0) & (before[0] < 0)
    assert int(gone.sum()) > 100 and bool((i32(state[0])[gone] == -2 ** 31).all())
    assert torch.equal(state[2], before[2] * state[4]) and torch.equal(state[1], before[1] * state[4])


# ---- routing ---------------------------------------------------------------------------------------------------------------
class FakeEngine(_mask_fixtures.FakeEngine):
    """mask_prune_global is the restatement"""

    def __init__(self, model):
        super().__init__(model)
        self.trials = []

    def mask_update(self, *a):
        raise AssertionError("the per-layer update is not the route of global pruning")

    def mask_prune_global(self, layers, target, prune_rate, threshold, increment, tolerance, dense_gradients, stats):
        self.quiet = True
        state, slices = self.state_and_slices(layers)
        rows = prune_global_ref(*state, slices, target, prune_rate, threshold, increment, tolerance, dense_gradients)
        stats.copy_(rows)
        self.trials.append(int(rows[-1, TRIALS]))
        self.updates += 1
        self.quiet = False


class NoGlobalEngine(FakeEngine):
    mask_prune_global = None


def test_device_route_equals_the_host_path_over_five_updates():
    ma, oa, ka, eng = pruning_model(bind=FakeEngine, device_update="auto")
    mb, ob, kb, _ = pruning_model(device_update="auto")
    assert ka._device_plan().route == GLOBAL_ROUTE and kb._device_plan() is None
    for u in range(5):
        train_a_little(ma, oa, ka, 100 + u)
        train_a_little(mb, ob, kb, 100 + u)
        assert ka.prune_rate == kb.prune_rate > 0
        ka.update_connections()
        kb.update_connections()
        assert eng.updates == u + 1 and len(ka._pending) == 1
        assert list(ka.mask_dict) == list(kb.mask_dict)
        for n in kb.mask_dict:
            assert torch.equal(ka.mask_dict[n], kb.mask_dict[n]), (u, n)
            assert ka.mask_dict[n].data_ptr() != eng.vecs["masks"].data_ptr()      # its own tensors, not views
        for pa, pb in zip(ma._param_list(), mb._param_list()):
            assert torch.equal(i32(pa.data), i32(pb.data)), u
        assert threshold_bits(ka.prune_threshold) == threshold_bits(kb.prune_threshold) and not ka._pending
        assert isinstance(ka.prune_threshold, float)
        assert ka.stats == kb.stats and ka.name2prune_rate == kb.name2prune_rate
        assert ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth
        assert ka.mask_step == kb.mask_step
    assert ka.stats.total_density < 0.95 and all(0 < t < TRIAL_CAP for t in eng.trials)


@pytest.mark.parametrize("why", ["knob", "off", "padded", "growth", "no_method", "old_library", "momentum_redistribution"])
def test_ineligible_configurations_take_the_host_path(monkeypatch, why):
    over = {"growth": dict(growth_mode="random"), "momentum_redistribution": dict(redistribution_mode="momentum")}.get(why, {})
    m, optim, mask, eng = pruning_model(bind=NoGlobalEngine if why == "no_method" else FakeEngine, device_update="auto", **over)
    if why == "padded":
        m._padded = True
    if why == "knob":
        monkeypatch.setenv("SIREN_FIT_DEVICE_MASK", "0")
    if why == "off":
        mask.device_update = "off"
    if why == "old_library":
        eng.lib = SimpleNamespace(sf_mask_update=None)
    train_a_little(m, optim, mask, 5)
    assert mask._device_plan() is None
    if why == "growth":
        # the host path is taken - and, as in the reference, cannot finish: global pruning fills no per-layer removed_dict,
        # so truncate_weights() finds no regrowth budget for the first layer and raises; the engine is never called
        with pytest.raises(KeyError, match="weight"):
            mask.update_connections()
        assert eng.updates == 0 and not mask._pending
        return
    before ={n: k.clone() for n, k in mask.mask_dict.items()}
    mask.update_connections()
    assert eng.updates == 0 and mask.mask_step == 4 and len(mask.adjustments) == 1 and not mask._pending
    assert any(not torch.equal(before[n], mask.mask_dict[n]) for n in before)
    if why == "knob":
        monkeypatch.setenv("SIREN_FIT_DEVICE_MASK", "1")
        assert mask._device_plan().route == GLOBAL_ROUTE


def test_device_route_reads_back_only_a_pending_update(monkeypatch):
    """no Tensor.item / tolist / cpu / numpy / bool(tensor) inside update_connections() when nothing is pending; an update
    that finds the one before it pending completes it with exactly one transfer (it starts from that threshold)"""
    m, optim, mask, eng = pruning_model(bind=FakeEngine, device_update="auto")
    counts = defaultdict(int)

    def counted(name):
        plain = getattr(torch.Tensor, name)

        def wrapper(self, *a, **kw):
            if not eng.quiet:
                counts[name] += 1
            return plain(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, wrapper)
    train_a_little(m, optim, mask, 1)
    mask.prune_threshold = 0.002                                  # assigned and read back as a plain float
    assert mask.prune_threshold == 0.002
    for name in ("item", "tolist", "cpu", "numpy", "__bool__"):
        counted(name)
    mask.update_connections()
    assert dict(counts) == {} and eng.updates == 1 and len(mask._pending) == 1 and mask.mask_step == 4
    mask.update_connections()                                     # the first update is pending: one transfer
    assert counts["cpu"] == 1 and counts["tolist"] == 1 and counts["item"] == 0 and counts["numpy"] == 0 and counts["__bool__"] == 0
    assert eng.updates == 2 and len(mask._pending) == 1 and len(mask._adjustments) == 1
    threshold = mask.prune_threshold
    assert counts["cpu"] == 2 and not mask._pending and isinstance(threshold, float) and threshold != 0.002
    mask.stats, mask.name2prune_rate, mask.adjusted_growth, mask.adjustments
    assert counts["cpu"] == 2 and len(mask.adjustments) == 2
    mask.update_connections()                                     # nothing pending: nothing read
    assert counts["cpu"] == 2 and counts["tolist"] == 2 and eng.updates == 3


def test_trial_cap_raises_on_the_first_read():
    m, optim, mask, eng = pruning_model(bind=FakeEngine, device_update="auto")
    train_a_little(m, optim, mask, 2)

    def capped(layers, target, prune_rate, threshold, increment, tolerance, dense_gradients, stats):
        stats.zero_()
        stats[-1, STATUS], stats[-1, TRIALS] = 2, TRIAL_CAP
    eng.mask_prune_global = capped
    mask.update_connections()
    with pytest.raises(RuntimeError, match="sf_mask_prune_global"):
        mask.stats
