"""Child of tests/test_gpu_quant_phase.py: the quantise phase on the device (sf_quant_pass / sf_quant_nudge / sf_quant_step,
csrc/siren_quant.hip) on an MI355X against the contract on the CPU (tests/_kmeans_ref.py, tests/_quant_phase_ref.py) and
against the step-by-step path, bit for bit unless a bound is named.  One case per process."""
import ctypes as C
import json
import os

import numpy as np
import torch

import _kmeans_ref as R
import _quant_phase_ref as Q
from _gpu_child import ROOT, child_main
from _gpu_fixtures import launches, recorder
from implicit_image import _engine as E

SENTINEL = 7.0


def i32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def cpu(t):
    return t.detach().cpu().numpy()


class Phase:
    """a handle with the per-layer buffers of a quantise phase over `layers`, every buffer holding a sentinel"""

    def __init__(self, eng, layers, bits, **kw):
        self.eng, self.layers, self.K = eng, list(layers), 2 ** bits - 1
        self.off = [eng.param_offsets(l) for l in self.layers]
        self.n = [b - w for w, b in self.off]
        K = self.K
        self.centres = [torch.full((K,), SENTINEL, device="cuda") for _ in self.layers]
        self.centroids = [torch.full((K + 1,), SENTINEL, device="cuda") for _ in self.layers]
        self.counts = [torch.full((1,), -1, dtype=torch.int32, device="cuda") for _ in self.layers]
        self.labels = [torch.full((n,), -1, dtype=torch.int64, device="cuda") for n in self.n]
        self.args = eng.quant_args(self.layers, self.centres, self.centroids, self.counts, self.labels, K, **kw)

    def weights(self, flat):
        return [cpu(flat[w:b]) for w, b in self.off]

    def got(self, j):
        w, b = self.off[j]
        return {"centroids": cpu(self.centroids[j]), "n_centroids": int(self.counts[j].item()), "labels": cpu(self.labels[j]),
                "new_weight": cpu(self.eng.view("params")[w:b]), "centres": cpu(self.centres[j])}

    def untouched(self):
        return (all(bool((t == SENTINEL).all()) for t in self.centres + self.centroids)
                and all(bool((t == -1).all()) for t in self.counts + self.labels))


def mismatches(got, ref, K):
    cent = np.zeros(K + 1, np.float32)
    cent[:ref.centroids.size] = ref.centroids[:K + 1]
    return {"centroids": int((i32(got["centroids"]) != i32(cent)).sum()),
            "new_weight": int((i32(got["new_weight"]) != i32(ref.new_weight)).sum()),
            "centres": int((i32(got["centres"]) != i32(ref.centres)).sum()),
            "labels": int((got["labels"] != ref.labels).sum()),
            "n_centroids": int(got["n_centroids"] != ref.n_centroids)}


def same_bits(a, b):
    return all(np.array_equal(a[k] if k in ("labels", "n_centroids") else i32(a[k]), b[k] if k in ("labels", "n_centroids") else i32(b[k]))
               for k in a)


def seeded_params(eng, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(eng.num_params, generator=g) * scale).float()


# ---- the guess against torch.linspace on the device ------------------------------------------------------------------------
def guess_pairs():
    pairs = []
    for name, K, _ in R.TABLE:
        pairs.append(tuple(float(v) for v in Q.guess_ends(R.make_input(name))))
    g = torch.Generator().manual_seed(2024)
    a = torch.randn(1000, generator=g) * torch.exp(torch.rand(1000, generator=g) * 20 - 16)
    b = torch.randn(1000, generator=g) * torch.exp(torch.rand(1000, generator=g) * 20 - 16)
    lo, hi = torch.minimum(a, b).float(), torch.maximum(a, b).float()
    lo[:20] = hi[:20]                                               # min == max
    lo[20:60], hi[20:60] = -hi[20:60].abs() - 1e-3, hi[20:60].abs() + 1e-3       # opposite signs
    lo[60:80] = torch.tensor(1e-39) * torch.arange(1, 21)           # subnormal spans
    hi[60:80] = lo[60:80] + torch.tensor(3e-41) * torch.arange(1, 21)
    lo[80:90], hi[80:90] = -hi[60:70], -lo[60:70]
    pairs += [(float(x), float(y)) for x, y in zip(lo.tolist(), hi.tolist()) if x != 0 and y != 0]
    return pairs


def case_guess():
    eng = E.SirenEngine(8, 8, 32, 16)
    layers = list(range(16))
    pairs = guess_pairs()
    out = {"pairs": len(pairs), "K": {}}
    for bits in (2, 4, 5, 8, 9):
        ph = Phase(eng, layers, bits, iter_limit=0)
        K = ph.K
        diff_torch = diff_fused = diff_unfused = torch_vs_fused = entries = 0
        for c in range(0, len(pairs), 16):
            chunk = pairs[c:c + 16]
            flat = torch.zeros(eng.num_params)
            for j, (mn, mx) in enumerate(chunk):
                w, b = ph.off[j]
                flat[w + 1], flat[b - 1] = mn, mx                   # (zeros, -0.0 included, around them)
                flat[w] = -0.0
            eng.set_params(flat.cuda())
            eng.quant_pass(ph.args)
            for j, (mn, mx) in enumerate(chunk):
                got = cpu(ph.centres[j])
                t = cpu(torch.linspace(mn, mx, K, device="cuda", dtype=torch.float32))
                diff_torch += int((i32(got) != i32(t)).sum())
                diff_fused += int((i32(got) != i32(Q.guess_from_ends(mn, mx, K))).sum())
                diff_unfused += int((i32(t) != i32(Q.guess_from_ends(mn, mx, K, fused=False))).sum())
                torch_vs_fused += int((i32(t) != i32(Q.guess_from_ends(mn, mx, K))).sum())
                entries += K
        out["K"][str(K)] = {"entries": entries, "kernel_vs_torch": diff_torch, "kernel_vs_restatement": diff_fused,
                            "torch_vs_unfused_restatement": diff_unfused, "torch_vs_fused_restatement": torch_vs_fused}
    # a layer without a non-zero weight: non-finite ends, the empty call
    ph = Phase(eng, [0, 1, 2], 5, iter_limit=5)
    flat = seeded_params(eng, 5)
    w, b = ph.off[1]
    flat[w:b] = 0.0
    flat[w:b:3] = -0.0
    eng.set_params(flat.cuda())
    eng.quant_pass(ph.args)
    g = ph.got(1)
    out["empty"] = {"ends_finite": bool(np.isfinite(g["centres"][[0, -1]]).any()), "n_centroids": g["n_centroids"],
                    "labels_nonzero": int((g["labels"] != 0).sum()), "weight_bits_set": bool(i32(g["new_weight"]).any()),
                    "centroid_bits_set": bool(i32(g["centroids"]).any()),
                    "torch_ends_finite": bool(torch.isfinite(torch.linspace(float("inf"), float("-inf"), 31, device="cuda")[[0, -1]]).any())}
    eng.close()
    return out


# ---- sf_quant_pass against the restatement, layer by layer -----------------------------------------------------------------
def pass_shapes():
    return {"64x4_bits4": (64, 4, 4, [0, 1, 2, 3], None), "64x4_bits8": (64, 4, 8, [0, 1, 2, 3], None),
            "32x3_bits9": (32, 3, 9, [0, 1, 2], None), "64x4_zero_layer": (64, 4, 5, [0, 1, 2, 3], "zero"),
            "64x4_pruned": (64, 4, 5, [1, 2], "pruned"), "512x3_bits8": (512, 3, 8, [0, 1, 2], None),
            "64x4_stops": (64, 4, 5, [1, 2], "stops")}


def case_pass(name):
    hidden, depth, bits, layers, special = pass_shapes()[name]
    eng = E.SirenEngine(8, 8, hidden, depth)
    ph = Phase(eng, layers, bits)
    flat = seeded_params(eng, 100 + hidden + bits)
    if special == "zero":
        w, b = ph.off[1]
        flat[w:b] = 0.0
    if special == "pruned":
        w, b = ph.off[0]
        keep = (torch.rand(b - w, generator=torch.Generator().manual_seed(3)) > 0.4).float()
        flat[w:b] = flat[w:b] * keep                                # a product: a pruned negative weight becomes -0.0
    if special == "stops":                                          # layer 1 stops early, layer 2 runs all five
        w, b = ph.off[0]
        flat[w:b] = flat[w:b] * (R.STOPS_AT_THREE_SCALE / 0.1)
    before = ph.weights(flat)
    eng.set_params(flat.cuda())
    eng.quant_pass(ph.args)
    torch.cuda.synchronize()
    first = [ph.got(j) for j in range(len(layers))]
    other = cpu(eng.view("params")).copy()
    eng.set_params(flat.cuda())                                     # the same call again on the same handle
    eng.quant_pass(ph.args)
    second = [ph.got(j) for j in range(len(layers))]
    out = {"layers": {}, "n": ph.n, "K": ph.K}
    # what is not a listed layer's weight stays as it was
    keep_mask = np.ones(eng.num_params, bool)
    for w, b in ph.off:
        keep_mask[w:b] = False
    out["other_params_untouched"] = bool(np.array_equal(i32(other[keep_mask]), i32(cpu(flat)[keep_mask])))
    for j, l in enumerate(layers):
        ref, guess = Q.quant_pass_ref(before[j], ph.K)
        wt = torch.tensor(before[j]).cuda()
        single = eng.kmeans_fit(wt, torch.tensor(guess).cuda())     # sf_kmeans_fit on the restated guess
        out["layers"][str(l)] = {"diff": mismatches(first[j], ref, ph.K), "repeat": same_bits(first[j], second[j]),
                                 "iterations": int(ref.iterations), "n_centroids": first[j]["n_centroids"], "empty": bool(ref.empty),
                                 "padding_zero": not i32(first[j]["centroids"][first[j]["n_centroids"]:]).any(),
                                 "as_single_call": bool(np.array_equal(cpu(single[2]).reshape(-1), first[j]["labels"])
                                                        and np.array_equal(i32(cpu(single[0])), i32(first[j]["centroids"]))),
                                 "minus_zero_in": int(((before[j] == 0) & np.signbit(before[j])).sum()),
                                 "minus_zero_out": int(((first[j]["new_weight"] == 0) & np.signbit(first[j]["new_weight"])).sum())}
    eng.close()
    return out


# ---- sf_quant_nudge ----------------------------------------------------------------------------------------------------------
def case_nudge():
    eng = E.SirenEngine(8, 8, 64, 4)
    lr = 3e-4
    ph = Phase(eng, [0, 1, 2, 3], 8, nudge_lr=lr)
    flat = seeded_params(eng, 77)
    w, b = ph.off[2]
    flat[w:b] = 0.0                                                 # an empty layer: one centroid, every label 0
    eng.set_params(flat.cuda())
    eng.quant_pass(ph.args)
    grads = seeded_params(eng, 78, scale=1e-2)
    w, b = ph.off[3]
    grads[w:b] = 0.0                                                # all gradients zero, one of them -0.0
    grads[w + 5] = -0.0
    w, b = ph.off[1]
    grads[w:w + 64] *= 1e-30                                        # far below the unit of the fixed-point sums
    eng.set_grads(grads.cuda())
    before = [cpu(c).copy() for c in ph.centroids]
    labels = [cpu(l) for l in ph.labels]
    host = []
    for j in range(len(ph.layers)):                                 # the host path's scatter_add_ (float atomics)
        w, b = ph.off[j]
        dw = torch.zeros_like(ph.centroids[j])
        dw.scatter_add_(0, ph.labels[j], grads[w:b].cuda())
        host.append(cpu(ph.centroids[j] - lr * dw))
    eng.quant_nudge(ph.args)
    torch.cuda.synchronize()
    after = [cpu(c).copy() for c in ph.centroids]
    eng.set_params(flat.cuda())                                     # a second run from the same state: the same bits
    eng.quant_pass(ph.args)
    eng.quant_nudge(ph.args)
    again = [cpu(c) for c in ph.centroids]
    out = {"layers": {}}
    for j, l in enumerate(ph.layers):
        w, b = ph.off[j]
        g = cpu(grads[w:b])
        ref, dw, unit = Q.nudge_ref(before[j], labels[j], g, lr)
        exact, bound = Q.nudge_bound(before[j], labels[j], g, lr)
        out["layers"][str(l)] = {"diff": int((i32(after[j]) != i32(ref)).sum()), "repeat": bool(np.array_equal(i32(after[j]), i32(again[j]))),
                                 "device_over_bound": float(np.max(np.abs(after[j].astype(np.float64) - exact) - bound)),
                                 "host_over_bound": float(np.max(np.abs(host[j].astype(np.float64) - exact) - bound)),
                                 "host_differs_in": int((i32(host[j]) != i32(after[j])).sum()),
                                 "moved": int((i32(after[j]) != i32(before[j])).sum()), "unit_log2": float(np.log2(unit))}
    eng.close()
    return out


# ---- sf_quant_step against the step-by-step path -----------------------------------------------------------------------------
def _model_pair(masked):
    """two copies of one SIREN 64x4 on 32x32 in one state: step by step (device_phase off) and through sf_quant_step"""
    import copy
    from implicit_image.data import get_grid, synthetic_image
    from implicit_image.models import registry
    from implicit_image.pipeline.quant import KmeansQuant
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler
    torch.manual_seed(0)
    base = registry["siren"](depth=4, hidden_size=64, first_omega_0=50, hidden_omega_0=30).cuda()
    grid, img = get_grid(32, 32).cuda(), synthetic_image(32, 32, 3).cuda()
    mask = None
    if masked:
        g = torch.Generator().manual_seed(9)
        parts = []
        for i, p in enumerate(base._param_list()):
            live = i in (2, 4)                                      # the weights of layers 1 and 2 at density 0.5
            parts.append((torch.rand(p.numel(), generator=g) < 0.5).float() if live else torch.ones(p.numel()))
        mask = torch.cat(parts).cuda()
        with torch.no_grad():
            off = 0
            for p in base._param_list():
                p.mul_(mask[off:off + p.numel()].view(p.shape))
                off += p.numel()
    sides = {}
    for name, phase in (("host", "off"), ("device", "auto")):
        m = copy.deepcopy(base)
        opt, sched = get_optimizer_lr_scheduler(m, dict(name="adam", lr=3e-4), quantize_mode=True)
        if mask is not None:
            m.engine(grid, img)
            m.set_engine_masks(mask)
        kq = KmeansQuant(m, opt, bits=8, skip_ll=["layers.0.linear", "layers.3.linear"], device_phase=phase)
        sides[name] = (m, opt, sched, kq)
    return sides, grid, img, mask


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _state(m, kq):
    eng = m.bound_engine
    st = {k: cpu(eng.view(k)).copy() for k in ("params", "exp_avg", "exp_avg_sq")}
    for i, t in enumerate(kq._targets):
        n = int(t.n_centroids.item())
        st[f"labels{i}"] = cpu(t.labeled_weight).reshape(-1).copy()
        st[f"centroids{i}"] = cpu(t.centroids).reshape(-1)[:n].copy()
    return st


def case_step(masked):
    from implicit_image.utils.train_helper import eval_epoch, train_epoch, train_steps
    masked = masked == "masked"
    sides, grid, img, mask = _model_pair(masked)
    losses, evals, states = {}, {}, {}
    for name, (m, opt, sched, kq) in sides.items():
        losses[name], evals[name] = [], []
        for chunk in range(3):
            if name == "host":
                losses[name] += [train_epoch(m, opt, grid, img, lr_scheduler=sched) for _ in range(4)]
            else:
                losses[name] += train_steps(m, opt, grid, img, 4, lr_scheduler=sched)
            evals[name].append(float(eval_epoch(m, grid, img)[1]))
        states[name] = _state(m, kq)
    dev = sides["device"]
    out = {"losses_equal": bool(np.array_equal(np.array(losses["host"], np.float32).view(np.int32), np.array(losses["device"], np.float32).view(np.int32))),
           "losses": losses, "evals_equal": evals["host"] == evals["device"], "plan": dev[3].device_plan() is not None,
           "host_plan": sides["host"][3].device_plan() is not None, "adam_steps": [s[0].bound_engine.adam_steps for s in sides.values()],
           "opt_steps": [float(next(iter(s[1].state.values()))["step"]) for s in sides.values()],
           "lr": [float(s[1].param_groups[0]["lr"]) for s in sides.values()],
           "diff": {k: (int((_bits(states["host"][k]) != _bits(states["device"][k])).sum())
                        if states["host"][k].shape == states["device"][k].shape else -1) for k in states["host"]},
           "rep": {k: v for k, v in dev[0].bound_engine.profile_report().items() if v["launches"]}}
    if masked:
        out["pruned_nonzero"] = int((states["device"]["params"][cpu(mask) == 0] != 0).sum())
        out["pruned"] = int((cpu(mask) == 0).sum())
    return out


def case_step_no_eval():
    """the state right after a train step, no eval after it: the labels and the Lloyd centres of the step's pass, the nudged
    centroids"""
    from implicit_image.utils.train_helper import train_epoch, train_steps
    sides, grid, img, _ = _model_pair(False)
    m_h, opt_h, sched_h, kq_h = sides["host"]
    m_d, opt_d, sched_d, kq_d = sides["device"]
    for _ in range(3):
        train_epoch(m_h, opt_h, grid, img, lr_scheduler=sched_h)
    train_steps(m_d, opt_d, grid, img, 2, lr_scheduler=sched_d)
    # the third step alone, so that the weights its pass saw can be kept
    eng = m_d.bound_engine
    w_in = cpu(eng.view("params")).copy()
    train_steps(m_d, opt_d, grid, img, 1, lr_scheduler=sched_d)
    torch.cuda.synchronize()
    grads = cpu(eng.view("grads"))
    _, args = kq_d.device_plan()
    _, centres, centroids, counts, labels = args._keep
    out = {"layers": {}}
    for j, t in enumerate(kq_h._targets):
        l = args.layers[j].layer
        w, b = eng.param_offsets(l)
        ref, _ = Q.quant_pass_ref(w_in[w:b], 255)
        pre = np.zeros(256, np.float32)
        pre[:ref.centroids.size] = ref.centroids
        want, _dw, _ = Q.nudge_ref(pre, ref.labels, grads[w:b], opt_d.defaults["lr"])
        exact, bound = Q.nudge_bound(pre, ref.labels, grads[w:b], opt_d.defaults["lr"])
        host_c = np.zeros(256, np.float32)
        hc = cpu(t.centroids).reshape(-1)
        host_c[:hc.size] = hc
        out["layers"][str(l)] = {"labels": int((cpu(labels[j]).reshape(-1) != cpu(t.labeled_weight).reshape(-1)).sum()),
                                 "labels_vs_ref": int((cpu(labels[j]).reshape(-1) != ref.labels).sum()),
                                 "centres_vs_ref": int((i32(cpu(centres[j])) != i32(ref.centres)).sum()),
                                 "nudged_vs_ref": int((i32(cpu(centroids[j])) != i32(want)).sum()),
                                 "host_over_bound": float(np.max(np.abs(host_c.astype(np.float64) - exact) - bound)),
                                 "device_over_bound": float(np.max(np.abs(cpu(centroids[j]).astype(np.float64) - exact) - bound)),
                                 "nudge_moved": int((i32(cpu(centroids[j])) != i32(pre)).sum()),
                                 "where": [(int(k), float(pre[k]).hex(), float(cpu(centroids[j])[k]).hex(), float(want[k]).hex(),
                                            float(_dw[k]).hex(), int((ref.labels == k).sum()))
                                           for k in np.nonzero(i32(cpu(centroids[j])) != i32(want))[0][:8]]}
    return out


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    eng = E.SirenEngine(8, 8, 64, 4)
    eng.set_params(seeded_params(eng, 1).cuda())
    torch.cuda.synchronize()
    params0 = cpu(eng.view("params")).copy()
    ph = Phase(eng, [1, 2], 5)
    render, fourier, wavelet = E.RenderEngine(8, 8, 64, 3), E.FourierEngine(8, 8, 64, 3, 64), E.WaveletEngine(8, 8, 64, 3)
    feather = E.SirenEngine(8, 8, 64, 3)
    feather.feather_attach(68, 8, [64, 64, 3], [2, 64, 64])
    handles = [eng, render, fourier, wavelet, feather]
    for e in handles:
        e.profile(True)
    lr = (C.c_float * 2)(1e-3, 1e-3)
    entries = {"sf_quant_pass": lambda h, a: lib.sf_quant_pass(h, a), "sf_quant_nudge": lambda h, a: lib.sf_quant_nudge(h, a),
               "sf_quant_step": lambda h, a: lib.sf_quant_step(h, a, lr, 2, None)}

    def variant(**kw):
        rows = (E.sf_quant_layer * 2)(*[E.sf_quant_layer(layer=l, centers_dev=c.data_ptr(), centroids_dev=k.data_ptr(),
                                                         n_centroids_dev=n.data_ptr(), labels_dev=lab.data_ptr())
                                        for l, c, k, n, lab in zip(kw.pop("layers", [1, 2]), ph.centres, ph.centroids, ph.counts, ph.labels)])
        if kw.pop("null_centroids", False):
            rows[1].centroids_dev = None
        a = E.sf_quant_args(abi_version=E.SF_ABI_VERSION, n_layers=2, layers=rows, K=31, iter_limit=5, tol=1e-4, nudge_lr=1e-3)
        for k, v in kw.items():
            setattr(a, k, v)
        a._rows = rows
        return a
    good = variant()
    cases = {"abi": variant(abi_version=E.SF_ABI_VERSION + 1), "K_1": variant(K=1), "K_512": variant(K=512),
             "iter_limit_negative": variant(iter_limit=-1), "layer_out_of_range": variant(layers=[1, 4]),
             "layer_negative": variant(layers=[-1, 2]), "not_ascending": variant(layers=[2, 1]), "repeated": variant(layers=[1, 1]),
             "n_layers_0": variant(n_layers=0), "n_layers_5": variant(n_layers=5), "null_centroids": variant(null_centroids=True)}
    no_layers = variant()
    no_layers.layers = C.POINTER(E.sf_quant_layer)()
    for fn, call in entries.items():
        for name, a in cases.items():
            rec(f"{fn}/{name}", call(eng.h, C.byref(a)))
        rec(f"{fn}/null_args", call(eng.h, None))
        rec(f"{fn}/null_layers", call(eng.h, C.byref(no_layers)))
        rec(f"{fn}/null_handle", call(None, C.byref(good)))
        rec(f"{fn}/render", call(render.h, C.byref(good)))
        rec(f"{fn}/fourier", call(fourier.h, C.byref(good)))
        rec(f"{fn}/wavelet", call(wavelet.h, C.byref(good)))
        rec(f"{fn}/feather", call(feather.h, C.byref(good)))
    rec("sf_quant_step/null_lr", lib.sf_quant_step(eng.h, C.byref(good), None, 2, None))
    rec("sf_quant_step/n_negative", lib.sf_quant_step(eng.h, C.byref(good), lr, -1, None))
    rec("sf_quant_step/no_coords", lib.sf_quant_step(eng.h, C.byref(good), lr, 2, None))
    from oracle import siren_oracle as so
    gh, gw = so.grid_vectors(8, 8)
    eng.set_coords(gh.cuda(), gw.cuda())
    rec("sf_quant_step/no_target", lib.sf_quant_step(eng.h, C.byref(good), lr, 2, None))
    torch.cuda.synchronize()
    out["launches_after_refusals"] = {n: launches(e) for n, e in zip(("train", "render", "fourier", "wavelet", "feather"), handles)}
    out["buffers_untouched"] = ph.untouched()
    out["params_untouched"] = bool(np.array_equal(i32(cpu(eng.view("params"))), i32(params0)))
    rec("ok_pass", lib.sf_quant_pass(eng.h, C.byref(good)))
    rec("ok_nudge", lib.sf_quant_nudge(eng.h, C.byref(good)))
    torch.cuda.synchronize()
    out["ok_wrote"] = not ph.untouched() and not bool((ph.labels[0] == -1).any())
    for e in handles:
        e.profile(False)
        e.close()
    return out


# ---- launch counts -----------------------------------------------------------------------------------------------------------
def case_launches():
    from oracle import siren_oracle as so
    eng = E.SirenEngine(16, 16, 64, 8)
    gh, gw = so.grid_vectors(16, 16)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_target(so.synthetic_image(16, 16, seed=3).cuda().contiguous())
    eng.set_params(torch.tensor(so.flatten(so.siren_init(64, 8, seed=0))).cuda())
    ph = Phase(eng, [1, 2, 3, 4, 5, 6], 8, nudge_lr=3e-4)
    eng.forward_backward(sync=True)                                 # (scratch and images exist before anything is counted)
    plan = lambda: {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"]}
    eng.profile(True)
    eng.profile_reset()
    eng.quant_pass(ph.args)
    out = {"pass": plan()}
    eng.profile_reset()
    eng.quant_nudge(ph.args)
    out["nudge"] = plan()
    eng.forward(want_pred=False, want_sse=False)                   # (the images follow the pass's weights before the count)
    eng.profile_reset()
    eng.forward_backward(sync=False)
    eng.adam_step(3e-4)
    out["plain_step"] = plan()
    eng.profile_reset()
    losses = eng.quant_step(ph.args, [3e-4] * 3, want_loss=True)
    out["quant_step_3"] = plan()
    out["losses_finite"] = bool(np.isfinite(losses).all()) and len(losses) == 3
    eng.profile_reset()
    eng.quant_step(ph.args, [3e-4] * 2, want_loss=False)
    out["quant_step_2_no_loss"] = plan()
    eng.profile(False)
    eng.close()
    return out


# ---- make fit ----------------------------------------------------------------------------------------------------------------
BASE = ["masking=none", "quant=kmeans", "mlp.hidden_size=64", "mlp.depth=4", "img.height=32", "img.width=32", "train.num_steps=20",
        "train.log_steps=20", "quant.num_steps=6", "quant.log_steps=3", "entropy_coding=plain"]


def _read_container(run_dir):
    qdir = os.path.join(run_dir, "model_quantized")
    return (open(os.path.join(qdir, "compressed_weights.data"), "rb").read(), json.load(open(os.path.join(qdir, "meta_data.json"))))


def case_fit_bits9(workdir):
    from implicit_image import decode as dec, fit
    from implicit_image.config import load_config
    from implicit_image.data import read_ppm
    from implicit_image.pipeline import entropy_coding
    from _gpu_fixtures import u8_ref
    from oracle import siren_oracle as so
    run = os.path.join(workdir, "run")
    res = fit.fit_one(load_config(os.path.join(ROOT, "conf"), BASE + ["quant.bits=9"]), torch.device("cuda", 0), run)
    raw, meta = _read_container(run)
    got = dec.decode([f"decode.dir={run}", "decode.truth=synthetic"])
    ppm = read_ppm(got["out"])
    sd = entropy_coding.decompress_state_dict(os.path.join(run, "model_quantized"), "plain")
    eng = E.SirenEngine(32, 32, 64, 4)
    gh, gw = so.grid_vectors(32, 32)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_params(dec.flat_params(sd, 4).cuda())
    pred, _ = eng.forward(want_pred=True, want_sse=False)
    torch.cuda.synchronize()
    pred = pred.cpu()
    eng.close()
    return {"result": {k: float(v) for k, v in res.items()}, "saved": json.load(open(os.path.join(run, "result.json"))),
            "dtypes": {m["name"]: m["dtype"] for m in meta.values()}, "container_bytes": len(raw),
            "path": got["path"], "source": got["source"], "ppm_equal": bool(torch.equal(ppm, u8_ref(pred).int())),
            "psnr8_decode": got["PSNR_8bit"], "psnr8_fit": float(res["Quant PSNR 8bit"]),
            "outside_01": int(((pred < 0) | (pred > 1)).sum())}


def case_fit_routes(workdir):
    from implicit_image import fit
    from implicit_image.config import load_config
    out = {}
    for phase in ("off", "auto"):
        run = os.path.join(workdir, phase)
        res = fit.fit_one(load_config(os.path.join(ROOT, "conf"), BASE + ["quant.bits=8", f"quant.device_phase={phase}"]),
                          torch.device("cuda", 0), run)
        raw, meta = _read_container(run)
        saved = json.load(open(os.path.join(run, "result.json")))
        out[phase] = {"result": {k: repr(v) for k, v in saved.items() if k != "seconds"}, "returned_equal_saved":
                      all(saved[k] == res[k] for k in saved if k != "seconds"), "container": raw.hex(), "meta": meta}
    return out


if __name__ == "__main__":
    child_main({"guess": case_guess, "pass": case_pass, "nudge": case_nudge, "step": case_step, "step_no_eval": case_step_no_eval,
                "refuse": case_refuse, "launches": case_launches, "fit_bits9": case_fit_bits9, "fit_routes": case_fit_routes})
