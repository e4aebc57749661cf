"""Child of tests/test_gpu_prune_global.py: sf_mask_prune_global on an MI355X against tests/_prune_global_ref.py (the contract on
the CPU), against the host path of Masking.update_connections(), against the real reference's captured updates
(tests/golden/masking_pruning.npz), its refusals, its launch count and a whole `fit`.  One case per process."""
import ctypes as C
import math
import os
import struct

import torch

from _gpu_child import child_main
from _gpu_fixtures import launches, recorder
from _mask_fixtures import KNOB, PRUNING, Cfg, bits, fit_on_both_routes, flat_state, load_captured, seeded_sides, slices_of, update_captured
from _mask_update_ref import WORDS
from _prune_global_ref import REMOVED, TRIALS, prune_global_ref, threshold_of
from implicit_image import _engine as E
from oracle import siren_oracle as so

# layers of 128 .. 2^20 elements: below one workgroup's stride, 4 096-element hidden layers; one 65 536-element layer (many
# buckets); 262 144 (more keys than LDS would hold); 2^20 (several strides per layer)
HANDLES = [(64, 4), (256, 3), (512, 3), (1024, 3)]
HOST_SHAPES = [(64, 4), (256, 3), (512, 3)]                # hidden, depth; on 16 x 16


# ---- the ABI against the restatement ---------------------------------------------------------------------------------------
def make_state(eng, seed, quantised=False, zero=False):
    """[w, g, m, v, k] on the CPU: 80 % of every weight tensor live, dead weights zero"""
    gen = torch.Generator().manual_seed(seed)
    P = eng.num_params
    w, g = torch.randn(P, generator=gen) * 0.05, torch.randn(P, generator=gen) * 1e-3
    m, v, k = torch.randn(P, generator=gen) * 1e-3, torch.rand(P, generator=gen) * 1e-6, torch.ones(P)
    if quantised:
        w = torch.round(w * 128) / 128
    if zero:
        w.zero_()
    for off, n in slices_of(eng, range(eng.depth)):
        k[off:off + n] = (torch.rand(n, generator=gen) < 0.8).float()
        w[off:off + n] *= k[off:off + n]
    return [w.contiguous(), g.contiguous(), m, v, k]


def run_update(eng, state, layers, target, threshold, dense, rate=0.1):
    w, g, m, v, k = (t.cuda() for t in state)
    eng.set_params(w)
    eng.set_masks(k)
    eng.set_grads(g)
    eng.set_adam_state(m, v, 3)
    rows = torch.full((len(layers) + 1, WORDS), -1, dtype=torch.int64, device="cuda")
    eng.mask_prune_global(layers, target, rate, threshold, 0.2, 1e-6, dense, rows)
    mm, vv, _ = eng.get_adam_state()
    return [bits(t) for t in (eng.get_params(), eng.get_grads(), mm, vv, eng.view("masks").clone())], rows.cpu()


def case_abi(which):
    hidden, depth = HANDLES[int(which)]
    eng = E.SirenEngine(8, 8, hidden, depth)
    everything = list(range(depth))
    probe = make_state(eng, 100)
    alive = int(sum(probe[4][o:o + n].sum() for o, n in slices_of(eng, everything)))
    mags = torch.cat([probe[0][o:o + n] for o, n in slices_of(eng, everything)]).abs()
    a_weight = float(mags[mags > 0].sort().values[alive // 7])
    strict_target = alive - int((mags > a_weight).sum())
    #            name, seed, quantised, zero, target, threshold, dense, layers
    variants = [("natural_d0", 100, False, False, alive // 10, 0.001, 0, everything),
                ("natural_d1", 101, False, False, alive // 10, 0.001, 1, everything),
                ("half_d0", 102, False, False, alive // 2, 0.02, 0, everything),
                ("target_zero", 103, False, False, 0, 0.001, 0, everything),
                ("target_above_alive", 104, False, False, alive + alive // 2, 0.001, 0, everything),
                ("quantised", 105, True, False, alive // 3, 0.001, 0, everything),
                ("strict", 100, False, False, strict_target, a_weight, 1, everything),
                ("from_above", 106, False, False, alive // 10, 1.0, 0, everything),
                ("from_below", 107, False, False, alive // 10, 1e-6, 1, everything),
                ("without_layer0", 108, False, False, alive // 10, 0.001, 1, everything[1:]),
                ("all_zero", 109, False, True, 100, 0.001, 0, everything)]
    out = {"sizes": [n for _, n in slices_of(eng, everything)], "alive": alive, "strict_target": strict_target, "variants": {}}
    for name, seed, q, zero, target, threshold, dense, layers in variants:
        state = make_state(eng, seed, q, zero)
        before = [bits(t).clone() for t in state]
        got, rows = run_update(eng, state, layers, target, threshold, dense)
        again, rows2 = run_update(eng, state, layers, target, threshold, dense)
        ref_rows = prune_global_ref(*state, slices_of(eng, layers), target, 0.1, threshold, 0.2, 1e-6, bool(dense))   # (in place)
        same = bool(torch.equal(rows, ref_rows))
        out["variants"][name] = {
            "diff": {key: int((a != bits(b)).sum()) for key, a, b in zip("wgmvk", got, state)},
            "rows_equal": same, "repeat": all(torch.equal(a, b) for a, b in zip(got, again)) and bool(torch.equal(rows, rows2)),
            "status": rows[-1].tolist(), "ref_status": ref_rows[-1].tolist(), "threshold": threshold_of(rows.tolist()),
            "removed": rows[:-1, 3].tolist(), "rows": None if same else rows.tolist(), "ref_rows": None if same else ref_rows.tolist(),
            "untouched": all(torch.equal(a, b) for a, b in zip(got, before)),
            "masks_changed": int((got[4] != before[4]).sum()),
            "minus_zero": int(((got[0] == -2 ** 31) & (before[0] != -2 ** 31)).sum())}
    eng.close()
    return out


# ---- against the host path -------------------------------------------------------------------------------------------------
def case_host(which, dense):
    from implicit_image.data import get_grid
    from implicit_image.utils.train_helper import train_epoch
    hidden, depth = HOST_SHAPES[int(which)]
    grid, img = get_grid(16, 16).cuda(), so.synthetic_image(16, 16, seed=3).cuda().contiguous()
    sides = seeded_sides(Cfg(PRUNING, dense_gradients=dense == "1"), hidden, depth)
    out = {"updates": [], "device_updates": [0, 0], "trials": []}
    calls, plain = [0], E.SirenEngine.mask_prune_global

    def counted(self, layers, target, prune_rate, threshold, increment, tolerance, dense_gradients, stats=None):
        calls[0] += 1
        plain(self, layers, target, prune_rate, threshold, increment, tolerance, dense_gradients, stats)
        out["trials"].append(int(stats[-1, TRIALS]))
    E.SirenEngine.mask_prune_global = counted
    for u in range(4):
        losses = [[train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask) for _ in range(3)]
                  for m, optim, sched, mask in sides]
        for side, (m, optim, sched, mask) in enumerate(sides):
            os.environ[KNOB] = "0" if side == 0 else "1"
            calls[0] = 0
            mask.update_connections()
            out["device_updates"][side] += calls[0]
        os.environ.pop(KNOB)
        (ma, _, _, ka), (mb, _, _, kb) = sides
        sa, sb = flat_state(ma, ka), flat_state(mb, kb)
        names = list(ka.mask_dict)
        out["updates"].append({
            "losses_equal": losses[0] == losses[1],
            "state_equal": [bool(torch.equal(bits(a), bits(b))) for a, b in zip(sa, sb)],
            "masks_equal": all(torch.equal(ka.mask_dict[n], kb.mask_dict[n]) for n in names) and names == list(kb.mask_dict),
            "threshold_equal": struct.pack("<d", ka.prune_threshold) == struct.pack("<d", kb.prune_threshold),
            "stats_equal": bool(ka.stats == kb.stats), "rates_equal": bool(ka.name2prune_rate == kb.name2prune_rate),
            "adjustments_equal": bool(ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth),
            "mask_step": [ka.mask_step, kb.mask_step], "density": kb.stats.total_density, "threshold": kb.prune_threshold})
    after = [[train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask) for _ in range(3)] for m, optim, sched, mask in sides]
    out["next_losses"] = after
    out["next_losses_equal"] = after[0] == after[1]
    return out


# ---- against the real reference --------------------------------------------------------------------------------------------
def case_golden(upd):
    c = load_captured("masking_pruning", Cfg(PRUNING, start_when=5, end_when=60, interval=5), upd)
    mask, d = c.mask, c.d
    mask.prune_threshold = float(d[c.pre + "prune_threshold"])
    mask.prune_rate_decay.current_prune_rate = float(d[c.pre + "rate"])
    c.out["target"] = math.ceil(mask.prune_rate * mask.baseline_nonzero)
    out = update_captured(c)
    want_t, want_g = float(d[c.post + "prune_threshold"]), float(d[c.post + "adjusted_growth"])
    out.update(threshold_rel_error=abs(mask.prune_threshold - want_t) / abs(want_t),
               growth_rel_error=abs(mask.adjusted_growth - want_g) / max(abs(want_g), 1.0))
    return out


# ---- refusals, launch count ------------------------------------------------------------------------------------------------
def prune_args(layers, target=10, rate=0.1, threshold=0.001, increment=0.2, tolerance=1e-6, dense=1, abi=E.SF_ABI_VERSION, n=None):
    arr = (C.c_int32 * max(len(layers), 1))(*layers)
    return E.sf_mask_prune_global_args(abi_version=abi, n_layers=len(layers) if n is None else n, layers=arr, target=target,
                                       prune_rate=rate, threshold=threshold, increment=increment, tolerance=tolerance,
                                       dense_gradients=dense, stats_dev=None), arr


def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    good = E.SirenEngine(8, 8, 64, 3)
    ones = torch.ones(good.num_params, device="cuda")
    handles = {"render": E.RenderEngine(8, 8, 64, 3), "fourier": E.FourierEngine(8, 8, 64, 3, 64),
               "wavelet": E.WaveletEngine(8, 8, 64, 3), "feather": E.SirenEngine(8, 8, 64, 3), "no_masks": E.SirenEngine(8, 8, 64, 3)}
    handles["feather"].feather_attach(68, 8, [64, 64, 3], [2, 64, 64])
    for eng in list(handles.values()) + [good]:
        eng.profile(True)
    args, keep = prune_args([0, 1, 2])
    for name, eng in handles.items():
        rec(name, lib.sf_mask_prune_global(eng.h, C.byref(args)))
    good.set_masks(ones)
    rec("null_handle", lib.sf_mask_prune_global(None, C.byref(args)))
    rec("null_args", lib.sf_mask_prune_global(good.h, None))
    bad, keep1 = prune_args([0, 1, 2])
    bad.layers = None
    rec("null_layers", lib.sf_mask_prune_global(good.h, C.byref(bad)))
    inf, nan = float("inf"), float("nan")
    for name, kw in (("wrong_abi", dict(abi=2)), ("layer_out_of_range", dict(layers=[0, 1, 3])),
                     ("layer_negative", dict(layers=[-1, 1])), ("not_ascending", dict(layers=[1, 1])),
                     ("descending", dict(layers=[2, 1])), ("no_layers", dict(layers=[])), ("too_many_layers", dict(n=4)),
                     ("threshold_zero", dict(threshold=0.0)), ("threshold_negative", dict(threshold=-0.001)),
                     ("threshold_inf", dict(threshold=inf)), ("threshold_nan", dict(threshold=nan)),
                     ("increment_zero", dict(increment=0.0)), ("increment_one", dict(increment=1.0)),
                     ("increment_nan", dict(increment=nan)), ("tolerance_negative", dict(tolerance=-1e-6)),
                     ("tolerance_inf", dict(tolerance=inf)), ("tolerance_nan", dict(tolerance=nan)),
                     ("target_negative", dict(target=-1))):
        a, keep2 = prune_args(**{"layers": [0, 1, 2], **kw})
        rec(name, lib.sf_mask_prune_global(good.h, C.byref(a)))
    out["launches_after_refusals"] = {name: launches(eng) for name, eng in list(handles.items()) + [("good", good)]}
    try:
        handles["wavelet"].mask_prune_global([0], 1, 0.1, 0.001, 0.2, 1e-6, True)
    except TypeError as e:
        out["binding_wavelet"] = "TypeError: " + str(e)
    rec("ok_update", lib.sf_mask_prune_global(good.h, C.byref(args)))
    rec("ok_without_stats_again", lib.sf_mask_prune_global(good.h, C.byref(args)))
    rep = good.profile_report()
    out["plan_after_two_updates"] = {k: v["launches"] for k, v in rep.items() if v["launches"]}
    for eng in list(handles.values()) + [good]:
        eng.profile(False)
        eng.close()
    return out


KERNELS = ("k_mask_count", "k_prune_file", "k_prune_scan", "k_prune_search", "k_prune_apply", "k_mask_update")


def traced(fn):
    """-> (fn(), how often each kernel of csrc/siren_mask.hip ran on the device meanwhile), from the device activity records
    of torch.profiler - the kernels themselves, not the engine's one profile record per call"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        got = fn()
        torch.cuda.synchronize()
    ran = {}
    for ev in prof.events():
        if "cuda" in str(ev.device_type).lower():
            for k in KERNELS:
                if k in ev.name:
                    ran[k] = ran.get(k, 0) + 1
    return got, ran


def case_launches():
    """the profile records and the kernels of one update: depth 3 and depth 8; a search of one trial and one of more than fifty"""
    out = {}
    for depth in (3, 8):
        eng = E.SirenEngine(8, 8, 64, depth)
        state = make_state(eng, 11)
        eng.profile(True)
        alive = int(state[4].sum())
        (_, rows), out[f"kernels_{depth}"] = traced(lambda: run_update(eng, state, list(range(depth)), alive // 10, 0.001, 0))
        out[str(depth)] = {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"]}
        out[f"trials_{depth}"] = int(rows[-1, TRIALS])
        eng.profile(False)
        eng.close()
    eng = E.SirenEngine(8, 8, 256, 3)
    state = make_state(eng, 12)
    sl = slices_of(eng, [0, 1, 2])
    mags = torch.cat([state[0][o:o + n] for o, n in sl]).abs()
    alive = int(sum(state[4][o:o + n].sum() for o, n in sl))
    exact = float(mags[mags > 0].sort().values[alive // 10])     # a threshold whose first count is the target
    target = alive - int((mags > exact).sum())
    eng.close()
    for name, threshold in (("few", exact), ("many", 0.05)):
        eng = E.SirenEngine(8, 8, 256, 3)       # (a handle's profile counters add up: one handle per search)
        eng.profile(True)
        (_, rows), out[f"kernels_{name}"] = traced(lambda: run_update(eng, state, [0, 1, 2], target, threshold, 1))
        out[name] = {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"]}
        out[f"trials_{name}"] = int(rows[-1, TRIALS])
        out[f"removed_{name}"] = int(rows[-1, REMOVED])
        eng.profile(False)
        eng.close()
    out["target"] = target
    return out


# ---- a whole fit -------------------------------------------------------------------------------------------------------------
def case_e2e(workdir):
    over = ["masking=Pruning", "quant=none", "img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4",
            "train.num_steps=60", "train.log_steps=20"]
    return fit_on_both_routes(workdir, over, "mask_prune_global")


if __name__ == "__main__":
    child_main({"abi": case_abi, "host": case_host, "golden": case_golden, "refuse": case_refuse, "launches": case_launches,
                "e2e": case_e2e})
