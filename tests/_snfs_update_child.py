"""Child of tests/test_gpu_snfs_update.py: sf_mask_update_snfs on an MI355X against tests/_snfs_ref.py (the contract on the
CPU), against the real reference's captured updates (tests/golden/masking_snfs.npz), against the host path of
Masking.update_connections(), its refusals, its launch count and a whole `fit`.  One case per process."""
import ctypes as C
import json
import os

import torch

from _gpu_child import child_main
from _gpu_fixtures import launches, recorder
from _mask_fixtures import KNOB, Cfg, bits, flat_state, load_captured, slices_of, update_captured
from _mask_update_child import HANDLES, make_state
from _snfs_ref import WORDS, snfs_update_ref
from implicit_image import _engine as E
from oracle import siren_oracle as so

# conf/masking/SNFS.yaml
SNFS = Cfg(name="SNFS", density=0.05, sparse_init="erdos-renyi-kernel", dense_gradients=True, growth_mode="momentum",
           prune_mode="magnitude", redistribution_mode="momentum", dense=False, prune_rate=0.1, decay_schedule="cosine",
           end_when=1500, interval=20)
HOST_SHAPES = [(64, 4, 32, 0), (256, 4, 64, 1)]             # hidden, depth, image side, model seed
MARGIN = 1e-4       # a rounding or truncation margin below this is reported: the statistic's relative distance from an fp32
#                     mean, about 2^-22, times a pool of a few hundred, times ten


# ---- the ABI against the restatement -----------------------------------------------------------------------------------
def snfs_state(eng, seed, quantised, special):
    """make_state's [w, g, m, v, k] with moments to match: quantised - m in multiples of 0.5 over v = 0.25, so that the
    momentum keys tie heavily; all_live / capped - the largest layer, wholly or 90 % live, also holds four times the
    momentum of the others, so that its share of the statistic exceeds 1 / L and the rate cap applies to it;
    one_adam_step - the moments one Adam step leaves behind gradients of order one (every |momentum| within a few ulp of
    sqrt(10)); few_candidates - a moment in one element of a hundred, so that the budget exceeds the non-zero candidates"""
    w, g, m, v, k = make_state(eng, seed, quantised, special if special in ("all_live", "capped") else None)
    gen = torch.Generator().manual_seed(seed + 1000)
    if quantised:
        m, v = torch.round(m * 2000) * 0.5, torch.full_like(v, 0.25)
    if special in ("all_live", "capped"):
        off, n = max(slices_of(eng, range(eng.depth)), key=lambda s: s[1])
        m[off:off + n] *= 4.0
    if special == "one_adam_step":
        g = g * 1000.0
        m, v = 0.1 * g, 0.001 * g * g
    if special == "few_candidates":
        m = m * (torch.rand(m.numel(), generator=gen) < 0.01).float()
    return [w, g, m.contiguous(), v.contiguous(), k]


def load(eng, state):
    w, g, m, v, k = (t.cuda() for t in state)
    eng.set_params(w)
    eng.set_masks(k)
    eng.set_grads(g)
    eng.set_adam_state(m, v, 3)


def read(eng):
    mm, vv, _ = eng.get_adam_state()
    return [bits(t) for t in (eng.get_params(), eng.get_grads(), mm, vv, eng.view("masks").clone())]


def run_update(eng, state, layers, rate, adj, growth, statistic, dense):
    load(eng, state)
    rows = torch.full((len(layers) + 1, WORDS), -1, dtype=torch.int64, device="cuda")
    eng.mask_update_snfs(layers, rate, adj, growth, statistic, dense, rows)
    return read(eng), rows.cpu()


def case_abi(which):
    hidden, depth = HANDLES[int(which)]
    eng = E.SirenEngine(8, 8, hidden, depth)
    everything = list(range(depth))
    variants, i = [], 0
    for q in (False, True):
        for rate in (0.0, 0.1, 0.3):
            for growth in (1, 2):
                for statistic in (0, 1):
                    dense, adj = (i // 3) & 1, (0.0, 3.5)[(i // 5) & 1]       # (periods that share nothing with the loops')
                    variants.append((f"{'q' if q else 'c'}_r{rate}_g{growth}_s{statistic}_d{dense}_a{adj}", q, None, rate, adj, growth,
                                     statistic, dense, everything))
                    i += 1
    variants += [("all_live", False, "all_live", 0.3, 3.5, 2, 1, 1, everything),
                 ("capped", False, "capped", 0.3, 0.0, 2, 1, 0, everything),
                 ("one_adam_step", False, "one_adam_step", 0.3, 3.5, 2, 1, 1, everything),
                 ("few_candidates", False, "few_candidates", 0.3, 0.0, 2, 1, 1, everything),
                 ("without_layer0", False, None, 0.1, 3.5, 2, 1, 1, everything[1:])]
    out = {"sizes": [n for _, n in slices_of(eng, everything)], "variants": {}}
    for seed, (name, q, special, rate, adj, growth, statistic, dense, layers) in enumerate(variants):
        state = snfs_state(eng, 200 + seed, q, special)
        got, rows = run_update(eng, state, layers, rate, adj, growth, statistic, dense)
        again, rows2 = run_update(eng, state, layers, rate, adj, growth, statistic, dense)
        sl = slices_of(eng, layers)
        ref_rows, info = snfs_update_ref(*state, sl, rate, adj, growth, statistic, bool(dense))      # (in place)
        big = max(range(len(layers)), key=lambda j: sl[j][1])
        same = bool(torch.equal(rows, ref_rows))
        out["variants"][name] = {
            "diff": {key: int((a != bits(b)).sum()) for key, a, b in zip("wgmvk", got, state)}, "rows_equal": same,
            "repeat": all(torch.equal(a, b) for a, b in zip(got, again)) and bool(torch.equal(rows, rows2)),
            "tied": [any(t[0] for t in info["tied"]), any(t[1] for t in info["tied"])], "status": rows[-1].tolist(),
            "removed": rows[:-1, 3].tolist(), "grown": rows[:-1, 10].tolist(), "layers": len(layers),
            "big": {"live_before": int(rows[big, 0]), "dead_before": int(rows[big, 1]), "removed": int(rows[big, 3]),
                    "grown": int(rows[big, 10]), "rate": E.sf_mask_snfs_stats.from_buffer_copy(rows[big].numpy().tobytes()).prune_rate},
            "rows": None if same else rows.tolist(), "ref_rows": None if same else ref_rows.tolist()}
    # what leaves the state untouched: every moment zero (status 1), a layer with no live weight, one NaN moment (status 3)
    for name, status in (("all_moments_zero", 1), ("no_live_weight", 3), ("nan_moment", 3)):
        state = snfs_state(eng, 7, False, None)
        off, n = slices_of(eng, everything)[1]
        if name == "all_moments_zero":
            state[2].zero_()
        if name == "no_live_weight":
            state[4][off:off + n] = 0.0
            state[0][off:off + n] = 0.0
        if name == "nan_moment":
            state[2][off + n // 2] = float("nan")
        got, rows = run_update(eng, state, everything, 0.3, 3.5, 2, 1, 0)
        before = [bits(t).clone() for t in state]
        ref_rows, _ = snfs_update_ref(*state, slices_of(eng, everything), 0.3, 3.5, 2, 1, False)
        out[name] = {"status": int(rows[-1, 0]), "untouched": all(torch.equal(a, b) for a, b in zip(got, before)),
                     "rows_equal": bool(torch.equal(rows, ref_rows)), "expected": status}
    # growth 1, statistic 0 against sf_mask_update on the same state
    state = snfs_state(eng, 9, False, None)
    got, _ = run_update(eng, state, everything, 0.3, 0.0, 1, 0, 0)
    load(eng, state)
    eng.mask_update(everything, 0.3, 1, False)
    out["equals_sf_mask_update"] = all(torch.equal(a, b) for a, b in zip(got, read(eng)))
    eng.close()
    return out


# ---- against the real reference ----------------------------------------------------------------------------------------
def case_golden(upd):
    c = load_captured("masking_snfs", Cfg(SNFS, density=0.3, end_when=60, interval=5), upd)
    mask, d = c.mask, c.d
    for s_ in range(mask.mask_step):
        mask.prune_rate_decay.step(s_)
    c.out["rate_error"] = abs(mask.prune_rate - float(d[c.pre + "rate"]))
    out = update_captured(c)
    out["growth_error"] = abs(mask.adjusted_growth - float(d[c.post + "adjusted_growth"]))
    return out


# ---- the device route against the host path ----------------------------------------------------------------------------
def seeded_sides(mcfg, hidden, depth, seed):
    """two (model, optimiser, scheduler, mask) from the seed `seed` on the device: the host side and the device side"""
    from implicit_image.models import registry
    from implicit_image.utils.train_helper import get_optimizer_lr_scheduler, setup_mask
    sides = []
    for _ in range(2):
        torch.manual_seed(seed)
        m = registry["siren"](depth=depth, hidden_size=hidden, first_omega_0=50, hidden_omega_0=30).to("cuda")
        optim, sched = get_optimizer_lr_scheduler(m, Cfg(name="adam", lr=3e-4))
        sides.append((m, optim, sched, setup_mask(m, optim, mcfg)))
    return sides


def case_host(which):
    from implicit_image.data import get_grid
    from implicit_image.utils.train_helper import train_epoch
    hidden, depth, side, seed = HOST_SHAPES[int(which)]
    grid, img = get_grid(side, side).cuda(), so.synthetic_image(side, side, seed=3).cuda().contiguous()
    sides = seeded_sides(SNFS, hidden, depth, seed)
    out = {"updates": [], "flags": [], "device_updates": [0, 0], "fallbacks": 0}
    for u in range(6):                          # (until four updates ran on the device: one that finds adjusted_growth negative does not)
        if out["device_updates"][1] == 4:
            break
        losses = [[train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask) for _ in range(5)]
                  for m, optim, sched, mask in sides]
        # the restatement on the host side's tensors: is a boundary tied or nearly so, is a budget near its rounding?
        m0, _, _, k0 = sides[0]
        layers = [i // 2 for i, (n, _) in enumerate(m0.named_parameters()) if n in k0.mask_dict]
        names = [n for n, _ in m0.named_parameters() if n in k0.mask_dict]
        pool_extra = float(k0.adjusted_growth)
        if pool_extra < 0:                      # this update runs on the host on both sides: nothing of the route to flag
            out["fallbacks"] += 1
            out["flags"].append({"tied": False, "near": False, "margin": False, "fallback": True})
        else:
            _, info = snfs_update_ref(*flat_state(m0, k0), slices_of(m0.bound_engine, layers), k0.prune_rate, pool_extra, 2, 1, True)
            out["flags"].append({"tied": any(any(t) for t in info["tied"]), "near": any(info["near"]),
                                 "margin": bool(min(info["half"], info["whole"]) < MARGIN), "half": info["half"],
                                 "whole": info["whole"]})
        for side_, (m, optim, sched, mask) in enumerate(sides):
            os.environ[KNOB] = "0" if side_ == 0 else "1"
            before = len(mask._pending)
            mask.update_connections()
            out["device_updates"][side_] += len(mask._pending) - before      # (nothing was pending: the statistics were read)
        os.environ.pop(KNOB)
        (ma, _, _, ka), (mb, _, _, kb) = sides
        sa, sb = flat_state(ma, ka), flat_state(mb, kb)
        close = lambda x, y: abs(x - y) <= 1e-5 * abs(y)
        out["updates"].append({
            "losses_equal": losses[0] == losses[1],
            "state_equal": [bool(torch.equal(bits(a), bits(b))) for a, b in zip(sa, sb)],
            "masks_equal": all(torch.equal(ka.mask_dict[n], kb.mask_dict[n]) for n in names) and list(ka.mask_dict) == list(kb.mask_dict),
            "counts_equal": bool(ka.stats.nonzeros_dict == kb.stats.nonzeros_dict and ka.stats.zeros_dict == kb.stats.zeros_dict),
            "variance_close": all(close(kb.stats.variance_dict[n], ka.stats.variance_dict[n]) for n in names),
            "rates_equal": bool(ka.name2prune_rate == kb.name2prune_rate),
            "adjustments_equal": bool(ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth),
            "mask_step": [ka.mask_step, kb.mask_step], "adjustments": [int(x) for x in ka.adjustments]})
    return out


# ---- refusals, the launch count ----------------------------------------------------------------------------------------
def snfs_args(layers, rate=0.1, adj=0.0, growth=2, statistic=1, dense=1, abi=E.SF_ABI_VERSION, n=None):
    arr = (C.c_int32 * max(len(layers), 1))(*layers)
    return E.sf_mask_update_snfs_args(abi_version=abi, n_layers=len(layers) if n is None else n, layers=arr, prune_rate=rate,
                                      adjusted_growth=adj, growth=growth, statistic=statistic, dense_gradients=dense,
                                      stats_dev=None), arr


def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    good = E.SirenEngine(8, 8, 64, 3)
    handles = {"render": E.RenderEngine(8, 8, 64, 3), "fourier": E.FourierEngine(8, 8, 64, 3, 64),
               "wavelet": E.WaveletEngine(8, 8, 64, 3), "feather": E.SirenEngine(8, 8, 64, 3), "no_masks": E.SirenEngine(8, 8, 64, 3)}
    handles["feather"].feather_attach(68, 8, [64, 64, 3], [2, 64, 64])
    for eng in list(handles.values()) + [good]:
        eng.profile(True)
    args, keep = snfs_args([0, 1, 2])
    for name, eng in handles.items():
        rec(name, lib.sf_mask_update_snfs(eng.h, C.byref(args)))
    load(good, snfs_state(good, 5, False, None))
    rec("null_handle", lib.sf_mask_update_snfs(None, C.byref(args)))
    rec("null_args", lib.sf_mask_update_snfs(good.h, None))
    bad, keep1 = snfs_args([0, 1, 2])
    bad.layers = None
    rec("null_layers", lib.sf_mask_update_snfs(good.h, C.byref(bad)))
    for name, kw in (("wrong_abi", dict(abi=2)), ("layer_out_of_range", dict(layers=[0, 1, 3])), ("layer_negative", dict(layers=[-1, 1])),
                     ("not_ascending", dict(layers=[1, 1])), ("descending", dict(layers=[2, 1])), ("no_layers", dict(layers=[])),
                     ("too_many_layers", dict(n=4)), ("growth_0", dict(growth=0)), ("growth_3", dict(growth=3)),
                     ("statistic_2", dict(statistic=2)), ("adjusted_growth_negative", dict(adj=-1.0)),
                     ("adjusted_growth_nan", dict(adj=float("nan"))), ("adjusted_growth_inf", dict(adj=float("inf")))):
        a, keep2 = snfs_args(**{"layers": [0, 1, 2], **kw})
        rec(name, lib.sf_mask_update_snfs(good.h, C.byref(a)))
    out["launches_after_refusals"] = {name: launches(eng) for name, eng in list(handles.items()) + [("good", good)]}
    try:
        handles["wavelet"].mask_update_snfs([0], 0.1, 0.0, 2, 1, True)
    except TypeError as e:
        out["binding_wavelet"] = "TypeError: " + str(e)
    rec("ok_update", lib.sf_mask_update_snfs(good.h, C.byref(args)))
    rec("ok_without_stats_again", lib.sf_mask_update_snfs(good.h, C.byref(args)))
    out["plan_after_two_updates"] = {k: v["launches"] for k, v in good.profile_report().items() if v["launches"]}
    for eng in list(handles.values()) + [good]:
        eng.profile(False)
        eng.close()
    return out


def case_launches():
    out = {}
    # (rate 0: the pool is adjusted_growth alone, no layer reaches its cap, one round; all_live: a cap of 0, until underflow)
    for name, depth, special, rate in (("3", 3, None, 0.0), ("8", 8, None, 0.3), ("underflow", 3, "all_live", 0.3)):
        eng = E.SirenEngine(8, 8, 64, depth)
        state = snfs_state(eng, 11, False, special)
        eng.profile(True)
        _, rows = run_update(eng, state, list(range(depth)), rate, 3.5, 2, 1, 1)
        out[name] = {"plan": {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"]},
                     "rounds": int(rows[-1, 1]), "status": int(rows[-1, 0])}
        eng.profile(False)
        eng.close()
    return out


# ---- a whole fit -------------------------------------------------------------------------------------------------------
def case_e2e(workdir):
    from _gpu_child import ROOT
    from implicit_image import fit
    from implicit_image.config import load_config
    over = ["masking=SNFS", "quant=none", "img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4",
            "train.num_steps=60", "train.log_steps=20", "masking.interval=10"]
    out, calls, masks, plain, plain_setup = {}, [0], [], E.SirenEngine.mask_update_snfs, fit.setup_mask

    def counted(self, *a, **kw):
        calls[0] += 1
        return plain(self, *a, **kw)

    def kept(*a, **kw):
        masks.append(plain_setup(*a, **kw))
        return masks[-1]
    E.SirenEngine.mask_update_snfs, fit.setup_mask = counted, kept
    for side, knob in (("host", "0"), ("device", "1"), ("device_again", "1")):
        os.environ[KNOB] = knob
        calls[0] = 0
        run_dir = os.path.join(workdir, side)
        fit.fit_one(load_config(os.path.join(ROOT, "conf"), over), torch.device("cuda", 0), run_dir)
        sd = torch.load(os.path.join(run_dir, "model.pth"), weights_only=True)["state_dict"]
        mask = masks[-1]
        dead_nonzero = sum(int(((mask.mask_dict[n].cpu() == 0) & (sd[n] != 0)).sum()) for n in mask.mask_dict)
        live = sum(int(k.sum().item()) for k in mask.mask_dict.values())
        out[side] = {"device_updates": calls[0], "PSNR": json.load(open(os.path.join(run_dir, "result.json")))["PSNR"],
                     "dead_nonzero": dead_nonzero, "live": live, "booked": int(mask.baseline_nonzero - mask.adjustments[-1]),
                     "updates": len(mask.adjustments), "density": live / max(mask.total_params, 1)}
    os.environ.pop(KNOB)
    a, b = (open(os.path.join(workdir, s, "model.pth"), "rb").read() for s in ("device", "device_again"))
    out["pth_equal"], out["pth_bytes"] = a == b, len(a)
    return out


if __name__ == "__main__":
    child_main({"abi": case_abi, "golden": case_golden, "host": case_host, "refuse": case_refuse, "launches": case_launches,
                "e2e": case_e2e})
