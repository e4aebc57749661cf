"""Child of tests/test_gpu_mask_update.py: sf_mask_update on an MI355X against tests/_mask_update_ref.py (the contract on the
CPU), against the host path of Masking.update_connections(), against the real reference's captured update
(tests/golden/masking_rigl.npz), its refusals, its launch count and a whole `fit`.  One case per process."""
import ctypes as C
import os

import torch

from _gpu_child import child_main
from _gpu_fixtures import launches, recorder
from _mask_fixtures import KNOB, RIGL, Cfg, bits, fit_on_both_routes, flat_state, load_captured, seeded_sides, slices_of, update_captured
from _mask_update_ref import WORDS, bits_rate, mask_update_ref
from implicit_image import _engine as E
from oracle import siren_oracle as so

HANDLES = [(32, 3), (64, 4), (256, 3), (512, 3)]           # layers of 64 .. 262 144 elements: below one workgroup, several
DENSITY = (0.5, 0.3, 0.6, 0.5)                             # 64-element steps per wave, the metric width's layer, the wide path
HOST_SHAPES = [(64, 4, 32), (256, 4, 64), (512, 3, 64)]    # hidden, depth, image side


# ---- 5. the ABI against the restatement ------------------------------------------------------------------------------------
def make_state(eng, seed, quantised, special):
    """[w, g, m, v, k] on the CPU.  quantised: multiples of 0.5 (heavy ties, live zeros, more zeros than dead + drop).
    special: all_live / capped - the largest layer wholly or 90 % live; few_candidates - nearly every gradient zero, so the
    growth budget exceeds the non-zero candidates"""
    gen = torch.Generator().manual_seed(seed)
    P = eng.num_params
    w, g = torch.randn(P, generator=gen) * 0.1, torch.randn(P, generator=gen) * 1e-3
    m, v, k = torch.randn(P, generator=gen) * 1e-3, torch.rand(P, generator=gen) * 1e-6, torch.ones(P)
    if quantised:
        w, g = torch.round(w * 20) * 0.5, torch.round(g * (250 if special == "few_candidates" else 2000)) * 0.5
    sl = slices_of(eng, range(eng.depth))
    big = max(range(eng.depth), key=lambda l: sl[l][1])
    for l, (off, n) in enumerate(sl):
        dens = {"all_live": 1.0, "capped": 0.9}.get(special, DENSITY[l % 4]) if l == big else DENSITY[l % 4]
        k[off:off + n] = (torch.rand(n, generator=gen) < dens).float()
        w[off:off + n] *= k[off:off + n]
    return [w.contiguous(), g.contiguous(), m, v, k]


def run_update(eng, state, layers, rate, growth, dense):
    w, g, m, v, k = (t.cuda() for t in state)
    eng.set_params(w)
    eng.set_masks(k)
    eng.set_grads(g)
    eng.set_adam_state(m, v, 3)
    rows = torch.full((len(layers) + 1, WORDS), -1, dtype=torch.int64, device="cuda")
    eng.mask_update(layers, rate, growth, dense, rows)
    mm, vv, _ = eng.get_adam_state()
    return [bits(t) for t in (eng.get_params(), eng.get_grads(), mm, vv, eng.view("masks").clone())], rows.cpu()


def case_abi(which):
    hidden, depth = HANDLES[int(which)]
    eng = E.SirenEngine(8, 8, hidden, depth)
    everything = list(range(depth))
    variants = [(f"{'q' if q else 'c'}_r{rate}_g{growth}_d{dense}", q, None, rate, growth, dense, everything)
                for q in (False, True) for rate in (0.0, 0.1, 0.3) for growth in (0, 1) for dense in (0, 1)]
    variants += [("all_live", False, "all_live", 0.3, 1, 0, everything), ("capped", False, "capped", 0.3, 1, 0, everything),
                 ("few_candidates", True, "few_candidates", 0.3, 1, 0, everything),
                 ("without_layer0", False, None, 0.1, 1, 1, everything[1:])]
    out = {"sizes": [n for _, n in slices_of(eng, everything)], "variants": {}}
    for seed, (name, q, special, rate, growth, dense, layers) in enumerate(variants):
        state = make_state(eng, 100 + seed, q, special)
        got, rows = run_update(eng, state, layers, rate, growth, dense)
        again, rows2 = run_update(eng, state, layers, rate, growth, dense)
        w_before = bits(state[0]).clone()
        ref_rows, tied = mask_update_ref(*state, slices_of(eng, layers), rate, growth, bool(dense))      # (in place: state is now the answer)
        diff = {key: int((a != bits(b)).sum()) for key, a, b in zip("wgmvk", got, state)}
        big = max(range(len(layers)), key=lambda j: slices_of(eng, layers)[j][1])
        out["variants"][name] = {
            "diff": diff, "rows_equal": bool(torch.equal(rows, ref_rows)),
            "repeat": all(torch.equal(a, b) for a, b in zip(got, again)) and bool(torch.equal(rows, rows2)),
            "tied": any(any(t) for t in tied), "removed": rows[:-1, 3].tolist(), "status": rows[-1].tolist(),
            "big_rate": bits_rate(rows[big, 7]), "big_removed": int(rows[big, 3]),
            "minus_zero": int(((got[0] == -2 ** 31) & (w_before != -2 ** 31)).sum()),
            "rows": rows.tolist() if not torch.equal(rows, ref_rows) else None,
            "ref_rows": ref_rows.tolist() if not torch.equal(rows, ref_rows) else None}
    # an all-zero network: the state is left alone and the status row says so
    state = make_state(eng, 7, False, None)
    state[0].zero_()
    got, rows = run_update(eng, state, everything, 0.3, 1, 0)
    out["all_zero"] = {"status": int(rows[-1, 0]), "untouched": all(torch.equal(a, bits(b)) for a, b in zip(got, state))}
    eng.close()
    return out


# ---- 6. against the host path ----------------------------------------------------------------------------------------------
def case_host(which, density, dense):
    from implicit_image.data import get_grid
    from implicit_image.utils.train_helper import train_epoch
    hidden, depth, side = HOST_SHAPES[int(which)]
    grid, img = get_grid(side, side).cuda(), so.synthetic_image(side, side, seed=3).cuda().contiguous()
    sides = seeded_sides(Cfg(RIGL, density=float(density), dense_gradients=dense == "1"), hidden, depth)
    out = {"updates": [], "tied": [], "device_updates": [0, 0]}
    for u in range(4):
        losses = [[train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask) for _ in range(3)]
                  for m, optim, sched, mask in sides]
        # is any selection boundary of this update tied?  from the host side's tensors, with the restatement
        m0, _, _, k0 = sides[0]
        names = [n for n, _ in m0.named_parameters() if n in k0.mask_dict]
        layers = [i // 2 for i, (n, _) in enumerate(m0.named_parameters()) if n in k0.mask_dict]
        _, tied = mask_update_ref(*flat_state(m0, k0), slices_of(m0.bound_engine, layers), k0.prune_rate, 1, dense == "1")
        out["tied"].append(any(any(t) for t in tied))
        for side, (m, optim, sched, mask) in enumerate(sides):
            os.environ[KNOB] = "0" if side == 0 else "1"
            pending = len(mask._pending)
            mask.update_connections()
            out["device_updates"][side] += len(mask._pending) - pending
        os.environ.pop(KNOB)
        (ma, _, _, ka), (mb, _, _, kb) = sides
        sa, sb = flat_state(ma, ka), flat_state(mb, kb)
        out["updates"].append({
            "losses_equal": losses[0] == losses[1],
            "state_equal": [bool(torch.equal(bits(a), bits(b))) for a, b in zip(sa, sb)],
            "masks_equal": all(torch.equal(ka.mask_dict[n], kb.mask_dict[n]) for n in names) and list(ka.mask_dict) == list(kb.mask_dict),
            "stats_equal": bool(ka.stats == kb.stats), "rates_equal": bool(ka.name2prune_rate == kb.name2prune_rate),
            "adjustments_equal": bool(ka.adjustments == kb.adjustments and ka.adjusted_growth == kb.adjusted_growth),
            "mask_step": [ka.mask_step, kb.mask_step], "removed_total": int(sum(ka.adjustments)),
            "nonzero": ka.stats.total_nonzero})
    after = [[train_epoch(m, optim, grid, img, lr_scheduler=sched, mask=mask) for _ in range(3)] for m, optim, sched, mask in sides]
    out["next_losses"] = after
    out["next_losses_equal"] = after[0] == after[1]
    return out


# ---- 7. against the real reference -----------------------------------------------------------------------------------------
def case_golden(upd):
    c = load_captured("masking_rigl", Cfg(RIGL, end_when=60, interval=5), upd)
    mask, d = c.mask, c.d
    for s_ in range(mask.mask_step):
        mask.prune_rate_decay.step(s_)
    c.out["rate_error"] = abs(mask.prune_rate - float(d[c.pre + "rate"]))
    out = update_captured(c)
    out["growth_error"] = abs(mask.adjusted_growth - float(d[c.post + "adjusted_growth"]))
    return out


# ---- 8. refusals, 9. launch count ------------------------------------------------------------------------------------------
def update_args(layers, rate=0.1, growth=1, dense=1, abi=E.SF_ABI_VERSION, n=None):
    arr = (C.c_int32 * max(len(layers), 1))(*layers)
    return E.sf_mask_update_args(abi_version=abi, n_layers=len(layers) if n is None else n, layers=arr, prune_rate=rate,
                                 growth=growth, dense_gradients=dense, stats_dev=None), arr


def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    lin = torch.linspace(0, 1, 8).cuda()
    good = E.SirenEngine(8, 8, 64, 3)
    ones = torch.ones(good.num_params, device="cuda")
    handles = {"render": E.RenderEngine(8, 8, 64, 3), "fourier": E.FourierEngine(8, 8, 64, 3, 64),
               "wavelet": E.WaveletEngine(8, 8, 64, 3), "feather": E.SirenEngine(8, 8, 64, 3), "no_masks": E.SirenEngine(8, 8, 64, 3)}
    handles["feather"].feather_attach(68, 8, [64, 64, 3], [2, 64, 64])
    for eng in list(handles.values()) + [good]:
        eng.profile(True)
    args, keep = update_args([0, 1, 2])
    for name, eng in handles.items():
        rec(name, lib.sf_mask_update(eng.h, C.byref(args)))
    good.set_masks(ones)
    rec("null_handle", lib.sf_mask_update(None, C.byref(args)))
    rec("null_args", lib.sf_mask_update(good.h, None))
    bad, keep1 = update_args([0, 1, 2])
    bad.layers = None
    rec("null_layers", lib.sf_mask_update(good.h, C.byref(bad)))
    for name, kw in (("wrong_abi", dict(layers=[0, 1, 2], abi=2)), ("layer_out_of_range", dict(layers=[0, 1, 3])),
                     ("layer_negative", dict(layers=[-1, 1])), ("not_ascending", dict(layers=[1, 1])),
                     ("descending", dict(layers=[2, 1])), ("no_layers", dict(layers=[])),
                     ("too_many_layers", dict(layers=[0, 1, 2], n=4)), ("growth_2", dict(layers=[0, 1, 2], growth=2)),
                     ("growth_negative", dict(layers=[0, 1, 2], growth=-1))):
        a, keep2 = update_args(**kw)
        rec(name, lib.sf_mask_update(good.h, C.byref(a)))
    out["launches_after_refusals"] = {name: launches(eng) for name, eng in list(handles.items()) + [("good", good)]}
    try:
        handles["wavelet"].mask_update([0], 0.1, 1, True)
    except TypeError as e:
        out["binding_wavelet"] = "TypeError: " + str(e)
    rec("ok_update", lib.sf_mask_update(good.h, C.byref(args)))
    rec("ok_without_stats_again", lib.sf_mask_update(good.h, C.byref(args)))
    rep = good.profile_report()
    out["plan_after_two_updates"] = {k: v["launches"] for k, v in rep.items() if v["launches"]}
    for eng in list(handles.values()) + [good]:
        eng.profile(False)
        eng.close()
    return out


def case_launches():
    out = {}
    for depth in (3, 8):
        eng = E.SirenEngine(8, 8, 64, depth)
        state = make_state(eng, 11, False, None)
        eng.profile(True)
        run_update(eng, state, list(range(depth)), 0.3, 1, 0)
        out[str(depth)] = {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"]}
        eng.profile(False)
        eng.close()
    return out


# ---- 10. a whole fit -------------------------------------------------------------------------------------------------------
def case_e2e(workdir):
    over = ["masking=RigL", "quant=none", "img.height=64", "img.width=64", "mlp.hidden_size=64", "mlp.depth=4",
            "train.num_steps=60", "train.log_steps=20", "masking.interval=10"]
    return fit_on_both_routes(workdir, over, "mask_update")


if __name__ == "__main__":
    child_main({"abi": case_abi, "host": case_host, "golden": case_golden, "refuse": case_refuse, "launches": case_launches,
                "e2e": case_e2e})
