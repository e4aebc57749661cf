"""Child of tests/test_gpu_kmeans.py: sf_kmeans_fit on an MI355X against tests/_kmeans_ref.py (the contract on the CPU), bit
for bit: the rows of the case table through SirenEngine.kmeans_fit, the raw C ABI with its optional outputs, a handle that
is used again, the refusals, and a quantise phase over a layer without a non-zero weight.  One case per process."""
import ctypes as C
import json
import os

import numpy as np
import torch

import _kmeans_ref as R
from _gpu_child import ROOT, child_main
from _gpu_fixtures import launches, recorder
from implicit_image import _engine as E
from implicit_image.pipeline.quant.kmeans import native_guess

GROUPS = [["five_iterations", "stops_at_three", "bits8_empty_bins", "fewer_points_than_centres", "constant_layer", "plus_minus",
           "quantised", "wide_range", "single_weight"],
          ["bits9_limit"],
          ["pruned_minus_zero", "grid_stride"]]
SENTINEL = 7.0                                 # what the output buffers of a raw call hold before it


def i32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def engine():
    return E.SirenEngine(8, 8, 64, 3)


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def all_zero():
    """a layer without a non-zero weight, both zeros in it"""
    w = np.zeros(4097, np.float32)
    w[::3] = -0.0
    return w


def device_fit(eng, w, K, **kw):
    """w through eng.kmeans_fit with the guess find_centroids_native builds -> (the outputs on the CPU, that guess)"""
    wt = torch.tensor(w).cuda()
    guess = native_guess(wt, K)
    centres = torch.empty(K, device="cuda")
    cent, ncent, labels, new_w = eng.kmeans_fit(wt, guess, centres_out=centres, **kw)
    return {"centroids": cent.cpu().numpy(), "n_centroids": int(ncent.item()), "labels": labels.cpu().numpy(),
            "new_weight": new_w.cpu().numpy(), "centres": centres.cpu().numpy()}, guess.cpu().numpy()


def mismatches(got, ref):
    """how many entries of each output the call wrote differ from the restatement's: floats as int32 views (-0.0 counts)"""
    out = {}
    for key in ("centroids", "new_weight", "centres"):
        if key in got:
            out[key] = int((i32(got[key]) != i32(ref[key])).sum()) if got[key].shape == ref[key].shape else -1
    if "labels" in got:
        out["labels"] = int((got["labels"].astype(np.int64) != ref["labels"]).sum())
    if "n_centroids" in got:
        out["n_centroids"] = int(got["n_centroids"] != ref["n_centroids"])
    return out


def same_bits(a, b):
    def bits(k, v):
        return v if k in ("labels", "n_centroids") else i32(v)
    return a.keys() == b.keys() and all(np.array_equal(bits(k, a[k]), bits(k, b[k])) for k in a)


# ---- the case table through the binding ------------------------------------------------------------------------------------
def case_abi(group):
    eng, out = engine(), {"cus": cus(), "rows": {}}
    for name in GROUPS[int(group)]:
        K = R.K_OF[name]
        w = R.make_input(name, out["cus"])
        got, guess = device_fit(eng, w, K)
        again, _ = device_fit(eng, w, K)
        ref = R.kmeans_ref(w, guess)
        n = ref.n_centroids
        row = {"n": int(w.size), "K": K, "diff": mismatches(got, ref), "repeat": same_bits(got, again),
               "iterations": ref.iterations, "n_centroids": got["n_centroids"], "ref_n_centroids": n,
               "padding_zero": not i32(got["centroids"][got["n_centroids"]:]).any(),
               "condition": R.row_condition(name, w, ref, out["cus"]),
               "guess_as_on_the_cpu": bool(np.array_equal(i32(guess), i32(R.linspace_guess(w, K)))),
               "minus_zero_in": int(((w == 0) & np.signbit(w)).sum()),
               "minus_zero_out": int(((got["new_weight"] == 0) & np.signbit(got["new_weight"])).sum())}
        if name == "stops_at_three":           # the launches after `done` leave the centres alone: iter_limit 3 gives the same
            at3, _ = device_fit(eng, w, K, iter_limit=3)        # centres as 5, iter_limit 2 other ones
            at2, _ = device_fit(eng, w, K, iter_limit=2)
            row["same_at_3"] = bool(np.array_equal(i32(at3["centres"]), i32(got["centres"])))
            row["same_at_2"] = bool(np.array_equal(i32(at2["centres"]), i32(got["centres"])))
        out["rows"][name] = row
    # a layer without a non-zero weight, and the same through find_centroids_native
    w = all_zero()
    got, guess = device_fit(eng, w, 31)
    ref = R.kmeans_ref(w, guess)
    out["all_zero"] = {"diff": mismatches(got, ref), "n_centroids": got["n_centroids"], "empty": bool(ref.empty),
                       "guess_finite": bool(np.isfinite(guess).any()), "labels_nonzero": int((got["labels"] != 0).sum()),
                       "new_weight_bits_set": bool(i32(got["new_weight"]).any()), "centroid_bits_set": bool(i32(got["centroids"]).any())}
    eng.close()
    return out


# ---- the C ABI itself ------------------------------------------------------------------------------------------------------
def raw_fit(lib, eng, w, guess, iter_limit=5, tol=1e-4, cap=None, labels=True, new_w=True, ncent=True):
    """lib.sf_kmeans_fit with output buffers that hold a sentinel before the call -> (rc, the outputs that were asked for)"""
    K = guess.size
    cap = K + 1 if cap is None else cap
    wt, centres = torch.tensor(w).cuda(), torch.tensor(guess).cuda()
    cent = torch.full((cap,), SENTINEL, device="cuda")
    nc = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    lab = torch.full((w.size,), -1, dtype=torch.int64, device="cuda")
    nw = torch.full((w.size,), SENTINEL, device="cuda")
    rc = lib.sf_kmeans_fit(eng.h, wt.data_ptr(), w.size, centres.data_ptr(), K, iter_limit, tol, cent.data_ptr(), cap,
                           nc.data_ptr() if ncent else None, lab.data_ptr() if labels else None, nw.data_ptr() if new_w else None)
    torch.cuda.synchronize()
    got = {"centroids": cent.cpu().numpy(), "centres": centres.cpu().numpy()}
    if ncent:
        got["n_centroids"] = int(nc.item())
    if labels:
        got["labels"] = lab.cpu().numpy()
    if new_w:
        got["new_weight"] = nw.cpu().numpy()
    untouched = bool((nc == -1).all()) == (not ncent) and bool((lab == -1).all()) == (not labels) and bool((nw == SENTINEL).all()) == (not new_w)
    return int(rc), got, untouched


def case_abi_raw():
    lib, eng, out = E.load_library(), engine(), {}
    w = R.make_input("five_iterations")
    guess = R.linspace_guess(w, 31)
    variants = {"full": {}, "iter_limit_0": dict(iter_limit=0), "iter_limit_1": dict(iter_limit=1), "tol_0": dict(tol=0.0),
                "tol_1e30": dict(tol=1e30), "no_labels": dict(labels=False), "no_new_weight": dict(new_w=False),
                "no_n_centroids": dict(ncent=False), "centroids_only": dict(labels=False, new_w=False, ncent=False),
                "cap_larger": dict(cap=31 + 1 + 9)}
    full = None
    for name, kw in variants.items():
        rc, got, untouched = raw_fit(lib, eng, w, guess, **kw)
        ref = R.kmeans_ref(w, guess, **{k: v for k, v in kw.items() if k in ("iter_limit", "tol", "cap")})
        full = got if name == "full" else full
        out[name] = {"rc": rc, "diff": mismatches(got, ref), "iterations": ref.iterations, "n_centroids": ref.n_centroids,
                     "null_outputs_untouched": untouched, "outputs": sorted(got),
                     "as_full": all(np.array_equal(got[k], full[k]) for k in got) if "cap" not in kw and not (
                         "iter_limit" in kw or "tol" in kw) else None,
                     "centres_are_the_guess": bool(np.array_equal(i32(got["centres"]), i32(guess)))}
    # tol = 0 on the input that stops at three: it never stops
    w3 = R.make_input("stops_at_three")
    g3 = R.linspace_guess(w3, 31)
    rc, got, _ = raw_fit(lib, eng, w3, g3, tol=0.0)
    ref = R.kmeans_ref(w3, g3, tol=0.0)
    out["tol_0_where_it_would_stop"] = {"rc": rc, "diff": mismatches(got, ref), "iterations": ref.iterations}
    # a layer without a non-zero weight at iter_limit 0: no k_km_update turns the NaN guess into empty bins before k_km_finish
    wz = all_zero()
    gz = R.linspace_guess(wz, 31)
    rc, got, _ = raw_fit(lib, eng, wz, gz, iter_limit=0)
    ref = R.kmeans_ref(wz, gz, iter_limit=0)
    out["all_zero_iter_limit_0"] = {"rc": rc, "diff": mismatches(got, ref), "iterations": ref.iterations,
                                    "n_centroids": got["n_centroids"], "empty": bool(ref.empty)}
    eng.close()
    return out


# ---- a used workspace ------------------------------------------------------------------------------------------------------
def case_reuse():
    order = [("bits9_limit", R.K_OF["bits9_limit"]), ("single_weight", R.K_OF["single_weight"]), ("all_zero", 31),
             ("five_iterations", R.K_OF["five_iterations"])]
    inputs = {name: all_zero() if name == "all_zero" else R.make_input(name) for name, _ in order}
    used, out = engine(), {}
    for name, K in order:
        got, guess = device_fit(used, inputs[name], K)
        fresh_eng = engine()
        fresh, _ = device_fit(fresh_eng, inputs[name], K)
        fresh_eng.close()
        out[name] = {"as_fresh": same_bits(got, fresh), "diff": mismatches(got, R.kmeans_ref(inputs[name], guess)),
                     "n_centroids": got["n_centroids"]}
    used.close()
    return out


# ---- refusals --------------------------------------------------------------------------------------------------------------
def case_refuse():
    lib = E.load_library()
    out, rec = recorder(lib)
    eng, render = engine(), E.RenderEngine(8, 8, 64, 3)
    for e in (eng, render):
        e.profile(True)
    w = torch.randn(64, generator=torch.Generator().manual_seed(0)).clamp(-3, 3).cuda()
    guess = torch.linspace(-4, -3, 511).cuda()                     # (any 2 .. 511 of them bracket the weights in magnitude)
    cent = torch.full((600,), SENTINEL, device="cuda")
    lab = torch.full((64,), -1, dtype=torch.int64, device="cuda")
    p = dict(h=eng.h, w=w.data_ptr(), n=64, centers=guess.data_ptr(), K=31, iters=5, cent=cent.data_ptr(), cap=32)

    def call(**kw):
        a = dict(p, **kw)
        return lib.sf_kmeans_fit(a["h"], a["w"], a["n"], a["centers"], a["K"], a["iters"], 1e-4, a["cent"], a["cap"], None,
                                 lab.data_ptr(), None)
    rec("K_0", call(K=0, cap=32))
    rec("K_1", call(K=1, cap=32))
    rec("K_512", call(K=512, cap=600))
    rec("n_0", call(n=0))
    rec("n_negative", call(n=-1))
    rec("cap_K", call(cap=31))
    rec("iter_limit_negative", call(iters=-1))
    rec("null_w", call(w=None))
    rec("null_centers", call(centers=None))
    rec("null_centroids", call(cent=None))
    rec("null_handle", call(h=None))
    rec("render", call(h=render.h))
    torch.cuda.synchronize()
    out["launches_after_refusals"] = {"train": launches(eng), "render": launches(render)}
    out["outputs_untouched"] = bool((cent == SENTINEL).all()) and bool((lab == -1).all())
    out["guess_untouched"] = bool(torch.equal(guess, torch.linspace(-4, -3, 511).cuda()))
    rec("ok_K_2", call(K=2, cap=3))
    rec("ok_K_511", call(K=511, cap=512))
    torch.cuda.synchronize()
    out["ok_wrote"] = not bool((lab == -1).any())
    for e in (eng, render):
        e.profile(False)
        e.close()
    return out


# ---- a quantise phase over a layer without a non-zero weight ---------------------------------------------------------------
def case_phase(workdir):
    from implicit_image import fit
    from implicit_image.config import load_config
    name = "layers.1.linear"

    class PrunedAwayLayer(fit.Quantize):
        """layers.1.linear.weight is zero before the quantise phase and, as under a mask that has pruned the layer away,
        before every pass of it: the callback stands in front of the quantiser's"""

        def __enter__(self):
            weight = self.model.layers[1].linear.weight

            def zero():
                weight.data.zero_()
            zero()
            self.model.pre_pass_callbacks.insert(0, zero)
            return super().__enter__()
    fit.Quantize = PrunedAwayLayer
    over = ["masking=none", "quant=kmeans", "quant.num_steps=3", "quant.log_steps=3", "train.num_steps=20", "train.log_steps=20",
            "img.height=32", "img.width=32", "mlp.hidden_size=64", "mlp.depth=4"]
    run_dir = os.path.join(workdir, "run")
    res = fit.fit_one(load_config(os.path.join(ROOT, "conf"), over), torch.device("cuda", 0), run_dir)
    saved = json.load(open(os.path.join(run_dir, "result.json")))
    qdir = os.path.join(run_dir, "model_quantized")
    meta = json.load(open(os.path.join(qdir, "meta_data.json")))
    raw, arrays, off = open(os.path.join(qdir, "compressed_weights.data"), "rb").read(), {}, 0
    for order in sorted(meta, key=int):
        m = meta[order]
        dt, count = np.dtype(m["dtype"]), int(np.prod(m["shape"], dtype=np.int64)) if m["shape"] else 1
        arrays[m["name"]] = np.frombuffer(raw, dt, count, off).reshape(m["shape"])
        off += count * dt.itemsize
    other = arrays["layers.2.linear.centroids"]
    return {"returned": {k: float(v) for k, v in res.items()}, "PSNR": saved["PSNR"], "quant_PSNR": saved["Quant PSNR"],
            "codebook": arrays[name + ".centroids"].astype(np.float64).tolist(),
            "codebook_sign_bits": int(np.signbit(arrays[name + ".centroids"]).sum()),
            "labels_nonzero": int((arrays[name + ".labeled_weight"] != 0).sum()),
            "labels_shape": list(arrays[name + ".labeled_weight"].shape),
            "other_layer_codebook": int(other.size), "other_layer_finite": bool(np.isfinite(other.astype(np.float64)).all())}


if __name__ == "__main__":
    child_main({"abi": case_abi, "abi_raw": case_abi_raw, "reuse": case_reuse, "refuse": case_refuse, "phase": case_phase})
