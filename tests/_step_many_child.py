"""Child of tests/test_gpu_step_many.py, one case per process: sf_step_many against its oracle - fresh handles in the same
initial state, stepped by sf_step one handle after the other.  Every tensor comparison is on the int32 view; what goes to the
parent is the number of words that differ (0 everywhere for a pass), the scalars themselves, and the refusals."""
import ctypes as C
import struct

import torch

from _gpu_child import child_main
from _gpu_fixtures import launches, recorder, siren_engine
from implicit_image import _engine as E
from oracle import siren_oracle as so

SHAPES = {"32x2": (32, 2, 8, 8, 2), "64x3": (64, 3, 24, 20, 3), "64x4": (64, 4, 32, 32, 5), "128x4": (128, 4, 40, 24, 2),
          "128x8": (128, 8, 32, 32, 4)}


def member(hidden, depth, H, W, seed, fmt=16, **kw):
    """a handle with seed-`seed` parameters and target"""
    return siren_engine(H, W, hidden, depth, params=so.siren_init(hidden, depth, seed=seed), img=so.synthetic_image(H, W, seed=seed + 100),
                        scratch_format=fmt, **kw)


def lr_rows(n, B, first=0):
    """lrs[s][b]: a different learning rate for every step and member"""
    return [[3e-4 * (1 + 0.25 * b) * 0.9 ** (first + s) for b in range(B)] for s in range(n)]


def column(rows, b):
    return [r[b] for r in rows]


def bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def snapshot(eng):
    m, v, step = eng.get_adam_state()
    tensors = {"params": eng.get_params(), "grads": eng.get_grads(), "exp_avg": m, "exp_avg_sq": v}
    sse, sse8 = eng.eval_sums()
    return tensors, {"step": step, "eval_sse": sse, "eval_sse8": sse8}


def compare(got, want):
    """words that differ per tensor, and the scalars of both sides"""
    (gt, gs), (wt, ws) = snapshot(got), snapshot(want)
    diff = {k: int((gt[k].view(torch.int32) != wt[k].view(torch.int32)).sum()) for k in gt}
    return {"diff": diff, "got": gs, "want": ws, "nonzero": int((gt["params"] != 0).sum())}


def run_pair(batch, oracle, calls, first=0):
    """`calls` (step counts) as sf_step_many calls on `batch` and as sf_step calls per handle on `oracle` -> per member the
    comparison and both loss curves as bit patterns"""
    B = len(batch)
    got, want = [[] for _ in range(B)], [[] for _ in range(B)]
    done = first
    for n in calls:
        rows = lr_rows(n, B, done)
        for b, l in enumerate(E.step_many(batch, rows, want_loss=True)):
            got[b] += l
        for b, eng in enumerate(oracle):
            want[b] += eng.step(column(rows, b), want_loss=True)
        done += n
    out = []
    for b in range(B):
        r = compare(batch[b], oracle[b])
        r["loss_got"], r["loss_want"] = [bits(x) for x in got[b]], [bits(x) for x in want[b]]
        out.append(r)
    return out


def case_identity(name):
    hidden, depth, H, W, B = SHAPES[name]
    batch = [member(hidden, depth, H, W, b) for b in range(B)]
    oracle = [member(hidden, depth, H, W, b) for b in range(B)]
    return {"members": run_pair(batch, oracle, [1, 2, 3]), "formats": [e.scratch_format for e in batch]}


def case_masks():
    def trio():
        engs = [member(64, 4, 32, 32, b, fmt=0 if b < 2 else 16) for b in range(3)]
        before = [e.scratch_format for e in engs]
        masks = []
        for b, e in enumerate(engs[:2]):
            g = torch.Generator().manual_seed(7 + b)
            mk = (torch.rand(e.num_params, generator=g) < 0.5).float()
            for l in range(4):                                  # biases stay
                w0, b0 = e.param_offsets(l)
                mk[b0:b0 + (3 if l == 3 else 64)] = 1.0
            e.set_masks(mk.cuda())
            masks.append(mk)
        return engs, before, masks
    batch, before, masks = trio()
    oracle, _, _ = trio()
    res = run_pair(batch, oracle, [1, 2, 3])
    pruned = [int((batch[b].get_params().cpu()[masks[b] == 0] != 0).sum()) for b in range(2)]
    return {"members": res, "formats_before": before, "formats": [e.scratch_format for e in batch], "pruned_nonzero": pruned,
            "pruned": [int((mk == 0).sum()) for mk in masks]}


def case_history():
    batch = [member(64, 3, 24, 20, b) for b in range(2)]
    oracle = [member(64, 3, 24, 20, b) for b in range(2)]
    for engs in (batch, oracle):
        engs[0].step([2e-4, 3e-4, 4e-4])
    return {"members": run_pair(batch, oracle, [4])}


def case_interleave():
    batch = [member(64, 4, 32, 32, b) for b in range(2)]
    oracle = [member(64, 4, 32, 32, b) for b in range(2)]
    r1, r2 = lr_rows(3, 2), lr_rows(2, 2, 5)
    mid0, mid1 = [1e-4, 2e-4], 5e-4

    def middle(engs):
        engs[0].set_graph_replay(True)
        losses = engs[0].step(mid0, want_loss=True)
        engs[1].forward_backward()
        engs[1].adam_step(mid1)
        return losses
    got = E.step_many(batch, r1, want_loss=True)
    got[0] += middle(batch)
    for b, l in enumerate(E.step_many(batch, r2, want_loss=True)):
        got[b] += l
    want = [e.step(column(r1, b), want_loss=True) for b, e in enumerate(oracle)]
    want[0] += middle(oracle)
    for b, e in enumerate(oracle):
        want[b] += e.step(column(r2, b), want_loss=True)
    out = []
    for b in range(2):
        r = compare(batch[b], oracle[b])
        r["loss_got"], r["loss_want"] = [bits(x) for x in got[b]], [bits(x) for x in want[b]]
        out.append(r)
    return {"members": out}


def case_bounds():
    engs = [member(32, 2, 8, 8, b) for b in range(65)]
    oracle = [member(32, 2, 8, 8, b) for b in range(65)]
    lib = engs[0].lib
    hs = (C.c_void_p * 65)(*[e.h for e in engs])
    lr = (C.c_float * 65)(*([1e-3] * 65))
    rc = lib.sf_step_many(hs, 65, lr, 1, None)
    refused = {"rc": rc, "msg": lib.sf_last_error().decode(), "steps": [e.adam_steps for e in engs]}
    one = run_pair(engs[64:], oracle[64:], [3])
    full = run_pair(engs[:64], oracle[:64], [3])
    return {"refused": refused, "B1": one, "B64": full}


def case_refuse():
    torch.manual_seed(0)
    lib = E.load_library()
    good = [member(64, 3, 8, 8, b) for b in range(2)]
    out, rec = recorder(lib)
    keep = []

    def bad(name, eng, prepared=True):
        """`eng` as member 1 behind a good member 0"""
        keep.append(eng)
        if prepared:
            gh, gw = so.grid_vectors(eng.height, eng.width)
            eng.set_coords(gh.cuda(), gw.cuda())
            img = so.synthetic_image(eng.height, eng.width, seed=5)
            eng.set_target(img[eng.row_begin:eng.row_end, :, :eng.out_features].contiguous().cuda())
        eng.profile(True)
        eng.profile_reset()
        hs = (C.c_void_p * 2)(good[0].h, eng.h)
        rec(name, lib.sf_step_many(hs, 2, lr2, 1, loss2))

    lr2, loss2 = (C.c_float * 2)(1e-3, 1e-3), (C.c_float * 2)()
    for e in good:
        e.forward(want_pred=False)
        e.profile(True)
        e.profile_reset()
    before = [(e.get_params().clone(), e.adam_steps) for e in good]
    hs = (C.c_void_p * 2)(good[0].h, good[1].h)
    rec("null_handles", lib.sf_step_many(None, 2, lr2, 1, None))
    rec("null_lr", lib.sf_step_many(hs, 2, None, 1, None))
    rec("null_member", lib.sf_step_many((C.c_void_p * 2)(good[0].h, None), 2, lr2, 1, None))
    rec("n_fits_0", lib.sf_step_many(hs, 0, lr2, 1, None))
    rec("n_fits_65", lib.sf_step_many(hs, 65, lr2, 1, None))
    rec("n_steps_negative", lib.sf_step_many(hs, 2, lr2, -1, None))
    rec("twice", lib.sf_step_many((C.c_void_p * 2)(good[0].h, good[0].h), 2, lr2, 1, None))
    S = E.SirenEngine
    bad("render", E.RenderEngine(8, 8, 64, 3), prepared=False)
    bad("fourier", E.FourierEngine(8, 8, 64, 3, 64), prepared=False)
    bad("wavelet", E.WaveletEngine(8, 8, 64, 3), prepared=False)
    fth = S(8, 8, 64, 3, scratch_format=16)
    fth.feather_attach(68, 8, [64, 64, 3], [2, 64, 64])
    bad("feather", fth)
    bad("hidden_256", S(8, 8, 256, 3, scratch_format=16))
    bad("bf16", S(8, 8, 64, 3, compute_dtype="bf16", scratch_format=16))
    bad("format_12", S(8, 8, 64, 3))
    bad("format_8", S(8, 8, 64, 3, scratch_format=8))
    bad("chunks", S(32, 32, 64, 3, scratch_format=16, chunk_pixels=256))
    bad("rows", S(8, 8, 64, 3, scratch_format=16, row_begin=0, row_end=4))
    bad("no_coords", S(8, 8, 64, 3, scratch_format=16), prepared=False)
    no_target = S(8, 8, 64, 3, scratch_format=16)
    gh, gw = so.grid_vectors(8, 8)
    no_target.set_coords(gh.cuda(), gw.cuda())
    bad("no_target", no_target, prepared=False)
    bad("height", S(16, 8, 64, 3, scratch_format=16))
    bad("width", S(8, 16, 64, 3, scratch_format=16))
    bad("hidden", S(8, 8, 32, 3, scratch_format=16))
    bad("depth", S(8, 8, 64, 4, scratch_format=16))
    bad("out_features", S(8, 8, 64, 3, out_features=1, scratch_format=16))
    bad("first_omega", S(8, 8, 64, 3, first_omega_0=30.0, scratch_format=16))
    bad("hidden_omega", S(8, 8, 64, 3, hidden_omega_0=20.0, scratch_format=16))
    bad("outermost_linear", S(8, 8, 64, 3, outermost_linear=False, scratch_format=16))
    bad("betas", S(8, 8, 64, 3, betas=(0.8, 0.999), scratch_format=16))
    bad("eps", S(8, 8, 64, 3, eps=1e-6, scratch_format=16))
    with torch.cuda.stream(torch.cuda.Stream()):
        other = S(8, 8, 64, 3, scratch_format=16)
    bad("stream", other)
    torch.cuda.synchronize()
    counts = {"good": [launches(e) for e in good], "bad": [launches(e) for e in keep]}
    untouched = [int((e.get_params().view(torch.int32) != p.view(torch.int32)).sum()) for e, (p, _) in zip(good, before)]
    steps = [e.adam_steps for e in good]
    E.step_many(good, [[1e-3, 1e-3]], want_loss=True)
    changed = [int((e.get_params().view(torch.int32) != p.view(torch.int32)).sum()) for e, (p, _) in zip(good, before)]
    return {"refusals": out, "launches": counts, "untouched": untouched, "steps": steps, "steps_before": [s for _, s in before],
            "changed": changed, "steps_after": [e.adam_steps for e in good], "launches_after": launches(good[0])}


def case_launches():
    def report(B, batched):
        engs = [member(64, 4, 32, 32, b) for b in range(B)]
        for e in engs:
            e.forward(want_pred=False)                           # the weight images are current: the call starts no refresh
        engs[0].profile(True)
        engs[0].profile_reset()
        if batched:
            E.step_many(engs, lr_rows(3, B))
        else:
            engs[0].step(column(lr_rows(3, 1), 0))
        rep = {k: v["launches"] for k, v in engs[0].profile_report().items() if v["launches"]}
        engs[0].profile(False)
        return rep
    return {"single": report(1, False), "B1": report(1, True), "B4": report(4, True)}


SWEEP = ["seed=0,1,2", "mlp.hidden_size=64", "mlp.depth=4", "img.height=32", "img.width=32", "train.num_steps=40",
         "train.log_steps=20", "masking.interval=10", "masking.end_when=30", "quant.num_steps=4", "quant.log_steps=2"]
ARTEFACTS = ["model.pth", "compressed_weights.data", "meta_data.json"]


def case_fit(workdir):
    """fit.main on SWEEP with train.batch_jobs=3 and with 1, in two work directories -> per job and artefact whether the
    bytes are equal (result.json without `seconds`), and what train_steps_many counted in each run"""
    import hashlib
    import json
    import os

    from implicit_image import fit
    from implicit_image.utils import train_helper as th
    runs, counters, home = {}, {}, os.getcwd()
    for batch in (3, 1):
        where = os.path.join(workdir, f"batch{batch}")
        os.makedirs(where)
        os.chdir(where)
        before = dict(th.MANY_STATS)
        fit.main(SWEEP + [f"train.batch_jobs={batch}"])
        counters[str(batch)] = {k: th.MANY_STATS[k] - before[k] for k in before}
        found = {}
        for top, _, files in os.walk(os.path.join(where, "outputs")):
            if "result.json" in files:
                job = os.path.relpath(top, os.path.join(where, "outputs")).replace(f"train.batch_jobs={batch}", "train.batch_jobs=N")
                res = json.load(open(os.path.join(top, "result.json")))
                res.pop("seconds")
                found[job] = {"result.json": json.dumps(res, sort_keys=True)}
                for top2, _, files2 in os.walk(top):
                    for name in files2:
                        if name in ARTEFACTS:
                            found[job][name] = hashlib.sha256(open(os.path.join(top2, name), "rb").read()).hexdigest()
        runs[batch] = found
        os.chdir(home)
    jobs = sorted(runs[1])
    equal = {job: {name: runs[3].get(job, {}).get(name) == runs[1][job][name] for name in runs[1][job]} for job in jobs}
    return {"jobs": jobs, "jobs_batched": sorted(runs[3]), "equal": equal, "counters": counters,
            "results": {job: runs[1][job]["result.json"] for job in jobs}}


if __name__ == "__main__":
    child_main({"fit": case_fit, "identity": case_identity, "masks": case_masks, "history": case_history, "interleave": case_interleave,
                "bounds": case_bounds, "refuse": case_refuse, "launches": case_launches})
