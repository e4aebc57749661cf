"""Child of tests/test_gpu_pixel_split_fit.py: `make fit` with train.pixel_split on cuda:0, one fresh process per rank.

  python _pixel_split_fit_child.py CASE OUT.json [ARG ...]      one process (run_case): identity, single SPEC
  python _pixel_split_fit_child.py ranks WORKDIR SPEC           one rank of RANK / WORLD_SIZE / MASTER_* (run_ranks): the fit
                                                                through fit.main's own group set-up -> WORKDIR/r<RANK>.json

A fit is observed from outside: fit.train_steps, fit.eval_metrics, fit.setup_mask and Masking.update_connections are wrapped
to record what they return; nothing in the product path is replaced."""
import hashlib
import json
import os
import sys

import torch

from _gpu_child import ROOT, child_main

CONF = os.path.join(ROOT, "conf")
SMALL = ["mlp.hidden_size=64", "mlp.depth=4", "entropy_coding=plain"]
SPECS = {
    # the default composition: RigL, k-means bits 8, plain container
    "identity": SMALL + ["img.height=32", "img.width=32", "train.num_steps=20", "train.log_steps=20", "masking.interval=10",
                         "quant.num_steps=6", "quant.log_steps=3", "quant.bits=8"],
    "dense": SMALL + ["img.height=64", "img.width=48", "masking=none", "quant=none", "train.num_steps=12", "train.log_steps=5"],
    "tiny": ["mlp.hidden_size=32", "mlp.depth=3", "img.height=10", "img.width=12", "masking=none", "quant=none",
             "train.num_steps=4", "train.log_steps=4"],
    "wide": ["mlp.hidden_size=512", "mlp.depth=3", "img.height=16", "img.width=16", "masking=none", "quant=none",
             "train.num_steps=3", "train.log_steps=3"],
    "quant8": SMALL + ["img.height=32", "img.width=32", "masking=none", "quant=kmeans", "quant.bits=8", "train.num_steps=10",
                       "train.log_steps=10", "quant.num_steps=6", "quant.log_steps=3"],
}
SPECS["quant9"] = [o.replace("bits=8", "bits=9") for o in SPECS["quant8"]]
MASKED = SMALL + ["img.height=64", "img.width=48", "quant=none", "train.num_steps=40", "train.log_steps=40", "masking.interval=10"]
SPECS["RigL"] = MASKED + ["masking=RigL", "masking.density=0.5"]
SPECS["Pruning"] = MASKED + ["masking=Pruning"]
SPECS["SNFS"] = MASKED + ["masking=SNFS"]
SPECS["SET"] = MASKED + ["masking=RigL", "masking.density=0.5", "masking.growth_mode=random"]    # SET: random growth


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def observed_fit(spec, out_dir, split, rank=None, world=None):
    """fit_one of SPECS[spec] (train.pixel_split=`split`) -> what the test compares"""
    from implicit_image import fit
    from implicit_image.config import load_config
    from implicit_image.pipeline.masking import Masking
    rec = {"losses": [], "evals": [], "updates": []}
    models, masks = [], []
    plain = (fit.train_steps, fit.eval_metrics, fit.setup_mask, Masking.update_connections)

    def steps(model, *a, **kw):
        if not any(m is model for m in models):
            models.append(model)
        rec["losses"].append(plain[0](model, *a, **kw))
        return rec["losses"][-1]

    def evaluate(*a, **kw):
        rec["evals"].append(list(plain[1](*a, **kw)))
        return tuple(rec["evals"][-1])

    def setup(*a, **kw):
        masks.append(plain[2](*a, **kw))
        return masks[-1]

    def update(self):
        eng = self.module.bound_engine
        eng.profile(True)
        eng.profile_reset()
        plain[3](self)
        eng = self.module.bound_engine
        launches = {k: v["launches"] for k, v in eng.profile_report().items() if v["launches"] and k.startswith("k_mask")}
        eng.profile(False)
        rec["updates"].append({"mask": sha(self.flat_mask()), "launches": launches,
                               "nonzero": [int(k.sum().item()) for _, _, k in self._masked()]})
    fit.train_steps, fit.eval_metrics, fit.setup_mask, Masking.update_connections = steps, evaluate, setup, update
    try:
        cfg = load_config(CONF, SPECS[spec] + [f"train.pixel_split={'true' if split else 'false'}"])
        res = fit.fit_one(cfg, torch.device("cuda", 0), out_dir, rank, world)
    finally:
        fit.train_steps, fit.eval_metrics, fit.setup_mask, Masking.update_connections = plain
    rec["result"] = {k: repr(v) for k, v in res.items() if k != "seconds"}
    eng = models[0].bound_engine
    m, v, step = eng.get_adam_state()
    rec["state"] = {"params": sha(eng.get_params()), "exp_avg": sha(m), "exp_avg_sq": sha(v), "adam_steps": step,
                    "rows": [eng.row_begin, eng.row_end]}
    if masks and masks[0] is not None:
        sd = models[0].state_dict()
        rec["dead_nonzero"] = sum(int(((k == 0) & (sd[n] != 0)).sum().item()) for n, k in masks[0].mask_dict.items())
    if len(models) > 1:                         # the quantised copy: what update_weights() froze
        rec["codebooks"] = {n: sha(p) for n, p in models[1].state_dict().items()
                            if n.endswith(("centroids", "labeled_weight"))}
        rec["codebook_sizes"] = {n: p.numel() for n, p in models[1].state_dict().items() if n.endswith("centroids")}
    rec["wrote"] = sorted(os.listdir(out_dir)) if os.path.isdir(out_dir) else []
    return rec


def artefacts(run):
    """what a run directory holds, to the bit"""
    pth = torch.load(os.path.join(run, "model.pth"), weights_only=True)["state_dict"]
    qdir = os.path.join(run, "model_quantized")
    return {"pth": {k: sha(v) for k, v in pth.items()},
            "container": hashlib.sha256(open(os.path.join(qdir, "compressed_weights.data"), "rb").read()).hexdigest(),
            "meta": json.load(open(os.path.join(qdir, "meta_data.json"))),
            "result": {k: repr(v) for k, v in json.load(open(os.path.join(run, "result.json"))).items() if k != "seconds"}}


def case_identity(workdir):
    """the default composition with train.pixel_split=true and no WORLD_SIZE, and without"""
    assert "WORLD_SIZE" not in os.environ and "RANK" not in os.environ
    out = {}
    for side, split in (("split", True), ("plain", False)):
        run = os.path.join(workdir, side)
        out[side] = observed_fit("identity", run, split)
        out[side]["artefacts"] = artefacts(run)
    return out


def case_single(workdir, spec):
    """the ordinary one-process fit of SPEC: the reference of the shard-composition bound"""
    return observed_fit(spec, os.path.join(workdir, "single"), False)


def decoded(run, height, width, depth):
    """`make decode` of a run directory, and the prediction of its container as case_fit_bits9 takes it"""
    from implicit_image import _engine as E, decode as dec
    from implicit_image.pipeline import entropy_coding
    from oracle import siren_oracle as so
    got = dec.decode([f"decode.dir={run}", "decode.truth=synthetic"])
    sd = entropy_coding.decompress_state_dict(os.path.join(run, "model_quantized"), "plain")
    eng = E.SirenEngine(height, width, 64, depth)
    gh, gw = so.grid_vectors(height, width)
    eng.set_coords(gh.cuda(), gw.cuda())
    eng.set_params(dec.flat_params(sd, depth).cuda())
    pred, _ = eng.forward(want_pred=True, want_sse=False)
    torch.cuda.synchronize()
    outside = int(((pred < 0) | (pred > 1)).sum())
    eng.close()
    return {"path": got["path"], "source": got["source"], "psnr8_decode": got["PSNR_8bit"], "outside_01": outside}


def rank_main(workdir, spec):
    """one rank: the group as fit.main makes it (backend rule `auto`: the ranks share cuda:0 here -> gloo), the fit, the
    group's end; rank 0 then decodes what it wrote"""
    from implicit_image import fit
    from implicit_image.config import load_config
    from implicit_image.parallel import init_split_group
    import torch.distributed as dist
    cfg = load_config(CONF, SPECS[spec] + ["train.pixel_split=true"])
    world = int(os.environ["WORLD_SIZE"])
    fit.check_pixel_split(cfg, world)
    rank, world, grouped = init_split_group(fit.split_backend_setting(cfg))
    assert grouped and dist.get_backend() == "gloo"
    torch.cuda.set_device(0)
    run = os.path.join(workdir, f"run_r{rank}")
    try:
        rec = observed_fit(spec, run, True, rank, world)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    rec["rank"] = rank
    if rank == 0 and spec.startswith("quant"):
        rec["decode"] = decoded(run, 32, 32, 4)
    with open(os.path.join(workdir, f"r{rank}.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    if sys.argv[1] == "ranks":
        rank_main(*sys.argv[2:])
    else:
        child_main({"identity": case_identity, "single": case_single})
