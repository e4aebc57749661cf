"""`make fit` entry: the reference's fit loop (implicit_image/compress.py:54-170) on the HIP engine.

    python -m implicit_image.fit [key=value ...]         # same override grammar as the Hydra entry

Reads conf/ (implicit_image/config.py), builds the registry model, fits with train_epoch /
update_connections / eval_epoch exactly in the reference's order, logs loss / PSNR / PSNR_8bit,
and saves `model.pth` (fp32 state_dict with the reference's parameter names) in the run directory.
One loop serves every fit: fit_group (_setup per member, the boundaries, train_steps / train_steps_many, _after_steps,
_finish); fit_one is the group of one, and main calls fit_group for every group of group_jobs.
Comma sweeps expand to a job list; under torch.distributed.run the jobs are sharded over ranks
(per-image sharding: one fit per GPU, no collectives).  With train.pixel_split=true every rank runs every job and fits its
rows of the one picture (pixel-split: gradient, SSE and evaluation sums all-reduced; rank 0 writes).
"""
import contextlib
import copy
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np
import torch

from .config import Cfg, expand_sweeps, load_config
from .data import get_grid, load_img
from .models import registry as model_registry
from .models.fourier import PIXEL_SPLIT_UNSUPPORTED as FOURIER_SPLIT_UNSUPPORTED
from .models.siren import Siren, next_kernel_width
from .models.wavelet_siren import PIXEL_SPLIT_UNSUPPORTED as WAVELET_SPLIT_UNSUPPORTED, check_image as check_wavelet_image
from .parallel import SPLIT_BACKENDS, RowSplit, init_split_group, shard_jobs
from .pipeline import entropy_coding
from .pipeline.feathermap import FeatherNet
from .pipeline.feathermap.feathernet import DEEPCOPY_UNSUPPORTED, PIXEL_SPLIT_UNSUPPORTED as FEATHER_SPLIT_UNSUPPORTED
from .pipeline.quant import Quantize
from .utils.train_helper import (SPLIT_EVAL_EPOCH_UNSUPPORTED, SPLIT_PADDED_UNSUPPORTED, device_eval_wanted, eval_epoch,
                                 eval_metrics, get_device, get_optimizer_lr_scheduler, setup_mask, train_epoch, train_steps,
                                 train_steps_many)
from .utils import train_helper

REPO = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))


def pixel_split_wanted(cfg: Cfg) -> bool:
    """train.pixel_split (default false): fit ONE picture across the ranks by image rows"""
    v = cfg.train.get("pixel_split", False)
    v = {"true": True, "false": False, "on": True, "off": False}.get(v.lower(), v) if isinstance(v, str) else v
    if not isinstance(v, bool):
        raise ValueError(f"train.pixel_split: true or false, got {v!r}")
    return v


def split_backend_setting(cfg: Cfg) -> str:
    """train.split_backend (default auto): auto | nccl | gloo, what parallel.split_backend takes"""
    v = cfg.train.get("split_backend", "auto")
    if v not in SPLIT_BACKENDS:
        raise ValueError(f"train.split_backend: one of {' | '.join(SPLIT_BACKENDS)}, got {v!r}")
    return v


def engine_width(cfg: Cfg):
    """(the Small_Dense density or 1, the hidden width Siren gives the model at it, whether the engine zero-pads that width to
    the next one its kernels are instantiated for): the configuration-side statement of Siren.__init__'s rule"""
    masking = cfg.get("masking") or {}
    small = masking.get("density") if masking.get("name") == "Small_Dense" else 1.0
    hidden = int(cfg.mlp.hidden_size * np.sqrt(small))
    return small, hidden, next_kernel_width(hidden, Siren.WIDTHS) != hidden


def check_pixel_split(cfg: Cfg, world: int = 1):
    """What a fit split by rows refuses, from the configuration and the world size alone: before any GPU work and before the
    process group is touched, and the same on every rank, so no rank waits in a collective for one that raised."""
    split_backend_setting(cfg)
    if cfg.mlp.name == "fourier":
        raise NotImplementedError(f"train.pixel_split with mlp=fourier: {FOURIER_SPLIT_UNSUPPORTED}")
    if cfg.mlp.name == "wavelet_siren":
        raise NotImplementedError(f"train.pixel_split with mlp=wavelet_siren: {WAVELET_SPLIT_UNSUPPORTED}")
    masking = cfg.get("masking") or {}
    if masking.get("name") == "Feathermap":
        raise NotImplementedError(f"train.pixel_split: {FEATHER_SPLIT_UNSUPPORTED}")
    if not device_eval_wanted(cfg.train.get("device_eval", "auto")):
        raise NotImplementedError(SPLIT_EVAL_EPOCH_UNSUPPORTED)
    _, hidden, padded = engine_width(cfg)
    if padded:
        raise NotImplementedError(f"train.pixel_split with hidden width {hidden}: {SPLIT_PADDED_UNSUPPORTED}")
    if cfg.img.height < world:
        raise NotImplementedError(f"train.pixel_split: {cfg.img.height} image rows cannot be shared out over {world} ranks "
                                  "(every rank needs a row)")


class _Fit:
    """One fit between its phases (_setup, the step loop, _finish), so that fit_group can run the phases of several fits at
    once.  rng: the CPU and device generator states the fit owns; scope: what fit_group enters around every piece of the
    fit's host work - own_random_state for a member of several, nothing for a fit alone, which never reads or sets a state."""

    def __init__(self, cfg: Cfg, device: torch.device, alone: bool = True):
        self.cfg, self.device = cfg, device
        self.rng = None
        self.scope = contextlib.nullcontext if alone else self.own_random_state

    @contextlib.contextmanager
    def own_random_state(self):
        """the fit's generators while its host work runs: restored on entry (once there is a state: the set-up seeds them
        itself), saved on exit"""
        cuda = self.device.type == "cuda"
        if self.rng is not None:
            torch.set_rng_state(self.rng[0])
            if cuda:
                torch.cuda.set_rng_state(self.rng[1], self.device)
        try:
            yield self
        finally:
            self.rng = (torch.get_rng_state(), torch.cuda.get_rng_state(self.device) if cuda else None)


def _setup(f: _Fit, rank: int = None, world: int = None):
    """everything of a fit before its first step, into `f`: refusals, seed, picture, grid, model, optimiser, mask, the
    evaluation route, the start of its clock"""
    cfg, device = f.cfg, f.device
    split = None
    if pixel_split_wanted(cfg):
        rank = int(os.environ.get("RANK", "0")) if rank is None else rank
        world = int(os.environ.get("WORLD_SIZE", "1")) if world is None else world
        check_pixel_split(cfg, world)                                              # before any GPU work
        if world > 1 and not (torch.distributed.is_available() and torch.distributed.is_initialized()):
            raise RuntimeError("train.pixel_split with WORLD_SIZE > 1 needs an initialised torch.distributed process group "
                               "(python -m implicit_image.fit makes one)")
    feather = bool(cfg.get("masking") and cfg.masking.get("name") == "Feathermap")
    if feather and cfg.mlp.name != "siren":
        raise NotImplementedError("masking=Feathermap runs on the SIREN engine only (mlp=siren)")
    if feather and cfg.get("quant"):
        raise NotImplementedError(f"masking=Feathermap with quant={cfg.quant.get('name', cfg.quant)}: {DEEPCOPY_UNSUPPORTED}")
    if cfg.mlp.name == "wavelet_siren":
        if cfg.get("quant"):
            raise NotImplementedError(f"quant={cfg.quant.get('name', cfg.quant)} on WaveletSiren is not built on the engine: "
                                      "use quant=none")
        check_wavelet_image(cfg.img.height, cfg.img.width)                          # before any GPU work
    torch.manual_seed(cfg.seed)                                                   # compress.py:58
    img = load_img(**cfg.img)                                                      # compress.py:64
    grid = get_grid(cfg.img.height, cfg.img.width)                                 # compress.py:67
    eng_kw = dict(cfg.get("engine") or {})
    model = model_registry[cfg.mlp.name](**cfg.mlp, small_dense_density=engine_width(cfg)[0], **eng_kw)   # compress.py:77
    if feather:                                                                    # compress.py:80-81
        model = FeatherNet(model, compress=cfg.masking.density)
    if pixel_split_wanted(cfg):
        # this rank's rows of grid and picture alone go to the device; the handle indexes rows absolutely, so the split
        # carries the row coordinates of the whole grid
        split = RowSplit(cfg.img.height, rank, world, row_coords=grid[:, 0, 0].contiguous())
        model.set_row_split(split)
        grid, img = grid[split.row_begin:split.row_end], img[split.row_begin:split.row_end].contiguous()
    f.feather = feather
    f.writes = split is None or split.rank == 0                                    # rank 0 alone writes the artefacts
    f.model, f.grid, f.img = model.to(device), grid.to(device), img.to(device)    # compress.py:84-86
    f.model.train()
    f.optim, f.lr_scheduler = get_optimizer_lr_scheduler(f.model, cfg.optim)       # compress.py:105
    mult = cfg.train.multiplier
    f.num_steps = cfg.train.num_steps * mult                                       # compress.py:110-120
    mcfg = copy.deepcopy(cfg.get("masking")) if cfg.get("masking") else None
    if mcfg:
        if mcfg.get("end_when"):
            mcfg.end_when = int(mcfg.end_when * mult)
        if mcfg.get("interval"):
            mcfg.interval = int(mcfg.interval * mult)
    f.mcfg = mcfg
    f.mask = setup_mask(f.model, f.optim, mcfg)                                    # compress.py:127
    # the three figures of an evaluation; the prediction eval_epoch returns is not used here.  train.device_eval auto: sf_eval
    # (no picture stored, one read), off: eval_epoch.  Same loss and PSNR; PSNR_8bit exact instead of torch's fp32 mean
    if device_eval_wanted(cfg.train.get("device_eval", "auto")):
        f.evaluate = eval_metrics
    else:
        def evaluate(m, g, im):
            return eval_epoch(m, g, im)[1:]
        f.evaluate = evaluate
    f.t0, f.last = time.time(), {}


def _update_due(f: _Fit, i: int) -> bool:
    """iteration i ends with a topology update"""
    return bool(f.mask and i <= f.mcfg.end_when and i % f.mcfg.interval == 0)


def _log_due(f: _Fit, i: int) -> bool:
    return (i + 1) % f.cfg.train.log_steps == 0 or i + 1 == f.num_steps


def _next_boundary(f: _Fit, first: int) -> int:
    """the iterations from `first` up to the next one that needs the host (topology update / logging) go to the engine in
    one call: the last of them"""
    i = first
    while not (_update_due(f, i) or _log_due(f, i)):
        i += 1
    return i


def _after_steps(f: _Fit, i: int):
    """what the host does after iteration i: the topology update, the evaluation and its log line"""
    if _update_due(f, i):
        f.mask.update_connections()
    if _log_due(f, i):
        loss, psnr, psnr8 = f.evaluate(f.model, f.grid, f.img)
        f.last = {"loss": loss, "PSNR": psnr, "PSNR_8bit": psnr8}
        msg = f"Train | Step: {i + 1} | " + " | ".join(f"{k}: {v:.4f}" for k, v in f.last.items())
        if f.mask:
            msg += f" | Prune Rate: {f.mask.prune_rate:.4f} | Density: {f.mask.stats.total_density:.4f}"
        logging.info(msg)


def _finish(f: _Fit, out_dir: str = None):
    """everything of a fit after its last step: the quantise phase, the artefacts, the result"""
    cfg, model, grid, img, mask, evaluate, num_steps, writes = f.cfg, f.model, f.grid, f.img, f.mask, f.evaluate, f.num_steps, f.writes
    last = f.last
    last.update(steps=num_steps, seconds=time.time() - f.t0)
    if f.feather:
        last.update({"Stored Params": model.num_stored(), "Dense Params": model.get_num_WandB()})
    quantized_model = None
    if cfg.get("quant"):                                                           # compress.py:172-240
        qcfg = copy.deepcopy(cfg.quant)
        depth = cfg.mlp.depth
        qcfg.skip_ll = [s.replace("layers.first.", "layers.0.").replace("layers.last.", f"layers.{depth - 1}.")
                        for s in (qcfg.get("skip_ll") or [])]
        quantized_model = copy.deepcopy(model)
        q_optim, q_sched = get_optimizer_lr_scheduler(quantized_model, cfg.optim, quantize_mode=True)
        # NOTE: the reference passes the ORIGINAL model's mask here, which makes the quant phase step the
        # wrong optimiser: its quantised copy is never updated and stays sparse.
        # This entry does fine-tune the copy, with the final topology held fixed: the copy's engine gets the
        # mask, so k_adam keeps every pruned weight at exactly 0 and find_centroids' label 0 stays the pruned set
        # (Quant PSNR, Compressed Bytes and Density then describe the artefact that is saved).
        if mask is not None:
            quantized_model.engine(grid, img)
            quantized_model.set_engine_masks(mask.flat_mask())
        with Quantize(quantized_model, q_optim, qcfg) as q:
            i = -1
            while i + 1 < qcfg.num_steps:
                # as above: the steps up to the next logging boundary in one train_steps() call, which is sf_quant_step when
                # the quantiser has a device plan and the train_epoch() loop otherwise
                first = i + 1
                i = min(first + qcfg.log_steps - 1 - first % qcfg.log_steps, qcfg.num_steps - 1)
                train_steps(quantized_model, q_optim, grid, img, i - first + 1, lr_scheduler=q_sched)
                if (i + 1) % qcfg.log_steps == 0:
                    l, p, p8 = evaluate(quantized_model, grid, img)
                    logging.info(f"Quant | Step: {i + 1} | loss: {l:.4f} | PSNR: {p:.4f} | PSNR_8bit: {p8:.4f}")
        quantized_model = q.convert()
        l, p, p8 = evaluate(quantized_model, grid, img)
        last.update({"Quant loss": l, "Quant PSNR": p, "Quant PSNR 8bit": p8})
        if mask is not None:      # what fraction of the masked layers' weights the saved artefact really holds at zero
            zeros = sum(int((w == 0).sum().item()) for n, w in quantized_model.named_parameters() if n in mask.mask_dict)
            total = sum(w.numel() for n, w in quantized_model.named_parameters() if n in mask.mask_dict)
            last["Quant zero fraction"] = zeros / max(total, 1)
            last["Density"] = float(mask.stats.total_density)
        logging.info(f"Post Quant | Train step: {num_steps} | Quant step: {qcfg.num_steps} | Quant PSNR: {p:.4f}")
    if out_dir and cfg.train.save_weights:
        if writes:
            os.makedirs(out_dir, exist_ok=True)
            torch.save({"state_dict": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}},
                       os.path.join(out_dir, "model.pth"))                        # compress.py:243-244
        if quantized_model is not None and cfg.get("entropy_coding"):              # compress.py:249-263
            ec = dict(cfg.entropy_coding)
            # (a rank that does not write still reports the byte count: its identical replica, coded into a directory it drops)
            with (contextlib.nullcontext(out_dir) if writes else tempfile.TemporaryDirectory()) as where:
                nbytes = entropy_coding.compress_state_dict(quantized_model.half(), os.path.join(where, "model_quantized"),
                                                            **ec)
            last["Compressed Bytes"] = nbytes
            logging.info(f"Compressed bytes {nbytes}")
        if writes:
            with open(os.path.join(out_dir, "result.json"), "w") as fh:
                json.dump(last, fh)
            from .decode import write_decode_json                                  # what `make decode` rebuilds the network from
            write_decode_json(out_dir, cfg, list(model.state_dict().keys()))
    return last


def fit_one(cfg: Cfg, device: torch.device, out_dir: str = None, rank: int = None, world: int = None):
    """One fit - the group of one; returns dict(loss, PSNR, PSNR_8bit, steps, seconds).

    train.pixel_split: rank `rank` of `world` (default: RANK / WORLD_SIZE, a world of one without them) fits rows
    shard_rows(H, world, rank) of the picture; the model carries a parallel.RowSplit, under which every step and every
    evaluation reduces over the ranks (utils/train_helper.py).  Seed, init, mask draw and schedules are the ordinary fit's on
    every rank, so the replicas stay identical; every rank returns the same dict, rank 0 alone writes into out_dir.  The
    caller has initialised torch.distributed when world > 1 (main does)."""
    return fit_group([cfg], device, [out_dir], rank, world)[0]


# ---- train.batch_jobs: several fits of one shape at once (sf_step_many) -------------------------------------------------------
BATCH_JOBS_MAX = 64                      # SF_STEP_MANY_MAX
# what the members of a group may differ in; everything else of their configurations is equal
GROUP_FREE_KEYS = ("seed", "exp_name", "img.name", "img.path", "img.seed", "optim.lr", "masking.density",
                   "masking.prune_rate", "masking.sparse_init")


def batch_jobs_setting(cfg: Cfg) -> int:
    """train.batch_jobs (default 1): how many jobs of a sweep a rank fits at once, 1 .. 64"""
    v = cfg.train.get("batch_jobs", 1)
    if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= BATCH_JOBS_MAX:
        raise ValueError(f"train.batch_jobs: an integer from 1 to {BATCH_JOBS_MAX}, got {v!r}")
    return v


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def group_key(cfg: Cfg):
    """What decides whether two jobs can share a group: None for a job that joins none (not mlp=siren, Feathermap,
    pixel_split, an engine width that is zero-padded or above 128), else the configuration without GROUP_FREE_KEYS as text"""
    masking = cfg.get("masking") or {}
    if cfg.mlp.name != "siren" or masking.get("name") == "Feathermap" or pixel_split_wanted(cfg):
        return None
    _, hidden, padded = engine_width(cfg)
    if padded or hidden > 128:
        return None
    rest = _plain(cfg)
    for dotted in GROUP_FREE_KEYS:
        d, keys = rest, dotted.split(".")
        for k in keys[:-1]:
            d = d.get(k) if isinstance(d, dict) else None
        if isinstance(d, dict):
            d.pop(keys[-1], None)
    return json.dumps(rest, sort_keys=True, default=repr)


def group_jobs(cfgs, n: int):
    """The jobs of a rank (their configurations, in job order) as groups of at most n: lists of job indices, every job in
    exactly one.  Jobs share a group when group_key gives them the same text; a job goes to the earliest group of its key
    that has room, else it opens one; a job without a key is a group of its own.  Members stay in job order, groups in the
    order of their first members.  A pure function of its arguments."""
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= BATCH_JOBS_MAX:
        raise ValueError(f"group_jobs: n must be an integer from 1 to {BATCH_JOBS_MAX}, got {n!r}")
    groups, open_by_key = [], {}
    for j, cfg in enumerate(cfgs):
        key = group_key(cfg) if n > 1 else None
        g = open_by_key.get(key) if key is not None else None
        if g is None or len(g) >= n:
            g = []
            groups.append(g)
            if key is not None:
                open_by_key[key] = g
        g.append(j)
    return groups


def fit_group(cfgs, device: torch.device, out_dirs=None, rank: int = None, world: int = None):
    """The fits of one group (group_jobs) at once, their fit_one dicts in order: the one fit loop (compress.py:137-170).

    The iterations up to the next one that needs the host (topology update / logging: the boundaries follow from keys the
    members share) go to train_steps for a fit alone, else to train_steps_many - one sf_step_many call where the members
    qualify, train_steps per member where not -, then each member's topology update and evaluation; after the loop each member's
    quantise phase and artefacts (_finish).  Every member of several owns the generator states its torch.manual_seed(cfg.seed)
    gave it: they are swapped in before any host work of the member and saved after, so every draw falls as in a run of the
    member alone, and result.json apart from `seconds` (counted from the last member's set-up), model.pth and the container
    are byte for byte those of train.batch_jobs=1.  A fit alone enters no such scope.  rank / world: fit_one's."""
    out_dirs = list(out_dirs) if out_dirs is not None else [None] * len(cfgs)
    fits = [_Fit(cfg, device, alone=len(cfgs) == 1) for cfg in cfgs]
    for f in fits:
        with f.scope():
            _setup(f, rank, world)
    head = fits[0]
    if any(f.num_steps != head.num_steps or bool(f.mask) != bool(head.mask) for f in fits):
        raise ValueError("fit_group: the members differ in their step count or in having a mask (group_jobs keeps such jobs apart)")
    if len(fits) > 1:
        t0 = time.time()
        for f in fits:
            f.t0 = t0
    i = -1
    while i + 1 < head.num_steps:
        first = i + 1
        i = _next_boundary(head, first)
        if len(fits) == 1:     # (what train_steps_many makes of one member, under this module's name, which observers wrap)
            train_steps(head.model, head.optim, head.grid, head.img, i - first + 1, lr_scheduler=head.lr_scheduler,
                        mask=head.mask)
        else:
            train_steps_many([f.model for f in fits], [f.optim for f in fits], head.grid, [f.img for f in fits], i - first + 1,
                             lr_schedulers=[f.lr_scheduler for f in fits], masks=[f.mask for f in fits],
                             scopes=[f.scope for f in fits])
        for f in fits:
            with f.scope():
                _after_steps(f, i)
    results = []
    for f, out_dir in zip(fits, out_dirs):
        with f.scope():
            results.append(_finish(f, out_dir))
    return results


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    logging.basicConfig(level=logging.INFO, format="[%(asctime)s] %(message)s")
    conf_dir = os.environ.get("IIC_CONF", os.path.join(REPO, "conf"))
    jobs = expand_sweeps(argv)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    cfgs = [load_config(conf_dir, ov) for ov in jobs]
    split = [pixel_split_wanted(c) for c in cfgs]
    batch = {batch_jobs_setting(c) for c in cfgs}
    if len(batch) != 1:
        raise ValueError("train.batch_jobs is one setting for the whole sweep")
    batch = batch.pop()
    if batch > 1 and any(split):                               # before the GPU and the process group are touched
        raise ValueError("train.batch_jobs > 1 with train.pixel_split=true: a fit split by image rows steps with a collective "
                         "between its kernels and joins no group; use one or the other")
    grouped = False
    if any(split):
        # one picture across the ranks: EVERY job on EVERY rank, in order; what is refused is refused here, on every rank
        # alike, before the GPU and the process group are touched
        if not all(split):
            raise ValueError("train.pixel_split is one setting for the whole sweep: every rank runs every job")
        for c in cfgs:
            check_pixel_split(c, world)
        rank, world, grouped = init_split_group(split_backend_setting(cfgs[0]))
        if torch.cuda.is_available():
            local_rank %= torch.cuda.device_count()        # (ranks that share a device: the rehearsal over gloo)
    else:
        jobs, cfgs = shard_jobs(jobs, world, rank), shard_jobs(cfgs, world, rank)
    results = []
    try:
        # train.batch_jobs = 1: every job is a group of its own, in job order - the loop this has always been
        for members in group_jobs(cfgs, batch):
            tags, out_dirs = [], []
            for j in members:
                ov, cfg = jobs[j], cfgs[j]
                device = get_device(cfg.device)
                if device.type == "cuda":
                    device = torch.device("cuda", local_rank)
                    torch.cuda.set_device(device)
                tags.append(",".join(o for o in ov if not o.startswith(("exp_name", "img.name"))) or "default")
                out_dirs.append(os.path.join("outputs", str(cfg.img.name), str(cfg.exp_name), tags[-1].replace("/", "_")))
            before = dict(train_helper.MANY_STATS)
            # (rank / world matter to a fit split by rows alone, which every rank runs; a sharded job never looks at them)
            done = fit_group([cfgs[j] for j in members], device, out_dirs, rank, world)
            if len(members) > 1:
                took = {k: v - before[k] for k, v in train_helper.MANY_STATS.items()}
                logging.info(f"[rank {rank}] group of {len(members)}: {took['steps']} steps each in {took['calls']} sf_step_many "
                             f"calls, {took['fallbacks']} stretches member by member")
            for tag, res in zip(tags, done):
                logging.info(f"[rank {rank}] {tag}: {res}")
                results.append((tag, res))
    finally:
        if grouped:
            torch.distributed.destroy_process_group()
    return results


if __name__ == "__main__":
    main()
