"""Multi-GPU modes of the fit.  One process per GPU (torch.distributed; backend
"nccl" is RCCL over xGMI on ROCm, "gloo" in the CPU tests).

  * per-image sharding  — `shard_jobs`: independent fits round-robin over ranks, NO collective;
  * pixel-split         — `PixelSplitFit`: each rank owns a block of image rows of ONE large image;
                          loss and gradient are sums over pixels, so one all-reduce(sum) of the flat fp32
                          gradient (+ the SSE scalar) per step makes every replica take the identical
                          Adam step.  The reference has no counterpart (it is single-device).

`RowSplit` is what `make fit` hangs on a model for train.pixel_split (EngineBound.set_row_split): the rank's row range and
the two reductions of a step and of an evaluation.  train_epoch / train_steps / eval_metrics, Masking and KmeansQuant then
all meet the one row-range handle that model.engine() makes.
"""
import ctypes
import logging
import os
from datetime import timedelta
from typing import List, Optional, Sequence, Tuple

import torch

SPLIT_BACKENDS = ("auto", "nccl", "gloo")
SPLIT_TIMEOUT_S = 600       # of the process group: a rank that dies ends the others' collective after this, not never


def shard_rows(height: int, world_size: int, rank: int) -> Tuple[int, int]:
    """Contiguous balanced row block [r0, r1) of rank `rank` (empty if height < world_size is avoided
    by giving the first height % world ranks one extra row)."""
    base, rem = divmod(height, world_size)
    r0 = rank * base + min(rank, rem)
    return r0, r0 + base + (1 if rank < rem else 0)


def shard_jobs(jobs: Sequence, world_size: int, rank: int) -> List:
    """Per-image sharding: job i runs on rank i % world_size."""
    return [j for i, j in enumerate(jobs) if i % world_size == rank]


def split_backend(setting, local_rank: int, local_world: int, device_count: int) -> Tuple[str, bool]:
    """train.split_backend -> (torch.distributed backend, do the node's ranks share a device).  `auto`: "nccl" (RCCL) when
    every rank of the node has a device of its own - LOCAL_WORLD_SIZE ranks fit into torch.cuda.device_count() devices and
    LOCAL_RANK names one of them -, else "gloo" (RCCL refuses two ranks on one device).  A pure function of its arguments."""
    if setting not in SPLIT_BACKENDS:
        raise ValueError(f"train.split_backend: one of {' | '.join(SPLIT_BACKENDS)}, got {setting!r}")
    own = device_count > 0 and 1 <= local_world <= device_count and 0 <= local_rank < device_count
    if setting == "auto":
        return ("nccl" if own else "gloo"), not own
    return setting, not own


def all_reduce_sum(dist, t: torch.Tensor, group=None):
    """in-place all-reduce (sum) of `t`; over gloo a device tensor is reduced on the host (the rehearsal path)"""
    if dist.get_backend(group) == "gloo" and t.is_cuda:
        host = t.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        t.copy_(host)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def reduced_pass(eng, all_reduce) -> torch.Tensor:
    """The pass of a split step: forward + backward of the local rows enqueued, the handle's own gradient view and SSE double
    summed in place by `all_reduce` -> the SSE view, to be read or copied before the next pass overwrites it."""
    eng.forward_backward(sync=False)
    sse = eng.sse_view()
    all_reduce(eng.grad_view())
    all_reduce(sse)
    return sse


class SseTable:
    """The SSE doubles of a run of steps, kept where the passes wrote them: put() is one device copy per step, read() the one
    transfer at the end of the run."""

    def __init__(self, n: int):
        self.n, self.table = n, None

    def put(self, k: int, sse: torch.Tensor):
        if self.table is None:
            self.table = torch.empty(self.n, dtype=sse.dtype, device=sse.device)
        self.table[k:k + 1].copy_(sse)

    def read(self) -> List[float]:
        return [] if self.table is None else self.table.cpu().tolist()


def as_float(x: float) -> float:
    """(float) x: what `.item()` of a float32 loss gives and what sf_step reports"""
    return ctypes.c_float(x).value


class RowSplit:
    """One rank's share of a fit split by image rows: rows [row_begin, row_end) of `full_height`, and the collectives.
    world == 1 is a world of one: the same code path, no process group and no collective.  `row_coords`: the row
    coordinate vector of the FULL grid (the handle indexes it by absolute row), for a model bound to its rows of the grid."""

    def __init__(self, full_height: int, rank: int = 0, world: int = 1, group=None, row_coords: Optional[torch.Tensor] = None):
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} of a world of {world}")
        if full_height < world:
            raise NotImplementedError(f"pixel-split: {full_height} image rows cannot be shared out over {world} ranks "
                                      "(every rank needs a row)")
        self.full_height, self.rank, self.world, self.group = int(full_height), rank, world, group
        self.row_begin, self.row_end = shard_rows(full_height, world, rank)
        self.row_coords = row_coords
        self._dist = None
        if world > 1:
            import torch.distributed as dist
            self._dist = dist

    def all_reduce(self, t: torch.Tensor):
        if self._dist is not None:
            all_reduce_sum(self._dist, t, self.group)

    def reduce_pass(self, eng) -> torch.Tensor:
        """reduced_pass over this split's ranks: the pass enqueued, gradient and SSE summed -> the SSE view"""
        return reduced_pass(eng, self.all_reduce)

    def reduce_eval(self, eng) -> Tuple[float, int]:
        """after eval_sums(sync=False): (sse, sse8) of the full image - the double and the exact 64-bit integer sum"""
        sse, sse8 = eng.sse_view(), eng.sse8_view()
        self.all_reduce(sse)
        self.all_reduce(sse8)
        return float(sse.item()), int(sse8.item())

    def n_values(self, img: torch.Tensor) -> int:
        """numel of the FULL image whose rows [row_begin, row_end) `img` holds"""
        return self.full_height * img.shape[1] * img.shape[2]


def init_split_group(setting: str = "auto"):
    """The process group of a pixel-split `make fit`, from RANK / WORLD_SIZE / MASTER_* (torch.distributed.run sets them):
    (rank, world, made a group).  One group per process, with a finite timeout.  No WORLD_SIZE, or 1: a world of one, no group."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    backend, shared = split_backend(setting, local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))),
                                    torch.cuda.device_count() if torch.cuda.is_available() else 0)
    if world <= 1:
        return 0, 1, False
    import torch.distributed as dist
    if shared:
        logging.info(f"[rank {rank}] pixel-split: the node's ranks share a device - collectives over {backend}"
                     + (" (a rehearsal: the reduction goes through the host)" if backend == "gloo" else ""))
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=timedelta(seconds=SPLIT_TIMEOUT_S))
    return rank, world, True


class PixelSplitFit:
    """Data-parallel over pixels.  `backend` is anything with
         forward_backward(sync=False)   enqueue forward + backward of the local rows (no host sync)
         grad_view() -> flat fp32       the backend's OWN gradient buffer, already scaled by 1/(3*H*W) of the
                                        full image; all-reduced in place
         sse_view()  -> float64[1]      local sum of squared residuals on the backend's device; all-reduced in place
         adam_step(lr)
       (SirenEngine created with row_begin/row_end satisfies it).  `n_values` = 3*H*W of the full image.

    One step = two collectives on the backend's own buffers (P floats + one double), no staging copies and no host
    synchronisation: the stream stays busy across steps, and the loss is read back only when asked for."""

    def __init__(self, backend, n_values: int, group=None):
        import torch.distributed as dist
        self.dist, self.backend, self.n_values, self.group = dist, backend, n_values, group

    def _all_reduce(self, t: torch.Tensor):
        all_reduce_sum(self.dist, t, self.group)

    def step(self, lr: float, want_loss: bool = True):
        """One optimiser step on the full image; returns the global MSE (same on every rank) or None."""
        sse = reduced_pass(self.backend, self._all_reduce)
        loss = float(sse.item()) / self.n_values if want_loss else None   # read before the next pass overwrites it
        self.backend.adam_step(lr)
        return loss

    def steps(self, lrs: Sequence[float]) -> List[float]:
        """len(lrs) optimiser steps with no host read between them: each step's all-reduced SSE is copied into a table where
        the pass wrote it, and the table is read once at the end.  -> the global MSE of every step, step()'s values."""
        lrs = list(lrs)
        table = SseTable(len(lrs))
        for k, lr in enumerate(lrs):
            table.put(k, reduced_pass(self.backend, self._all_reduce))   # before the next pass overwrites it
            self.backend.adam_step(lr)
        return [s / self.n_values for s in table.read()]
