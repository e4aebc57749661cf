"""Deep-Compression style k-means quantisation of Linear weights (reference:
pipeline/quant/kmeans.py:110-181, kmeans_helper.py:59-115).

Index path (labels -> uint8 in the container) is bit-exact given identical weights.  The centroid
update uses `scatter_mean`, a third-party op (torch_scatter, absent and unpinned): it is restated here
from its documented semantics, so centroid VALUES are "parity unpinned" at that boundary.

Engine coupling: the reference hangs a forward-pre-hook on every nn.Linear; the engine-backed Siren
never calls those modules, so `KmeansQuant` registers ONE model-level callback that re-clusters all
non-skipped layers in module order right before every engine pass (Siren.engine()), and one
post-backward callback for the centroid nudge (kmeans.py:163-181).

Device route (`device_phase: auto`, conf/quant/kmeans.yaml): on an unpadded SIREN whose handle has sf_quant_pass /
sf_quant_nudge / sf_quant_step (csrc/siren_quant.hip) the two callbacks are one batched call each over persistent per-layer
buffers - no torch op and no host read per layer -, and train_steps() hands whole runs of quantise-phase steps to
sf_quant_step.  The pass gives the bits of the step-by-step path; the nudge sums in 64-bit fixed point where scatter_add_
uses float atomics, so it is deterministic run to run and within rounding of the host path's.
"""
import os
from typing import List, Sequence

import torch
from torch import nn


def scatter_mean(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """torch_scatter.scatter_mean(src, index, dim=0): per-index mean of the rows of `src`; output has
    index.max()+1 rows; empty bins are 0 (count clamped to 1)."""
    n = int(index.max().item()) + 1
    out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    out.index_add_(0, index, src)
    cnt = torch.zeros(n, dtype=src.dtype, device=src.device)
    cnt.index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype, device=src.device))
    return out / cnt.clamp(min=1).reshape(-1, *([1] * (src.dim() - 1)))


def _sq_dist(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[n,f] x [m,f] -> [n,m] squared euclidean distances (kmeans_helper.py:10-22)."""
    return ((a[:, None, :] - b[None, :, :]) ** 2.0).sum(dim=-1)


def kmeans_fit(x: torch.Tensor, cluster_centers: torch.Tensor, tolerance: float = 1e-4, iter_limit: int = 5):
    """<= 5 Lloyd iterations from the given centres; stops when (sum_k ||dc_k||)^2 < tol
    (kmeans_helper.py:59-98)."""
    x = x.float()
    labels = None
    for _ in range(iter_limit):
        labels = torch.argmin(_sq_dist(x, cluster_centers), dim=1)
        new_centers = scatter_mean(x, labels)
        shift = torch.sqrt(torch.sum((cluster_centers - new_centers) ** 2, dim=1)).sum()
        cluster_centers = new_centers
        if shift ** 2 < tolerance:
            break
    return labels, cluster_centers


def kmeans_predict(x: torch.Tensor, cluster_centers: torch.Tensor) -> torch.Tensor:
    return torch.argmin(_sq_dist(x, cluster_centers), dim=1)        # first index wins ties


def find_centroids_native(weight: torch.Tensor, n_clusters: int, eng):
    """The same on the engine's stream WITHOUT a host synchronisation (sf_kmeans_fit, csrc/siren_kmeans.hip): returns
    (centroids zero-padded to n_clusters entries, n_centroids as a device int32, labels, new_weight).  The initial guess is
    torch.linspace over masked min / max, so it is bit-identical to the torch path's.  Without a non-zero weight that is
    linspace(inf, -inf), no finite entry: k_km_init takes the non-finite ends for an empty call (no host read here)."""
    w = weight.detach().float().contiguous()
    return eng.kmeans_fit(w, native_guess(w, n_clusters - 1))


def native_guess(w: torch.Tensor, n_centres: int) -> torch.Tensor:
    """linspace(min, max, n_centres) over the non-zero entries of w without indexing by a mask (no host read for a size)"""
    nz = w != 0
    inf = torch.tensor(float("inf"), device=w.device)
    mn = torch.where(nz, w, inf).min()
    mx = torch.where(nz, w, -inf).max()
    return torch.linspace(mn, mx, n_centres, device=w.device, dtype=w.dtype)


def find_centroids(weight: torch.Tensor, n_clusters: int):
    """(centroids, labels, new_weight) of one weight tensor (kmeans.py:110-150): linspace(min,max)
    guess over the NON-ZERO weights with n_clusters-1 centres, 0 prepended, torch.unique, sorted by
    |c|, labels = nearest centroid of every weight (zeros included).  A tensor without a non-zero weight (a layer
    RigL has pruned away) gets the one centroid +0.0 and every label 0, where the reference raises on the empty
    .min() (sf_kmeans_fit returns the same)."""
    shape = weight.shape
    w = weight.reshape(-1, 1)
    nz = w[w != 0].reshape(-1, 1)
    if nz.numel() == 0:
        centroids = torch.zeros(1, device=w.device, dtype=w.dtype)
        labels = torch.zeros(shape, device=w.device, dtype=torch.int64)
        return centroids, labels, centroids[labels]
    guess = torch.linspace(nz.min(), nz.max(), n_clusters - 1, device=w.device, dtype=w.dtype).reshape(-1, 1)
    _, centroids = kmeans_fit(nz, guess)
    centroids = torch.cat((torch.zeros_like(centroids)[:1], centroids))
    centroids = torch.unique(centroids)
    _, order = torch.sort(centroids.abs())
    centroids = centroids[order]
    labels = kmeans_predict(w, centroids.reshape(-1, 1)).reshape(*shape)
    return centroids, labels, centroids[labels]


class KmeansQuant:
    def __init__(self, model: nn.Module, optim, bits: int = 5, skip_ll: Sequence[str] = ("layers.0.linear", "layers.7.linear"),
                 device_phase: str = "auto"):
        assert device_phase in ("auto", "off"), "device_phase: 'auto' (sf_quant_step where it applies) or 'off'"
        self.model, self.optim, self.bits, self.skip_ll = model, optim, bits, list(skip_ll)
        self.device_phase = device_phase
        self._plan = None                       # (engine, sf_quant_args over this quantiser's persistent buffers)
        self._in_bulk = False                   # bind_handle is running engine(): the pass belongs to sf_quant_step
        self._targets: List[nn.Linear] = [m for n, m in model.named_modules()
                                         if isinstance(m, nn.Linear) and n not in self.skip_ll]
        self._pre = self.kmeans_modify_weights
        self._post = self.scalar_quantization
        model.pre_pass_callbacks.append(self._pre)
        model.post_backward_callbacks.append(self._post)

    @property
    def n_clusters(self) -> int:
        return 2 ** self.bits

    @property
    def learning_rate(self) -> float:
        return self.optim.defaults["lr"]

    def is_whole_phase_of(self, model, optim) -> bool:
        """are this quantiser's two callbacks `model`'s only pre-pass and post-backward ones, and does it step `optim`"""
        return (list(model.pre_pass_callbacks) == [self._pre] and list(model.post_backward_callbacks) == [self._post]
                and self.optim is optim)

    def bind_handle(self, grid, img):
        """model.engine(grid, img) without the pre-pass (it belongs to the sf_quant_step to come) -> device_plan() on that handle"""
        self._in_bulk = True
        try:
            self.model.engine(grid, img)
        finally:
            self._in_bulk = False
        return self.device_plan()

    def device_wanted(self) -> bool:
        """what device_plan asks before there is a handle: the configuration, the model, the bits, the two knobs"""
        from ...models.siren import Siren
        return (self.device_phase == "auto" and isinstance(self.model, Siren) and self.model.state_is_live
                and 4 <= self.n_clusters <= 512 and bool(self._targets)
                and os.environ.get("SIREN_FIT_DEVICE_QUANT") != "0" and os.environ.get("SIREN_FIT_NATIVE_KMEANS", "1") != "0")

    def device_plan(self):
        """(engine, sf_quant_args) when the phase can run through the batched entry points, else None: device_phase "auto",
        an unpadded SIREN (state_is_live) bound to a handle whose library has them, 4 <= 2^bits <= 512, every quantised Linear
        the weight of an engine layer, and neither SIREN_FIT_DEVICE_QUANT nor SIREN_FIT_NATIVE_KMEANS "0" (A/B knobs, named
        like SIREN_FIT_DEVICE_MASK).  The buffers - centres, centroids (zero padded to 2^bits), n_centroids, labels - are made
        once per handle and are what m.centroids / m.n_centroids / m.labeled_weight then name."""
        from ... import _engine
        if not self.device_wanted():
            return None
        eng = self.model.bound_engine
        if eng is None or not callable(eng.quant_step) or not _engine.has_quant_step(eng.lib):
            return None
        if self._plan is not None and self._plan[0] is eng:
            return self._plan
        weights = [p for p in self.model._param_list()][0::2]
        layers = []
        for m in self._targets:
            idx = [i for i, w in enumerate(weights) if w is m.weight]
            if len(idx) != 1:
                return None
            layers.append(idx[0])
        if layers != sorted(layers):
            return None
        K, dev = self.n_clusters - 1, eng.device
        centres = [torch.zeros(K, device=dev) for _ in layers]
        centroids = [torch.zeros(K + 1, device=dev) for _ in layers]
        counts = [torch.ones(1, dtype=torch.int32, device=dev) for _ in layers]
        labels = [torch.zeros(m.weight.shape, dtype=torch.int64, device=dev) for m in self._targets]
        args = eng.quant_args(layers, centres, centroids, counts, labels, K, nudge_lr=self.learning_rate)
        self._plan = (eng, args)
        return self._plan

    def _name_buffers(self, args):
        """the plan's buffers under the names the host path leaves its results in"""
        _, _, centroids, counts, labels = args._keep
        for m, c, n, l in zip(self._targets, centroids, counts, labels):
            m.labeled_weight, m.centroids, m.n_centroids = l, c, n

    def device_steps(self, lrs, want_loss: bool = True):
        """len(lrs) quantise-phase steps - pass, forward_backward, nudge, Adam - in one sf_quant_step call on the plan's handle"""
        eng, args = self.device_plan()
        args.nudge_lr = self.learning_rate
        losses = eng.quant_step(args, lrs, want_loss=want_loss)
        self._name_buffers(args)
        return losses

    @torch.no_grad()
    def kmeans_modify_weights(self):
        """forward-pre-hook of the reference, for every quantised layer in module order (kmeans.py:66-72)."""
        if self._in_bulk:
            return
        plan = self.device_plan()
        if plan is not None:                    # one batched call: guess, Lloyd, centroids, labels, the weights into params
            plan[0].quant_pass(plan[1])
            self._name_buffers(plan[1])
            return
        eng = self.model.bound_engine
        if os.environ.get("SIREN_FIT_NATIVE_KMEANS", "1") == "0":       # A/B knob: the torch host mirror
            eng = None
        for m in self._targets:
            if eng is not None and m.weight.is_cuda and 4 <= self.n_clusters <= 512:
                # native path: five small kernels per layer on the engine's stream, no host sync; the centroid tensor keeps
                # its full 2^bits length (zero padded) until update_weights() trims it to the count the device reports.
                # (bits = 1 is one centre: its guess does not bracket the weights, sf_kmeans_fit refuses it)
                centroids, m.n_centroids, labels, new_weight = find_centroids_native(m.weight.data, self.n_clusters, eng)
            else:
                centroids, labels, new_weight = find_centroids(m.weight.data, self.n_clusters)
                m.n_centroids = None
            m.labeled_weight, m.centroids = labels, centroids
            m.weight.data.copy_(new_weight)

    @torch.no_grad()
    def scalar_quantization(self):
        """backward hook (kmeans.py:163-181): centroids -= lr * scatter_add(labels, dL/dW)."""
        plan = self.device_plan()
        if plan is not None and all(m.centroids is c for m, c in zip(self._targets, plan[1]._keep[2])):
            plan[1].nudge_lr = self.learning_rate
            plan[0].quant_nudge(plan[1])        # in place on the plan's centroid buffers, fixed-point segment sums
            return
        for m in self._targets:
            dw = torch.zeros_like(m.centroids)
            dw.scatter_add_(0, m.labeled_weight.flatten(), m.weight.grad.flatten())
            m.centroids = m.centroids - self.learning_rate * dw

    def remove_hooks(self):
        for lst, cb in ((self.model.pre_pass_callbacks, self._pre), (self.model.post_backward_callbacks, self._post)):
            if cb in lst:
                lst.remove(cb)

    @torch.no_grad()
    def update_weights(self):
        """Freeze centroids + labels as (non-trainable) parameters and write the codebook weights
        (kmeans.py:73-100)."""
        self.remove_hooks()
        for m in self._targets:
            centroids, labels = m.centroids, m.labeled_weight
            if getattr(m, "n_centroids", None) is not None:
                centroids = centroids[:int(m.n_centroids.item())].clone()   # (the one host read of the quantise phase: at its end)
                labels = labels.clone()         # (the device route's buffers are persistent)
                m.n_centroids = None
            m.centroids = nn.Parameter(centroids, requires_grad=False)
            m.labeled_weight = nn.Parameter(labels, requires_grad=False)
            m.weight.data.copy_(centroids[labels])
