"""The contract of sf_mask_update (include/siren_fit.h, csrc/siren_mask.hip) restated as torch code on CPU tensors: stable
sorts, so equal keys keep their index order in both directions, exact integer counts, double rate arithmetic.  What the
kernels, the GPU tests and the routing tests are compared with."""
import math
import struct

import torch

WORDS = 8                                       # a statistics row: seven int64 counts and the bits of the double rate


def rate_bits(rate: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(rate)))[0]


def bits_rate(word: int) -> float:
    return struct.unpack("<d", struct.pack("<q", int(word)))[0]


def mask_update_ref(w, g, m, v, k, slices, prune_rate, growth, dense_gradients):
    """One update, in place, on the flat fp32 CPU vectors w, g, m, v, k; slices: [(offset, n)] of the masked layers.
    -> (rows int64 [len(slices) + 1, WORDS] as the device writes them, [per layer: is the prune boundary tied, is the
    growth boundary tied]).  A boundary is tied when the last element taken and the first one left hold the same key: the
    one place where the host path's unstable sorts may select another set."""
    L = len(slices)
    rows = torch.zeros(L + 1, WORDS, dtype=torch.int64)
    tied = [[False, False] for _ in slices]
    for j, (off, n) in enumerate(slices):
        kk, ww = k[off:off + n], w[off:off + n]
        live, dead, nnz = int((kk == 1).sum()), int((kk == 0).sum()), int((ww != 0).sum())
        rows[j, :7] = torch.tensor([live, dead, nnz, 0, live, dead, nnz])
    S = int(rows[:L, 2].sum())
    if S == 0:
        rows[L, 0] = 1
        return rows, tied
    for j, (off, n) in enumerate(slices):
        kk, ww, gg = k[off:off + n], w[off:off + n], g[off:off + n]
        live, dead, nnz = (int(x) for x in rows[j, :3])
        share, frac_dead = nnz / S, dead / n
        capped = frac_dead < 0.2 and (math.inf if share == 0 else (1.0 / L) / share) < 1.0
        rate = min(frac_dead, prune_rate) if capped else prune_rate
        drop = math.ceil(rate * live)
        removed = 0
        if drop > 0:
            take = min(dead + drop, n)
            mag, order = torch.sort(ww.abs(), stable=True)
            tied[j][0] = take < n and bool(mag[take - 1] == mag[take])
            kk[order[:take]] = 0.0
            removed = live - int(kk.sum())
        if growth == 1 and not bool((kk == 1).all()):
            cand, order = torch.sort(gg.abs() * (1.0 - kk), descending=True, stable=True)
            tied[j][1] = 0 < removed < n and bool(cand[removed - 1] == cand[removed])
            pick = order[:removed]
            kk[pick] = 1.0
            ww[pick] = 0.0
        ww.mul_(kk)
        if not dense_gradients:
            m[off:off + n].mul_(kk)
            v[off:off + n].mul_(kk)
            gg.mul_(kk)
        rows[j, 3:] = torch.tensor([removed, int((kk == 1).sum()), int((kk == 0).sum()), int((ww != 0).sum()), rate_bits(rate)])
    return rows, tied
