"""The contract of sf_mask_prune_global (include/siren_fit.h, csrc/siren_mask.hip) restated as torch code on CPU tensors:
exact integer counts, the threshold search in Python floats (IEEE doubles, one rounding per operation), fp32 comparisons.
What the kernels, the GPU tests and the routing tests are compared with."""
import math
import struct

import torch

from _mask_update_ref import WORDS, bits_rate, rate_bits

TRIAL_CAP = 4096                                # kPruneTrialCap
STATUS, TRIALS, ALIVE, REMOVED, TARGET, THRESHOLD = 0, 1, 2, 3, 4, 7       # words of the status row


def f32(x: float) -> torch.Tensor:
    """the double rounded to fp32, to nearest-even (beyond the fp32 range: inf, which no weight exceeds)"""
    return torch.tensor(x, dtype=torch.float64).to(torch.float32)


def threshold_of(rows) -> float:
    return bits_rate(rows[-1][THRESHOLD])


def prune_global_ref(w, g, m, v, k, slices, target, prune_rate, threshold, increment, tolerance, dense_gradients):
    """One update, in place, on the flat fp32 CPU vectors w, g, m, v, k; slices: [(offset, n)] of the masked layers.
    -> rows int64 [len(slices) + 1, WORDS] as the device writes them."""
    L = len(slices)
    rows = torch.zeros(L + 1, WORDS, dtype=torch.int64)
    for j, (off, n) in enumerate(slices):       # 1. counts
        kk, ww = k[off:off + n], w[off:off + n]
        live, dead, nnz = int((kk == 1).sum()), int((kk == 0).sum()), int((ww != 0).sum())
        rows[j, :7] = torch.tensor([live, dead, nnz, 0, live, dead, nnz])
    S, alive = int(rows[:L, 2].sum()), int(rows[:L, 0].sum())
    target = int(target)

    def status_row(status, trials, removed, thr):
        rows[L] = torch.tensor([status, trials, alive, removed, target, 0, 0, rate_bits(thr)])
        return rows

    if S == 0:
        return status_row(1, 0, 0, threshold)
    mags = torch.cat([w[off:off + n].abs() for off, n in slices])
    thr, removed, trials, searched = float(threshold), 0, 0, target > 0
    if searched:                                # 4. the search
        slack = target * tolerance
        step, previous, stalled = float(increment), 0, 0
        while abs(removed - target) > slack:
            if trials == TRIAL_CAP:
                return status_row(2, trials, removed, threshold)
            removed = alive - int((mags > f32(thr)).sum())
            trials += 1
            stalled = stalled + 1 if removed == previous else 0
            if stalled == 10:
                break
            previous = removed
            if removed > target * (1.0 + tolerance):
                thr *= 1.0 - step
                step *= 0.99
            elif removed < target * (1.0 - tolerance):
                thr *= 1.0 + step
                step *= 0.99
    for j, (off, n) in enumerate(slices):
        kk, ww = k[off:off + n], w[off:off + n]
        live, dead, nnz = (int(x) for x in rows[j, :3])
        share, frac_dead = nnz / S, dead / n    # 2. rates
        capped = frac_dead < 0.2 and (math.inf if share == 0 else (1.0 / L) / share) < 1.0
        rate = min(frac_dead, prune_rate) if capped else prune_rate
        if searched:                            # 5. masks
            kk.copy_((ww.abs() > f32(thr)).float())
        ww.mul_(kk)                             # 6. apply
        if not dense_gradients:
            m[off:off + n].mul_(kk)
            v[off:off + n].mul_(kk)
            g[off:off + n].mul_(kk)
        after = int((kk == 1).sum())
        rows[j, 3:] = torch.tensor([live - after, after, int((kk == 0).sum()), int((ww != 0).sum()), rate_bits(rate)])
    return status_row(0, trials, removed, thr)


def threshold_bits(x: float) -> bytes:
    return struct.pack("<d", float(x))
