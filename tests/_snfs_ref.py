"""The contract of sf_mask_update_snfs (include/siren_fit.h, csrc/siren_mask.hip) restated in numpy on CPU tensors: stable
sorts on the integer keys, so equal keys keep their index order in both directions, exact integer counts, an int64
fixed-point sum for the statistic, Python doubles for the rates and the water-filling.  What the kernels, the GPU tests and
the routing tests are compared with."""
import math
import struct

import numpy as np
import torch

WORDS = 12                                      # a statistics row: sf_mask_snfs_stats as int64 words (7, 8, 9, 11: doubles)
NAN_BITS = 0x7ff8000000000000


def dbits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def bits_d(word: int) -> float:
    return struct.unpack("<d", struct.pack("<q", int(word)))[0]


def momentum(m, v):
    """m / (sqrt(v) + 1e-8): three fp32 operations, each rounded to nearest (numpy float32 arithmetic is IEEE)"""
    with np.errstate(all="ignore"):
        return (m / (np.sqrt(v) + np.float32(1e-8))).astype(np.float32)


def statistic_of(m, v, k):
    """step 2 with statistic 1 for one layer -> (stat or None for status 3, A, s)"""
    a = np.abs(momentum(m, v))
    live = int((k == 1).sum())
    if not np.isfinite(a).all() or live == 0:
        return None
    amax = float(a.max())
    e = math.frexp(amax if amax > 0 else 1.0)[1]
    ln = 0
    while (1 << ln) < a.size + 1:
        ln += 1
    s = 60 - ln - e
    A = int(np.rint(a[k == 1].astype(np.float64) * math.ldexp(1.0, s)).astype(np.int64).sum())
    return (float(A) * math.ldexp(1.0, -s)) / float(live)


def water_filling(shares, pool, caps):
    """Masking.calc_redistributed_densities in doubles -> (budgets, rounds, the least |share * pool - half|)"""
    L = len(shares)
    asked = [sh * pool for sh in shares]
    half = min(abs(x - math.floor(x) - 0.5) for x in asked)
    budget = [float(round(x)) for x in asked]                   # (Python's round: half to even)
    share, rounds = 0.0, 0
    while rounds < 1000:
        excess = 0.0
        for j in range(L):
            want = budget[j] + share
            if want > caps[j]:
                excess = excess + (want - caps[j])
                want = caps[j]
            budget[j] = want
        share = excess / float(L)
        rounds += 1
        if not excess > 0.0:
            break
    return budget, rounds, half


def snfs_update_ref(w, g, m, v, k, slices, prune_rate, adjusted_growth, growth, statistic, dense_gradients):
    """One update, in place, on the flat fp32 CPU tensors w, g, m, v, k; slices: [(offset, n)] of the masked layers.
    -> (rows int64 [len(slices) + 1, WORDS] as the device writes them, info).  info: "tied": per layer [is the prune boundary
    tied, is the growth boundary tied] (the last element taken and the first one left hold the same key - the one place
    where the host path's unstable sorts may select another set); "near": per layer, the growth boundary's two keys are
    fewer than 4 ulp apart; "half": the least distance of share * pool from a half; "whole": the least distance of a budget
    from an integer (the truncation's margin; budgets that are integers exactly came out of the rounding and do not count)."""
    L = len(slices)
    W, G, M, V, K = (t.numpy() for t in (w, g, m, v, k))
    rows = np.zeros((L + 1, WORDS), dtype=np.int64)
    info = {"tied": [[False, False] for _ in slices], "near": [False] * L, "half": 1.0, "whole": 1.0}
    stats, bad = [], False
    for j, (off, n) in enumerate(slices):
        kk, ww = K[off:off + n], W[off:off + n]
        live, dead, nnz = int((kk == 1).sum()), int((kk == 0).sum()), int((ww != 0).sum())
        rows[j, :7] = [live, dead, nnz, 0, live, dead, nnz]
        st = float(nnz) if statistic == 0 else statistic_of(M[off:off + n], V[off:off + n], kk)
        bad |= st is None
        stats.append(st)
    if bad:
        rows[L, 0] = 3
        return torch.from_numpy(rows), info
    norm = 0.0
    for st in stats:
        norm = norm + st
    if norm == 0.0:
        rows[L, 0] = 1
        return torch.from_numpy(rows), info
    shares = [st / norm for st in stats]
    removed, rates = [], []
    for j, (off, n) in enumerate(slices):                       # 3. the rates and the prune
        kk, ww = K[off:off + n], W[off:off + n]
        live, dead = int(rows[j, 0]), int(rows[j, 1])
        frac_dead = dead / n
        capped = frac_dead < 0.2 and (math.inf if shares[j] == 0 else (1.0 / L) / shares[j]) < 1.0
        rate = min(frac_dead, prune_rate) if capped else prune_rate
        drop, gone = math.ceil(rate * live), 0
        if drop > 0:
            take = min(dead + drop, n)
            key = np.abs(ww).view(np.int32)
            order = np.argsort(key, kind="stable")
            info["tied"][j][0] = take < n and bool(key[order[take - 1]] == key[order[take]])
            kk[order[:take]] = 0.0
            gone = live - int(kk.sum())
        removed.append(gone)
        rates.append(rate)
    R = sum(removed)
    pool = float(R) + adjusted_growth
    rounds = 0
    if statistic == 0:                                          # 4. the budgets
        budget = [float(r) for r in removed]
    else:
        caps = [0.99 * float(int(rows[j, 1]) + removed[j]) for j in range(L)]
        budget, rounds, info["half"] = water_filling(shares, pool, caps)
        info["whole"] = min([min(b - math.floor(b), math.floor(b) + 1.0 - b) for b in budget if b != math.floor(b)] + [1.0])
    grown = [int(b) for b in budget]
    after = []
    for j, (off, n) in enumerate(slices):                       # 5. - 7.
        kk, ww, gg, mm, vv = (x[off:off + n] for x in (K, W, G, M, V))
        if grown[j] > 0:
            with np.errstate(all="ignore"):
                if growth == 2:
                    cand = np.abs((momentum(mm, vv) * (np.float32(1.0) - kk)).astype(np.float32))
                else:
                    cand = (np.abs(gg) * (np.float32(1.0) - kk)).astype(np.float32)
            key = ~cand.view(np.int32).astype(np.int64) & 0xffffffff          # the complement, as an unsigned word
            order = np.argsort(key, kind="stable")
            q = min(grown[j], n)
            if q < n:
                a, b = int(key[order[q - 1]]), int(key[order[q]])
                info["tied"][j][1] = a == b
                info["near"][j] = abs(a - b) < 4
            kk[order[:q]] = 1.0
            if growth == 1:
                ww[order[:q]] = 0.0
        ww *= kk
        if not dense_gradients:
            mm *= kk
            vv *= kk
            gg *= kk
        la = int((kk == 1).sum())
        st = float(int((ww != 0).sum())) if statistic == 0 else statistic_of(mm, vv, kk) if la else math.nan
        after.append(st)
        rows[j, 3:7] = [removed[j], la, int((kk == 0).sum()), int((ww != 0).sum())]
        rows[j, 7:] = [dbits(rates[j]), dbits(stats[j]), dbits(budget[j]), grown[j], NAN_BITS if math.isnan(st) else dbits(st)]
    norm_after = 0.0
    for st in after:
        if not math.isnan(st):
            norm_after = norm_after + st
    rows[L] = [0, rounds, R, sum(grown), 0, 0, 0, dbits(pool), dbits(norm), 0, 0, dbits(norm_after)]
    return torch.from_numpy(rows), info
