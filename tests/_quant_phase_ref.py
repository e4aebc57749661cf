"""What the batched kernels of the quantise phase compute beyond tests/_kmeans_ref.py (include/siren_fit.h, csrc/siren_quant.hip),
restated in numpy on the CPU: the guess of sf_quant_pass and the centroid nudge of sf_quant_nudge, every operation rounded
where the kernels round it, so nothing here has a tolerance.  The Lloyd iterations, the centroids and the labels are
_kmeans_ref.kmeans_ref's.

  guess   min / max over the non-zero weights (+inf / -inf without one); step = float32((max - min) / (K - 1)); entry i is
          fma(step, i, min) below K // 2 and fma(-step, K - 1 - i, max) from there on, one rounding each
  nudge   unit 2^(60 - ln - e) with n < 2^ln and max|g| < 2^e (frexp; 1 for a zero or non-finite maximum); a gradient enters
          its label's sum as rint(float64(g) * unit), an int64; dw = float32(float64(sum) / unit), one rounding;
          c <- float32(c - float32(lr * dw))
"""
import math

import numpy as np

import _kmeans_ref as R

F32 = np.float32


def fma_f32(a, b, c):
    """float32(a * b + c) rounded ONCE, for float32 arrays whose product is exact in float64 (a 24-bit by a <= 29-bit
    significand).  The float64 sum is rounded once already; where it lands exactly between two float32 values the sign of
    its own rounding error (TwoSum) says on which side the exact value lies."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b                                                  # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                            # s + err == p + c exactly
        r = s.astype(F32)
        r64 = r.astype(np.float64)
        other = np.nextafter(r, np.where(s > r64, F32(np.inf), F32(-np.inf)).astype(F32)).astype(np.float64)
        tie = np.isfinite(s) & np.isfinite(other) & (s != r64) & (np.abs(s - r64) == np.abs(other - s)) & (err != 0)
        up = np.maximum(r64, other)
        down = np.minimum(r64, other)
        fixed = np.where(err > 0, up, down).astype(F32)
    return np.where(tie, fixed, r).astype(F32)


def guess_ends(w):
    """(min, max) over the non-zero entries as float32; (+inf, -inf) without one"""
    w = np.asarray(w, F32).reshape(-1)
    x = w[w != 0]
    return (F32(np.inf), F32(-np.inf)) if x.size == 0 else (x.min(), x.max())


def guess_from_ends(start, end, K, fused=True):
    """torch.linspace(start, end, K) in ATen's fp32 device form.  fused=False: the product rounded before the sum"""
    start, end = F32(start), F32(end)
    with np.errstate(invalid="ignore", over="ignore"):
        step = F32(F32(end - start) / F32(K - 1))
        i = np.arange(K)
        lo, hi = i[:K // 2].astype(F32), (K - 1 - i[K // 2:]).astype(F32)
        if fused:
            return np.concatenate([fma_f32(np.full(lo.size, step, F32), lo, np.full(lo.size, start, F32)),
                                   fma_f32(np.full(hi.size, -step, F32), hi, np.full(hi.size, end, F32))])
        return np.concatenate([(start + (step * lo).astype(F32)).astype(F32), (end - (step * hi).astype(F32)).astype(F32)])


def guess(w, K, fused=True):
    return guess_from_ends(*guess_ends(w), K, fused)


def quant_pass_ref(w, K, iter_limit=5, tol=1e-4):
    """one layer of sf_quant_pass: the guess, then sf_kmeans_fit's contract with the centroids padded to K + 1"""
    g = guess(w, K)
    return R.kmeans_ref(w, g, iter_limit=iter_limit, tol=tol), g


def nudge_unit(g, n):
    g = np.asarray(g, F32).reshape(-1)
    m = float(np.abs(g).max()) if g.size else 0.0
    if not (m > 0 and math.isfinite(m)):
        m = 1.0
    _, e = math.frexp(m)                                           # m < 2^e
    ln = 0
    while (1 << ln) < n + 1:                                       # n < 2^ln
        ln += 1
    return math.ldexp(1.0, 60 - ln - e)


def nudge_ref(cent, labels, g, lr):
    """sf_quant_nudge on one layer -> (the new centroids float32 [len(cent)], dw float32, the unit)"""
    cent, g = np.asarray(cent, F32).reshape(-1), np.asarray(g, F32).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    unit = nudge_unit(g, g.size)
    q = np.rint(g.astype(np.float64) * unit).astype(np.int64)
    sums = np.zeros(cent.size, np.int64)
    np.add.at(sums, labels, q)
    dw = (sums.astype(np.float64) * (1.0 / unit)).astype(F32)
    step = (F32(lr) * dw).astype(F32)
    return (cent - step).astype(F32), dw, unit


def nudge_bound(cent, labels, g, lr):
    """Per centroid, how far c - lr * dw may lie from the exact c - lr * sum(g) (float64 segment sums), derived:
    lr * (n_k * 2^-24 * sum|g_i| + two float roundings).  A float32 sum of n_k terms in any order is within
    (n_k - 1) * 2^-24 * sum|g_i| of the exact one, the once-rounded fixed-point sum within 2^-24 * |sum| + n_k * 0.5 / unit; the
    two roundings are those of lr * dw and of the difference, half an ulp each: 2^-24 of the value (taken at the exact value,
    times 1 + 2^-20 for the second-order difference to the computed one) or half the smallest subnormal.
    -> (exact float64 result, the bound)"""
    cent, g = np.asarray(cent, F32).astype(np.float64).reshape(-1), np.asarray(g, F32).astype(np.float64).reshape(-1)
    labels = np.asarray(labels, np.int64).reshape(-1)
    lr = float(F32(lr))
    exact, mass, cnt = np.zeros(cent.size), np.zeros(cent.size), np.zeros(cent.size)
    np.add.at(exact, labels, g)                                    # (float64: 2^-53 per term, nothing at this scale)
    np.add.at(mass, labels, np.abs(g))
    np.add.at(cnt, labels, 1.0)
    u = 2.0 ** -24
    sub = 2.0 ** -149
    want = cent - lr * exact
    bound = lr * cnt * u * mass + (1 + 2.0 ** -20) * u * (np.abs(lr * exact) + np.abs(want)) + 2 * sub
    return want, bound
