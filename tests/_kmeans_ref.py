"""What sf_kmeans_fit computes (include/siren_fit.h, csrc/siren_kmeans.hip), restated in numpy on the CPU: the contract the
five kernels k_km_init / k_km_assign / k_km_update / k_km_finish / k_km_predict are held to, bit for bit.  Written from the
header and the kernel comments; every operation is rounded where the kernels round it, so nothing here has a tolerance.

  labels      argmin_k of (x - c_k) * (x - c_k), every operation rounded to float32, the first index wins ties.  The fit
              runs over the non-zero weights (x == 0 excludes -0.0 and +0.0), the prediction over all weights
  fixed point scale = 2^(60 - ln - e) with max(|guess[0]|, |guess[K-1]|) < 2^e (frexp; 1 for a zero maximum) and n < 2^ln;
              a weight enters its segment sum as rint(float64(x) * scale), an int64; integer sums
  centres     float32(float64(sum) * (1 / scale) / float64(count)); an empty bin gives +0.0
  stop test   shifts sqrt((old - new) * (old - new)) in float32, added in index order in float32; stop once s * s < tol
  finish      {+0.0} in front of the centres, unique (-0.0 and +0.0 merge, the +0.0 in front survives), ordered by |c| with
              the smaller value first among equal magnitudes, zero padded to the capacity
  empty call  a guess whose first or last entry is not finite: the centres stay, one centroid +0.0, every label 0

Below it two checks in exact / float64 arithmetic that do not use the restatement's arithmetic (centres are the means of
their clusters, labels are nearest), and the inputs of the case table that tests/test_kmeans_host.py (CPU) and
tests/_kmeans_child.py (MI355X) share."""
import math
from fractions import Fraction

import numpy as np

MAX_K = 512                                    # sf_kmeans_fit takes 2 <= K < 512
BLOCK = 4096                                   # rows per distance block: 4096 x 511 floats, not n x K at once
F32 = np.float32


class Fit(dict):
    __getattr__ = dict.get


def _argmin_f32(x, c, tie="first"):
    """labels of x [n] against c [K]: float32 (x - c) * (x - c), the first index wins ties.  -> (labels, how many elements
    had their smallest distance at more than one index)"""
    out, ties = np.empty(x.size, np.int64), 0
    for a in range(0, x.size, BLOCK):
        d = x[a:a + BLOCK, None] - c[None, :]                      # float32 - float32 -> float32, rounded once
        dd = d * d                                                 # rounded once
        if tie == "first":
            out[a:a + BLOCK] = np.argmin(dd, axis=1)
        else:                                                      # (the flipped rule the host tests try once)
            out[a:a + BLOCK] = c.size - 1 - np.argmin(dd[:, ::-1], axis=1)
        ties += int(((dd == dd.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    return out, ties


def fixed_point_scale(guess, n):
    """the unit of the segment sums (k_km_init): a power of two, as a float64"""
    m = max(abs(F32(guess[0])), abs(F32(guess[-1])))
    _, e = math.frexp(float(m) if m > 0 else 1.0)                  # m < 2^e
    ln = 0
    while (1 << ln) < n + 1:                                       # n < 2^ln
        ln += 1
    return math.ldexp(1.0, 60 - ln - e)


def _segment_means(x, labels, K, scale, fixed_point=True):
    if not fixed_point:                                            # (the float32 sum the host tests try once)
        sums, cnt = np.zeros(K, F32), np.zeros(K, np.int64)
        np.add.at(sums, labels, x)
        np.add.at(cnt, labels, 1)
        return np.where(cnt > 0, sums / np.maximum(cnt, 1).astype(F32), F32(0)).astype(F32), cnt
    q = np.rint(x.astype(np.float64) * scale).astype(np.int64)     # llrint: to nearest, ties to even
    sums, cnt = np.zeros(K, np.int64), np.zeros(K, np.int64)
    np.add.at(sums, labels, q)
    np.add.at(cnt, labels, 1)
    mean = sums.astype(np.float64) * (1.0 / scale) / np.maximum(cnt, 1).astype(np.float64)
    return np.where(cnt > 0, mean.astype(F32), F32(0)).astype(F32), cnt


def finish(centres, cap, abs_tie="smaller_first"):
    """{+0.0} U centres -> unique -> ordered by |c| -> (centroids zero padded to cap, how many are real)"""
    v = np.concatenate([np.zeros(1, F32), np.asarray(centres, F32)])
    s = v[np.argsort(v, kind="stable")]                            # ascending; equal values (-0.0 == +0.0) keep their order
    u = s[np.concatenate([[True], s[1:] != s[:-1]])]               # the first of every run of equal values
    if abs_tie != "smaller_first":                                 # (the reversed order the host tests try once)
        u = u[::-1]
    u = u[np.argsort(np.abs(u), kind="stable")]                    # by |c|; -c before +c
    out = np.zeros(cap, F32)
    out[:u.size] = u
    return out, int(u.size)


def kmeans_ref(w, guess, iter_limit=5, tol=1e-4, cap=None, tie="first", fixed_point=True, abs_tie="smaller_first"):
    """sf_kmeans_fit(w, guess as centers_dev, K = len(guess), iter_limit, tol, centroids_cap = cap or K + 1).
    -> Fit(centroids [cap], n_centroids, labels [n] int64, new_weight [n], centres [K] as left in centers_dev, iterations
    that ran, last_ss: the last s * s (None without an iteration), fit_labels: the last assignment of the non-zero weights,
    nonzero: those weights, scale, empty, ties: per assignment - the fit's, then the prediction's - how many elements had an
    exact tie at their smallest float32 distance).  tie / fixed_point / abs_tie are the three mutations of the host tests."""
    w = np.ascontiguousarray(w, F32).reshape(-1)
    centres = np.array(guess, F32).reshape(-1)
    K, n = centres.size, w.size
    assert n > 0 and 2 <= K < MAX_K and iter_limit >= 0
    cap = K + 1 if cap is None else cap
    assert cap >= K + 1
    tol = F32(tol)
    x = w[w != 0]
    res = Fit(nonzero=x, iterations=0, last_ss=None, fit_labels=None, ties=[], scale=fixed_point_scale(centres, n),
              empty=not (np.isfinite(centres[0]) and np.isfinite(centres[-1])))
    if res.empty:
        cent = np.zeros(cap, F32)
        return Fit(res, centroids=cent, n_centroids=1, labels=np.zeros(n, np.int64), new_weight=np.zeros(n, F32), centres=centres)
    for _ in range(iter_limit):
        lab, t = _argmin_f32(x, centres, tie)
        res.ties.append(t)
        new, _ = _segment_means(x, lab, K, res.scale, fixed_point)
        d = centres - new
        shift = np.sqrt(d * d)                                     # float32 throughout
        s = F32(0)
        for v in shift:                                            # index order
            s = F32(s + v)
        centres = new
        res.update(iterations=res.iterations + 1, last_ss=F32(s * s), fit_labels=lab)
        if res.last_ss < tol:
            break
    cent, nc = finish(centres, cap, abs_tie)
    labels, t = _argmin_f32(w, cent[:nc], tie)
    res.ties.append(t)
    return Fit(res, centroids=cent, n_centroids=nc, labels=labels, new_weight=cent[:nc][labels], centres=centres)


def linspace_guess(w, K):
    """torch.linspace(min, max, K) over the non-zero weights on the CPU: what find_centroids_native builds (for a tensor
    without one: linspace(inf, -inf, K))"""
    import torch
    t = torch.tensor(np.array(w, F32)).reshape(-1)
    nz = t != 0
    inf = torch.tensor(float("inf"))
    return torch.linspace(torch.where(nz, t, inf).min(), torch.where(nz, t, -inf).max(), K, dtype=torch.float32).numpy()


# ---- two checks that do not use the arithmetic above ----------------------------------------------------------------------
def _ulp32(v):
    """the spacing of float32 at |v| (a float64), 2^-149 in the subnormal range"""
    if v == 0:
        return math.ldexp(1.0, -149)
    _, e = math.frexp(abs(v))                                      # |v| in [2^(e-1), 2^e)
    return math.ldexp(1.0, max(e - 1 - 23, -149))


def check_centres_are_means(x, fit_labels, centres, scale):
    """For every non-empty cluster of the last assignment |centre - mean| <= 0.5 * ulp32(mean) + 0.5 / scale + 2^-51 * |mean|:
    one float rounding, one fixed-point rounding per element (their mean is at most 0.5 / scale), two double roundings
    (int64 -> double, the division; the product with the power of two 1 / scale is exact).  Derived, not measured.  The mean
    is exact: every float32 is an integer multiple of 2^-149, so the sum is an integer sum.  -> (worst ratio error / bound,
    clusters checked); an empty cluster must hold +0.0"""
    x64 = np.asarray(x, np.float64)
    worst, checked = 0.0, 0
    unit = Fraction(1, 2 ** 149)
    for k in range(len(centres)):
        sel = x64[fit_labels == k]
        if sel.size == 0:
            assert centres[k] == 0 and not np.signbit(centres[k]), (k, centres[k])
            continue
        total = sum(int(v) for v in sel * 2.0 ** 149)              # exact: a scaling by a power of two, then integers
        mean = Fraction(total, sel.size) * unit
        m64 = float(mean)
        bound = Fraction(0.5 * _ulp32(m64)) + Fraction(0.5 / scale) + Fraction(2.0 ** -51) * abs(mean)
        err = abs(Fraction(float(centres[k])) - mean)
        assert err <= bound, (k, float(centres[k]), m64, float(err), float(bound))
        worst, checked = max(worst, float(err / bound)), checked + 1
    return worst, checked


def check_labels_are_nearest(x, labels, cents):
    """(x - c_label)^2 <= min_k (x - c_k)^2 * (1 + 2^-21) in float64: the factor covers two float roundings of the difference
    and one of the square, on both sides.  Where the float32 distances tie exactly, the lowest index holds.  -> how many
    elements had such a tie"""
    x32, c32 = np.asarray(x, F32), np.asarray(cents, F32)
    x64, c64 = x32.astype(np.float64), c32.astype(np.float64)
    ties = 0
    for a in range(0, x32.size, BLOCK):
        lab = labels[a:a + BLOCK]
        rows = np.arange(lab.size)
        dd = (x64[a:a + BLOCK, None] - c64[None, :]) ** 2
        assert np.all(dd[rows, lab] <= dd.min(axis=1) * (1 + 2.0 ** -21)), "a label is not the nearest centroid"
        d32 = x32[a:a + BLOCK, None] - c32[None, :]
        d32 = d32 * d32
        at_min = d32 == d32.min(axis=1, keepdims=True)
        assert np.array_equal(at_min.argmax(axis=1), lab), "an exact float32 tie did not go to the lowest index"
        ties += int((at_min.sum(axis=1) > 1).sum())
    return ties


# ---- the inputs of the case table ------------------------------------------------------------------------------------------
STOPS_AT_THREE_SCALE = 0.06                    # found on the CPU between 0.03 (stops at 2) and 0.1 (stops at 5)
ASSUMED_CUS = 256                              # the host tests' CUs for `grid_stride`; the GPU child asks the device
#        name                          K    seed
TABLE = [("five_iterations",           31,  1001),
         ("stops_at_three",            31,  1002),
         ("bits8_empty_bins",          255, 1003),
         ("bits9_limit",               511, 1004),
         ("fewer_points_than_centres", 31,  1006),    # (1005 puts two of the five points into one cluster)
         ("constant_layer",            7,   0),
         ("plus_minus",                3,   1007),
         ("quantised",                 31,  1033),    # ties in the second assignment of the fit and in the prediction
         ("wide_range",                31,  1009),
         ("pruned_minus_zero",         31,  1010),
         ("grid_stride",               31,  1050),    # (a seed at which the float32 sums of the mirror tip no label)
         ("single_weight",             3,   0)]
K_OF = {name: K for name, K, _ in TABLE}
NOT_MIRRORED = ("pruned_minus_zero",)          # w[w != 0] is the same set as without the -0.0: nothing new for the mirror


def make_input(name, cus=ASSUMED_CUS):
    """the float32 weights of a table row, seeded on the CPU -> numpy [n]"""
    import torch
    gen = torch.Generator().manual_seed(dict((n, s) for n, _, s in TABLE)[name])
    randn = lambda n: torch.randn(n, generator=gen)
    if name == "five_iterations":
        w = randn(4097)
    elif name == "stops_at_three":
        w = randn(4097) * STOPS_AT_THREE_SCALE
    elif name == "bits8_empty_bins":
        w = randn(4097)
    elif name == "bits9_limit":
        w = randn(70001)
    elif name == "fewer_points_than_centres":
        w = randn(5)
    elif name == "constant_layer":
        w = torch.full((300,), 0.25)
    elif name == "plus_minus":
        w = torch.where(randn(1000) < 0, -0.5, 0.5)
    elif name == "quantised":
        w = torch.round(randn(4097) * 8) / 8
    elif name == "wide_range":
        w = randn(3000) * torch.exp(torch.rand(3000, generator=gen) * 33 - 30)
        w = torch.cat([w, torch.tensor([1e-40, -3e-41, 7e-45, -1e-39, 5e-42])])
    elif name == "pruned_minus_zero":
        w = randn(65536) * 0.1
        w = w * (torch.rand(65536, generator=gen) < 0.1).float()   # a product: a pruned negative weight becomes -0.0
    elif name == "grid_stride":
        w = randn(4 * cus * 256 + 257) * 0.05
    elif name == "single_weight":
        w = torch.zeros(65)
        w[17] = -0.375
    else:
        raise KeyError(name)
    return w.float().contiguous().numpy()


def row_condition(name, w, fit, cus=ASSUMED_CUS):
    """the last column of the table: what makes the row reach its path.  -> None or a message"""
    K, cent, nc = K_OF[name], fit.centroids, fit.n_centroids
    tol = F32(1e-4)
    if name == "five_iterations":
        ok = fit.iterations == 5 and fit.last_ss >= tol and w.size % 256 != 0
    elif name == "stops_at_three":
        ok = fit.iterations == 3 and fit.last_ss < tol
    elif name == "bits8_empty_bins":
        ok = nc < 256
    elif name == "bits9_limit":
        ok = nc < 512 and K > 256
    elif name == "fewer_points_than_centres":
        ok = nc == 6 and w.size < K
    elif name == "constant_layer":
        ok = nc == 2 and cent[:2].tolist() == [0.0, 0.25]
    elif name == "plus_minus":
        ok = nc == 3 and cent[:3].tolist() == [0.0, -0.5, 0.5]
    elif name == "quantised":
        ok = sum(fit.ties) > 0 and bool((w == 0).any())           # (a tie at the smallest distance, in any assignment)
    elif name == "wide_range":
        p = fit.nonzero.astype(np.float64) * fit.scale
        ok = bool((p != np.rint(p)).any()) and bool((np.abs(w[w != 0]) < 2.0 ** -126).any())
    elif name == "pruned_minus_zero":
        ok = int(((w == 0) & np.signbit(w)).sum()) >= 1000 and int(((w == 0) & ~np.signbit(w)).sum()) >= 1000
    elif name == "grid_stride":
        ok = w.size > 4 * cus * 256
    elif name == "single_weight":
        ok = nc == 2 and int((w != 0).sum()) == 1
    return None if ok else f"{name} no longer reaches its path (iterations {fit.iterations}, last s*s {fit.last_ss}, centroids {nc})"
