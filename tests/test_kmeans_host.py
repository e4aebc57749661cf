"""The k-means quantiser on the CPU: tests/_kmeans_ref.py (the contract of sf_kmeans_fit, restated in numpy) against the
reference-minted fixtures, against two float64 / exact checks that do not use its arithmetic, and against the torch mirror
(pipeline/quant/kmeans.py::find_centroids) on every input of the case table that tests/test_gpu_kmeans.py runs on the device;
the conditions that make each row reach its kernel path; the routing of KmeansQuant between the two."""
import functools

import numpy as np
import pytest
import torch
from torch import nn

import _kmeans_ref as R
from implicit_image.pipeline.quant import KmeansQuant, find_centroids

ROWS = [name for name, _, _ in R.TABLE]


@functools.lru_cache(maxsize=None)
def row(name):
    """(weights, the restatement's fit) of a table row, computed once"""
    w = R.make_input(name)
    w.setflags(write=False)
    return w, R.kmeans_ref(w, R.linspace_guess(w, R.K_OF[name]))


FIXTURES = [("kmeans_64x64", f"b{b}_l{l}_", f"b{b}_l{l}_weight", 2 ** b, it)
            for b, it in ((4, 1), (8, 2)) for l in (1, 2)] + [("kmeans_256x256", f"b{b}_", "weight", 2 ** b, 1) for b in (5, 8)]


@pytest.mark.parametrize("file,prefix,weight,clusters,iterations", FIXTURES, ids=[f[0][7:] + "_" + f[1][:-1] for f in FIXTURES])
def test_restatement_against_the_reference_fixtures(golden, file, prefix, weight, clusters, iterations):
    """labels and the centroid count bit-equal to what the reference's own code produced, centroids within the rtol 2e-6 /
    atol 1e-9 of the device tests (the reference sums in float32).  The fixtures end after one or two Lloyd iterations: if
    one ever reaches 3, the statement "iterations 3 to 5 are reached by the case table only" is out of date."""
    d = golden(file)
    w = d[weight]
    fit = R.kmeans_ref(w, R.linspace_guess(w, clusters - 1))
    ref_c = d[prefix + "centroids"]
    assert fit.n_centroids == ref_c.size
    assert np.array_equal(fit.labels.reshape(w.shape), d[prefix + "labels"])
    assert np.allclose(fit.centroids[:fit.n_centroids], ref_c, rtol=2e-6, atol=1e-9)
    assert not fit.centroids[fit.n_centroids:].any()
    assert fit.iterations == iterations, "the fixtures' iteration counts changed: the case table's claim is out of date"
    assert fit.iterations < 3
    assert R.check_centres_are_means(fit.nonzero, fit.fit_labels, fit.centres, fit.scale)[1] > 0
    R.check_labels_are_nearest(w.reshape(-1), fit.labels, fit.centroids[:fit.n_centroids])


@pytest.mark.parametrize("name", ROWS)
def test_row_reaches_its_path(name):
    """the last column of the case table, so that an edit of an input cannot make a row stop exercising its path"""
    w, fit = row(name)
    assert w.dtype == np.float32 and R.row_condition(name, w, fit) is None, R.row_condition(name, w, fit)


@pytest.mark.parametrize("name", ROWS)
def test_restatement_against_the_float64_checks(name):
    """centres are the exact means of their clusters to one float rounding, one fixed-point rounding and two double
    roundings; every label is the nearest centroid in float64 to the roundings of the float32 distance, and the lowest
    index where float32 distances tie"""
    w, fit = row(name)
    worst, checked = R.check_centres_are_means(fit.nonzero, fit.fit_labels, fit.centres, fit.scale)
    print(name, "iterations", fit.iterations, "centroids", fit.n_centroids, "worst error / bound", worst, "clusters", checked)
    assert checked > 0 and worst <= 1.0
    ties = R.check_labels_are_nearest(w, fit.labels, fit.centroids[:fit.n_centroids])
    assert ties == fit.ties[-1]
    assert np.array_equal(fit.new_weight.view(np.int32), fit.centroids[fit.labels].view(np.int32))
    assert not fit.centroids[fit.n_centroids:].any() and not np.signbit(fit.centroids[0]) and fit.centroids[0] == 0


@pytest.mark.parametrize("name", [n for n in ROWS if n not in R.NOT_MIRRORED])
def test_restatement_against_the_torch_mirror(name):
    """find_centroids on the CPU copy: the same labels and centroid count, centres within 2e-6 relative (the mirror sums in
    float32, so this holds where no point sits within rounding of a midpoint: if a seed breaks it, change the seed).
    Relative as relerr of tests/_gpu_fixtures.py has it: the largest difference over the largest centre.  Centre by centre
    the 2e-6 hold on every row but grid_stride, whose clusters of up to 17 000 elements put the rounding of a sequential
    float32 sum (about sqrt(count) * 2^-24 of it) above that: 4e-6 .. 6e-4 over forty seeds, 1.1e-4 at this one, for
    9.8e-7 of the largest centre."""
    w, fit = row(name)
    cent, labels, new_w = find_centroids(torch.tensor(w), R.K_OF[name] + 1)
    assert cent.numel() == fit.n_centroids
    assert np.array_equal(labels.numpy(), fit.labels)
    ref = fit.centroids[:fit.n_centroids].astype(np.float64)
    diff = np.abs(cent.numpy().astype(np.float64) - ref)
    print(name, "of the largest centre", diff.max() / np.abs(ref).max(), "centre by centre", (diff[1:] / np.abs(ref[1:])).max())
    assert diff.max() <= 2e-6 * np.abs(ref).max()
    assert np.abs(new_w.numpy().astype(np.float64) - fit.new_weight).max() <= 2e-6 * np.abs(ref).max()


@pytest.mark.parametrize("mutation,rows", [(dict(tie="last"), ("quantised",)),
                                           (dict(fixed_point=False), ("five_iterations", "bits9_limit")),
                                           (dict(abs_tie="larger_first"), ("plus_minus",))],
                         ids=["last_index_wins", "float32_sums", "abs_order_reversed"])
def test_the_checks_notice_a_wrong_restatement(mutation, rows):
    """the three ways the restatement could be subtly wrong and still look plausible - ties to the last index, float32
    segment sums, +c before -c - each fail a float64 check, a row condition or the comparison with the mirror"""
    for name in rows:
        w, _ = row(name)
        bad = R.kmeans_ref(w, R.linspace_guess(w, R.K_OF[name]), **mutation)
        caught = R.row_condition(name, w, bad) is not None
        try:
            R.check_centres_are_means(bad.nonzero, bad.fit_labels, bad.centres, bad.scale)
            R.check_labels_are_nearest(w, bad.labels, bad.centroids[:bad.n_centroids])
        except AssertionError:
            caught = True
        cent, labels, _ = find_centroids(torch.tensor(w), R.K_OF[name] + 1)
        bc = bad.centroids[:bad.n_centroids]
        caught = (caught or cent.numel() != bc.size or not np.array_equal(labels.numpy(), bad.labels)
                  or not np.allclose(cent.numpy(), bc, rtol=2e-6, atol=0))
        assert caught, (mutation, name)


def test_layer_without_a_non_zero_weight():
    """both zeros only: the guess is linspace(inf, -inf), not finite; the restatement and the mirror give one centroid
    +0.0, every label 0 and +0.0 weights (the reference raises: INTEGRATION.md section 4)"""
    w = np.zeros(300, np.float32)
    w[::3] = -0.0
    guess = R.linspace_guess(w, 31)
    assert not np.isfinite(guess[0]) and not np.isfinite(guess[-1])
    fit = R.kmeans_ref(w, guess)
    assert fit.empty and fit.n_centroids == 1 and fit.iterations == 0
    assert not fit.centroids.view(np.int32).any() and not fit.labels.any() and not fit.new_weight.view(np.int32).any()
    assert np.array_equal(fit.centres.view(np.int32), guess.view(np.int32))
    cent, labels, new_w = find_centroids(torch.tensor(w).reshape(10, 30), 32)
    assert cent.tolist() == [0.0] and labels.shape == (10, 30) and labels.dtype == torch.int64 and not labels.any()
    assert new_w.shape == (10, 30) and not new_w.numpy().view(np.int32).any()


# ---- routing ---------------------------------------------------------------------------------------------------------------
class LooksLikeCuda(torch.Tensor):
    """a CPU tensor that answers is_cuda with True: what the routing of KmeansQuant looks at"""
    is_cuda = property(lambda self: True)


class StubEngine:
    """records the calls of find_centroids_native and answers them with the restatement"""

    def __init__(self):
        self.calls = []

    def kmeans_fit(self, weight, guess):
        self.calls.append(guess.numel())
        fit = R.kmeans_ref(weight.numpy().reshape(-1), guess.numpy())
        return (torch.tensor(fit.centroids), torch.tensor([fit.n_centroids], dtype=torch.int32),
                torch.tensor(fit.labels).reshape(weight.shape), torch.tensor(fit.new_weight).reshape(weight.shape))


class Net(nn.Module):
    def __init__(self, cuda):
        super().__init__()
        self.lin = nn.Linear(16, 16)
        if cuda:
            self.lin.weight = nn.Parameter(self.lin.weight.data.as_subclass(LooksLikeCuda))
        self.pre_pass_callbacks, self.post_backward_callbacks, self.bound_engine = [], [], None


ROUTES = [(2, "1", True, True, "native"), (5, "1", True, True, "native"), (9, "1", True, True, "native"),
          (1, "1", True, True, "mirror"), (10, "1", True, True, "mirror"), (5, "0", True, True, "mirror"),
          (5, "1", False, True, "mirror"), (5, "1", True, False, "mirror")]


@pytest.mark.parametrize("bits,knob,cuda,bound,route", ROUTES,
                         ids=[f"bits{b}_knob{k}_{'cuda' if c else 'cpu'}_{'bound' if e else 'unbound'}" for b, k, c, e, _ in ROUTES])
def test_routing_of_kmeans_modify_weights(monkeypatch, bits, knob, cuda, bound, route):
    """the native path for 4 <= 2^bits <= 512 on a CUDA weight with an engine bound; the torch mirror for bits 1 (one
    centre: sf_kmeans_fit refuses K < 2), bits 10, SIREN_FIT_NATIVE_KMEANS=0, a CPU weight, no engine"""
    monkeypatch.setenv("SIREN_FIT_NATIVE_KMEANS", knob)
    torch.manual_seed(0)
    net, eng = Net(cuda), StubEngine()
    assert net.lin.weight.is_cuda == cuda
    net.bound_engine = eng if bound else None
    before = net.lin.weight.detach().clone()
    KmeansQuant(net, None, bits=bits, skip_ll=[]).kmeans_modify_weights()
    assert eng.calls == ([2 ** bits - 1] if route == "native" else [])
    assert (net.lin.n_centroids is not None) == (route == "native")
    n = int(net.lin.n_centroids) if route == "native" else net.lin.centroids.numel()
    assert 1 < n <= 2 ** bits and net.lin.labeled_weight.shape == (16, 16)
    assert torch.equal(net.lin.weight.detach().as_subclass(torch.Tensor), net.lin.centroids[net.lin.labeled_weight])
    assert not torch.equal(net.lin.weight.detach().as_subclass(torch.Tensor), before.as_subclass(torch.Tensor))
