"""The Gaussian classifier without a GPU: the NumPy restatement (tests/gaussian_ref.py) against NumPy's own covariance and solver, the
host part of the fit (`_fit_from_moments`) against it, `scatter_axes`, the host-only workspace size of the C library, and every
rejection the public functions make on the host before a device is needed (all inputs here are CPU tensors: a call that got past its
checks fails on the device test)."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.gaussian import _fit_from_moments, GaussianModel
from gaussian_ref import U, usable_labels, moments_ref, scatter_ref, fit_ref, score_ref, accept, blobs


def _labelled(n=400, width=6, k=5, seed=0):
    """Blobs over classes 0..k-1 with class 1 emptied (absent), class 3 cut to one row (absent too), some labels out of range."""
    z, ids = blobs(n, width, k, seed, sep=4.0, spread=1.0)
    lab = ids.copy()
    lab[lab == 1] = -1
    three = np.flatnonzero(lab == 3)
    lab[three[1:]] = k + 2
    return z, lab


def _moments(z, lab, k):
    counts, means = moments_ref(z, lab, k)
    s, _ = scatter_ref(z, usable_labels(z, lab, k), means.astype(np.float32), k)
    return counts, means.astype(np.float32), s


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_scatter_ref_is_the_covariance():
    z, lab = _labelled()
    counts, means, s = _moments(z, lab, 5)
    assert counts.tolist() == [80, 0, 80, 1, 80]
    for q in (0, 2, 4):
        cov = np.cov(z[lab == q].astype(np.float64), rowvar=False)
        assert np.allclose(s[q] / (counts[q] - 1), cov, rtol=1e-5, atol=1e-7)          # (the means are rounded to fp32)
    assert not s[1].any() and not s[3].any()
    assert np.array_equal(s, s.transpose(0, 2, 1))


def test_scatter_bound_is_what_it_says():
    z = np.array([[1.0, 2.0], [3.0, -4.0], [9.0, 9.0]], dtype=np.float32)
    s, b = scatter_ref(z, np.array([0, 0, 2]), np.zeros((3, 2), dtype=np.float32), 3)
    assert np.array_equal(s[0], [[10.0, -10.0], [-10.0, 20.0]]) and not s[1].any()
    assert np.array_equal(b[0], 4 * U * np.array([[10.0, 14.0], [14.0, 20.0]])) and not b[1].any()
    assert np.array_equal(b[2], 3 * U * 81.0 * np.ones((2, 2)))


def test_mahalanobis_is_the_whitened_norm():
    z, lab = _labelled()
    counts, means, s = _moments(z, lab, 5)
    for cov_kind in ("full", "tied"):
        w, off, logdet = fit_ref(counts, means, s, cov_kind, reg=0.0)
        for q in (0, 2, 4):
            if cov_kind == "full":
                sigma = s[q] / (counts[q] - 1)
            else:
                sigma = (s[0] + s[2] + s[4]) / (240 - 3)
            d = z[:50].astype(np.float64) - means[q]
            want = np.einsum("nl,ln->n", d, np.linalg.solve(sigma, d.T))
            wq = w[q if cov_kind == "full" else 0]
            assert np.allclose(((d @ wq) ** 2).sum(1), want, rtol=1e-9)
            assert np.isclose(logdet[q], np.linalg.slogdet(sigma)[1], rtol=1e-10, atol=1e-10)
        assert np.isinf(off[[1, 3]]).all() and np.isinf(logdet[[1, 3]]).all()


def test_score_ref_ties_absences_and_bad_rows():
    mu = np.array([[0.0], [0.0], [2.0]], dtype=np.float32)
    w = np.ones((1, 1, 1), dtype=np.float32)
    z = np.array([[0.0], [1.0], [3.0], [np.nan], [np.inf]], dtype=np.float32)
    score, d, lab, tau, tau_s = score_ref(z, mu, w, np.array([0.0, 0.0, 0.0], dtype=np.float32))
    assert lab.tolist() == [0, 0, 2, -1, -1]                                           # row 1 ties classes 0, 1 and 2: the lowest
    assert np.array_equal(d[:3], [[0, 0, 4], [1, 1, 1], [9, 9, 1]]) and np.isnan(score[3:]).all()
    assert (tau[:3] >= 0).all() and (tau_s[:3] >= tau[:3]).all()
    score, _, lab, _, _ = score_ref(z, mu, w, np.array([np.inf, 0.0, np.inf], dtype=np.float32))
    assert lab.tolist() == [1, 1, 1, -1, -1] and np.isinf(score[:3, [0, 2]]).all()
    assert (score_ref(z, mu, w, np.full(3, np.inf, dtype=np.float32))[2] == -1).all()
    accept(z, mu, w, np.zeros(3, dtype=np.float32), np.array([0, 0, 2, -1, -1]), np.array([0.0, 1.0, 1.0, np.nan, np.nan]))
    with pytest.raises(AssertionError):
        accept(z, mu, w, np.zeros(3, dtype=np.float32), np.array([0, 0, 0, -1, -1]))


# ---------------------------------------------------------------------------------------------------- _fit_from_moments
PRIORS = ["empirical", "uniform", torch.tensor([0.1, 0.2, 0.3, 0.25, 0.15], dtype=torch.float64)]


@pytest.mark.parametrize("covariance", ["full", "tied"])
@pytest.mark.parametrize("priors", PRIORS, ids=["empirical", "uniform", "tensor"])
@pytest.mark.parametrize("reg", [1e-3, 0.0, 0.2])
def test_fit_from_moments_against_the_reference(covariance, priors, reg):
    z, lab = _labelled()
    counts, means, s = _moments(z, lab, 5)
    m = _fit_from_moments(torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s.astype(np.float32)), covariance, reg, priors)
    assert isinstance(m, GaussianModel) and m.covariance == covariance and m.reg == reg
    w, off, logdet = fit_ref(counts, means, s.astype(np.float32), covariance, reg, priors if isinstance(priors, str) else priors.numpy())
    assert m.whiten.dtype == torch.float32 and tuple(m.whiten.shape) == ((5, 6, 6) if covariance == "full" else (1, 6, 6))
    assert m.offset.dtype == torch.float32 and m.means.dtype == torch.float32 and m.counts.dtype == torch.int64
    assert np.array_equal(m.means.numpy(), means) and np.array_equal(m.counts.numpy(), counts)
    assert np.allclose(m.whiten.numpy(), w, rtol=1e-6, atol=1e-9)                       # (one rounding to fp32)
    absent = np.array([False, True, False, True, False])
    assert np.isinf(m.offset.numpy()[absent]).all() and (m.offset.numpy()[absent] > 0).all()
    assert np.allclose(m.offset.numpy()[~absent], off[~absent], rtol=1e-6, atol=1e-6)
    assert np.allclose(m.logdet.numpy()[~absent], logdet[~absent], rtol=1e-10, atol=1e-10) and np.isinf(m.logdet.numpy()[absent]).all()
    if covariance == "full":
        assert not m.whiten.numpy()[absent].any()
    # the priors are normalised over the present classes: exp(-(offset - logdet) / 2) sums to 1
    pi = np.exp(-(m.offset.numpy()[~absent].astype(np.float64) - logdet[~absent]) / 2)
    assert np.isclose(pi.sum(), 1.0, atol=1e-5)


def test_fit_with_no_present_class():
    m = _fit_from_moments(torch.tensor([1, 0]), torch.zeros((2, 3)), torch.zeros((2, 3, 3)), "tied", 0.1)
    assert np.isinf(m.offset.numpy()).all() and not m.whiten.numpy().any() and tuple(m.whiten.shape) == (1, 3, 3)


def test_cholesky_failure_names_the_class():
    same = np.repeat(np.array([[1.0, 2.0, 3.0]], dtype=np.float32), 4, axis=0)                # identical rows: S = 0
    flat = np.array([[1.0, 2.0, -1.0], [-1.0, -2.0, 1.0], [0.0, 0.0, 0.0]], dtype=np.float32)  # rank 1 in L = 3: Sigma = d d^T, exactly
    rng = np.random.default_rng(0)
    fine = rng.standard_normal((20, 3)).astype(np.float32)
    z = np.concatenate([fine, same, flat])
    lab = np.array([0] * 20 + [1] * 4 + [2] * 3)
    counts, means, s = _moments(z, lab, 3)
    args = [torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s)]
    with pytest.raises(RuntimeError, match="class 1"):
        _fit_from_moments(*args, "full", 0.0)
    args[2][1] = args[2][0]                                                                    # class 1 mended: class 2 is next
    with pytest.raises(RuntimeError, match="class 2"):
        _fit_from_moments(*args, "full", 0.0)
    m = _fit_from_moments(*args, "full", 1e-3)                                                 # shrinkage makes every class definite
    assert np.isfinite(m.offset.numpy()).all()
    with pytest.raises(RuntimeError, match="tied"):
        _fit_from_moments(args[0], args[1], torch.zeros((3, 3, 3)), "tied", 0.0)


# ---------------------------------------------------------------------------------------------------- scatter_axes
def test_scatter_axes_pca_is_the_svd_of_the_centred_rows():
    z, ids = blobs(300, 7, 4, seed=3)
    counts, means, s = _moments(z, ids, 4)
    origin, axes, values = eae_amd.scatter_axes(torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s), kind="pca",
                                                n_components=3)
    assert origin.dtype == torch.float64 and tuple(axes.shape) == (7, 3) and tuple(values.shape) == (3,)
    zc = z.astype(np.float64) - z.astype(np.float64).mean(0)
    _, sv, vt = np.linalg.svd(zc, full_matrices=False)
    assert np.allclose(origin.numpy(), z.astype(np.float64).mean(0), atol=1e-6)
    assert np.allclose(values.numpy(), sv[:3] ** 2, rtol=1e-5)
    for j in range(3):
        assert abs(float(axes.numpy()[:, j] @ vt[j])) > 1 - 1e-6                        # up to sign
    assert np.allclose(axes.numpy().T @ axes.numpy(), np.eye(3), atol=1e-12)


def test_scatter_axes_lda_solves_the_generalised_problem():
    z, ids = blobs(300, 7, 4, seed=4)
    counts, means, s = _moments(z, ids, 4)
    origin, axes, values = eae_amd.scatter_axes(torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s))
    assert tuple(axes.shape) == (7, 2) and values[0] >= values[1] > 0
    sw = s.sum(0)
    dm = means.astype(np.float64) - origin.numpy()
    sb = (counts[:, None, None] * dm[:, :, None] * dm[:, None, :]).sum(0)
    v, lam = axes.numpy(), values.numpy()
    assert np.allclose(sb @ v, (sw @ v) * lam, rtol=1e-8, atol=1e-8 * np.abs(sb).max())
    assert np.allclose(v.T @ sw @ v, np.eye(2), atol=1e-9)
    full = eae_amd.scatter_axes(torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s), "lda", 7)[2].numpy()
    assert (np.abs(full[3:]) < 1e-9 * full[0]).all()                                   # K - 1 = 3 discriminant directions
    # the projected blobs separate: every row is nearest to its own projected class mean
    v3 = eae_amd.scatter_axes(torch.from_numpy(counts), torch.from_numpy(means), torch.from_numpy(s), "lda", 3)[1].numpy()
    pz = (z.astype(np.float64) - origin.numpy()) @ v3
    pm = dm @ v3
    assert np.array_equal(((pz[:, None, :] - pm[None]) ** 2).sum(2).argmin(1), ids)


def test_scatter_axes_rejections():
    c, m, s = torch.tensor([5, 5]), torch.zeros((2, 3)), torch.zeros((2, 3, 3))
    for kw in (dict(kind="ica"), dict(n_components=0), dict(n_components=4), dict(n_components=2.0)):
        with pytest.raises(RuntimeError):
            eae_amd.scatter_axes(c, m, s, **kw)
    for args in ((c.double(), m, s), (c, m, s[:, :2]), (c[:1], m, s), (c, m[0], s), (torch.tensor([0, 0]), m, s)):
        with pytest.raises(RuntimeError):
            eae_amd.scatter_axes(*args)
    with pytest.raises(RuntimeError, match="positive definite"):
        eae_amd.scatter_axes(c, m, s, kind="lda")


# ---------------------------------------------------------------------------------------------------- against scikit-learn
def test_reference_labels_equal_sklearn_qda():
    qda = pytest.importorskip("sklearn.discriminant_analysis").QuadraticDiscriminantAnalysis
    z, ids = blobs(600, 5, 4, seed=8, sep=6.0, spread=1.0)
    counts, means, s = _moments(z, ids, 4)
    w, off, _ = fit_ref(counts, means, s, "full", reg=0.0, priors="empirical")
    rng = np.random.default_rng(1)
    q = blobs(500, 5, 4, seed=8, sep=6.0, spread=1.0)[0] + rng.standard_normal((500, 5)).astype(np.float32) * 0.1
    lab = score_ref(q, means, w.astype(np.float32), off.astype(np.float32))[2]
    sk = qda(store_covariance=False).fit(z.astype(np.float64), ids)
    assert np.array_equal(lab, sk.predict(q.astype(np.float64)))


# ---------------------------------------------------------------------------------------------------- C ABI, host only
def test_workspace_bytes():
    lib = _lib.load()
    for n, width, k in ((1, 1, 1), (1000, 64, 10), (1 << 20, 64, 64), (2 ** 31 - 1, 256, 256), (5, 3, 2), (70001, 64, 10)):
        b = lib.eae_class_scatter_workspace_bytes(n, width, k)
        assert b > 0 and b % 4096 == 0, (n, width, k, b)
    assert lib.eae_class_scatter_workspace_bytes(1 << 20, 64, 64) <= 64 << 20
    assert lib.eae_class_scatter_workspace_bytes(70001, 64, 10) == 10 * 3 * 69 * 4096          # 69 chunks a class
    for n, width, k in ((0, 64, 10), (-5, 64, 10), (2 ** 31, 64, 10), (100, 0, 10), (100, 257, 10), (100, 64, 0), (100, 64, 257)):
        assert lib.eae_class_scatter_workspace_bytes(n, width, k) < 0, (n, width, k)
        assert b"class_scatter" in lib.eae_last_error()


def test_null_and_range_arguments_are_rejected_before_any_launch():
    """EAE_ERR_ARG comes from the host-side checks: no device is touched (this test runs without one)."""
    lib = _lib.load()
    p = 0x1000          # never dereferenced on the host
    need = lib.eae_class_scatter_workspace_bytes(10, 4, 2)
    for n, width, k in ((0, 4, 2), (2 ** 31, 4, 2), (10, 0, 2), (10, 257, 2), (10, 4, 0), (10, 4, 257)):
        assert lib.eae_class_scatter(None, p, n, width, p, p, p, k, p, p, p, 1 << 40) == -2
        assert lib.eae_gauss_score(None, p, n, width, p, p, 0, p, k, p, None, None, None) == -2
    for missing in range(6):
        args = [p] * 6
        args[missing] = None
        assert lib.eae_class_scatter(None, args[0], 10, 4, args[1], args[2], args[3], 2, args[4], args[5], p, need) == -2
        assert b"NULL" in lib.eae_last_error()
    assert lib.eae_class_scatter(None, p, 10, 4, p, p, p, 2, p, p, None, need) == -2
    assert lib.eae_class_scatter(None, p, 10, 4, p, p, p, 2, p, p, p, need - 1) == -2
    assert b"workspace" in lib.eae_last_error()
    for missing in range(5):
        args = [p] * 5
        args[missing] = None
        assert lib.eae_gauss_score(None, args[0], 10, 4, args[1], args[2], 16, args[3], 2, args[4], None, None, None) == -2
        assert b"NULL" in lib.eae_last_error()
    for stride in (1, 4, 15, 17, -16, 32):
        assert lib.eae_gauss_score(None, p, 10, 4, p, p, stride, p, 2, p, None, None, None) == -2
        assert b"w_stride" in lib.eae_last_error()


# ---------------------------------------------------------------------------------------------------- Python rejections
def _z(n=20, width=8):
    return torch.zeros((n, width), dtype=torch.float32)


def _lab(n=20):
    return torch.zeros(n, dtype=torch.int64)


def _model(k=3, width=8, tied=False):
    return GaussianModel(torch.zeros((k, width)), torch.zeros((1 if tied else k, width, width)), torch.zeros(k),
                         torch.zeros(k, dtype=torch.int64), torch.zeros(k, dtype=torch.float64), "tied" if tied else "full", 0.0)


BAD_ROWS = [torch.zeros(8), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 257)), torch.zeros((0, 8)), np.zeros((4, 8))]
BAD_FIT = [
    (dict(num_classes=0), "num_classes"), (dict(num_classes=257), "num_classes"), (dict(num_classes=2.0), "num_classes"),
    (dict(num_classes=True), "num_classes"), (dict(labels=torch.zeros(20)), "integer"), (dict(labels=_lab(19)), "entries"),
    (dict(labels=torch.zeros((20, 1), dtype=torch.int64)), "1-D"), (dict(labels=torch.zeros(20, dtype=torch.bool)), "integer"),
    (dict(labels=[0] * 20), "integer")]
BAD_MODEL = [
    (dict(covariance="diag"), "covariance"), (dict(reg=-0.1), "reg"), (dict(reg=1.5), "reg"), (dict(reg="0.1"), "reg"),
    (dict(reg=True), "reg"), (dict(priors="equal"), "priors"), (dict(priors=torch.ones(2)), "priors"),
    (dict(priors=torch.ones(3, dtype=torch.int64)), "priors"), (dict(priors=torch.tensor([0.5, -0.1, 0.6])), "priors"),
    (dict(priors=torch.zeros(3)), "priors"), (dict(priors=torch.tensor([0.5, float("nan"), 0.5])), "priors")]


@pytest.mark.parametrize("fn", [eae_amd.class_scatter, eae_amd.gaussian_fit])
def test_moment_argument_rejections(fn):
    for bad in BAD_ROWS:
        with pytest.raises(RuntimeError) as e:
            fn(bad, _lab(4), 3)
        assert "HIP device" not in str(e.value) and "z" in str(e.value)
    for kw, word in BAD_FIT:
        args = dict(z=_z(), labels=_lab(), num_classes=3)
        args.update(kw)
        with pytest.raises(RuntimeError) as e:
            fn(**args)
        assert "HIP device" not in str(e.value) and word in str(e.value), kw
    with pytest.raises(RuntimeError, match="HIP device"):               # with everything in order the one thing missing is the device
        fn(_z(), _lab(), 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        fn(_z(), _lab().to(torch.int32), 256)


def test_gaussian_fit_model_rejections():
    for kw, word in BAD_MODEL:
        with pytest.raises(RuntimeError) as e:
            eae_amd.gaussian_fit(_z(), _lab(), 3, **kw)
        assert "HIP device" not in str(e.value) and word in str(e.value), kw
        with pytest.raises(RuntimeError) as e:
            _fit_from_moments(torch.tensor([5, 5, 5]), torch.zeros((3, 8)), torch.zeros((3, 8, 8)), **kw)
        assert word in str(e.value), kw
    for kw in (dict(covariance="tied", reg=0.0, priors="uniform"), dict(priors=torch.tensor([0.2, 0.0, 0.8]), reg=1)):
        with pytest.raises(RuntimeError, match="HIP device"):
            eae_amd.gaussian_fit(_z(), _lab(), 3, **kw)


def test_gaussian_predict_rejections():
    m = _model()
    bad = [(m._replace(means=torch.zeros((3, 7))), "width"), (m._replace(whiten=torch.zeros((2, 8, 8))), "whiten"),
           (m._replace(whiten=torch.zeros((3, 8, 7))), "whiten"), (m._replace(whiten=torch.zeros((3, 8, 8), dtype=torch.float64)), "whiten"),
           (m._replace(offset=torch.zeros(4)), "offset"), (m._replace(offset=torch.zeros(3, dtype=torch.float64)), "offset"),
           (m._replace(means=torch.zeros((257, 8))), "means"), (m._replace(means=torch.zeros((3, 8), dtype=torch.float64)), "means"),
           ((m.means, m.whiten, m.offset), "GaussianModel"), (None, "GaussianModel")]
    for model, word in bad:
        with pytest.raises(RuntimeError) as e:
            eae_amd.gaussian_predict(_z(), model)
        assert "HIP device" not in str(e.value) and word in str(e.value), word
    for z in BAD_ROWS:
        with pytest.raises(RuntimeError) as e:
            eae_amd.gaussian_predict(z, m)
        assert "HIP device" not in str(e.value)
    with pytest.raises(RuntimeError, match="posteriors"):
        eae_amd.gaussian_predict(_z(), m, posteriors=1)
    for model in (m, _model(tied=True)):
        with pytest.raises(RuntimeError, match="HIP device"):
            eae_amd.gaussian_predict(_z(), model, posteriors=True)


def test_gaussian_classify_scene_rejections():
    enc = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3)
    scene = torch.zeros((3, 160, 224), dtype=torch.uint8)
    m = _model(4, 64)
    bad = [dict(model=_model(4, 32)), dict(model=None), dict(reject=-1.0), dict(reject="3"), dict(reject=float("nan")), dict(reject=True),
           dict(stride=65), dict(border="wrap"), dict(rule="some"), dict(max_invalid=1.0), dict(nodata=0.5),
           dict(windows=torch.tensor([0, 1]), nodata=0), dict(windows=torch.zeros(0, dtype=torch.int64)),
           dict(mask=torch.zeros((5, 5), dtype=torch.bool))]
    for kw in bad:
        args = dict(model=m)
        args.update(kw)
        with pytest.raises(RuntimeError) as e:
            eae_amd.gaussian_classify_scene(scene, enc, **args)
        assert "HIP device" not in str(e.value), kw
    with pytest.raises(RuntimeError) as e:
        eae_amd.gaussian_classify_scene(scene, torch.nn.Linear(2, 2), m)
    assert "Encoder" in str(e.value)
    for kw in (dict(), dict(reject=80.0), dict(reject=0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            eae_amd.gaussian_classify_scene(scene, enc, m, **kw)
