"""The Gaussian classifier on the device (eae_amd.gaussian): `eae_class_scatter` / `eae_gauss_score` through the C ABI by shape against
the NumPy float64 restatement (tests/gaussian_ref.py), then `class_scatter`, `gaussian_fit`, `gaussian_predict` and
`gaussian_classify_scene`.

Bounds (derived, not measured; gaussian_ref.scatter_ref / score_ref): a scatter element within (n_k + 2) 2^-24 sum |d_i d_j| of the
float64 sum of the same fp32 differences; a label accepted when its float64 score is within tau_s(n, chosen) + tau_s(n, argmin) of
the row's minimum, maha within tau of the float64 distance, for every row.  Symmetry, ties between equal classes, absences and
everything called "bitwise" are exact.  Every output is poisoned before a call and the workspace is filled with 0xFF."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from gaussian_ref import U, usable_labels, moments_ref, scatter_ref, fit_ref, score_ref, accept, blobs
from scene_util import _model, _scene, _divisor

pytestmark = pytest.mark.gpu

#          (N, L, K)
SHAPES = [(1, 1, 1), (63, 3, 2), (64, 4, 10), (65, 48, 17), (257, 33, 256), (130, 256, 3), (1031, 256, 40),
          (70001, 64, 10)]             # 547 row tiles for 512 workgroups: more than one grid round; 69 scatter chunks a class
POISON = -7


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    """Bitwise equality of tuples of arrays (NaN equals itself); None matches None."""
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------- the two C calls
def _c_scatter(z, labels, means, k, ws_bytes=None, ws_null=False, null=None):
    """One scatter call on a poisoned output and a 0xFF workspace, the rows grouped by a stable sort: (rc, scatter as NumPy)."""
    n, width = z.shape
    lib = _lib.load()
    need = lib.eae_class_scatter_workspace_bytes(n, width, k)
    assert need > 0
    key = np.where((labels >= 0) & (labels < k), labels, k).astype(np.int64)
    order = np.argsort(key, kind="stable").astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=k + 1)[:k])]).astype(np.int64)
    t = dict(z=torch.from_numpy(z).cuda(), labels=torch.from_numpy(labels.astype(np.int64)).cuda(), order=torch.from_numpy(order).cuda(),
             seg=torch.from_numpy(seg).cuda(), means=torch.from_numpy(means).cuda(),
             scatter=torch.full((k, width, width), float(POISON), dtype=torch.float32, device="cuda"))
    p = {name: None if name == null else _ptr(v) for name, v in t.items()}
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device="cuda")          # NaN bit patterns: every partial read must have been written
    rc = lib.eae_class_scatter(_stream(), p["z"], n, width, p["labels"], p["order"], p["seg"], k, p["means"], p["scatter"],
                               None if ws_null else _ptr(ws), nb)
    return rc, t["scatter"].cpu().numpy()


def _c_score(z, mu, w, off, stride=None, outputs=("maha", "best", "scores")):
    """One score call on poisoned outputs: (labels, maha, best, scores) as NumPy, None for an output that was not asked for."""
    n, width = z.shape
    k = mu.shape[0]
    zt, mt, wt, ot = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (z, mu, w, off))
    lab = torch.full((n,), POISON, dtype=torch.int64, device="cuda")
    out = {"maha": torch.full((n,), float(POISON), dtype=torch.float32, device="cuda") if "maha" in outputs else None,
           "best": torch.full((n,), float(POISON), dtype=torch.float32, device="cuda") if "best" in outputs else None,
           "scores": torch.full((n, k), float(POISON), dtype=torch.float32, device="cuda") if "scores" in outputs else None}
    if stride is None:
        stride = width * width if w.shape[0] == k else 0
    _lib.check(_lib.load().eae_gauss_score(_stream(), _ptr(zt), n, width, _ptr(mt), _ptr(wt), stride, _ptr(ot), k, _ptr(lab),
                                           _ptr(out["maha"]), _ptr(out["best"]), _ptr(out["scores"])))
    return (lab.cpu().numpy(),) + tuple(None if out[name] is None else out[name].cpu().numpy() for name in ("maha", "best", "scores"))


def _model_for(n, width, k, seed):
    """Rows, and a model with a matrix of its own for every class: (z, mu, W [K, L, L], offset), fp32."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n, width)).astype(np.float32)
    mu = rng.standard_normal((k, width)).astype(np.float32)
    w = (rng.standard_normal((k, width, width)) / np.sqrt(width)).astype(np.float32)
    off = rng.standard_normal(k).astype(np.float32) * 3
    return z, mu, w, off


def _check_scores(ref, labels, best, scores):
    """scores within tau_s of the float64 scores (+inf where they are +inf, NaN rows where they are NaN); best is the chosen one."""
    score64, _, _, _, tau_s = ref
    fin = np.isfinite(score64)
    assert np.array_equal(np.isnan(scores), np.isnan(score64)) and np.array_equal(np.isposinf(scores), np.isposinf(score64))
    assert (np.abs(scores[fin].astype(np.float64) - score64[fin]) <= tau_s[fin]).all()
    rows = np.flatnonzero(labels >= 0)
    assert np.array_equal(_bits(best[rows]), _bits(scores[rows, labels[rows]]))
    assert (scores[rows].min(axis=1) == best[rows]).all()


# ---------------------------------------------------------------------------------------------------- 1. scatter
def _labels_for(n, k, seed):
    """Random labels in [-1, K] (both ends out of range) and, for K > 1, at least one empty class."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, k + 1, n).astype(np.int64)
    if k > 1:
        lab[lab == k // 2] = -1
    if n > 4:
        lab[1], lab[n // 2] = k + 5, -3
    return lab


@pytest.mark.parametrize("n,width,k", SHAPES)
def test_scatter_by_shape(n, width, k):
    rng = np.random.default_rng(3 * n + k)
    z = (rng.standard_normal((n, width)) + rng.standard_normal(width) * 2).astype(np.float32)
    lab = _labels_for(n, k, seed=n)
    counts, means64 = moments_ref(z, lab, k)
    means = means64.astype(np.float32)
    ref, bound = scatter_ref(z, usable_labels(z, lab, k), means, k)
    rc, got = _c_scatter(z, lab, means, k)
    assert rc == 0
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()                   # every element: nothing keeps its poison
    assert np.array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))               # bitwise symmetric
    empty = counts == 0
    if k > 1:
        assert empty[k // 2]
    assert not _bits(got[empty]).any()                                             # exactly +0
    rc2, got2 = _c_scatter(z, lab, means, k)
    assert rc2 == 0 and np.array_equal(_bits(got2), _bits(got))


def test_scatter_rejects_null_pointers_and_a_short_or_missing_workspace():
    rng = np.random.default_rng(1)
    z = rng.standard_normal((300, 40)).astype(np.float32)
    lab = _labels_for(300, 10, seed=2)
    means = moments_ref(z, lab, 10)[1].astype(np.float32)
    need = _lib.load().eae_class_scatter_workspace_bytes(300, 40, 10)
    cases = [dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_null=True)] + [dict(null=name) for name in ("z", "labels", "order", "seg",
                                                                                                         "means", "scatter")]
    for kw in cases:
        rc, got = _c_scatter(z, lab, means, 10, **kw)
        assert rc == -2 and (b"workspace" if "null" not in kw else b"NULL") in _lib.load().eae_last_error()
        assert (got == POISON).all()                                               # nothing was launched


@pytest.mark.parametrize("n,width,k", [(500, 20, 6), (3000, 64, 10)])
def test_class_scatter(n, width, k):
    """The Python call: counts and means as the reference has them, the scatter about the means it returns; rows with a NaN or an Inf
    are unlabelled."""
    rng = np.random.default_rng(n)
    z = (rng.standard_normal((n, width)) * 0.5 + 1.0).astype(np.float32)
    lab = _labels_for(n, k, seed=k)
    z[7, 0], z[n - 1, width - 1], z[100, 3] = np.nan, np.inf, -np.inf
    lab[7], lab[n - 1], lab[100] = 0, 1, k - 1
    zt, lt = torch.from_numpy(z).cuda(), torch.from_numpy(lab).cuda()
    counts, means, scatter = eae_amd.class_scatter(zt, lt, k)
    assert counts.dtype == torch.int64 and means.dtype == torch.float32 and scatter.dtype == torch.float32
    ref_counts, ref_means = moments_ref(z, lab, k)
    assert np.array_equal(counts.cpu().numpy(), ref_counts)
    m = means.cpu().numpy()
    use = usable_labels(z, lab, k)
    for q in range(k):                                                             # (n_k + 1) 2^-24 sum |z| / n_k: kmeans_ref.update_bound
        rows = use == q
        if rows.any():
            assert (np.abs(m[q] - ref_means[q]) <= (rows.sum() + 1) * U * np.abs(z[rows]).astype(np.float64).sum(0) / rows.sum()).all()
        else:
            assert not m[q].any()
    ref, bound = scatter_ref(z, use, m, k)
    got = scatter.cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(got.astype(np.float64) - ref) <= bound).all()
    assert np.array_equal(_bits(got), _bits(got.transpose(0, 2, 1)))
    again = eae_amd.class_scatter(zt, lt.to(torch.int32), k)
    assert _same([t.cpu().numpy() for t in again], [counts.cpu().numpy(), m, got])


# ---------------------------------------------------------------------------------------------------- 2. score
@pytest.mark.parametrize("n,width,k", SHAPES)
def test_score_by_shape(n, width, k):
    z, mu, w, off = _model_for(n, width, k, seed=n + width + k)
    full = _c_score(z, mu, w, off)
    labels, maha, best, scores = full
    ref = accept(z, mu, w, off, labels, maha)
    _check_scores(ref, labels, best, scores)
    assert _same(_c_score(z, mu, w, off), full)                                    # two runs
    only = _c_score(z, mu, w, off, outputs=())
    assert only[1:] == (None, None, None) and np.array_equal(only[0], labels)      # labels alone
    # one shared matrix: stride 0 equals stride L * L with that matrix replicated
    shared = _c_score(z, mu, w[:1], off, stride=0)
    accept(z, mu, w[:1], off, shared[0], shared[1])
    assert _same(_c_score(z, mu, np.repeat(w[:1], k, axis=0), off, stride=width * width), shared)
    # a row's outputs are its own: a slice gives the slice (another grid, another place in the tile)
    for lo, hi in {(0, 1), (n // 2, n // 2 + 1), (n // 3, n // 3 + min(n - n // 3, 200)), (n - 1, n)}:
        part = _c_score(z[lo:hi].copy(), mu, w, off)
        assert _same(part, [a[lo:hi] for a in full]), (lo, hi)


# ---------------------------------------------------------------------------------------------------- 3. ties and absences
@pytest.mark.parametrize("n,width,k", [(65, 48, 17), (300, 64, 70), (257, 33, 256), (40, 5, 3)])
def test_duplicated_classes_lower_index_wins(n, width, k):
    z, mu, w, off = _model_for(n, width, k, seed=7 * n)
    dup = np.random.default_rng(k).permutation(k)
    src, dst = dup[:k - k // 2], dup[k // 2:]                                      # every class of the second half copies one of the first
    mu[dst], w[dst], off[dst] = mu[src], w[src], off[src]
    labels, maha, best, scores = _c_score(z, mu, w, off)
    accept(z, mu, w, off, labels, maha)
    same = [np.flatnonzero((mu == mu[q]).all(1) & (w == w[q]).all((1, 2)) & (off == off[q]))[0] for q in range(k)]
    assert len(set(same)) < k
    assert np.array_equal(np.array(same)[labels], labels)                          # the label is the lowest index among its equals
    assert np.array_equal(_bits(scores), _bits(scores[:, same]))                   # equal classes give equal scores
    mu[:], w[:], off[:] = mu[0], w[0], off[0]                                      # all classes equal: every row goes to 0
    assert (_c_score(z, mu, w, off)[0] == 0).all()


@pytest.mark.parametrize("n,width,k", [(200, 64, 10), (131, 67, 40), (64, 1, 2)])
def test_absent_classes(n, width, k):
    z, mu, w, off = _model_for(n, width, k, seed=n)
    present, _, _, pscores = _c_score(z, mu, w, off)
    gone = np.unique(np.concatenate([np.bincount(present, minlength=k).argsort()[-max(1, k // 3):], [0]]))    # the most chosen ones, and 0
    if len(gone) == k:
        gone = gone[1:]
    off[gone] = np.inf
    labels, maha, best, scores = _c_score(z, mu, w, off)
    ref = accept(z, mu, w, off, labels, maha)
    _check_scores(ref, labels, best, scores)
    assert not np.isin(labels, gone).any() and np.isposinf(scores[:, gone]).all()
    keep = np.setdiff1d(np.arange(k), gone)
    assert np.array_equal(_bits(scores[:, keep]), _bits(pscores[:, keep]))         # the other classes' scores are undisturbed
    off[:] = np.inf                                                                # nothing left to choose
    labels, maha, best, scores = _c_score(z, mu, w, off)
    assert (labels == -1).all() and np.isnan(maha).all() and np.isposinf(best).all() and np.isposinf(scores).all()


@pytest.mark.parametrize("n,width,k", [(200, 64, 10), (131, 67, 40), (64, 1, 2)])
def test_non_finite_rows(n, width, k):
    z, mu, w, off = _model_for(n, width, k, seed=n)
    clean = _c_score(z, mu, w, off)
    bad = {3: (0, np.nan), 17: (width // 2, np.inf), 31: (width - 1, -np.inf), 32: (width - 1, np.nan), n - 1: (0, np.inf)}
    for row, (col, v) in bad.items():
        z[row, col] = v
    got = _c_score(z, mu, w, off)
    labels, maha, best, scores = got
    rows = np.array(sorted(bad))
    assert (labels[rows] == -1).all() and np.isnan(maha[rows]).all() and np.isnan(best[rows]).all() and np.isnan(scores[rows]).all()
    keep = np.ones(n, dtype=bool)
    keep[rows] = False
    assert _same([a[keep] for a in got], [a[keep] for a in clean])                 # neighbours undisturbed, bit for bit
    accept(z, mu, w, off, labels, maha)
    assert np.array_equal(_c_score(z, mu, w, off, outputs=())[0], labels)


# ---------------------------------------------------------------------------------------------------- 4. end to end
E2E = [(600, 16, 4), (2000, 64, 10)]


def _reference_fit(z, ids, k, covariance, reg):
    """The float64 pipeline: moments, scatter about the float64 means, fit; the model as fp32 tensors hold it."""
    counts, means = moments_ref(z, ids, k)
    s = np.zeros((k, z.shape[1], z.shape[1]))
    for q in range(k):
        d = z[ids == q].astype(np.float64) - means[q]
        s[q] = d.T @ d
    w, off, _ = fit_ref(counts, means, s, covariance, reg)
    return means.astype(np.float32), w.astype(np.float32), off.astype(np.float32)


@pytest.mark.parametrize("covariance", ["full", "tied"])
@pytest.mark.parametrize("n,width,k", E2E)
def test_fit_predict_end_to_end(n, width, k, covariance):
    """Blobs of separation 4 and unit spread: in the float64 reference alone at most 1 % of the rows have a margin under 2 tau (checked
    on the CPU when this was written: none has), and on the rest fp32 rounding cannot move a label."""
    z, ids = blobs(2 * n, width, k, seed=n + width, sep=4.0, spread=1.0)
    train, query = z[:n], z[n:]
    mu, w, off = _reference_fit(train, ids[:n], k, covariance, 1e-3)
    score64, _, lab_ref, tau, tau_s = score_ref(query, mu, w, off)
    srt = np.sort(score64, axis=1)
    sure = (srt[:, 1] - srt[:, 0]) > 2 * tau_s.max(axis=1) if k > 1 else np.ones(n, dtype=bool)
    assert (~sure).mean() <= 0.01
    zt = torch.from_numpy(train).cuda()
    model = eae_amd.gaussian_fit(zt, torch.from_numpy(ids[:n]).cuda(), k, covariance=covariance, reg=1e-3)
    assert isinstance(model, eae_amd.GaussianModel) and model.covariance == covariance
    assert tuple(model.whiten.shape) == ((k if covariance == "full" else 1), width, width) and model.whiten.is_cuda
    assert np.array_equal(model.counts.cpu().numpy(), np.bincount(ids[:n], minlength=k))
    qt = torch.from_numpy(query).cuda()
    labels, maha, logp = eae_amd.gaussian_predict(qt, model, posteriors=True)
    lab = labels.cpu().numpy()
    assert np.array_equal(lab[sure], lab_ref[sure])
    accept(query, model.means.cpu().numpy(), model.whiten.cpu().numpy(), model.offset.cpu().numpy(), lab, maha.cpu().numpy())
    assert (lab == ids[n:]).mean() > 0.99                                          # and the blobs are recovered
    p = logp.double().exp()
    assert tuple(logp.shape) == (n, k) and torch.allclose(p.sum(1), torch.ones(n, dtype=torch.float64, device="cuda"), atol=1e-5)
    assert torch.equal(logp.argmax(dim=1), labels)
    two = eae_amd.gaussian_predict(qt, model)
    assert len(two) == 2 and torch.equal(two[0], labels) and torch.equal(two[1], maha)
    again = eae_amd.gaussian_fit(zt, torch.from_numpy(ids[:n]).cuda(), k, covariance=covariance, reg=1e-3)
    assert all(torch.equal(a, b) for a, b in zip(again[:5], model[:5]))            # no seed, no atomics: the same model bit for bit


def test_fit_with_an_absent_class_and_given_priors():
    z, ids = blobs(800, 16, 5, seed=5, sep=4.0, spread=1.0)
    lab = ids.copy()
    lab[lab == 2] = -1                                                             # class 2 has no rows, class 4 one row
    lab[np.flatnonzero(lab == 4)[1:]] = 7
    zt = torch.from_numpy(z).cuda()
    pri = torch.tensor([0.5, 0.3, 9.0, 0.2, 9.0], device="cuda")
    model = eae_amd.gaussian_fit(zt, torch.from_numpy(lab).cuda(), 5, priors=pri)
    off = model.offset.cpu().numpy()
    assert np.isposinf(off[[2, 4]]).all() and np.isfinite(off[[0, 1, 3]]).all() and model.counts.tolist() == [160, 160, 0, 160, 1]
    got, maha = eae_amd.gaussian_predict(zt, model)
    got = got.cpu().numpy()
    assert not np.isin(got, [2, 4]).any() and (got[np.isin(ids, [0, 1, 3])] == ids[np.isin(ids, [0, 1, 3])]).all()
    accept(z, model.means.cpu().numpy(), model.whiten.cpu().numpy(), off, got, maha.cpu().numpy())
    flat = z.copy()
    flat[ids == 1] = 1.0                                                           # identical rows (sums of ones are exact): S_1 = 0
    with pytest.raises(RuntimeError, match="class 1"):                             # and no shrinkage
        eae_amd.gaussian_fit(torch.from_numpy(flat).cuda(), torch.from_numpy(ids).cuda(), 5, reg=0.0)


# ---------------------------------------------------------------------------------------------------- 5. scenes
@pytest.fixture(scope="module")
def scene_case():
    m = _model(3, seed=5, latent=64, batch=16)
    scene = _scene(3, 160, 224, torch.uint8, seed=21)
    div = _divisor(3, torch.uint8)
    z = eae_amd.encode_scene(scene, m, divisor=div, stride=32)
    lab = torch.arange(z.shape[0], device="cuda") % 3
    return m, scene, div, eae_amd.gaussian_fit(z, lab, 3, covariance="tied", reg=0.1)


def _maps_equal(label_map, maha_map, labels, maha):
    return (torch.equal(label_map.reshape(-1), labels)
            and torch.equal(maha_map.reshape(-1).view(torch.int32), maha.view(torch.int32)))


def test_classify_scene_plain_and_windows(scene_case):
    m, scene, div, model = scene_case
    labels, maha = eae_amd.gaussian_predict(eae_amd.encode_scene(scene, m, divisor=div, stride=32), model)
    lmap, dmap = eae_amd.gaussian_classify_scene(scene, m, model, divisor=div, stride=32)
    assert lmap.shape == (4, 6) and lmap.dtype == torch.int64 and dmap.shape == (4, 6) and dmap.dtype == torch.float32
    assert _maps_equal(lmap, dmap, labels, maha) and int(lmap.min()) >= 0
    # reject: exactly the windows above the threshold turn to -1, the distances stay
    t = float(maha.median())
    assert 0 < int((maha > t).sum()) < 24
    rmap, rdmap = eae_amd.gaussian_classify_scene(scene, m, model, reject=t, divisor=div, stride=32)
    assert torch.equal(rmap.reshape(-1), torch.where(maha > t, -1, labels)) and torch.equal(rdmap, dmap)
    # windows=
    ids = torch.tensor([20, 3, 7, 11, 12, 0, 23], device="cuda")
    lw, mw = eae_amd.gaussian_predict(eae_amd.encode_scene(scene, m, divisor=div, stride=32, windows=ids), model)
    lmapw, dmapw = eae_amd.gaussian_classify_scene(scene, m, model, divisor=div, stride=32, windows=ids)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    assert _maps_equal(lmapw.reshape(-1)[ids], dmapw.reshape(-1)[ids], lw, mw)
    assert (lmapw.reshape(-1)[rest] == -1).all() and torch.isnan(dmapw.reshape(-1)[rest]).all()


def test_classify_scene_nodata(scene_case):
    m, scene, div, model = scene_case
    holed = scene.clone()
    holed[:, :, 100:110] = 0                                               # a stripe of nodata through window columns 2 and 3 (stride 32)
    ids = eae_amd.valid_windows(holed, 64, 32, nodata=0)
    assert 0 < ids.numel() < 24
    lw, mw = eae_amd.gaussian_predict(eae_amd.encode_scene(holed, m, divisor=div, stride=32, windows=ids), model)
    lmap, dmap = eae_amd.gaussian_classify_scene(holed, m, model, divisor=div, stride=32, nodata=0)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    assert _maps_equal(lmap.reshape(-1)[ids], dmap.reshape(-1)[ids], lw, mw)
    assert (lmap.reshape(-1)[rest] == -1).all() and torch.isnan(dmap.reshape(-1)[rest]).all() and (lmap.reshape(-1)[ids] >= 0).all()
