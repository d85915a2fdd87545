"""Nearest-neighbour search on the device (eae_amd.neighbors): `eae_knn_search` through the C ABI by shape against the NumPy float64
restatement (tests/knn_ref.py), its exact properties (ties, self exclusion, non-finite rows, independence of the batch and of the
bank split, repeatability), then `knn_search`, `knn_classify`, `similar_windows` and `knn_classify_scene`.

Bound (derived, not measured; knn_ref.accept): with d64 the float64 distances and tau_n = kmeans_ref.tau(q, bank)[n], slot j of row
n is accepted when |d64[n, idx[n, j]] - sort(d64[n])[j]| <= tau_n -- each fp32 score is within tau / 2 of the truth and order
statistics are 1-Lipschitz in the sup norm -- and dist when it is within tau_n of d64.  Every row is checked.  Everything called
"bitwise", the order of equal scores and the -1 / NaN slots are exact.  Outputs are poisoned before each call."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from kmeans_ref import blobs
from knn_ref import SHAPES, BOUNDARY_SHAPES, knn_ref, accept, bound
from scene_util import _model, _scene, _divisor

pytestmark = pytest.mark.gpu

POISON = -7


def _data(nq, m, width, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, width)).astype(np.float32), rng.standard_normal((m, width)).astype(np.float32)


def _dev(a, offset=False):
    """a on the device: a fresh allocation (16-byte aligned), or the same rows as a view that starts 4 bytes into one"""
    if not offset:
        return torch.from_numpy(a).cuda()
    t = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


def _c_search(q, bank, k, self_offset=-1, want_dist=True, ws_bytes=None, ws_null=False, q_offset=False, bank_offset=False):
    """One search call on poisoned outputs and a workspace of NaN bit patterns: (rc, idx, dist) as NumPy."""
    nq, width = q.shape
    m = bank.shape[0]
    lib = _lib.load()
    need = lib.eae_knn_workspace_bytes(nq, m, width, k)
    assert need >= 0
    qt, bt = _dev(q, q_offset), _dev(bank, bank_offset)
    idx = torch.full((nq, k), POISON, dtype=torch.int64, device="cuda")
    dist = torch.full((nq, k), float(POISON), dtype=torch.float32, device="cuda") if want_dist else None
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.eae_knn_search(_stream(), _ptr(qt), nq, _ptr(bt), m, width, k, self_offset, _ptr(idx), _ptr(dist), None if ws_null else _ptr(ws), nb)
    return rc, idx.cpu().numpy(), None if dist is None else dist.cpu().numpy()


def _search(q, bank, k, **kw):
    rc, idx, dist = _c_search(q, bank, k, **kw)
    assert rc == 0, _lib.load().eae_last_error()
    return idx, dist


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


# ---------------------------------------------------------------------------------------------------- 1. by shape
@pytest.mark.parametrize("nq,m,width,k", SHAPES + BOUNDARY_SHAPES)
def test_search_by_shape(nq, m, width, k):
    q, bank = _data(nq, m, width, seed=nq + m + width + k)
    idx, dist = _search(q, bank, k)
    accept(q, bank, k, idx, dist)
    if m < k:
        assert (idx[:, m:] == -1).all() and np.isnan(dist[:, m:]).all() and (idx[:, :m] >= 0).all()
    # two runs are bitwise equal; dist = NULL leaves idx unchanged
    assert _same(_search(q, bank, k), (idx, dist))
    only, none = _search(q, bank, k, want_dist=False)
    assert none is None and np.array_equal(only, idx)


def test_the_shapes_cover_both_plans():
    lib = _lib.load()
    s = [lib.eae_knn_slices(*shape) for shape in SHAPES]
    assert min(s) == 1 and max(s) > 1 and lib.eae_knn_slices(33, 70001, 64, 10) > 1


@pytest.mark.parametrize("nq,m,width,k,slices", [(130, 600, 68, 5, 3), (40, 200, 8, 3, 1)])
def test_the_result_does_not_depend_on_the_alignment_of_the_rows(nq, m, width, k, slices):
    """Rows of a width that is a multiple of 4 are staged with 16-byte loads from a 16-byte aligned base and float by float from any
    other, queries and bank each for itself: the four combinations give the same bits (staging changes no arithmetic).  The first
    shape has two query tiles (the second of 2 rows), ten bank tiles (the last of 24 rows) in three slices and two column passes
    (the second 4 wide); the second one pass, one slice and queries that are staged once."""
    lib = _lib.load()
    assert lib.eae_knn_slices(nq, m, width, k) == slices and (lib.eae_knn_workspace_bytes(nq, m, width, k) > 0) == (slices > 1)
    q, bank = _data(nq, m, width, seed=nq + m + width + k)
    aligned = _search(q, bank, k)
    accept(q, bank, k, *aligned)
    for q_offset, bank_offset in ((False, True), (True, False), (True, True)):
        assert _same(_search(q, bank, k, q_offset=q_offset, bank_offset=bank_offset), aligned), (q_offset, bank_offset)


# ---------------------------------------------------------------------------------------------------- 2. exact order of equal scores
@pytest.mark.parametrize("nq,m,width,k", [(65, 200, 48, 32), (40, 1000, 5, 7), (3, 6000, 64, 10), (130, 70, 130, 9)])
def test_duplicated_bank_rows_ascend_and_are_adjacent(nq, m, width, k):
    q, bank = _data(nq, m, width, seed=3 * m)
    perm = np.random.default_rng(m).permutation(m)
    bank[perm[m // 2:]] = bank[perm[:m - m // 2]]              # every row of the second half copies one of the first: pairs of twins
    idx, dist = _search(q, bank, k)
    accept(q, bank, k, idx, dist)
    twin = np.empty(m, dtype=np.int64)
    twin[perm[m // 2:]] = perm[:m - m // 2]
    twin[perm[:m - m // 2]] = perm[m // 2:]
    for n in range(nq):
        row = idx[n].tolist()
        for j, r in enumerate(row):
            t = int(twin[r])
            if not (bank[t] == bank[r]).all():
                continue                                       # (m odd: one row has no twin)
            lo, hi = min(r, t), max(r, t)
            if r == lo and j + 1 < k:
                assert row[j + 1] == hi, (n, j, row)           # the twins take adjacent slots, the lower index first
            if r == hi:
                assert j > 0 and row[j - 1] == lo, (n, j, row)
            if lo in row and hi in row:
                assert np.array_equal(_bits(dist[n, row.index(lo)]), _bits(dist[n, row.index(hi)]))
    # all bank rows equal: 0 .. k-1
    bank[:] = bank[0]
    idx, _ = _search(q, bank, k)
    assert (idx == np.arange(k)[None, :]).all()


# ---------------------------------------------------------------------------------------------------- 3. self_offset
@pytest.mark.parametrize("n,width,k", [(300, 16, 5), (129, 64, 31), (2000, 3, 8)])
def test_leave_one_out_equals_the_longer_search_without_self(n, width, k):
    z, _ = _data(n, 1, width, seed=n)
    z[7] = z[2]                                                # a twin pair: for row 7 the own entry is not the unique zero
    idx, dist = _search(z, z, k, self_offset=0)
    accept(z, z, k, idx, dist, self_offset=0)
    assert (idx != np.arange(n)[:, None]).all()
    full, fdist = _search(z, z, k + 1)
    for r in range(n):
        row = full[r].tolist()
        if row.count(r) == 1 and r not in (2, 7):
            j = row.index(r)
            assert np.array_equal(idx[r], np.delete(full[r], j)) and np.array_equal(_bits(dist[r]), _bits(np.delete(fdist[r], j)))
    assert idx[7, 0] == 2 and idx[2, 0] == 7


def test_self_offset_of_a_bank_slice():
    _, bank = _data(1, 900, 24, seed=5)
    for off, nq in ((0, 10), (130, 300), (899, 1), (600, 300)):
        q = bank[off:off + nq].copy()
        idx, dist = _search(q, bank, 6, self_offset=off)
        accept(q, bank, 6, idx, dist, self_offset=off)
        assert (idx != (np.arange(len(q)) + off)[:, None]).all()
    q = bank[850:900].copy()
    idx, dist = _search(np.concatenate([q, q]), bank, 6, self_offset=850)          # rows 50.. point past the bank: nothing is excluded
    assert (idx[:50] != (np.arange(50) + 850)[:, None]).all() and (idx[50:, 0] == np.arange(50) + 850).all()


# ---------------------------------------------------------------------------------------------------- 4. non-finite rows
@pytest.mark.parametrize("nq,m,width,k", [(200, 3000, 64, 10), (131, 6000, 67, 5), (64, 400, 1, 3)])
def test_non_finite_rows(nq, m, width, k):
    q, bank = _data(nq, m, width, seed=nq + m)
    clean = _search(q, bank, k)
    ridx, _, d = knn_ref(q, bank, min(k + 3, m))
    # poison bank rows that the reference puts nowhere near any query's k + 3 nearest, so that no clean row loses a neighbour
    far = np.setdiff1d(np.arange(m), np.unique(ridx))
    assert len(far) >= 4
    brows = far[[0, 1, len(far) // 2, -1]]
    bank2 = bank.copy()
    for r, (col, v) in zip(brows, ((0, np.nan), (width // 2, np.inf), (width - 1, -np.inf), (width - 1, np.nan))):
        bank2[r, col] = v
    qbad = {3: (0, np.nan), 17: (width // 2, np.inf), 31: (width - 1, -np.inf), 32: (width - 1, np.nan), nq - 1: (0, np.inf)}
    q2 = q.copy()
    for r, (col, v) in qbad.items():
        q2[r, col] = v
    idx, dist = _search(q2, bank2, k)
    rows = np.array(sorted(qbad))
    assert (idx[rows] == -1).all() and np.isnan(dist[rows]).all()
    assert not np.isin(idx, brows).any()
    keep = np.ones(nq, dtype=bool)
    keep[rows] = False
    assert np.array_equal(idx[keep], clean[0][keep]) and np.array_equal(_bits(dist[keep]), _bits(clean[1][keep]))      # bit for bit
    accept(q2, bank2, k, idx, dist)
    # a bank of nothing but non-finite rows: every slot is empty
    bank3 = np.full((5, width), np.nan, dtype=np.float32)
    idx, dist = _search(q, bank3, k)
    assert (idx == -1).all() and np.isnan(dist).all()


# ---------------------------------------------------------------------------------------------------- 5. independence
def test_a_row_does_not_depend_on_its_batch_or_on_the_bank_split():
    """A query's results are bitwise the same alone, in a long batch and under plans that cut the bank differently (the same query
    under another Nq)."""
    lib = _lib.load()
    q, bank = _data(40000, 5000, 64, seed=11)
    k = 10
    plans = {nq: lib.eae_knn_slices(nq, 5000, 64, k) for nq in (1, 8000, 40000)}
    assert plans[40000] == 1 and len(set(plans.values())) == 3, plans
    whole = _search(q, bank, k)
    accept(q[:300], bank, k, whole[0][:300], whole[1][:300])
    part = _search(q[:8000].copy(), bank, k)
    assert _same(part, (whole[0][:8000], whole[1][:8000]))
    for lo, hi in ((0, 1), (7999, 8000), (129, 400), (39999, 40000)):
        assert _same(_search(q[lo:hi].copy(), bank, k), (whole[0][lo:hi], whole[1][lo:hi]))
    # and with L > 64 (the queries are staged once per pass) and k = 32
    q, bank = _data(700, 3000, 200, seed=12)
    whole = _search(q, bank, 32)
    for lo, hi in ((0, 1), (128, 257), (699, 700)):
        assert _same(_search(q[lo:hi].copy(), bank, 32), (whole[0][lo:hi], whole[1][lo:hi]))


def test_a_short_or_missing_workspace_is_rejected_and_nothing_is_written():
    q, bank = _data(33, 70001, 64, seed=1)
    need = _lib.load().eae_knn_workspace_bytes(33, 70001, 64, 10)
    assert need > 0
    for kw in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_null=True)):
        rc, idx, dist = _c_search(q, bank, 10, **kw)
        assert rc == -2 and b"workspace" in _lib.load().eae_last_error()
        assert (idx == POISON).all() and (dist == POISON).all()
    # no workspace is needed where the bank is not cut
    assert _lib.load().eae_knn_workspace_bytes(40000, 50, 8, 3) == 0
    q, bank = _data(40000, 50, 8, seed=2)
    rc, idx, dist = _c_search(q, bank, 3, ws_null=True)
    assert rc == 0
    accept(q, bank, 3, idx, dist)


# ---------------------------------------------------------------------------------------------------- 6. knn_search / knn_classify
def test_knn_search_metrics_and_exclude_self():
    q, bank = _data(300, 700, 32, seed=21)
    bank[5] = 0.0
    q[9] = 0.0
    qt, bt = torch.from_numpy(q).cuda(), torch.from_numpy(bank).cuda()
    res = eae_amd.knn_search(qt, bt, 7)
    assert isinstance(res, eae_amd.KNNResult) and res.idx.dtype == torch.int64 and res.dist.dtype == torch.float32
    assert _same((res.idx.cpu().numpy(), res.dist.cpu().numpy()), _search(q, bank, 7))
    cos = eae_amd.knn_search(qt, bt, 7, metric="cosine")
    assert torch.equal(qt, torch.from_numpy(q).cuda()) and torch.equal(bt, torch.from_numpy(bank).cuda())      # scaled out of place
    ci, cd = cos.idx.cpu().numpy(), cos.dist.cpu().numpy()
    assert (ci[9] == -1).all() and np.isnan(cd[9]).all() and not (ci == 5).any()       # a zero row has no direction
    with np.errstate(invalid="ignore"):
        qu = (qt / qt.norm(dim=1, keepdim=True)).cpu().numpy()
        bu = (bt / bt.norm(dim=1, keepdim=True)).cpu().numpy()
    accept(qu, bu, 7, ci, (cd * 2).astype(np.float32))                                   # dist = d^2 / 2, exactly
    cosines = 1.0 - (qu.astype(np.float64)[:, None, :] * bu.astype(np.float64)[ci.clip(0)]).sum(-1)
    ok = ci >= 0
    # 1 - cos of the unit rows against d^2 / 2: half the bound of d^2, and the rows' norms are 1 to a few 2^-24
    assert (np.abs(cosines - cd)[ok] <= np.broadcast_to(bound(qu, bu)[:, None], ci.shape)[ok]).all()
    loo = eae_amd.knn_search(bt, bt, 7, exclude_self=True)
    assert _same((loo.idx.cpu().numpy(), loo.dist.cpu().numpy()), _search(bank, bank, 7, self_offset=0))
    assert not (loo.idx == torch.arange(700, device="cuda")[:, None]).any()


@pytest.mark.parametrize("metric", ["l2", "cosine"])
@pytest.mark.parametrize("weights", ["uniform", "distance"])
def test_knn_classify_recovers_the_blobs(weights, metric):
    z, ids, _ = blobs(600, 64, 10, seed=5)
    zt, lt = torch.from_numpy(z).cuda(), torch.from_numpy(ids).cuda()
    for k in (1, 5, 32):
        labels, votes = eae_amd.knn_classify(zt, zt, lt, k, 10, weights=weights, exclude_self=True, metric=metric)
        assert labels.dtype == torch.int64 and votes.shape == (600, 10) and votes.dtype == torch.float32
        assert torch.equal(labels, lt)
        if weights == "uniform":
            assert torch.equal(votes, torch.nn.functional.one_hot(lt, 10).float() * k)


def test_knn_classify_votes_on_random_data():
    """Votes through the tau-acceptance of the search only: the labels of random data are not compared (near-ties at the k-th slot)."""
    q, bank = _data(500, 900, 16, seed=31)
    lab = np.random.default_rng(1).integers(-1, 6, 900)                    # -1 and 5: outside [0, 5), no vote
    qt, bt, lt = torch.from_numpy(q).cuda(), torch.from_numpy(bank).cuda(), torch.from_numpy(lab).cuda()
    q[4, 2] = np.nan
    qt[4, 2] = float("nan")
    res = eae_amd.knn_search(qt, bt, 9)
    idx, dist = res.idx.cpu().numpy(), res.dist.cpu().numpy()
    accept(q, bank, 9, idx, dist)
    for weights in ("uniform", "distance"):
        labels, votes = eae_amd.knn_classify(qt, bt, lt, 9, 5, weights=weights)
        labels, votes = labels.cpu().numpy(), votes.cpu().numpy()
        ref = np.zeros((500, 5))
        for n in range(500):
            for j in range(9):
                if idx[n, j] >= 0 and 0 <= lab[idx[n, j]] < 5:
                    ref[n, lab[idx[n, j]]] += 1.0 if weights == "uniform" else 1.0 / (float(dist[n, j]) + 1e-12)
        assert np.allclose(votes, ref, rtol=12 * 2.0 ** -24, atol=0)          # k - 1 adds, an add and a division per term and (votes[4] == 0).all() and labels[4] == -1
        has = votes.sum(1) > 0
        assert np.array_equal(labels[has], votes[has].argmax(1)) and (labels[~has] == -1).all()      # first maximum: the lowest class
    # a vote tie goes to the lowest class id; a row whose neighbours are all unlabelled gets -1
    b2 = torch.tensor([[0.0], [1.0], [2.0], [50.0], [51.0]], device="cuda")
    l2 = torch.tensor([3, 1, 7, -1, 9], device="cuda")
    labels, votes = eae_amd.knn_classify(torch.tensor([[0.4], [50.4]], device="cuda"), b2, l2, 2, 5)
    assert labels.tolist() == [1, -1] and votes.tolist() == [[0, 1, 0, 1, 0], [0, 0, 0, 0, 0]]


# ---------------------------------------------------------------------------------------------------- 7. scenes
@pytest.fixture(scope="module")
def scene_case():
    m = _model(3, seed=5, latent=64, batch=16)
    scene = _scene(3, 160, 224, torch.uint8, seed=21)
    g = torch.Generator().manual_seed(3)
    bank = (torch.randn((40, 64), generator=g) * 0.5).cuda()
    labels = torch.randint(-1, 4, (40,), generator=g).cuda()
    return m, scene, _divisor(3, torch.uint8), bank, labels


def _tb(a, b):
    """bitwise equality of two results (NaN equals itself)"""
    return all(torch.equal(x, y) if x.dtype == torch.int64 else torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _without_self(z, pos, k, metric="l2"):
    """encode_scene + knn_search by hand: k + 1 neighbours of z[pos], the own entry removed"""
    res = eae_amd.knn_search(z[pos].contiguous(), z, k + 1, metric=metric)
    idx, dist = [], []
    for r in range(pos.numel()):
        row = res.idx[r].tolist()
        j = row.index(int(pos[r])) if int(pos[r]) in row else k
        keep = [c for c in range(k + 1) if c != j]
        idx.append(res.idx[r, keep])
        dist.append(res.dist[r, keep])
    return torch.stack(idx), torch.stack(dist)


def test_similar_windows(scene_case):
    m, scene, div, bank, _ = scene_case
    z = eae_amd.encode_scene(scene, m, divisor=div, stride=32)                   # a 4 x 6 grid
    query = torch.tensor([0, 13, 23, 13], device="cuda")
    res = eae_amd.similar_windows(scene, m, query, 5, divisor=div, stride=32)
    assert isinstance(res, eae_amd.KNNResult) and res.idx.shape == (4, 5)
    assert _tb(res, _without_self(z, query, 5))
    assert not (res.idx == query[:, None]).any() and int(res.idx.min()) >= 0 and int(res.idx.max()) < 24
    assert _tb(eae_amd.similar_windows(scene, m, query, 5, divisor=div, stride=32, metric="cosine"), _without_self(z, query, 5, "cosine"))
    # latents as the query: searched as they are
    res = eae_amd.similar_windows(scene, m, bank[:3], 4, divisor=div, stride=32)
    assert _tb(res, eae_amd.knn_search(bank[:3], z, 4))
    # windows=: the bank is those windows, the result holds their ids, more slots than windows are empty
    ids = torch.tensor([20, 3, 7, 11, 12, 0, 23], device="cuda")
    zw = eae_amd.encode_scene(scene, m, divisor=div, stride=32, windows=ids)
    q2 = torch.tensor([7, 23], device="cuda")
    res = eae_amd.similar_windows(scene, m, q2, 8, divisor=div, stride=32, windows=ids)
    hidx, hdist = _without_self(zw, torch.tensor([2, 6], device="cuda"), 8)
    assert torch.equal(res.idx, torch.where(hidx >= 0, ids[hidx.clamp(min=0)], -1)) and _tb((res.dist,), (hdist,))
    assert (res.idx[:, 6:] == -1).all() and torch.isnan(res.dist[:, 6:]).all() and (res.idx[:, :6] >= 0).all()
    assert not (res.idx == q2[:, None]).any() and bool(torch.isin(res.idx[:, :6], ids).all())
    with pytest.raises(RuntimeError, match="window set"):
        eae_amd.similar_windows(scene, m, torch.tensor([1], device="cuda"), 2, divisor=div, stride=32, windows=ids)


def test_similar_windows_nodata_and_border(scene_case):
    m, scene, div, _, _ = scene_case
    holed = scene.clone()
    holed[:, :, 100:110] = 0                                               # a stripe of nodata through window columns 2 and 3 (stride 32)
    ids = eae_amd.valid_windows(holed, 64, 32, nodata=0)
    assert 0 < ids.numel() < 24
    zw = eae_amd.encode_scene(holed, m, divisor=div, stride=32, windows=ids)
    pos = torch.tensor([0, int(ids.numel()) - 1], device="cuda")
    res = eae_amd.similar_windows(holed, m, ids[pos], 3, divisor=div, stride=32, nodata=0)
    hidx, hdist = _without_self(zw, pos, 3)
    assert torch.equal(res.idx, ids[hidx]) and _tb((res.dist,), (hdist,)) and not (res.idx == ids[pos][:, None]).any()
    zb = eae_amd.encode_scene(scene, m, divisor=div, border="reflect")     # the 3 x 4 grid that covers the scene
    qb = torch.tensor([11, 0], device="cuda")
    res = eae_amd.similar_windows(scene, m, qb, 4, divisor=div, border="reflect")
    assert _tb(res, _without_self(zb, qb, 4)) and int(res.idx.max()) < 12


def test_knn_classify_scene(scene_case):
    m, scene, div, bank, labels = scene_case
    for weights, metric in (("uniform", "l2"), ("distance", "cosine")):
        z = eae_amd.encode_scene(scene, m, divisor=div, stride=32)
        lab, votes = eae_amd.knn_classify(z, bank, labels, 5, 4, weights=weights, metric=metric)
        lmap, vmap = eae_amd.knn_classify_scene(scene, m, bank, labels, 5, 4, weights=weights, metric=metric, divisor=div, stride=32)
        assert lmap.shape == (4, 6) and lmap.dtype == torch.int64 and vmap.shape == (4, 4, 6) and vmap.dtype == torch.float32
        assert torch.equal(lmap.reshape(-1), lab) and _tb((vmap.reshape(4, -1).t().contiguous(),), (votes,))
    # windows=
    ids = torch.tensor([20, 3, 7, 11, 12, 0, 23], device="cuda")
    zw = eae_amd.encode_scene(scene, m, divisor=div, stride=32, windows=ids)
    lab, votes = eae_amd.knn_classify(zw, bank, labels, 5, 4)
    lmap, vmap = eae_amd.knn_classify_scene(scene, m, bank, labels, 5, 4, divisor=div, stride=32, windows=ids)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    flat, vflat = lmap.reshape(-1), vmap.reshape(4, -1)
    assert torch.equal(flat[ids], lab) and torch.equal(vflat[:, ids], votes.t())
    assert (flat[rest] == -1).all() and (vflat[:, rest] == 0).all()                       # windows not run: -1 and 0 votes
    # nodata=
    holed = scene.clone()
    holed[:, :, 100:110] = 0
    vids = eae_amd.valid_windows(holed, 64, 32, nodata=0)
    lab, votes = eae_amd.knn_classify(eae_amd.encode_scene(holed, m, divisor=div, stride=32, windows=vids), bank, labels, 5, 4)
    lmap, vmap = eae_amd.knn_classify_scene(holed, m, bank, labels, 5, 4, divisor=div, stride=32, nodata=0)
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[vids] = False
    flat, vflat = lmap.reshape(-1), vmap.reshape(4, -1)
    assert torch.equal(flat[vids], lab) and torch.equal(vflat[:, vids], votes.t()) and (flat[rest] == -1).all() and (vflat[:, rest] == 0).all()
    # border=
    zb = eae_amd.encode_scene(scene, m, divisor=div, border="edge")
    lab, votes = eae_amd.knn_classify(zb, bank, labels, 5, 4)
    lmap, vmap = eae_amd.knn_classify_scene(scene, m, bank, labels, 5, 4, divisor=div, border="edge")
    assert lmap.shape == (3, 4) and torch.equal(lmap.reshape(-1), lab) and torch.equal(vmap.reshape(4, -1), votes.t())
