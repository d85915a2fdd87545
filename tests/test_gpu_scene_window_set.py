"""The latent functions of a scene (`cluster_scene`, `knn_classify_scene`, `similar_windows`) go from a window set to latents one way
(`scene._scene_latents`): under nodata / mask they select the valid windows once -- the path's one host synchronisation -- and do not
read the ids the selection produced back; only a caller's ``windows=`` has its range read, once.  Every result is compared bitwise
with the composition by hand: `valid_windows` + `encode_scene` + `kmeans_fit` / `knn_classify` / `knn_search`."""
import pytest
import torch

import eae_amd
from eae_amd import scene as S
from scene_util import _model, _scene, _divisor

pytestmark = pytest.mark.gpu

K_NEAR = 3


@pytest.fixture(scope="module")
def case():
    """The 160 x 224 scene (2 x 3 windows, 4 x 6 at stride 32) with window (1, 2) of the stride-32 grid zeroed, and the references."""
    m = _model(3, seed=5, latent=64, batch=16)
    scene = _scene(3, 160, 224, torch.uint8, seed=21)
    scene[:, 32:96, 64:128] = 0
    div = _divisor(3, torch.uint8)
    g = torch.Generator().manual_seed(3)
    bank = (torch.randn((40, 64), generator=g) * 0.5).cuda()
    labels = torch.randint(-1, 4, (40,), generator=g).cuda()
    valid = eae_amd.valid_windows(scene, 64, 32, nodata=0)
    assert 2 < valid.numel() < 24
    given = torch.tensor([20, 3, 7, 11, 12, 0, 23], device="cuda")       # any order; some of them hold nodata
    ref = {}
    for name, ids in (("nodata", valid), ("windows", given)):
        z = eae_amd.encode_scene(scene, m, divisor=div, stride=32, windows=ids)
        pos = torch.tensor([0, int(ids.numel()) - 1], device="cuda")
        ref[name] = dict(ids=ids, pos=pos, fit=eae_amd.kmeans_fit(z, 2, seed=4), vote=eae_amd.knn_classify(z, bank, labels, 5, 4),
                         near=eae_amd.knn_search(z[pos].contiguous(), z, K_NEAR + 1))
    return m, scene, div, bank, labels, ref


@pytest.fixture
def calls(monkeypatch):
    """Counts of `scene._select` and of the id-range read, `scene._windows_arg(check_range=True)`."""
    n = {"select": 0, "range": 0}
    select, windows_arg = S._select, S._windows_arg

    def counted_select(*a, **kw):
        n["select"] += 1
        return select(*a, **kw)

    def counted_windows_arg(windows, device, n_windows, allow_empty, check_range=True):
        n["range"] += bool(check_range)
        return windows_arg(windows, device, n_windows, allow_empty, check_range)

    monkeypatch.setattr(S, "_select", counted_select)
    monkeypatch.setattr(S, "_windows_arg", counted_windows_arg)
    return n


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _rest(ids):
    rest = torch.ones(24, dtype=torch.bool, device="cuda")
    rest[ids] = False
    return rest


@pytest.mark.parametrize("name", ["nodata", "windows"])
def test_one_select_no_range_read_of_selected_ids(case, calls, name):
    m, scene, div, bank, labels, ref = case
    r = ref[name]
    ids, rest = r["ids"], _rest(r["ids"])
    how = dict(nodata=0) if name == "nodata" else dict(windows=ids)
    want = {"select": 1, "range": 0} if name == "nodata" else {"select": 0, "range": 1}

    calls.update(select=0, range=0)
    cmap, res = eae_amd.cluster_scene(scene, m, k=2, divisor=div, stride=32, seed=4, **how)
    assert calls == want
    fit = r["fit"]
    assert _same(res[:5], fit[:5]) and res.n_iter == fit.n_iter          # centroids, labels, dist, counts, inertia
    flat = cmap.reshape(-1)
    assert cmap.shape == (4, 6) and torch.equal(flat[ids], fit.labels) and (flat[rest] == -1).all()

    calls.update(select=0, range=0)
    lmap, vmap = eae_amd.knn_classify_scene(scene, m, bank, labels, 5, 4, divisor=div, stride=32, **how)
    assert calls == want
    lab, votes = r["vote"]
    flat, vflat = lmap.reshape(-1), vmap.reshape(4, -1)
    assert lmap.shape == (4, 6) and vmap.shape == (4, 4, 6) and vmap.is_contiguous()
    assert torch.equal(flat[ids], lab) and _same((vflat[:, ids],), (votes.t(),)) and (flat[rest] == -1).all() and (vflat[:, rest] == 0).all()

    calls.update(select=0, range=0)
    near = eae_amd.similar_windows(scene, m, ids[r["pos"]], K_NEAR, divisor=div, stride=32, **how)
    assert calls == want
    # by hand: K_NEAR + 1 neighbours of the query rows, the own entry (or, lying beyond, the last) dropped, rows turned into ids
    hand = r["near"]
    for q in range(2):
        row = hand.idx[q].tolist()
        own = row.index(int(r["pos"][q])) if int(r["pos"][q]) in row else K_NEAR
        keep = [c for c in range(K_NEAR + 1) if c != own]
        assert torch.equal(near.idx[q], ids[hand.idx[q, keep]]) and _same((near.dist[q],), (hand.dist[q, keep],))
