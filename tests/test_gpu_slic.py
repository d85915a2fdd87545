"""Superpixels on the device (eae_amd.segment): `eae_slic_step` and `eae_slic_centres` by shape against the NumPy restatement of their
semantics (tests/slic_ref.py), `eae_map_regions_wide` against the flood fill of tests/regions_ref.py, ``num_classes=None`` in
`label_regions` and `sieve`, and `slic_scene` / `classify_superpixels` end to end.  Integers throughout: every comparison is exact
equality, outputs are pre-filled with -7, and a second run equals the first."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from eae_amd.postprocess import _workspace
import regions_ref as G
import slic_ref as R
from scene_util import _model, _mlp

pytestmark = pytest.mark.gpu

M_DEFAULT = R.weight_ref(0.1)


def _tensor(a):
    """A device tensor of a NumPy array (uint16 through a view: torch.from_numpy has no uint16 on every version)."""
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def _dirty(shape, dtype):
    return torch.full(shape, -7, dtype=dtype, device="cuda")


def _step(scene, div, mask, step, m, centres, want_labels=True):
    """One `eae_slic_step` + `eae_slic_centres` into dirty buffers: (labels or None, sums, centres) as NumPy arrays."""
    c, h, w = scene.shape
    n_h, n_w = R.grid_ref(h, w, step)
    sums = _dirty((n_h * n_w, c + 3), torch.int64)
    labels = _dirty((h, w), torch.int32) if want_labels else None
    lib = _lib.load()
    _lib.check(lib.eae_slic_step(_stream(), _ptr(scene), {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}[scene.dtype], c, h, w,
                                 _ptr(div), _ptr(mask), step, m, _ptr(centres), _ptr(sums), _ptr(labels)))
    cen = _dirty((n_h * n_w, c + 3), torch.int32)
    _lib.check(lib.eae_slic_centres(_stream(), _ptr(sums), n_h * n_w, c, _ptr(cen)))
    return labels, sums, cen


def _rand_scene(c, h, w, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        s = (rng.random((c, h, w)) * 1.3 - 0.1).astype(np.float32)          # values below 0 and above the divisor
        flat = s.reshape(-1)
        special = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, -0.0, 1e30, -1e30, np.nan], dtype=np.float32)
        flat[rng.permutation(flat.size)[:special.size]] = special
        return s
    # blocks of similar values with noise, so that clusters move; the full range of the dtype
    top = np.iinfo(dtype).max
    coarse = rng.integers(0, top + 1, (c, -(-h // 6), -(-w // 9)))
    s = np.repeat(np.repeat(coarse, 6, 1), 9, 2)[:, :h, :w] + rng.integers(-top // 10, top // 10 + 1, (c, h, w))
    return np.clip(s, 0, top).astype(dtype)


def _mask(h, w, step, seed):
    """Runs and single pixels, and the cell (1, 2) of the grid (clipped to the raster) masked entirely."""
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) < 0.1) | (np.repeat(rng.random((h, -(-w // 8))) < 0.15, 8, 1)[:, :w])
    m[step:2 * step, 2 * step:3 * step] = True
    return m


def _case(name):
    """(scene, divisor, step, M, mask or None, iterations to compare)."""
    its = (0, 1, 2, 5)
    div8, div16 = 255.0, 65535.0
    if name == "1x1":
        return np.array([[[200]]], dtype=np.uint8), div8, 2, M_DEFAULT, None, its
    if name == "hand 4x6":
        return R.HAND_SCENE, div8, 3, 1000, None, its
    if name == "37x41 u8 S=5":
        return _rand_scene(3, 37, 41, np.uint8, 1), [255.0, 200.0, 300.0], 5, M_DEFAULT, None, its
    if name == "64x257 u16 S=7":
        return _rand_scene(4, 64, 257, np.uint16, 2), [65535.0, 40000.0, 65535.0, 70000.0], 7, M_DEFAULT, None, its
    if name == "33x70 f32 C=16 S=4":
        return _rand_scene(16, 33, 70, np.float32, 3), [0.5 + 0.05 * i for i in range(16)], 4, M_DEFAULT, None, its
    if name == "40x40 S=2":
        return _rand_scene(16, 40, 40, np.uint8, 4), div8, 2, M_DEFAULT, None, its
    if name == "70x90 S=33":
        return _rand_scene(2, 70, 90, np.uint16, 5), div16, 33, M_DEFAULT, None, its
    if name == "50x60 S=256":
        return _rand_scene(3, 50, 60, np.uint8, 6), div8, 256, M_DEFAULT, None, its
    if name == "5000x1 S=3":
        return _rand_scene(2, 5000, 1, np.uint8, 7), div8, 3, M_DEFAULT, None, its
    if name == "200x300 mask":
        return _rand_scene(3, 200, 300, np.uint8, 8), div8, 8, M_DEFAULT, _mask(200, 300, 8, 8), its
    if name == "200x300 constant":
        return np.full((3, 200, 300), 99, dtype=np.uint8), div8, 8, M_DEFAULT, None, its
    if name == "200x300 M=0":
        return _rand_scene(3, 200, 300, np.uint8, 9), div8, 8, 0, None, its
    if name == "200x300 M=2^40":
        s = (np.random.default_rng(10).random((16, 200, 300)) < 0.5).astype(np.uint16) * 65535
        return s, div16, 8, 2 ** 40, None, its
    if name == "2100x4100 S=16":
        return _rand_scene(1, 2100, 4100, np.uint8, 11), div8, 16, M_DEFAULT, None, (0, 1)
    raise KeyError(name)


CASES = ["1x1", "hand 4x6", "37x41 u8 S=5", "64x257 u16 S=7", "33x70 f32 C=16 S=4", "40x40 S=2", "70x90 S=33", "50x60 S=256",
         "5000x1 S=3", "200x300 mask", "200x300 constant", "200x300 M=0", "200x300 M=2^40", "2100x4100 S=16"]


@pytest.mark.parametrize("name", CASES)
def test_step_by_shape(name):
    scene_np, divisor, step, m, mask_np, its = _case(name)
    c, h, w = scene_np.shape
    hist = R.slic_ref(scene_np, divisor, step, m, max(its), mask_np, history=True)
    scene = _tensor(scene_np)
    div = torch.tensor(np.broadcast_to(np.asarray(divisor, dtype=np.float32).reshape(-1), (c,)).copy(), device="cuda")
    mask = None if mask_np is None else torch.from_numpy(mask_np).cuda().view(torch.uint8)
    unmasked = h * w if mask_np is None else int((~mask_np).sum())
    centres = None
    for t in range(max(its) + 1):
        labels, sums, cen = _step(scene, div, mask, step, m, centres)
        if t in its:
            rl, rs, rc = hist[t]
            assert int(sums[:, 0].sum()) == unmasked, t
            assert np.array_equal(sums.cpu().numpy(), rs), t
            assert np.array_equal(cen.cpu().numpy(), rc), t
            assert np.array_equal(labels.cpu().numpy(), rl), t
            if mask_np is not None:
                assert bool((labels[mask.bool()] == -1).all())
            labels2, sums2, cen2 = _step(scene, div, mask, step, m, centres)                 # a second run equals the first
            assert torch.equal(labels2, labels) and torch.equal(sums2, sums) and torch.equal(cen2, cen), t
            none, sums3, _ = _step(scene, div, mask, step, m, centres, want_labels=False)   # without labels: the same sums
            assert none is None and torch.equal(sums3, sums), t
        centres = cen
    if name == "200x300 mask":
        n_w = R.grid_ref(h, w, step)[1]
        assert hist[0][2][1 * n_w + 2].tolist() == [0] * (c + 3)                              # the masked cell: empty from the start


# ---------------------------------------------------------------------------------------------------- eae_map_regions_wide
def _regions_wide(labels, connectivity):
    h, w = labels.shape
    out = _dirty((h, w), torch.int64)
    ws = _workspace(h, w, labels.device)
    _lib.check(_lib.load().eae_map_regions_wide(_stream(), _ptr(labels), h, w, connectivity, _ptr(out), _ptr(ws), ws.numel()))
    return out


def _sparse(pattern, seed):
    """The pattern's classes mapped to sparse ids far above 64."""
    ids = np.random.default_rng(seed).integers(100, 2 ** 40, 16)
    return ids[pattern]


WIDE = {"serpentine": lambda: _sparse(G.serpentine(33, 65), 1), "spiral": lambda: _sparse(G.spiral(33, 65), 2),
        "checkerboard": lambda: _sparse(G.checkerboard(33, 65), 3), "percolation": lambda: _sparse(G.percolation(70, 45, seed=4), 4),
        # ids that differ only in the high word
        "high word": lambda: np.array([5, 5 + 2 ** 32, 5 + 2 ** 33, 5 + 2 ** 62])[G.blobs(33, 65, seed=5, k=4).clip(0, 3)],
        # negatives of every size are unclassified; 0 and 2^63 - 2 are labels
        "negatives": lambda: np.array([-1, 0, 2 ** 63 - 2, -2 ** 63, -2 ** 32, 7])[np.random.default_rng(6).integers(0, 6, (33, 65))]}


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(WIDE))
def test_regions_wide(name, connectivity):
    labels = WIDE[name]().astype(np.int64)
    ref = G.label_regions_ref(labels, np.iinfo(np.int64).max, connectivity)
    assert ((ref >= 0) == (labels >= 0)).all()
    got = _regions_wide(torch.from_numpy(labels).cuda(), connectivity)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert torch.equal(_regions_wide(torch.from_numpy(labels).cuda(), connectivity), got)
    assert torch.equal(eae_amd.label_regions(torch.from_numpy(labels).cuda(), None, connectivity), got)


@pytest.mark.parametrize("connectivity", [4, 8])
def test_num_classes_none_equals_the_class_call(connectivity):
    labels = torch.from_numpy(G.blobs(70, 95, seed=2)).cuda()                 # classes 0..9 and -1
    assert torch.equal(eae_amd.label_regions(labels, None, connectivity), eae_amd.label_regions(labels, 10, connectivity))
    for min_size, passes in ((4, 1), (9, 2)):
        a, ca = eae_amd.sieve(labels, None, min_size, connectivity, passes, return_changed=True)
        b, cb = eae_amd.sieve(labels, 10, min_size, connectivity, passes, return_changed=True)
        assert torch.equal(a, b) and int(ca) == int(cb) and int(ca) > 0
    regions = eae_amd.label_regions(labels, None, connectivity)
    ta, tb = eae_amd.region_table(labels, regions), eae_amd.region_table(labels, regions, 10)
    assert all(torch.equal(ta[k], tb[k]) for k in ta)


# ---------------------------------------------------------------------------------------------------- slic_scene, end to end
@pytest.fixture(scope="module")
def parcels():
    scene, truth = R.parcel_scene()
    return scene, truth, torch.from_numpy(scene).cuda()


@pytest.mark.parametrize("step,compactness,connectivity", [(8, 0.1, 4), (8, 0.3, 8), (5, 0.05, 4)])
def test_slic_scene_on_the_parcel_scene(parcels, step, compactness, connectivity):
    scene_np, truth, scene = parcels
    h, w = truth.shape
    rz, z, rl, rc = R.slic_scene_ref(scene_np, 255.0, step, compactness, 6, connectivity=connectivity)
    sp = eae_amd.slic_scene(scene, step, compactness, iterations=6, divisor=255.0, connectivity=connectivity)
    assert isinstance(sp, eae_amd.Superpixels) and sp.zones.dtype == torch.int32 and sp.clusters.dtype == torch.int32
    assert sp.num_zones == z and np.array_equal(sp.zones.cpu().numpy(), rz)
    assert np.array_equal(sp.clusters.cpu().numpy(), rl) and np.array_equal(sp.centres.cpu().numpy(), rc)
    labels, centres = eae_amd.slic_clusters(scene, step, compactness, iterations=6, divisor=255.0)
    assert torch.equal(labels, sp.clusters) and torch.equal(centres, sp.centres)
    zones = sp.zones.cpu().numpy()
    assert R.purity(zones, truth) >= 0.99 and R.purity(R.grid_zones(h, w, 8), truth) < 0.95
    assert np.unique(G.label_regions_ref(zones, z, connectivity)).size == z     # every zone is connected
    assert np.bincount(zones.reshape(-1)).min() >= R.default_min_size(step)
    edges = eae_amd.zone_boundaries(sp.zones, connectivity)
    assert edges.is_cuda and np.array_equal(edges.cpu().numpy(), R.boundaries_ref(zones, connectivity))


def test_slic_scene_masked_and_min_size(parcels):
    scene_np, truth, scene = parcels
    mask_np = _mask(96, 128, 8, 3)
    mask_np[40:60, 50:] = True                                                  # a band that cuts clusters apart
    mask = torch.from_numpy(mask_np).cuda()
    rz, z, rl, rc = R.slic_scene_ref(scene_np, 255.0, 8, 0.1, 4, mask=mask_np, min_size=5)
    sp = eae_amd.slic_scene(scene, 8, iterations=4, divisor=255.0, mask=mask, min_size=5)
    assert sp.num_zones == z and np.array_equal(sp.zones.cpu().numpy(), rz) and np.array_equal(sp.clusters.cpu().numpy(), rl)
    assert np.array_equal(sp.centres.cpu().numpy(), rc)
    assert bool((sp.zones[mask] == -1).all()) and bool((sp.clusters[mask] == -1).all())
    assert bool((sp.zones[~mask] >= 0).all()) and bool((sp.clusters[~mask] >= 0).all())
    everything = eae_amd.slic_scene(scene, 8, iterations=1, divisor=255.0, mask=torch.ones((96, 128), dtype=torch.uint8, device="cuda"))
    assert everything.num_zones == 0 and bool((everything.zones == -1).all()) and bool((everything.centres == 0).all())


def test_classify_superpixels_equals_classify_zones():
    g = torch.Generator().manual_seed(17)
    coarse = torch.randint(1, 256, (3, 10, 13), generator=g, dtype=torch.int64)
    scene = (coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :150, :200]
             + torch.randint(-5, 6, (3, 150, 200), generator=g)).clamp(1, 255).to(torch.uint8).cuda()
    mask = torch.zeros((150, 200), dtype=torch.bool, device="cuda")
    mask[100:, 150:] = True
    model, mlp = _model(3, batch=64), _mlp()
    kw = dict(divisor=255.0, stride=32, batch=64, blend=True, rule="votes", min_coverage=0.25, mask=mask)
    out = eae_amd.classify_superpixels(scene, model, mlp, 12, compactness=0.2, iterations=3, **kw)
    sp = eae_amd.slic_scene(scene, 12, 0.2, iterations=3, divisor=255.0, mask=mask)
    got = out["superpixels"]
    assert got.num_zones == sp.num_zones > 1 and torch.equal(got.zones, sp.zones) and torch.equal(got.clusters, sp.clusters)
    ref = eae_amd.classify_zones(scene, model, mlp, sp.zones, num_zones=sp.num_zones, **kw)
    assert set(out) == set(ref) | {"superpixels"}
    for key in ("zone_labels", "coverage", "map", "labels", "probs"):
        assert torch.equal(out[key], ref[key]), key
    assert torch.equal(out["confidence"].nan_to_num(-1), ref["confidence"].nan_to_num(-1))
    assert torch.equal(out["stats"].votes, ref["stats"].votes) and torch.equal(out["stats"].prob_sums, ref["stats"].prob_sums)
    assert bool((out["map"][mask] == -1).all()) and bool((got.zones[mask] == -1).all())
