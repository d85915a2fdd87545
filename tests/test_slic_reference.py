"""Superpixels (eae_amd.segment; include/eae.h, "superpixels"): the three entry points in the header, the library and the ctypes
table; the argument errors of the C calls and of the wrappers, all raised before a device is touched; and the NumPy restatement of
the semantics (tests/slic_ref.py) itself: the quantiser's edge values, a hand-worked case, ties, colour-only clustering, its
invariants on random inputs, and the conditions the pipeline meets on the synthetic parcel scene.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd import segment as S
from regions_ref import label_regions_ref
import slic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eae_slic_step", "eae_slic_centres", "eae_map_regions_wide")
PUBLIC = ("slic_clusters", "slic_scene", "classify_superpixels", "zone_boundaries")


def test_symbols_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    assert "superpixels" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.EXPORTS
    for name in PUBLIC:
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))
    assert "Superpixels" in eae_amd.__all__ and eae_amd.Superpixels is S.Superpixels
    from eae_amd import build as B
    assert "eae_slic.hip" in B.SOURCES


# ---------------------------------------------------------------------------------------------------- the C entry points
def _buf():
    buf = (C.c_longlong * 64)()
    return buf, C.cast(buf, C.c_void_p)


def test_slic_step_rejects_bad_arguments():
    """The checks of the C call come before any launch, so they run without a device (the pointers are never dereferenced)."""
    lib = _lib.load()
    keep, p = _buf()
    ok = dict(data=p, dtype=0, c=3, h=4, w=6, div=p, mask=None, step=2, m=10, cen=None, sums=p, labels=None)
    bad = [dict(data=None), dict(div=None), dict(sums=None), dict(dtype=3), dict(dtype=-1), dict(c=0), dict(c=17), dict(step=1),
           dict(step=257), dict(m=-1), dict(m=2 ** 40 + 1), dict(h=0), dict(w=0), dict(h=2 ** 16, w=2 ** 15),
           dict(h=46000, w=46000, c=16),                                   # 23000^2 clusters x 19 columns: above 2^31 - 1
           dict(data=C.c_void_p(p.value + 1), dtype=1)]                    # uint16 at an odd address
    for change in bad:
        a = dict(ok, **change)
        rc = lib.eae_slic_step(None, a["data"], a["dtype"], a["c"], a["h"], a["w"], a["div"], a["mask"], a["step"], a["m"], a["cen"],
                               a["sums"], a["labels"])
        assert rc == -2 and b"slic_step" in lib.eae_last_error(), change
    # the limits themselves pass their checks (and fail on the next one: a NULL sums_out)
    for change in (dict(step=2, m=2 ** 40), dict(step=256, m=0), dict(c=16), dict(h=46000, w=46000, c=1)):
        a = dict(ok, **change)
        rc = lib.eae_slic_step(None, a["data"], a["dtype"], a["c"], a["h"], a["w"], a["div"], None, a["step"], a["m"], None, None, None)
        assert rc == -2 and b"NULL data, divisor or sums_out" in lib.eae_last_error(), change


def test_slic_centres_and_regions_wide_reject_bad_arguments():
    lib = _lib.load()
    keep, p = _buf()
    for sums, n, c, cen in ((None, 4, 3, p), (p, 4, 3, None), (p, 0, 3, p), (p, 4, 0, p), (p, 4, 17, p), (p, 2 ** 31 // 4, 1, p)):
        assert lib.eae_slic_centres(None, sums, n, c, cen) == -2 and b"slic_centres" in lib.eae_last_error()
    ok = dict(labels=p, h=4, w=4, conn=4, regions=p, ws=p, nbytes=128)
    for change in (dict(labels=None), dict(regions=None), dict(conn=5), dict(conn=0), dict(ws=None), dict(nbytes=127), dict(h=0),
                   dict(w=0), dict(h=2 ** 16, w=2 ** 15)):
        a = dict(ok, **change)
        rc = lib.eae_map_regions_wide(None, a["labels"], a["h"], a["w"], a["conn"], a["regions"], a["ws"], a["nbytes"])
        assert rc == -2, change
        if "h" not in change and "w" not in change:
            assert b"map_regions_wide" in lib.eae_last_error(), change


# ---------------------------------------------------------------------------------------------------- the wrappers' host errors
def test_slic_host_errors():
    scene = torch.zeros((3, 40, 50), dtype=torch.uint8)
    for f in (eae_amd.slic_clusters, eae_amd.slic_scene):
        with pytest.raises(RuntimeError, match=r"planar tensor \[C,H,W\]"):
            f(scene[0], 8)
        with pytest.raises(RuntimeError, match="scene dtype must be uint8, uint16 or float32"):
            f(scene.to(torch.int32), 8)
        with pytest.raises(RuntimeError, match="bands must be in 1..16"):
            f(torch.zeros((17, 4, 4), dtype=torch.uint8), 2)
        with pytest.raises(RuntimeError, match="scene is empty"):
            f(scene[:, :0], 8)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            f(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 2 ** 16, 2 ** 15), 8)
        for step in (1, 257, 8.0, True, None):
            with pytest.raises(RuntimeError, match="step must be an integer in 2..256"):
                f(scene, step)
        for comp in (-0.1, float("nan"), float("inf"), "x", True, 16.1):
            with pytest.raises(RuntimeError, match="compactness|spatial weight"):
                f(scene, 8, compactness=comp)
        for it in (0, -1, 2.5):
            with pytest.raises(RuntimeError, match="iterations must be an integer"):
                f(scene, 8, iterations=it)
        with pytest.raises(RuntimeError, match="n_h \\* n_w \\* \\(C \\+ 3\\)"):
            f(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(16, 46000, 46000), 2)
        with pytest.raises(RuntimeError, match="divisor must have one value per band"):
            f(scene, 8, divisor=[1.0, 2.0])
        with pytest.raises(RuntimeError, match=r"mask must be a \[H, W\]"):
            f(scene, 8, mask=torch.zeros((40, 49), dtype=torch.bool))
        with pytest.raises(RuntimeError, match="mask dtype"):
            f(scene, 8, mask=torch.zeros((40, 50), dtype=torch.int32))
        with pytest.raises(RuntimeError, match="HIP device"):              # everything is in order but the scene is a host tensor
            f(scene, 8, divisor=255.0, mask=torch.zeros((40, 50), dtype=torch.bool))
    for m in (0, -3, 1.5):
        with pytest.raises(RuntimeError, match="min_size must be an integer"):
            eae_amd.slic_scene(scene, 8, min_size=m)
    for conn in (5, 6, True):
        with pytest.raises(RuntimeError, match="connectivity must be 4 or 8"):
            eae_amd.slic_scene(scene, 8, connectivity=conn)
    assert S.spatial_weight(0.1) == R.weight_ref(0.1) == 42948362 and S.spatial_weight(0) == 0 and S.spatial_weight(16.0) == 2 ** 40 - 2 ** 25 + 256


def test_classify_superpixels_host_errors():
    torch.manual_seed(0)
    ae = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3).eval()
    mlp = eae_amd.MLP(64, 10).eval()
    scene = torch.zeros((3, 150, 200), dtype=torch.uint8)
    f = eae_amd.classify_superpixels
    with pytest.raises(RuntimeError, match="step must be an integer"):
        f(scene, ae, mlp, 1, divisor=255.0)
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8"):
        f(scene, ae, mlp, 8, connectivity=3, divisor=255.0)
    with pytest.raises(RuntimeError, match="rule must be 'probs' or 'votes'"):
        f(scene, ae, mlp, 8, rule="all", divisor=255.0)
    with pytest.raises(RuntimeError, match="min_coverage must be a number in"):
        f(scene, ae, mlp, 8, min_coverage=1.5, divisor=255.0)
    with pytest.raises(RuntimeError, match="mlp must be an MLP"):
        f(scene, ae, ae, 8, divisor=255.0)
    with pytest.raises(RuntimeError):                                       # everything is in order but the scene is a host tensor
        f(scene, ae, mlp, 8, divisor=255.0)


def test_num_classes_none_host_errors():
    labels = torch.zeros((4, 5), dtype=torch.int64)
    for k in (0, 65, 2.0, True):
        with pytest.raises(RuntimeError, match="num_classes must be an integer in 1..64"):
            eae_amd.label_regions(labels, k)
        with pytest.raises(RuntimeError, match="num_classes must be an integer in 1..64"):
            eae_amd.sieve(labels, k, 2)
        with pytest.raises(RuntimeError, match="num_classes must be an integer in 1..64"):
            eae_amd.region_table(labels, labels, k)
    with pytest.raises(RuntimeError, match="HIP device"):                  # None passes the host checks
        eae_amd.label_regions(labels, None)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.sieve(labels, None, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.region_table(labels, labels)
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8"):
        eae_amd.label_regions(labels, None, connectivity=5)


# ---------------------------------------------------------------------------------------------------- the quantiser
def test_quantiser_edge_values():
    d = np.float32(0.7)
    v = np.array([0.0, d, 0.8, 1e30, -0.1, -1e30, np.nan, np.inf, -np.inf, 0.35], dtype=np.float32).reshape(1, 1, -1)
    u = R.quantise_ref(v, d)[0, 0]
    half = int(np.rint(65535 * (np.float64(np.float32(0.35)) / np.float64(d))))
    assert u.tolist() == [0, 65535, 65535, 65535, 0, 0, 0, 65535, 0, half]
    # a half-way case: 65535 * v / d = 2.5 and 3.5 exactly (d = 65535, a float32), which round to the even neighbours
    assert R.quantise_ref(np.array([[[2.5, 3.5, 0.5, 1.5]]], dtype=np.float32), 65535.0)[0, 0].tolist() == [2, 4, 0, 2]
    # uint8 with divisor 255: v * 257, exactly
    v8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    assert np.array_equal(R.quantise_ref(v8, 255.0)[0], v8[0].astype(np.int64) * 257)
    # uint16 with divisor 65535: the identity; one divisor per band
    v16 = np.array([[[0, 1, 40000, 65535]], [[0, 1, 40000, 65535]]], dtype=np.uint16)
    u = R.quantise_ref(v16, [65535.0, 40000.0])
    assert u[0, 0].tolist() == [0, 1, 40000, 65535] and u[1, 0].tolist() == [0, 2, 65535, 65535]
    # a zero and a negative divisor follow the expression: v / 0 = +Inf -> 1, 0 / 0 = NaN -> 0, v / -d < 0 -> 0
    assert R.quantise_ref(np.array([[[0.0, 1.0]]], dtype=np.float32), 0.0)[0, 0].tolist() == [0, 65535]
    assert R.quantise_ref(np.array([[[0.5, -0.5]]], dtype=np.float32), -1.0)[0, 0].tolist() == [0, 32768]


# ---------------------------------------------------------------------------------------------------- hand-worked
HAND = R.HAND_SCENE            # uint8 [1, 4, 6]: rows (0 0 0 10 10 10), (0 0 10 10 10 10), (0 0 0 10 10 10), (20 20 20 20 20 0)
# step 3: cells (rows 0-2 | row 3) x (columns 0-2 | 3-5), clusters 0..3; u = 257 v: 0, 2570, 5140
HAND_SUMS0 = [[9, 9, 9, 2570], [9, 9, 36, 23130], [3, 9, 3, 15420], [3, 9, 12, 10280]]
HAND_CEN0 = [[9, 1, 1, 286], [9, 1, 4, 2570], [3, 3, 1, 5140], [3, 3, 4, 3427]]
# iteration 1, M = 1000: the colour terms (9 (u - mu)^2 >= 6.6e6 between the wrong pairs) outweigh every spatial term (<= 34000), so
# u = 0 goes to cluster 0 (286), u = 2570 to cluster 1 and u = 5140 to cluster 2; cluster 3 (3427) keeps nothing and stays empty
HAND_LABELS1 = [[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1], [2, 2, 2, 2, 2, 0]]
HAND_SUMS1 = [[9, 11, 12, 0], [10, 10, 38, 25700], [5, 15, 10, 25700], [0, 0, 0, 0]]
HAND_CEN1 = [[9, 1, 1, 0], [10, 1, 4, 2570], [5, 3, 2, 5140], [0, 0, 0, 0]]


def test_hand_worked_case():
    hist = R.slic_ref(HAND, 255.0, 3, 1000, 3, history=True)
    labels, sums, centres = hist[0]
    assert labels.tolist() == [[0, 0, 0, 1, 1, 1]] * 3 + [[2, 2, 2, 3, 3, 3]]
    assert sums.tolist() == HAND_SUMS0 and centres.tolist() == HAND_CEN0 and centres.dtype == np.int32 and sums.dtype == np.int64
    labels, sums, centres = hist[1]
    assert labels.tolist() == HAND_LABELS1 and sums.tolist() == HAND_SUMS1 and centres.tolist() == HAND_CEN1
    for labels, sums, centres in hist[2:]:                                 # a fixed point; the empty cluster stays empty
        assert labels.tolist() == HAND_LABELS1 and sums.tolist() == HAND_SUMS1 and centres.tolist() == HAND_CEN1


def test_constant_image_ties_go_to_the_lowest_id():
    """A constant image with M > 0: the colour term is 0 everywhere, so a pixel takes the nearest centre and, at equal distance, the
    lowest cluster id."""
    scene = np.full((1, 8, 8), 7, dtype=np.uint8)
    hist = R.slic_ref(scene, 255.0, 4, 5, 1, history=True)
    cen = hist[0][2]
    assert cen.tolist() == [[16, 2, 2, 1799], [16, 2, 6, 1799], [16, 6, 2, 1799], [16, 6, 6, 1799]]    # (2 * 24 + 16) // 32 = 2
    labels = hist[1][0]
    # centres at rows / columns 2 and 6: row 4 (and column 4) is equally far from both and goes to the lower id
    assert labels[:, 0].tolist() == [0, 0, 0, 0, 0, 2, 2, 2] and labels[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1]
    assert labels[4, 4] == 0 and labels[5, 5] == 3 and labels[4, 5] == 1 and labels[5, 4] == 2


def test_weight_zero_is_colour_only():
    """M = 0: D is the colour term alone, so within its nine candidates a pixel takes the closest mean wherever the centre lies; two
    pixels of one home cell with the same value get the same cluster."""
    rng = np.random.default_rng(5)
    scene = rng.integers(0, 4, (2, 20, 24)).astype(np.uint8) * 60
    labels = R.slic_ref(scene, 255.0, 4, 0, 2)[0]
    y, x = np.mgrid[:20, :24]
    key = ((y // 4) * 6 + x // 4) * 10000 + scene[0].astype(np.int64) * 100 + scene[1] // 60
    for k in np.unique(key):
        assert np.unique(labels[key == k]).size == 1
    assert not np.array_equal(labels, R.slic_ref(scene, 255.0, 4, 10 ** 9, 2)[0])


@pytest.mark.parametrize("seed,dtype,c,step", [(0, np.uint8, 3, 5), (1, np.uint16, 4, 7), (2, np.float32, 16, 4), (3, np.uint8, 1, 2)])
def test_reference_invariants(seed, dtype, c, step):
    rng = np.random.default_rng(seed)
    h, w = 33, 41
    div = 1.0 if dtype == np.float32 else float(np.iinfo(dtype).max)
    scene = (rng.random((c, h, w)) * (1.2 if dtype == np.float32 else div)).astype(dtype)
    mask = rng.random((h, w)) < 0.2
    mask[:step, :step] = True                                              # a fully masked cell: an empty cluster from the start
    n_h, n_w = R.grid_ref(h, w, step)
    for labels, sums, centres in R.slic_ref(scene, div, step, R.weight_ref(0.1), 3, mask, history=True):
        assert ((labels >= 0) == ~mask).all() and (labels[mask] == -1).all() and labels.max() < n_h * n_w
        assert sums[:, 0].sum() == (~mask).sum() and sums.shape == (n_h * n_w, c + 3)
        assert (sums[0] == 0).all() and (centres[0] == 0).all()            # the empty cluster stays empty
        assert np.array_equal(np.bincount(labels[~mask], minlength=n_h * n_w), sums[:, 0])
        live = centres[:, 0] > 0
        assert (centres[live, 1] < h).all() and (centres[live, 2] < w).all() and (centres[:, 3:] <= 65535).all() and (centres >= 0).all()
        # a pixel stays within the cells around its cluster's own cell
        y, x = np.mgrid[:h, :w]
        k = labels[~mask]
        assert (np.abs(y[~mask] // step - k // n_w) <= 1).all() and (np.abs(x[~mask] // step - k % n_w) <= 1).all()


# ---------------------------------------------------------------------------------------------------- the parcel scene
@pytest.fixture(scope="module")
def parcels():
    return R.parcel_scene()


@pytest.mark.parametrize("step,compactness", [(8, 0.1), (8, 0.3), (5, 0.05)])
def test_parcel_scene_conditions(parcels, step, compactness):
    scene, truth = parcels
    h, w = truth.shape
    zones, z, labels, _ = R.slic_scene_ref(scene, 255.0, step, compactness, 6)
    assert R.purity(zones, truth) >= 0.99
    assert R.purity(R.grid_zones(h, w, 8), truth) < 0.95
    assert zones.min() == 0 and zones.max() == z - 1 and np.unique(zones).size == z
    regions = label_regions_ref(zones, z, 4)
    assert np.unique(regions).size == z                                    # every zone is one connected region
    assert np.bincount(zones.reshape(-1)).min() >= R.default_min_size(step)
    first = np.array([np.flatnonzero(zones.reshape(-1) == i)[0] for i in range(z)])
    assert (np.diff(first) > 0).all()                                      # ids ascend with a zone's smallest linear index


def test_zones_of_masked_and_detached_clusters():
    """Two detached fragments of one cluster become two zones; a fragment below min_size dissolves into its largest neighbour; masked
    pixels stay -1."""
    labels = np.array([[5, 5, 9, 9, 5, 5],
                       [5, 5, 9, 9, 5, 5],
                       [-1, 7, 9, 9, 5, 5]], dtype=np.int64)
    zones, z = R.zones_ref(labels, 2)
    assert z == 3 and zones.tolist() == [[0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 2, 2], [-1, 1, 1, 1, 2, 2]]


# ---------------------------------------------------------------------------------------------------- zone_boundaries
@pytest.mark.parametrize("connectivity", [4, 8])
def test_zone_boundaries_against_numpy(connectivity):
    rng = np.random.default_rng(11)
    zones = np.repeat(np.repeat(rng.integers(-1, 5, (5, 6)), 3, 0), 3, 1)[:13, :17]
    for dtype in (torch.int32, torch.int64):
        got = eae_amd.zone_boundaries(torch.from_numpy(zones).to(dtype), connectivity)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), R.boundaries_ref(zones, connectivity))
    one = eae_amd.zone_boundaries(torch.zeros((1, 1), dtype=torch.int32))
    assert one.shape == (1, 1) and not bool(one.any())
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.zone_boundaries(torch.zeros((3, 3)))
    with pytest.raises(RuntimeError, match="connectivity must be 4 or 8"):
        eae_amd.zone_boundaries(torch.zeros((3, 3), dtype=torch.int32), 6)
