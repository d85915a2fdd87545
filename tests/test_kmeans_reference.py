"""Latent clustering without a GPU: the NumPy restatement (tests/kmeans_ref.py) on hand-worked cases, the two `report` helpers, the
host-only workspace size of the C library, and every rejection `kmeans_fit` / `kmeans_predict` / `cluster_scene` make on the host
before a device is needed (all inputs here are CPU tensors: a call that got past its checks would fail on the device test)."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib, report
from kmeans_ref import assign_ref, update_ref, fit_ref, tau, update_bound, blobs


# ---------------------------------------------------------------------------------------------------- the reference, by hand
def test_two_points_two_centroids():
    z = np.array([[0.0, 0.0], [4.0, 0.0]])
    c = np.array([[1.0, 0.0], [3.0, 1.0]])
    d, lab = assign_ref(z, c)
    assert np.array_equal(d, [[1.0, 10.0], [9.0, 2.0]]) and lab.tolist() == [0, 1]
    m, cnt = update_ref(z, lab, c)
    assert np.array_equal(m, z) and cnt.tolist() == [1, 1]
    cf, lf, df, nf, it = fit_ref(z, c)
    assert np.array_equal(cf, z) and lf.tolist() == [0, 1] and nf.tolist() == [1, 1] and it == 1 and np.array_equal(df, [[0, 16], [16, 0]])


def test_tie_goes_to_the_lower_index():
    z = np.array([[0.0], [2.0]])
    c = np.array([[1.0], [-1.0], [1.0], [3.0]])
    d, lab = assign_ref(z, c)
    assert d[0].tolist() == [1.0, 1.0, 1.0, 9.0] and d[1].tolist() == [1.0, 9.0, 1.0, 1.0]
    assert lab.tolist() == [0, 0]


def test_empty_cluster_keeps_its_centroid_and_bad_labels_are_skipped():
    z = np.array([[1.0, 2.0], [3.0, 4.0], [100.0, 100.0], [7.0, 7.0]])
    c = np.array([[0.0, 0.0], [9.0, 9.0], [5.0, 5.0]])
    m, cnt = update_ref(z, np.array([0, 0, -1, 3]), c)
    assert cnt.tolist() == [2, 0, 0]
    assert np.array_equal(m, [[2.0, 3.0], [9.0, 9.0], [5.0, 5.0]])


def test_nan_row():
    z = np.array([[0.0, 0.0], [np.nan, 0.0], [1.0, np.inf], [1.0, 1.0]])
    c = np.array([[0.0, 0.0], [1.0, 1.0]])
    d, lab = assign_ref(z, c)
    assert lab.tolist() == [0, -1, -1, 1]
    assert np.isnan(d[1]).all() and np.isnan(d[2]).all() and np.array_equal(d[[0, 3]], [[0.0, 2.0], [2.0, 0.0]])
    m, cnt = update_ref(z, lab, c)
    assert cnt.tolist() == [1, 1] and np.array_equal(m, c)


def test_bounds_are_what_they_say():
    z = np.array([[3.0, 4.0]])
    c = np.array([[0.0, 1.0], [0.0, -2.0]])
    assert tau(z, c)[0] == 4 * 4 * 2.0 ** -24 * 49.0
    b = update_bound(np.array([[1.0, -2.0], [3.0, 4.0], [9.0, 9.0]]), np.array([0, 0, 2]), 3)
    assert np.array_equal(b[0], 3 * 2.0 ** -24 * np.array([4.0, 6.0]) / 2) and np.isinf(b[1]).all()


def test_blob_recipe_margins():
    """The recipe of the exact-trajectory GPU test: along the reference trajectory every row's margin exceeds 100 tau."""
    for n, width, k in ((3000, 64, 10), (1000, 3, 4)):
        z, ids, init = blobs(n, width, k, seed=n + width)
        trace = []
        c, lab, d, cnt, it = fit_ref(z, init, trace=trace)
        assert np.array_equal(lab, ids) and it >= 1
        for dd, ll, cc in trace:
            s = np.sort(dd, axis=1)
            assert ((s[:, 1] - s[:, 0]) > 100 * tau(z, cc)).all()


# ---------------------------------------------------------------------------------------------------- report helpers
def test_cluster_class_table_and_names():
    clusters = torch.tensor([[0, 0, 1], [2, -1, 5], [1, 1, 0]])
    classes = torch.tensor([[1, 1, 0], [9, 0, 0], [-1, 0, 1]])
    t = report.cluster_class_table(clusters, classes, 4, 2)
    assert t.dtype == torch.int64 and t.tolist() == [[0, 3], [2, 0], [0, 0], [0, 0]]
    assert report.name_clusters(t).tolist() == [1, 0, -1, -1]
    # a tie names the lowest class; uint8 class labels (window_labels' raster values) are taken as they are
    t2 = report.cluster_class_table(torch.tensor([0, 0, 1]), torch.tensor([2, 1, 255], dtype=torch.uint8), 2, 3)
    assert t2.tolist() == [[0, 1, 1], [0, 0, 0]] and report.name_clusters(t2).tolist() == [1, -1]
    assert eae_amd.cluster_class_table is report.cluster_class_table and eae_amd.name_clusters is report.name_clusters
    with pytest.raises(ValueError):
        report.cluster_class_table(torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), 2, 2)
    with pytest.raises(ValueError):
        report.cluster_class_table(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), 0, 2)


# ---------------------------------------------------------------------------------------------------- C ABI, host only
def test_workspace_bytes():
    lib = _lib.load()
    for n, width, k in ((1, 1, 1), (1000, 64, 10), (1 << 20, 64, 256), (2 ** 31 - 1, 256, 256), (5, 3, 2)):
        b = lib.eae_kmeans_workspace_bytes(n, width, k)
        assert b > 0 and b % 4 == 0, (n, width, k, b)
    assert lib.eae_kmeans_workspace_bytes(1 << 20, 64, 256) <= 64 << 20
    for n, width, k in ((0, 64, 10), (-5, 64, 10), (2 ** 31, 64, 10), (100, 0, 10), (100, 257, 10), (100, 64, 0), (100, 64, 257)):
        assert lib.eae_kmeans_workspace_bytes(n, width, k) < 0, (n, width, k)
        assert b"kmeans" in lib.eae_last_error()


def test_null_and_range_arguments_are_rejected_before_any_launch():
    """EAE_ERR_ARG comes from the host-side checks: no device is touched (this test runs without one)."""
    lib = _lib.load()
    p = 0x1000          # never dereferenced on the host
    assert lib.eae_kmeans_assign(None, None, 10, 4, p, 2, p, 0, None, None) == -2
    assert lib.eae_kmeans_assign(None, p, 10, 4, None, 2, p, 0, None, None) == -2
    assert lib.eae_kmeans_assign(None, p, 10, 4, p, 2, None, 0, None, None) == -2
    for n, width, k in ((0, 4, 2), (2 ** 31, 4, 2), (10, 0, 2), (10, 257, 2), (10, 4, 0), (10, 4, 257)):
        assert lib.eae_kmeans_assign(None, p, n, width, p, k, p, 0, None, None) == -2
        assert lib.eae_kmeans_update(None, p, n, width, p, k, p, p, p, 1 << 40) == -2
    need = lib.eae_kmeans_workspace_bytes(10, 4, 2)
    assert lib.eae_kmeans_update(None, p, 10, 4, p, 2, p, p, None, need) == -2
    assert lib.eae_kmeans_update(None, p, 10, 4, p, 2, p, p, p, need - 1) == -2
    assert b"workspace" in lib.eae_last_error()
    for missing in range(4):
        args = [p, p, p, p]
        args[missing] = None
        assert lib.eae_kmeans_update(None, args[0], 10, 4, args[1], 2, args[2], args[3], p, need) == -2


# ---------------------------------------------------------------------------------------------------- Python rejections
def _z(n=20, width=8):
    return torch.zeros((n, width), dtype=torch.float32)


@pytest.mark.parametrize("kwargs", [
    dict(k=0), dict(k=257), dict(k=21), dict(k=2.0), dict(k=True), dict(k=3, max_iter=-1), dict(k=3, max_iter=1.5), dict(k=3, tol=-0.1),
    dict(k=3, tol=1.0), dict(k=3, init="random"), dict(k=3, init=torch.zeros((3, 7))), dict(k=3, init=torch.zeros((3, 8), dtype=torch.float64)),
    dict(k=3, init=torch.zeros((21, 8))), dict(k=3, init=torch.zeros(8))])
def test_kmeans_fit_rejections(kwargs):
    with pytest.raises(RuntimeError) as e:
        eae_amd.kmeans_fit(_z(), **kwargs)
    assert "HIP device" not in str(e.value)


def test_latent_and_centroid_rejections():
    for bad in (torch.zeros(8), torch.zeros((4, 8), dtype=torch.float64), torch.zeros((4, 257)), torch.zeros((0, 8)), np.zeros((4, 8))):
        with pytest.raises(RuntimeError) as e:
            eae_amd.kmeans_fit(bad, 2)
        assert "HIP device" not in str(e.value)
    for c in (torch.zeros((2, 7)), torch.zeros((257, 8)), torch.zeros((2, 8), dtype=torch.float16), torch.zeros(8)):
        with pytest.raises(RuntimeError) as e:
            eae_amd.kmeans_predict(_z(), c)
        assert "HIP device" not in str(e.value)
    with pytest.raises(RuntimeError) as e:
        eae_amd.kmeans_init(_z(), 21)
    assert "HIP device" not in str(e.value)
    # with everything in order the one thing missing is the device
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.kmeans_fit(_z(), 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.kmeans_predict(_z(), torch.zeros((2, 8)))


def test_cluster_scene_rejections():
    model = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3)
    scene = torch.zeros((3, 160, 224), dtype=torch.uint8)                   # a 2 x 3 grid at the default stride
    ok_c = torch.zeros((4, 64))
    bad = [dict(), dict(k=0), dict(k=257), dict(k=7), dict(k=2, windows=torch.tensor([0])), dict(k=2, windows=torch.tensor([0.5, 1.0])),
           dict(centroids=torch.zeros((4, 32))), dict(centroids=ok_c.double()), dict(centroids=torch.zeros((0, 64))),
           dict(k=2, windows=torch.tensor([0, 1]), nodata=0), dict(k=2, stride=65), dict(k=2, border="wrap"), dict(k=2, rule="some"),
           dict(k=2, max_invalid=1.0), dict(k=2, nodata=0.5), dict(k=2, mask=torch.zeros((5, 5), dtype=torch.bool)),
           dict(k=2, max_iter=-1), dict(k=2, tol=2.0), dict(centroids=ok_c, windows=torch.zeros(0, dtype=torch.int64))]
    for kw in bad:
        with pytest.raises(RuntimeError) as e:
            eae_amd.cluster_scene(scene, model, **kw)
        assert "HIP device" not in str(e.value), kw
    with pytest.raises(RuntimeError) as e:
        eae_amd.cluster_scene(scene, torch.nn.Linear(2, 2), k=2)
    assert "Encoder" in str(e.value)
    with pytest.raises(RuntimeError) as e:
        eae_amd.cluster_scene(torch.zeros((3, 160, 224), dtype=torch.int32), model, k=2)
    assert "dtype" in str(e.value)
    # a border grid has more windows: k = 7 fits the 3 x 4 grid that covers the scene
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.cluster_scene(scene, model, k=7, border="reflect")
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.cluster_scene(scene, model, centroids=ok_c)
