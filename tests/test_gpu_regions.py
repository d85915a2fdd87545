"""Map post-processing on the device (eae_amd.postprocess; include/eae.h, "map post-processing") against the NumPy restatement of
its semantics (tests/regions_ref.py).  Every output is an integer array that the semantics define uniquely -- a region's id is the
smallest linear index of its cells, every tie has a rule -- so every comparison is `torch.equal`: there is no tolerance.

The labelling kernel works on 32 x 32 tiles and the statistics kernel on 64-cell row segments, so the map sizes sit around 32 and 64
(and 1 x 1, one row, one column); the largest, 129 x 257, has 5 x 9 tiles.  Each case of `label_regions` runs twice and must give the
same bits: the merge across tile borders is a race of atomics whose outcome must not depend on who arrives first."""
import functools

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
import regions_ref as R
from scene_util import _model, _mlp

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 70), (70, 1), (31, 33), (32, 32), (33, 31), (32, 64), (63, 65), (64, 64), (65, 63), (64, 33), (129, 257)]
#            name: (maker, K)
PATTERNS = {"one_class": (R.one_class, 3), "checkerboard": (R.checkerboard, 2), "h_stripes": (R.h_stripes, 3),
            "v_stripes": (R.v_stripes, 3), "serpentine": (R.serpentine, 2), "spiral": (R.spiral, 2), "u_shapes": (R.u_shapes, 3),
            "diagonals": (R.diagonals, 2), "percolation": (R.percolation, 2), "ten_class": (R.ten_class, 10)}


@functools.lru_cache(maxsize=None)
def _map(name, h, w):
    m = PATTERNS[name][0](h, w)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _regions_ref(name, h, w, conn):
    r = R.label_regions_ref(_map(name, h, w), PATTERNS[name][1], conn)
    r.setflags(write=False)
    return r


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # (a copy: the cached maps are read-only)


def _same(got, ref):
    return torch.equal(got.cpu(), torch.from_numpy(np.ascontiguousarray(ref)))


# ---------------------------------------------------------------------------------------------------- label_regions
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("name", list(PATTERNS))
def test_label_regions(name, h, w):
    k = PATTERNS[name][1]
    labels = _dev(_map(name, h, w))
    for conn in (4, 8):
        got = eae_amd.label_regions(labels, k, connectivity=conn)
        assert got.dtype == torch.int64 and tuple(got.shape) == (h, w)
        assert _same(got, _regions_ref(name, h, w, conn)), (name, h, w, conn)
        again = eae_amd.label_regions(labels, k, connectivity=conn)
        assert torch.equal(again, got)


def test_the_patterns_are_what_they_claim():
    """The single regions the patterns are built for, on the device: long chains across every tile border."""
    h, w = 129, 257
    one = eae_amd.label_regions(_dev(_map("one_class", h, w)), 3)
    assert int(one.min()) == 0 == int(one.max())
    for name in ("serpentine", "spiral"):
        m = _map(name, h, w)
        r = eae_amd.label_regions(_dev(m), 2).cpu().numpy()
        assert np.unique(r[m == 1]).tolist() == [0], name
    cb4 = eae_amd.label_regions(_dev(_map("checkerboard", h, w)), 2, 4)
    assert torch.equal(cb4.cpu(), torch.arange(h * w).reshape(h, w))
    cb8 = eae_amd.label_regions(_dev(_map("checkerboard", h, w)), 2, 8)
    assert torch.unique(cb8).tolist() == [0, 1]


def test_views_and_the_c_entry_checks():
    """A non-contiguous view is read as what it shows; a NULL or short workspace is an argument error and launches nothing."""
    m = _map("ten_class", 65, 63)
    wide = _dev(np.repeat(m, 2, axis=1))
    view = wide[:, ::2]
    assert not view.is_contiguous()
    assert _same(eae_amd.label_regions(view, 10, 8), _regions_ref("ten_class", 65, 63, 8))
    lib = _lib.load()
    labels = _dev(m)
    out = torch.full_like(labels, -7)
    ws = torch.empty(65 * 63 * 8, dtype=torch.uint8, device="cuda")
    assert lib.eae_map_regions(_stream(), _ptr(labels), 65, 63, 10, 4, _ptr(out), None, 0) == -2
    assert lib.eae_map_regions(_stream(), _ptr(labels), 65, 63, 10, 4, _ptr(out), _ptr(ws), ws.numel() - 1) == -2
    assert b"workspace" in lib.eae_last_error()
    assert lib.eae_map_regions(_stream(), _ptr(labels), 65, 63, 10, 6, _ptr(out), _ptr(ws), ws.numel()) == -2
    assert lib.eae_map_regions(_stream(), _ptr(labels), 65, 63, 65, 4, _ptr(out), _ptr(ws), ws.numel()) == -2
    assert lib.eae_map_majority(_stream(), _ptr(labels), 65, 63, 10, 1, 0, _ptr(labels)) == -2          # in == out
    assert lib.eae_map_majority(_stream(), _ptr(labels), 65, 63, 10, 8, 0, _ptr(out)) == -2
    torch.cuda.synchronize()
    assert int((out != -7).sum()) == 0
    assert lib.eae_map_regions(_stream(), _ptr(labels), 65, 63, 10, 4, _ptr(out), _ptr(ws), ws.numel()) == 0
    assert _same(out, _regions_ref("ten_class", 65, 63, 4))


# ---------------------------------------------------------------------------------------------------- region_table
@pytest.mark.parametrize("name,h,w,conn", [("ten_class", 65, 63, 4), ("ten_class", 129, 257, 8), ("percolation", 64, 64, 4),
                                           ("u_shapes", 63, 65, 4), ("spiral", 33, 31, 8), ("one_class", 129, 257, 4),
                                           ("h_stripes", 70, 1, 4), ("v_stripes", 1, 70, 4), ("one_class", 1, 1, 4)])
def test_region_table(name, h, w, conn):
    m, k = _map(name, h, w), PATTERNS[name][1]
    labels = _dev(m)
    regions = eae_amd.label_regions(labels, k, conn)
    t = eae_amd.region_table(labels, regions)
    ref = R.region_table_ref(m, _regions_ref(name, h, w, conn))
    assert int(t["area"].sum()) == int(R.classified(m, k).sum())
    for key in ("id", "cls", "area", "bbox"):
        assert t[key].dtype == torch.int64 and t[key].device == labels.device
        assert _same(t[key], ref[key]), key
    assert tuple(t["bbox"].shape) == (len(ref["id"]), 4)


# ---------------------------------------------------------------------------------------------------- majority_filter
def _classes_map(h, w, k, seed):
    """Noisy 3 x 3 patches of the classes of [0, k) with -1 holes (k = 1: zeros and holes); k = 64: every cell its own draw, with
    -1, k and k + 5 among them."""
    return R.blobs(h, w, seed=seed, k=k) if k < 64 else R.ten_class(h, w, seed=seed, k=k)


#           (h, w, K, radius, fill, passes)
MAJORITY = [(33, 65, 10, 1, False, 1), (33, 65, 10, 1, True, 3), (65, 63, 10, 3, True, 1), (65, 63, 10, 3, False, 3),
            (40, 70, 64, 1, False, 1), (40, 70, 64, 3, True, 1), (31, 33, 1, 1, True, 1), (31, 33, 1, 1, False, 3),
            (5, 5, 3, 7, True, 1), (5, 5, 3, 7, False, 3), (1, 70, 10, 1, True, 1), (70, 1, 10, 3, False, 1), (1, 1, 10, 7, True, 1),
            (129, 257, 10, 1, False, 1)]


@pytest.mark.parametrize("h,w,k,radius,fill,passes", MAJORITY)
def test_majority_filter(h, w, k, radius, fill, passes):
    m = _classes_map(h, w, k, seed=h + w + radius)
    got = eae_amd.majority_filter(_dev(m), k, radius=radius, fill=fill, passes=passes)
    assert _same(got, R.majority_ref(m, k, radius, fill, passes))


def test_majority_ties_and_stored_values():
    """The constructed ties of tests/test_regions_reference.py, and unclassified values of every kind kept as stored."""
    cases = [([[0, 0, 0], [0, 1, 1], [1, 1, -1]], 2), ([[3, 3, 3], [3, 5, 2], [2, 2, 2]], 6), ([[4, 4, 4], [4, 1, 1], [4, 1, 0]], 5),
             ([[0, 0, 9], [9, 9, 9], [9, 1, 1]], 3), ([[1, 0, 0], [0, 0, 0], [0, 0, 2]], 3),
             ([[-1, -1, -1, -1], [-1, -1, -1, -1], [-1, -1, 3, -1], [-1, -1, -1, -1]], 4),
             ([[2 ** 40, -2 ** 40, 7], [64, 0, 2 ** 32], [-1, 1, 1]], 2)]
    for rows, k in cases:
        m = np.asarray(rows, dtype=np.int64)
        for fill in (False, True):
            for passes in (1, 2):
                got = eae_amd.majority_filter(_dev(m), k, fill=fill, passes=passes)
                assert _same(got, R.majority_ref(m, k, 1, fill, passes)), (rows, fill, passes)


# ---------------------------------------------------------------------------------------------------- sieve
#        (h, w, min_size, connectivity, passes)
SIEVE = [(65, 63, 2, 4, 1), (65, 63, 5, 4, 1), (65, 63, 5, 8, 1), (65, 63, 5, 4, 3), (65, 63, 2, 8, 3), (33, 70, 5, 8, 3),
         (129, 257, 5, 4, 1), (1, 70, 3, 4, 1), (70, 1, 3, 8, 3), (64, 64, 12, 4, 3)]


@pytest.mark.parametrize("h,w,min_size,conn,passes", SIEVE)
def test_sieve(h, w, min_size, conn, passes):
    m = R.blobs(h, w, seed=h * w + min_size)
    ref, ref_changed = R.sieve_ref(m, 10, min_size, conn, passes)
    got, changed = eae_amd.sieve(_dev(m), 10, min_size, connectivity=conn, passes=passes, return_changed=True)
    assert _same(got, ref)
    assert changed.dtype == torch.int64 and changed.device.type == "cuda" and int(changed) == ref_changed
    assert passes > 1 or ref_changed > 0
    assert torch.equal(eae_amd.sieve(_dev(m), 10, min_size, connectivity=conn, passes=passes), got)


@pytest.mark.parametrize("conn", [4, 8])
def test_sieve_identity_cases(conn):
    m = R.blobs(63, 65, seed=9)
    labels = _dev(m)
    same, changed = eae_amd.sieve(labels, 10, 1, connectivity=conn, return_changed=True)
    assert torch.equal(same, labels) and int(changed) == 0 and same.data_ptr() != labels.data_ptr()
    # nothing is large enough to receive
    same, changed = eae_amd.sieve(labels, 10, m.size + 1, connectivity=conn, passes=3, return_changed=True)
    assert torch.equal(same, labels) and int(changed) == 0


def test_sieve_constructed_cases():
    """The worked example, equal areas (the lowest region id wins), small regions enclosed by -1 or by small regions, a diagonal
    touch, and the second pass that lets a merged region receive."""
    cases = [([[0, 0, 0, 2], [0, 1, 0, 2], [0, 0, 0, 3]], 4, 3),
             ([[1, 1, 2, 2], [1, 1, 2, 2], [3, 5, 5, 3], [3, 3, 3, 3]], 6, 3),
             ([[1, 1, 1, 2, 2], [1, 5, 5, 5, 2], [3, 3, 3, 2, 2], [3, 3, 0, 0, 0]], 6, 4),
             ([[4, 4, -1, 0, 0], [-1, -1, -1, 0, 0], [2, -1, 0, 0, 0], [-1, -1, 0, 0, 1]], 5, 3),
             ([[1, -1, 0], [-1, 0, 0], [0, 0, 0]], 2, 2),
             ([[2, 2, 2, 1, 0, 0], [3, 3, 3, 1, 0, 0]], 4, 4),
             ([[7, 7, 7], [7, 7, 7]], 8, 100)]
    for rows, k, min_size in cases:
        m = np.asarray(rows, dtype=np.int64)
        for conn in (4, 8):
            for passes in (1, 2):
                ref, ref_changed = R.sieve_ref(m, k, min_size, conn, passes)
                got, changed = eae_amd.sieve(_dev(m), k, min_size, connectivity=conn, passes=passes, return_changed=True)
                assert _same(got, ref) and int(changed) == ref_changed, (rows, conn, passes)
    # a tie between two neighbours of equal area at many places of a larger map: 2 x 2 blocks of classes 1 and 2 between pairs of 0s
    y, x = np.mgrid[:66, :66]
    m = np.where((y % 3 == 2) | (x % 3 == 2), 0, 1 + ((y // 3 + x // 3) & 1)).astype(np.int64)
    m[(y % 3 == 2) & (x % 3 == 2)] = -1                        # holes at the crossings: the 0s between two blocks are pairs
    ref, ref_changed = R.sieve_ref(m, 3, 3)
    assert ref_changed == (m == 0).sum() > 1000
    got, changed = eae_amd.sieve(_dev(m), 3, 3, return_changed=True)
    assert _same(got, ref) and int(changed) == ref_changed


# ---------------------------------------------------------------------------------------------------- end to end
def test_clean_a_classified_scene_and_score_it():
    """classify_scene -> majority_filter -> sieve -> scene_confusion, nothing leaving the device in between."""
    g = torch.Generator().manual_seed(7)
    scene = torch.randint(0, 256, (3, 256, 256), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    model, mlp = _model(3, batch=64), _mlp()
    _, labels = eae_amd.classify_scene(scene, model, mlp, divisor=255.0, stride=16, batch=64, blend=True)
    assert labels.dtype == torch.int64 and tuple(labels.shape) == (16, 16)
    smooth = eae_amd.majority_filter(labels, 10)
    clean = eae_amd.sieve(smooth, 10, 4)
    lab = labels.cpu().numpy()
    ref_smooth = R.majority_ref(lab, 10)
    assert _same(smooth, ref_smooth)
    assert _same(clean, R.sieve_ref(ref_smooth, 10, 4)[0])
    truth = torch.randint(0, 10, (256, 256), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    cm = eae_amd.scene_confusion(clean, truth, 10, cell=16, origin=(0, 0))
    assert int(cm.sum()) == 256 * 256
