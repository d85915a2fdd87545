"""Map post-processing without a GPU: the NumPy reference (tests/regions_ref.py) on the worked example and on hand-written cases for
every tie rule, the host checks of eae_amd.postprocess (they come before the device is asked for), and the host-only
`eae_map_workspace_bytes`.  Where scipy is installed the reference's partition is checked against `scipy.ndimage.label`."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib, postprocess as PP
import regions_ref as R

A = lambda rows: np.asarray(rows, dtype=np.int64)      # noqa: E731


# ---------------------------------------------------------------------------------------------------- regions
def test_regions_ids_are_the_smallest_linear_index():
    m = A([[0, 0, 1, 1],
           [1, 0, 1, 0],
           [1, 1, -1, 0],
           [7, 1, 0, 0]])
    r4 = R.label_regions_ref(m, 3, 4)
    assert r4.tolist() == [[0, 0, 2, 2],
                           [4, 0, 2, 7],
                           [4, 4, -1, 7],
                           [-1, 4, 7, 7]]
    r8 = R.label_regions_ref(m, 3, 8)
    # at 8-connectivity the 1s join through the corner (1, 2) - (2, 1); the two 0 regions touch nowhere
    assert r8.tolist() == [[0, 0, 2, 2],
                           [2, 0, 2, 7],
                           [2, 2, -1, 7],
                           [-1, 2, 7, 7]]
    t = R.region_table_ref(m, r4)
    assert t["id"].tolist() == [0, 2, 4, 7] and t["cls"].tolist() == [0, 1, 1, 0] and t["area"].tolist() == [3, 3, 4, 4]
    assert t["bbox"].tolist() == [[0, 0, 1, 1], [0, 2, 1, 3], [1, 0, 3, 1], [1, 2, 3, 3]]
    assert t["area"].sum() == R.classified(m, 3).sum()


def test_checkerboard_and_diagonals_differ_between_connectivities():
    c = R.checkerboard(5, 6)
    assert np.array_equal(R.label_regions_ref(c, 2, 4), np.arange(30).reshape(5, 6))
    assert np.unique(R.label_regions_ref(c, 2, 8)).tolist() == [0, 1]
    d = R.diagonals(6, 6)
    ones = d == 1
    assert np.array_equal(R.label_regions_ref(d, 2, 4)[ones], np.flatnonzero(ones))
    assert np.unique(R.label_regions_ref(d, 2, 8)[ones]).size == 3          # the main diagonal and the two at distance 4


@pytest.mark.parametrize("make", [R.serpentine, R.spiral])
@pytest.mark.parametrize("h,w", [(9, 11), (33, 40), (64, 35)])
def test_the_long_paths_are_one_region_of_class_1(make, h, w):
    m = make(h, w)
    r = R.label_regions_ref(m, 2, 4)
    assert np.unique(r[m == 1]).tolist() == [0]
    assert (m == 1).sum() > (h * w) // 3
    if make is R.spiral:
        assert np.unique(r[m == 0]).size == 1                               # the gap is one path as well


def test_u_shapes_join_only_at_the_bottom():
    m = R.u_shapes(40, 37)
    r = R.label_regions_ref(m, 3, 4)
    assert r[0, 0] == r[0, 36] == 0 and r[0, 2] == r[0, 34] == 2
    assert np.unique(R.label_regions_ref(m[:20], 3, 4)[0, [0, 36]]).size == 2     # cut above the joint: two regions


def test_partition_matches_scipy_ndimage_label():
    ndi = pytest.importorskip("scipy.ndimage")
    for m, k in ((R.percolation(37, 45, seed=1), 2), (R.ten_class(33, 29, seed=2), 10), (R.spiral(21, 23), 2), (R.diagonals(18, 31), 2)):
        for conn, structure in ((4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), (8, np.ones((3, 3), dtype=int))):
            ref = R.label_regions_ref(m, k, conn)
            assert np.array_equal(ref < 0, ~R.classified(m, k))
            total = 0
            for c in range(k):
                lab, n = ndi.label(m == c, structure=structure)
                total += n
                for i in range(1, n + 1):
                    cells = lab == i
                    ids = np.unique(ref[cells])
                    assert ids.size == 1 and ids[0] == np.flatnonzero(cells)[0]          # one id: the smallest linear index
                    assert (ref == ids[0]).sum() == cells.sum()
            assert np.unique(ref[ref >= 0]).size == total


# ---------------------------------------------------------------------------------------------------- majority filter
def test_majority_ties():
    # the centre's class wins a tie it is part of: 0 and 1 hold 4 cells each of the window around the centre 1 (the -1 counts nowhere)
    m = A([[0, 0, 0],
           [0, 1, 1],
           [1, 1, -1]])
    assert R.majority_ref(m, 2)[1, 1] == 1
    # the centre is not among the tied classes: the lowest id of them wins (2 and 3 hold 4 each, the centre 5 one)
    m = A([[3, 3, 3],
           [3, 5, 2],
           [2, 2, 2]])
    assert R.majority_ref(m, 6)[1, 1] == 2
    # a clear majority beats the centre
    m = A([[4, 4, 4],
           [4, 1, 1],
           [4, 1, 0]])
    assert R.majority_ref(m, 5)[1, 1] == 4
    # a value >= K is unclassified: it is not counted and, without fill, stays as stored
    m = A([[0, 0, 9],
           [9, 9, 9],
           [9, 1, 1]])
    out = R.majority_ref(m, 3)
    assert out[1, 1] == 9 and out[0, 0] == 0 and out[2, 2] == 1
    filled = R.majority_ref(m, 3, fill=True)
    assert filled[1, 1] == 0                                     # 0 and 1 tie with two cells each; the centre is no class: lowest id
    assert filled[2, 0] == 1 and filled[0, 2] == 0


def test_majority_unclassified_centre_fill_and_clipping():
    m = A([[-1, -1, -1, -1],
           [-1, -1, -1, -1],
           [-1, -1, 3, -1],
           [-1, -1, -1, -1]])
    assert np.array_equal(R.majority_ref(m, 4), m)               # nothing to fill with fill=False; the lone 3 keeps itself
    f1 = R.majority_ref(m, 4, fill=True)
    assert (f1 == 3).sum() == 9 and f1[0, 0] == -1 and f1[0, 1] == -1           # row 0 and column 0 are out of reach
    f2 = R.majority_ref(m, 4, fill=True, passes=2)
    assert (f2 == 3).all()
    assert np.array_equal(f2, R.majority_ref(f1, 4, fill=True))                 # passes chain: Jacobi, two buffers
    # radius 7 on a 5 x 5 map: every window is the whole map
    m5 = R.blobs(5, 5, seed=3, k=3)
    vals, cnt = np.unique(m5[R.classified(m5, 3)], return_counts=True)
    if (cnt == cnt.max()).sum() == 1:
        assert (R.majority_ref(m5, 3, radius=7, fill=True) == vals[cnt.argmax()]).all()


def test_majority_corner_window_is_clipped():
    m = A([[1, 0, 0],
           [0, 0, 0],
           [0, 0, 2]])
    out = R.majority_ref(m, 3)
    assert out[0, 0] == 0                                        # 3 zeros against the corner's single 1 in the 2 x 2 window
    assert out[2, 2] == 0


# ---------------------------------------------------------------------------------------------------- sieve
def test_sieve_worked_example():
    m = A([[0, 0, 0, 2],
           [0, 1, 0, 2],
           [0, 0, 0, 3]])
    out, changed = R.sieve_ref(m, 4, 3)
    assert (out == 0).all() and changed == 4
    same, none = R.sieve_ref(m, 4, 1)
    assert np.array_equal(same, m) and none == 0
    # min_size above the map's size: nothing is large enough to receive
    same, none = R.sieve_ref(m, 4, m.size + 1)
    assert np.array_equal(same, m) and none == 0


def test_sieve_ties_largest_area_then_lowest_id():
    # the 5 in the middle borders 1 (area 4, id 0), 2 (area 4, id 2) and 3 (area 6): the largest wins
    m = A([[1, 1, 2, 2],
           [1, 1, 2, 2],
           [3, 5, 5, 3],
           [3, 3, 3, 3]])
    out, changed = R.sieve_ref(m, 6, 3)
    assert out[2, 1] == 3 and out[2, 2] == 3 and changed == 2
    # equal areas: the lowest region id wins (the 5s border 1 with area 4, and 2 at id 3 and 3 at id 10 with area 5 each)
    m = A([[1, 1, 1, 2, 2],
           [1, 5, 5, 5, 2],
           [3, 3, 3, 2, 2],
           [3, 3, 0, 0, 0]])
    t = R.region_table_ref(m, R.label_regions_ref(m, 6))
    assert dict(zip(t["id"].tolist(), t["area"].tolist())) == {0: 4, 3: 5, 6: 3, 10: 5, 17: 3}
    out, _ = R.sieve_ref(m, 6, 4)
    assert (out[1, 1:4] == 2).all()                              # areas 5 and 5: id 3 (class 2) before id 10 (class 3)
    assert (out[3, 2:] == 2).all()                               # the 0s border both as well


def test_sieve_small_neighbours_unclassified_and_diagonals():
    # a small region whose only classified neighbour is small too stays (rule 5); one enclosed by -1 stays
    m = A([[4, 4, -1, 0, 0],
           [-1, -1, -1, 0, 0],
           [2, -1, 0, 0, 0],
           [-1, -1, 0, 0, 1]])
    out, changed = R.sieve_ref(m, 5, 3)
    assert out[0, 0] == 4 and out[2, 0] == 2 and out[3, 4] == 0 and changed == 1
    assert np.array_equal(out == -1, m == -1)
    # a diagonal touch is no neighbour, at 8-connectivity as well: the 1 at (0, 0) touches the 0 field only by its corner
    m = A([[1, -1, 0],
           [-1, 0, 0],
           [0, 0, 0]])
    for conn in (4, 8):
        out, changed = R.sieve_ref(m, 2, 2, connectivity=conn)
        assert np.array_equal(out, m) and changed == 0
    # a region that covers the whole map has no neighbour
    m = R.one_class(3, 4)
    assert np.array_equal(R.sieve_ref(m, 3, 100)[0], m)


def test_sieve_second_pass_lets_a_merged_region_receive():
    # pass 1: the 1s (area 2) take the class of the 0s (area 4); the 2s and 3s (area 3 each) have no neighbour that is large enough
    # until the merged 0 region (area 6) touches them in pass 2
    m = A([[2, 2, 2, 1, 0, 0],
           [3, 3, 3, 1, 0, 0]])
    p1, c1 = R.sieve_ref(m, 4, 4)
    assert p1.tolist() == [[2, 2, 2, 0, 0, 0], [3, 3, 3, 0, 0, 0]] and c1 == 2
    p2, c2 = R.sieve_ref(m, 4, 4, passes=2)
    assert (p2 == 0).all() and c2 == 6
    assert np.array_equal(p2, R.sieve_ref(p1, 4, 4)[0])


def test_sieve_connectivity_changes_what_is_small():
    d = R.diagonals(8, 8)
    out4, _ = R.sieve_ref(d, 2, 2, connectivity=4)
    out8, _ = R.sieve_ref(d, 2, 2, connectivity=8)
    assert (out4 == 0).sum() > (d == 0).sum()                    # singletons at 4-connectivity dissolve
    assert (out8[d == 1] == 1).sum() >= 8                        # the long diagonals are regions of >= 2 cells at 8-connectivity


# ---------------------------------------------------------------------------------------------------- host checks (no device)
def _ok():
    return torch.zeros((4, 5), dtype=torch.int64)


def test_exports():
    for name in ("majority_filter", "label_regions", "region_table", "sieve"):
        assert name in eae_amd.__all__ and getattr(eae_amd, name) is getattr(PP, name)


@pytest.mark.parametrize("bad", [None, np.zeros((4, 5), dtype=np.int64), torch.zeros((4, 5), dtype=torch.int32),
                                 torch.zeros((4, 5)), torch.zeros(20, dtype=torch.int64), torch.zeros((1, 4, 5), dtype=torch.int64),
                                 torch.zeros((0, 5), dtype=torch.int64), torch.zeros((4, 0), dtype=torch.int64)])
def test_every_function_rejects_a_bad_map(bad):
    for call in (lambda: PP.majority_filter(bad, 3), lambda: PP.label_regions(bad, 3), lambda: PP.sieve(bad, 3, 2),
                 lambda: PP.region_table(bad, _ok()), lambda: PP.region_table(_ok(), bad)):
        with pytest.raises(RuntimeError, match="int64 map|is empty"):
            call()


def test_too_many_cells_are_rejected():
    big = torch.zeros(1, dtype=torch.int64).expand(2 ** 16, 2 ** 15)       # 2^31 cells over one element of storage
    for call in (lambda: PP.majority_filter(big, 3), lambda: PP.label_regions(big, 3), lambda: PP.sieve(big, 3, 2),
                 lambda: PP.region_table(big, big)):
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            call()


@pytest.mark.parametrize("k", [0, 65, -1, 2.0, True, None])
def test_num_classes_outside_1_to_64(k):
    for call in (lambda: PP.majority_filter(_ok(), k), lambda: PP.label_regions(_ok(), k), lambda: PP.sieve(_ok(), k, 2)):
        with pytest.raises(RuntimeError, match="num_classes"):
            call()


def test_scalar_arguments():
    for r in (0, 8, -1, 1.5):
        with pytest.raises(RuntimeError, match="radius"):
            PP.majority_filter(_ok(), 3, radius=r)
    for c in (0, 1, 6, 16, "4", True):
        with pytest.raises(RuntimeError, match="connectivity"):
            PP.label_regions(_ok(), 3, connectivity=c)
        with pytest.raises(RuntimeError, match="connectivity"):
            PP.sieve(_ok(), 3, 2, connectivity=c)
    for s in (0, -3, 2.5):
        with pytest.raises(RuntimeError, match="min_size"):
            PP.sieve(_ok(), 3, s)
    for p in (0, -1, 1.0):
        with pytest.raises(RuntimeError, match="passes"):
            PP.majority_filter(_ok(), 3, passes=p)
        with pytest.raises(RuntimeError, match="passes"):
            PP.sieve(_ok(), 3, 2, passes=p)


def test_region_table_needs_matching_maps():
    with pytest.raises(RuntimeError, match="shape"):
        PP.region_table(_ok(), torch.zeros((5, 4), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="is on"):
        PP.region_table(_ok(), torch.zeros((4, 5), dtype=torch.int64, device="meta"))


def test_valid_arguments_reach_the_device_check():
    """Everything above is rejected before the device is asked for; valid arguments on a CPU tensor get as far as that."""
    for call in (lambda: PP.majority_filter(_ok(), 64, radius=7, fill=True, passes=3), lambda: PP.label_regions(_ok(), 1, 8),
                 lambda: PP.sieve(_ok(), 10, 21, connectivity=8, passes=2, return_changed=True),
                 lambda: PP.region_table(_ok(), _ok())):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()


# ---------------------------------------------------------------------------------------------------- the host-only C entry
def test_workspace_bytes():
    lib = _lib.load()
    assert lib.eae_map_workspace_bytes(1, 1) == 8
    assert lib.eae_map_workspace_bytes(129, 257) == 129 * 257 * 8
    assert lib.eae_map_workspace_bytes(2 ** 15, 2 ** 16 - 1) == (2 ** 31 - 2 ** 15) * 8
    for h, w in ((0, 5), (5, 0), (-1, 5), (5, -7), (2 ** 16, 2 ** 15), (2 ** 31 - 1, 2)):
        assert lib.eae_map_workspace_bytes(h, w) == -2            # EAE_ERR_ARG
        assert b"2^31" in lib.eae_last_error()
