"""Zonal statistics on the device (eae_amd.zonal): `eae_zonal_accumulate` and `eae_zonal_paint` by shape against the NumPy restatement
of their semantics (tests/zonal_ref.py), the wrapper's conversions, ``out=``, regions as zones, and `classify_zones` end to end.
Integer sums: every comparison is exact equality, a second run equals the first, and in every case the votes sum to the number of
unmasked pixels whose zone id is in range."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from zonal_ref import paint_ref, q_ref, zonal_ref, zone_labels_ref
from scene_util import _model, _mlp

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


def _zones(h, w, z, seed):
    """A zone raster with runs (3 x 3 blocks of one id) and single-pixel noise: ids in [0, Z), negatives and ids >= Z."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(-1, z + 1, (-(-h // 3), -(-w // 3)))
    t = np.repeat(np.repeat(coarse, 3, 0), 3, 1)[:h, :w].astype(np.int64)
    noise = rng.random((h, w)) < 0.2
    t[noise] = rng.integers(-3, z + 70, int(noise.sum()))
    return t


def _labels(c_h, c_w, k, seed):
    """A cell map with -1 and values >= K among the classes."""
    return np.random.default_rng(seed + 1000).integers(-1, k + 2, (c_h, c_w)).astype(np.int64)


def _probs(c_h, c_w, k, seed):
    """Probabilities with exact 0 and 1, values below 2^-32 (one of them half a unit: rounds to even), a NaN and a value above 1."""
    rng = np.random.default_rng(seed + 2000)
    p = rng.random((k, c_h, c_w)).astype(np.float32)
    flat = p.reshape(-1)
    special = np.array([0.0, 1.0, 2.0 ** -33, 2.0 ** -40, 1.5 * 2.0 ** -32, np.nan, 1.75, -0.5], dtype=np.float32)
    n = min(len(special), flat.size)
    flat[rng.permutation(flat.size)[:n]] = special[:n]
    return p


def _mask(h, w, seed):
    """A third of the pixels skipped, in runs and singly."""
    rng = np.random.default_rng(seed)
    return (rng.random((h, w)) < 0.2) | (np.repeat(rng.random((h, -(-w // 8))) < 0.15, 8, 1)[:, :w])


def _accumulate(zones, labels, probs, cell, oy, ox, mask, k, z, accumulate, votes, sums):
    h, w = zones.shape
    _lib.check(_lib.load().eae_zonal_accumulate(_stream(), _ptr(zones), zones.element_size(), h, w, _ptr(labels), _ptr(probs),
                                                labels.shape[0], labels.shape[1], cell, oy, ox, _ptr(mask), k, z, accumulate,
                                                _ptr(votes), _ptr(sums)))


def _paint(zones, values, fill, out):
    h, w = zones.shape
    _lib.check(_lib.load().eae_zonal_paint(_stream(), _ptr(zones), zones.element_size(), h, w, _ptr(values), values.numel(), fill,
                                           _ptr(out)))


def _dirty(*shape):
    return torch.full(shape, -7, dtype=torch.int64, device="cuda")


def _in_range(zn, z, mask=None):
    keep = (zn >= 0) & (zn < z)
    return int(keep.sum()) if mask is None else int((keep & ~mask).sum())


#        (H, W, cell, oy, ox, cH, cW, K, Z, zone dtype)
SHAPES = [(1, 1, 1, 0, 0, 1, 1, 1, 1, I32),
          (37, 41, 5, 3, 4, 8, 9, 3, 7, I32),              # an origin inside the first cell
          (37, 41, 5, 7, 11, 8, 9, 3, 7, I64),             # an origin larger than the cell; the last rows fall off the map
          (37, 41, 5, 0, 0, 4, 5, 3, 7, I32),              # a map smaller than the raster: uncovered pixels land in column K
          (64, 257, 16, 5, 9, 5, 17, 5, 40, I64),          # odd width: every row starts at another alignment
          (5000, 1, 3, 1, 0, 1667, 1, 4, 9, I32),          # one column: 256 rows per tile
          (33, 70, 4, 1, 2, 9, 18, 64, 5, I32),            # K = 64
          (23, 19, 1, 0, 0, 23, 19, 7, 437, I32),          # every pixel its own zone: nothing merges
          (1031, 2053, 7, 2, 5, 148, 294, 10, 1, I32),     # one zone takes every add
          (2100, 4100, 16, 2, 5, 132, 257, 10, 3000, I32)]  # more tiles than workgroups: every workgroup walks a strip


def _case(h, w, c_h, c_w, k, z):
    seed = h + w
    if (h, w, z) == (23, 19, 437):
        zn = np.arange(h * w, dtype=np.int64).reshape(h, w)           # every pixel is its own zone
    elif z == 1:
        zn = np.zeros((h, w), dtype=np.int64)                         # one zone takes every add
    else:
        zn = _zones(h, w, z, seed)
    lb, pr = _labels(c_h, c_w, k, seed), _probs(c_h, c_w, k, seed)
    if z == 1:
        lb[lb >= k] = 0
        pr[k - 1] = 1.0                                               # an all-ones class
    return zn, lb, pr


@pytest.mark.parametrize("h,w,cell,oy,ox,c_h,c_w,k,z,dtype", SHAPES)
def test_accumulate_by_shape(h, w, cell, oy, ox, c_h, c_w, k, z, dtype):
    zn, lb, pr = _case(h, w, c_h, c_w, k, z)
    zones, labels, probs = torch.from_numpy(zn).to(dtype).cuda(), torch.from_numpy(lb).cuda(), torch.from_numpy(pr).cuda()
    m = _mask(h, w, h * w)
    mask = torch.from_numpy(m).cuda().view(torch.uint8)
    for mk, mdev in ((None, None), (m, mask)):
        rv, rs = zonal_ref(zn, z, lb, k, pr, cell, (oy, ox), mask=mk)
        assert rv.sum() == _in_range(zn, z, mk)                       # the reference alone
        assert np.array_equal(zonal_ref(zn, z, lb, k, None, cell, (oy, ox), mask=mk)[0], rv)
        votes, sums = _dirty(z, k + 1), _dirty(z, k)
        _accumulate(zones, labels, probs, cell, oy, ox, mdev, k, z, 0, votes, sums)
        assert int(votes.sum()) == _in_range(zn, z, mk)
        assert np.array_equal(votes.cpu().numpy(), rv) and np.array_equal(sums.cpu().numpy(), rs)
        votes2, sums2 = _dirty(z, k + 1), _dirty(z, k)
        _accumulate(zones, labels, probs, cell, oy, ox, mdev, k, z, 0, votes2, sums2)
        assert torch.equal(votes2, votes) and torch.equal(sums2, sums)
        only = _dirty(z, k + 1)                                       # without probs: the votes alone, the same
        _accumulate(zones, labels, None, cell, oy, ox, mdev, k, z, 0, only, None)
        assert torch.equal(only, votes)
        if z == 1 and h > 1 and mk is None:                           # pixels * 2^32 for the all-ones class
            classified = int(rv[0, :k].sum())
            assert classified > 0 and int(sums[0, k - 1]) == classified * 2 ** 32


@pytest.mark.parametrize("cell,ox,dtype", [(16, 0, I32), (16, 5, I64), (32, 7, I32), (40, 0, I64), (8, 0, I32)])
def test_parcel_interiors(cell, ox, dtype):
    """Large blocks of one id: a thread's open key lives through whole runs of 16 equal ids and from one row to the next -- with
    cells of 16 aligned to the runs, cells that the runs straddle, cells of several runs, cells smaller than a run, a mask of long
    runs, and a few single pixels of other zones and of no zone inside the blocks."""
    h, w, k, z = 150, 336 if ox == 0 else 333, 4, 30
    rng = np.random.default_rng(cell + ox)
    zn = np.repeat(np.repeat(rng.integers(-1, z + 2, (4, 7)), 40, 0), 50, 1)[:h, :w].astype(np.int64)
    dots = rng.random((h, w)) < 0.01
    zn[dots] = rng.integers(-2, z + 3, int(dots.sum()))
    c_h, c_w = -(-(h + 3) // cell), -(-(w + ox) // cell)
    lb, pr = _labels(c_h, c_w, k, cell), _probs(c_h, c_w, k, cell)
    m = np.repeat(rng.random((h, -(-w // 64))) < 0.3, 64, 1)[:, :w] | (rng.random((h, w)) < 0.005)
    zones, labels, probs = torch.from_numpy(zn).to(dtype).cuda(), torch.from_numpy(lb).cuda(), torch.from_numpy(pr).cuda()
    for mk, mdev in ((None, None), (m, torch.from_numpy(m).cuda().view(torch.uint8))):
        rv, rs = zonal_ref(zn, z, lb, k, pr, cell, (3, ox), mask=mk)
        votes, sums = _dirty(z, k + 1), _dirty(z, k)
        _accumulate(zones, labels, probs, cell, 3, ox, mdev, k, z, 0, votes, sums)
        assert int(votes.sum()) == _in_range(zn, z, mk) == rv.sum()
        assert np.array_equal(votes.cpu().numpy(), rv) and np.array_equal(sums.cpu().numpy(), rs)


@pytest.mark.parametrize("h,w,cell,oy,ox,c_h,c_w,k,z,dtype", SHAPES)
@pytest.mark.parametrize("fill", [-1, 2 ** 40 + 3])
def test_paint_by_shape(h, w, cell, oy, ox, c_h, c_w, k, z, dtype, fill):
    zn, _, _ = _case(h, w, c_h, c_w, k, z)
    vals = np.random.default_rng(z).integers(-2 ** 62, 2 ** 62, z)
    vals[0] = -1
    zones, values = torch.from_numpy(zn).to(dtype).cuda(), torch.from_numpy(vals).cuda()
    out = _dirty(h, w)
    _paint(zones, values, fill, out)
    assert np.array_equal(out.cpu().numpy(), paint_ref(zn, vals, fill))
    again = _dirty(h, w)
    _paint(zones, values, fill, again)
    assert torch.equal(again, out)


@pytest.mark.parametrize("h,w", [(1, 1021), (1, 1022), (1, 1023), (1, 1024), (1, 1025), (2, 1023), (3, 1365)])
@pytest.mark.parametrize("offset", [0, 1, 3])
def test_paint_around_a_workgroup_of_units(h, w, offset):
    """Rasters that end just before, at and after the 1024 ids of a workgroup, from bases 0, 1 and 3 elements off a 16-byte boundary:
    the grid holds every unit, and nothing is written outside the raster."""
    n, z = h * w, 9
    zn = np.random.default_rng(n + offset).integers(-1, z + 1, (h, w)).astype(np.int64)
    zbuf = torch.zeros(n + 8, dtype=I32, device="cuda")
    zones = zbuf[offset:offset + n].view(h, w)
    zones.copy_(torch.from_numpy(zn).to(I32))
    vals = np.arange(50, 50 + z, dtype=np.int64)
    obuf = _dirty(n + 2)
    _paint(zones, torch.from_numpy(vals).cuda(), -3, obuf[1:1 + n].view(h, w))
    assert np.array_equal(obuf[1:1 + n].view(h, w).cpu().numpy(), paint_ref(zn, vals, -3))
    assert int(obuf[0]) == -7 and int(obuf[-1]) == -7


@pytest.mark.parametrize("dtype", [I32, I64])
def test_unaligned_base_pointers(dtype):
    """The raster and the mask start at odd element offsets that differ: clipped first runs and units, whole runs whose mask bytes are
    loaded one by one; the painted raster starts 8 bytes off a 16-byte boundary."""
    h, w, cell, k, z = 19, 131, 6, 5, 11
    zn, lb, pr = _zones(h, w, z, 5), _labels(4, 22, k, 5), _probs(4, 22, k, 5)
    m = np.random.default_rng(6).random((h, w)) < 0.3
    zbuf = torch.zeros(h * w + 3, dtype=dtype, device="cuda")
    mbuf = torch.zeros(h * w + 5, dtype=torch.uint8, device="cuda")
    zones, mask = zbuf[3:].view(h, w), mbuf[5:].view(h, w)
    zones.copy_(torch.from_numpy(zn).to(dtype))
    mask.copy_(torch.from_numpy(m).to(torch.uint8))
    votes, sums = _dirty(z, k + 1), _dirty(z, k)
    _accumulate(zones, torch.from_numpy(lb).cuda(), torch.from_numpy(pr).cuda(), cell, 2, 1, mask, k, z, 0, votes, sums)
    rv, rs = zonal_ref(zn, z, lb, k, pr, cell, (2, 1), mask=m)
    assert np.array_equal(votes.cpu().numpy(), rv) and np.array_equal(sums.cpu().numpy(), rs) and rv.sum() == _in_range(zn, z, m)
    vals = np.arange(100, 100 + z, dtype=np.int64)
    obuf = _dirty(h * w + 2)
    out = obuf[1:1 + h * w].view(h, w)
    _paint(zones, torch.from_numpy(vals).cuda(), -5, out)
    assert np.array_equal(out.cpu().numpy(), paint_ref(zn, vals, -5))
    assert int(obuf[0]) == -7 and int(obuf[-1]) == -7                 # nothing written outside the raster


def test_accumulate_adds_and_a_fresh_call_clears():
    k, z = 5, 9
    z1, l1, p1 = _zones(50, 60, z, 21), _labels(7, 8, k, 21), _probs(7, 8, k, 21)
    z2, l2, p2 = _zones(31, 90, z, 22), _labels(3, 9, k, 22), _probs(3, 9, k, 22)
    r1, r2 = zonal_ref(z1, z, l1, k, p1, 8), zonal_ref(z2, z, l2, k, p2, 10, (4, 0))
    dev = lambda a, t=None: torch.from_numpy(a).cuda() if t is None else torch.from_numpy(a).to(t).cuda()
    a = eae_amd.zonal_stats(dev(z1, I32), z, dev(l1), k, probs=dev(p1), cell=8)
    assert np.array_equal(a.votes.cpu().numpy(), r1[0]) and np.array_equal(a.prob_sums.cpu().numpy(), r1[1])
    b = eae_amd.zonal_stats(dev(z2), z, dev(l2), k, probs=dev(p2), cell=10, origin=(4, 0), out=a)
    assert b is a
    assert np.array_equal(a.votes.cpu().numpy(), r1[0] + r2[0]) and np.array_equal(a.prob_sums.cpu().numpy(), r1[1] + r2[1])
    # the C call with accumulate = 0 clears dirty tables, with accumulate = 1 it adds to them
    votes, sums = _dirty(z, k + 1), _dirty(z, k)
    _accumulate(dev(z1, I32), dev(l1), dev(p1), 8, 0, 0, None, k, z, 1, votes, sums)
    assert np.array_equal(votes.cpu().numpy(), r1[0] - 7) and np.array_equal(sums.cpu().numpy(), r1[1] - 7)
    _accumulate(dev(z1, I32), dev(l1), dev(p1), 8, 0, 0, None, k, z, 0, votes, sums)
    assert np.array_equal(votes.cpu().numpy(), r1[0]) and np.array_equal(sums.cpu().numpy(), r1[1])


@pytest.mark.parametrize("zdtype,ldtype", [(torch.uint8, I32), (torch.int16, I64), (I64, torch.int16)])
def test_wrapper_conversions_and_views(zdtype, ldtype):
    """uint8 / int16 zones are converted to int32, int32 labels to int64; non-contiguous views are read as what they show; an int64
    raster keeps ids that would alias zones if truncated to 32 bits."""
    h, w, cell, k, z = 45, 83, 8, 6, 9
    zn = _zones(h, 2 * w, z, 11)
    if zdtype == torch.uint8:
        zn = np.where(zn < 0, 200, zn)
    if zdtype == I64:
        zn[0, :8] = [2 ** 40, -2 ** 40, 2 ** 32 + 1, 2 ** 32, 2 ** 31, -1, 0, 8]
    lb, pr = _labels(6, 2 * 11, k, 11), _probs(6, 11, k, 11)
    zones, labels = torch.from_numpy(zn).to(zdtype).cuda()[:, ::2], torch.from_numpy(lb).to(ldtype).cuda()[:, 1::2]
    assert not zones.is_contiguous() and not labels.is_contiguous()
    zv, lv = zn[:, ::2], lb[:, 1::2]
    m = np.random.default_rng(12).random((h, w)) < 0.25
    got = eae_amd.zonal_stats(zones, z, labels, k, probs=torch.from_numpy(pr).cuda(), cell=cell, origin=(3, 2), mask=torch.from_numpy(m).cuda())
    rv, rs = zonal_ref(zv, z, lv, k, pr, cell, (3, 2), mask=m)
    assert np.array_equal(got.votes.cpu().numpy(), rv) and np.array_equal(got.prob_sums.cpu().numpy(), rs)
    votes_only = eae_amd.zonal_stats(zones, z, labels, k, cell=cell, origin=(3, 2), mask=torch.from_numpy(m).cuda().to(torch.uint8) * 200)
    assert votes_only.prob_sums is None and torch.equal(votes_only.votes, got.votes)
    vals = torch.arange(10, 10 + z, dtype=torch.int64, device="cuda")
    assert np.array_equal(eae_amd.paint_zones(zones, vals, fill=-9).cpu().numpy(), paint_ref(zv, vals.cpu().numpy(), -9))
    # the labels on the device agree with the reference decision
    for rule in ("probs", "votes"):
        dev = eae_amd.zone_labels(got, rule, 0.4)
        ref = zone_labels_ref(rv, rs, rule, 0.4)
        assert all(np.array_equal(d.cpu().numpy(), r, equal_nan=True) for d, r in zip(dev, ref))


def test_regions_as_zones():
    """`label_regions` -> `compact_zones` -> `zonal_stats(cell=1)` against the map itself: every zone's votes lie in one class, the
    region's, and equal `region_table`'s area."""
    k = 4
    coarse = np.random.default_rng(31).integers(-1, k, (30, 40))
    lb = np.repeat(np.repeat(coarse, 3, 0), 2, 1)[:83, :77].astype(np.int64)
    labels = torch.from_numpy(lb).cuda()
    regions = eae_amd.label_regions(labels, k)
    table = eae_amd.region_table(labels, regions)
    zones, ids = eae_amd.compact_zones(regions)
    assert torch.equal(ids, table["id"]) and zones.dtype == I32
    z = ids.numel()
    st = eae_amd.zonal_stats(zones, z, labels, k)
    assert st.prob_sums is None and int(st.votes.sum()) == int((labels >= 0).sum())
    assert torch.equal(st.votes.sum(1), table["area"])
    assert torch.equal(st.votes.gather(1, table["cls"][:, None])[:, 0], table["area"])
    label, conf, cov = eae_amd.zone_labels(st, "votes")
    assert torch.equal(label, table["cls"]) and bool((conf == 1).all()) and bool((cov == 1).all())
    assert torch.equal(eae_amd.paint_zones(zones, label), torch.where(labels >= 0, labels, -1))


# ---------------------------------------------------------------------------------------------------- classify_zones
C_, H_, W_, P_ = 3, 150, 200, 64
DIV = 255.0
NZ = 23


@pytest.fixture(scope="module")
def world():
    g = torch.Generator().manual_seed(41)
    scene = torch.randint(1, 256, (C_, H_, W_), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    rng = np.random.default_rng(41)
    zn = np.repeat(np.repeat(rng.integers(-1, NZ, (8, 9)), 19, 0), 23, 1)[:H_, :W_].astype(np.int64)   # parcels off the window grid
    return scene, zn, torch.from_numpy(zn).to(I32).cuda(), _model(C_, batch=64), _mlp()


def _check_zones(out, zn, stride, pads, rule, min_coverage, num_zones=NZ):
    lb, pr = out["labels"].cpu().numpy(), out["probs"].cpu().numpy()
    rv, rs = zonal_ref(zn, num_zones, lb, 10, pr, stride, (pads[0], pads[2]))
    assert np.array_equal(out["stats"].votes.cpu().numpy(), rv) and np.array_equal(out["stats"].prob_sums.cpu().numpy(), rs)
    assert int(out["stats"].votes.sum()) == _in_range(zn, num_zones)
    ref = zone_labels_ref(rv, rs, rule, min_coverage)
    for key, r in zip(("zone_labels", "confidence", "coverage"), ref):
        assert np.array_equal(out[key].cpu().numpy(), r, equal_nan=True), key
    assert out["map"].dtype == I64 and np.array_equal(out["map"].cpu().numpy(), paint_ref(zn, ref[0], -1))
    return rv, ref


@pytest.mark.parametrize("blend,stride,border", [(False, 64, None), (True, 32, "reflect"), (True, 16, None)])
def test_classify_zones(world, blend, stride, border):
    scene, zn, zones, model, mlp = world
    kw = dict(divisor=DIV, stride=stride, batch=64, blend=blend, border=border)
    out = eae_amd.classify_zones(scene, model, mlp, zones, num_zones=NZ, rule="probs", min_coverage=0.5, **kw)
    probs, labels = eae_amd.classify_scene(scene, model, mlp, **kw)
    assert torch.equal(out["labels"], labels) and torch.equal(out["probs"], probs)
    pads = (0, 0, 0, 0) if border is None else eae_amd.border_grid(H_, W_, P_, stride)[2]
    rv, ref = _check_zones(out, zn, stride, pads, "probs", 0.5)
    # without a border the pixels behind the grid's extent are not classified; with one every pixel is
    assert (rv[:, 10].sum() > 0) == (border is None)
    assert bool((ref[0] >= 0).any())
    # the pixel-wise score of the per-object map runs, and every pixel of a labelled zone is counted as classified
    truth = torch.from_numpy(np.random.default_rng(1).integers(0, 10, (H_, W_))).to(torch.uint8).cuda()
    cm = eae_amd.scene_confusion(out["map"], truth, 10, cell=1)
    assert int(cm.sum()) == H_ * W_ and int(cm[:, :10].sum()) == int((out["map"] >= 0).sum())
    # object-level accuracy against per-zone truth from the label raster
    tstats = eae_amd.zonal_stats(zones, NZ, truth, 10)
    tl = eae_amd.zone_labels(tstats, "votes")[0]
    zc = eae_amd.zone_confusion(out["zone_labels"], tl, 10)
    assert int(zc.sum()) == NZ and eae_amd.confusion_metrics(zc)["total"] == int((tl >= 0).sum())


def test_classify_zones_nodata_votes_and_num_zones(world):
    scene, zn, zones, model, mlp = world
    holed = scene.clone()
    holed[:, :70, :90] = 0                                       # a nodata corner: its windows get label -1
    out = eae_amd.classify_zones(holed, model, mlp, zones.to(I64), rule="votes", min_coverage=0.9, divisor=DIV, stride=32, batch=64,
                                 blend=True, nodata=0)
    assert bool((out["labels"] == -1).any()) and bool((out["labels"] >= 0).any())
    nz = int(zn.max()) + 1                                       # num_zones=None: the largest id + 1
    assert tuple(out["stats"].votes.shape) == (nz, 11)
    _, ref = _check_zones(out, zn, 32, (0, 0, 0, 0), "votes", 0.9, num_zones=nz)
    assert bool((ref[0] == -1).any()) and bool((ref[0] >= 0).any())             # zones in the hole fall below the coverage
