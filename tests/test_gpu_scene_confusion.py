"""Accuracy assessment on the device (eae_amd.scene): `eae_scene_confusion` by shape against the NumPy restatement of its semantics
(tests/confusion_ref.py), the Python wrapper's conversions, mask, ``ignore=`` and ``out=``, and `evaluate_scene` end to end.  Integer
counts: every comparison is exact equality, and in every case the entries sum to the number of unmasked pixels."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from confusion_ref import confusion_ref
from scene_util import _model, _mlp

pytestmark = pytest.mark.gpu

U8, I32 = torch.uint8, torch.int32


def _truth(h, w, k, dtype, seed):
    """A label raster with runs (3 x 3 blocks of one value) and single-pixel noise: classes, 255 and, for int32, negatives and
    values >= K as well."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, k + 1, (-(-h // 3), -(-w // 3)))
    t = np.repeat(np.repeat(coarse, 3, 0), 3, 1)[:h, :w].astype(np.int64)
    t[t == k] = 255
    noise = rng.random((h, w)) < 0.2
    lo, hi = (0, k + 3) if dtype == U8 else (-3, k + 70)
    t[noise] = rng.integers(lo, hi, int(noise.sum()))
    return t


def _pred(c_h, c_w, k, seed):
    """A cell map with -1 and values >= K among the classes."""
    return np.random.default_rng(seed + 1000).integers(-1, k + 2, (c_h, c_w)).astype(np.int64)


def _c_call(truth, pred, cell, oy, ox, mask, k, accumulate, counts):
    h, w = truth.shape
    _lib.check(_lib.load().eae_scene_confusion(_stream(), _ptr(truth), truth.element_size(), h, w, _ptr(pred), pred.shape[0],
                                               pred.shape[1], cell, oy, ox, _ptr(mask), k, accumulate, _ptr(counts)))


def _dirty(k):
    return torch.full((k + 1, k + 1), -7, dtype=torch.int64, device="cuda")


#        (H, W, cell, oy, ox, cH, cW, K, dtype)
SHAPES = [(1, 1, 1, 0, 0, 1, 1, 1, U8),
          (37, 41, 5, 0, 0, 8, 9, 3, U8),
          (37, 41, 5, 3, 4, 8, 9, 3, U8),                  # an origin inside the first cell
          (37, 41, 5, 7, 11, 8, 9, 3, U8),                 # an origin larger than the cell; the last rows fall off the map
          (37, 41, 5, 0, 0, 4, 5, 3, U8),                  # a map smaller than the raster: uncovered pixels land in column K
          (64, 257, 16, 0, 0, 4, 17, 5, U8),               # odd width: every row starts at another alignment
          (64, 257, 16, 5, 9, 5, 17, 5, I32),
          (5000, 1, 3, 1, 0, 1667, 1, 4, U8),              # one column: 256 rows per tile
          (33, 70, 4, 1, 2, 9, 18, 64, I32),               # K = 64; negatives, 255 and values >= K in the raster
          (23, 19, 1, 0, 0, 23, 19, 7, I32),               # cell = 1: two maps of one shape
          (1031, 2053, 7, 2, 5, 148, 294, 10, U8),         # many workgroups
          (2100, 4100, 16, 2, 5, 132, 257, 10, U8)]        # more tiles (2117) than the grid's 2048 workgroups: the grid stride


@pytest.mark.parametrize("h,w,cell,oy,ox,c_h,c_w,k,dtype", SHAPES)
def test_confusion_by_shape(h, w, cell, oy, ox, c_h, c_w, k, dtype):
    t, p = _truth(h, w, k, dtype, seed=h + w), _pred(c_h, c_w, k, seed=h + w)
    ref = confusion_ref(t, p, k, cell, (oy, ox))
    assert ref.sum() == h * w
    truth = torch.from_numpy(t).to(dtype).cuda()
    pred = torch.from_numpy(p).cuda()
    counts = _dirty(k)
    _c_call(truth, pred, cell, oy, ox, None, k, 0, counts)
    assert np.array_equal(counts.cpu().numpy(), ref)
    again = _dirty(k)
    _c_call(truth, pred, cell, oy, ox, None, k, 0, again)
    assert torch.equal(again, counts)
    # with a mask: a third of the pixels skipped, in runs and singly
    rng = np.random.default_rng(h * w)
    m = (rng.random((h, w)) < 0.2) | (np.repeat(rng.random((h, -(-w // 8))) < 0.15, 8, 1)[:, :w])
    ref_m = confusion_ref(t, p, k, cell, (oy, ox), mask=m)
    assert ref_m.sum() == h * w - int(m.sum())
    _c_call(truth, pred, cell, oy, ox, torch.from_numpy(m).cuda().view(torch.uint8), k, 0, counts)
    assert np.array_equal(counts.cpu().numpy(), ref_m)


@pytest.mark.parametrize("dtype", [U8, I32])
def test_unaligned_base_pointers(dtype):
    """The raster and the mask start at odd addresses that differ: clipped first runs, and whole runs whose mask bytes are loaded
    one by one."""
    h, w, cell, k = 19, 131, 6, 5
    t, p = _truth(h, w, k, dtype, seed=5), _pred(4, 22, k, seed=5)
    m = np.random.default_rng(6).random((h, w)) < 0.3
    tbuf = torch.zeros(h * w + 3, dtype=dtype, device="cuda")
    mbuf = torch.zeros(h * w + 5, dtype=torch.uint8, device="cuda")
    truth, mask = tbuf[3:].view(h, w), mbuf[5:].view(h, w)
    truth.copy_(torch.from_numpy(t).to(dtype))
    mask.copy_(torch.from_numpy(m).to(torch.uint8))
    counts = _dirty(k)
    _c_call(truth, torch.from_numpy(p).cuda(), cell, 2, 1, mask, k, 0, counts)
    ref = confusion_ref(t, p, k, cell, (2, 1), mask=m)
    assert np.array_equal(counts.cpu().numpy(), ref) and ref.sum() == h * w - int(m.sum())


def test_all_masked_gives_zeros():
    h, w, k = 40, 70, 4
    truth = torch.from_numpy(_truth(h, w, k, U8, 1)).to(U8).cuda()
    pred = torch.from_numpy(_pred(5, 9, k, 1)).cuda()
    got = eae_amd.scene_confusion(pred, truth, k, cell=8, mask=torch.ones((h, w), dtype=torch.bool, device="cuda"))
    assert got.dtype == torch.int64 and tuple(got.shape) == (k + 1, k + 1) and int(got.abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.int64, torch.int16, U8, I32])
def test_wrapper_conversions_ignore_and_views(dtype):
    """int64 / int16 rasters take the conversion path; ``ignore=`` moves classes to the unlabelled row; a non-contiguous view of a
    wider raster and of a wider map are read as what they show."""
    h, w, cell, k = 45, 83, 8, 6
    t = _truth(h, 2 * w, k, I32 if dtype != U8 else U8, seed=11)
    if dtype == torch.int64:
        t[0, :8] = [2 ** 40, -2 ** 40, 2 ** 32 + 1, 2 ** 31, -1, 0, 5, 6]        # would alias classes if truncated to 32 bits
    if dtype == torch.int16:
        t = np.clip(t, -2 ** 15, 2 ** 15 - 1)
    p = _pred(6, 2 * 11, k, seed=11)
    wide_t, wide_p = torch.from_numpy(t).to(dtype).cuda(), torch.from_numpy(p).cuda()
    truth, pred = wide_t[:, ::2], wide_p[:, 1::2]
    assert not truth.is_contiguous() and not pred.is_contiguous()
    tv, pv = t[:, ::2], p[:, 1::2]
    m = np.random.default_rng(12).random((h, w)) < 0.25
    mask = torch.from_numpy(m).cuda()
    for ignore, ign in ((None, ()), (1, (1,)), ([0, 4, 99, -5], (0, 4))):
        got = eae_amd.scene_confusion(pred, truth, k, cell=cell, origin=(3, 2), mask=mask, ignore=ignore)
        ref = confusion_ref(tv, pv, k, cell, (3, 2), mask=m, ignore=ign)
        assert np.array_equal(got.cpu().numpy(), ref), ignore
        assert int(got.sum()) == h * w - int(m.sum())
        assert all(int(got[c].sum()) == 0 for c in ign)
    u8mask = eae_amd.scene_confusion(pred, truth, k, cell=cell, origin=(3, 2), mask=mask.to(torch.uint8) * 200)
    assert np.array_equal(u8mask.cpu().numpy(), confusion_ref(tv, pv, k, cell, (3, 2), mask=m))


def test_out_accumulates_and_a_fresh_call_clears():
    k = 5
    t1, p1 = _truth(50, 60, k, U8, 21), _pred(7, 8, k, 21)
    t2, p2 = _truth(31, 90, k, I32, 22), _pred(3, 9, k, 22)
    a = eae_amd.scene_confusion(torch.from_numpy(p1).cuda(), torch.from_numpy(t1).to(U8).cuda(), k, cell=8)
    r1, r2 = confusion_ref(t1, p1, k, 8), confusion_ref(t2, p2, k, 10, (4, 0))
    assert np.array_equal(a.cpu().numpy(), r1)
    b = eae_amd.scene_confusion(torch.from_numpy(p2).cuda(), torch.from_numpy(t2).to(I32).cuda(), k, cell=10, origin=(4, 0), out=a)
    assert b is a and np.array_equal(a.cpu().numpy(), r1 + r2) and int(a.sum()) == 50 * 60 + 31 * 90
    # the C call with accumulate = 0 clears a dirty buffer, with accumulate = 1 it adds to it
    truth, pred = torch.from_numpy(t1).to(U8).cuda(), torch.from_numpy(p1).cuda()
    counts = _dirty(k)
    _c_call(truth, pred, 8, 0, 0, None, k, 0, counts)
    assert np.array_equal(counts.cpu().numpy(), r1)
    counts = _dirty(k)
    _c_call(truth, pred, 8, 0, 0, None, k, 1, counts)
    assert np.array_equal(counts.cpu().numpy(), r1 - 7)


def test_window_label_maps_compare_at_cell_one():
    """cell = 1: a window-label map against `window_labels`' majority map of the label raster."""
    k = 4
    t = _truth(150, 200, k, U8, 31)
    majority, _, _ = eae_amd.window_labels(torch.from_numpy(t).to(U8).cuda(), 64, 32, k)
    p = _pred(3, 5, k, 31)
    got = eae_amd.scene_confusion(torch.from_numpy(p).cuda(), majority, k)
    assert np.array_equal(got.cpu().numpy(), confusion_ref(majority.cpu().numpy(), p, k)) and int(got.sum()) == 15


# ---------------------------------------------------------------------------------------------------- evaluate_scene
C_, H_, W_, P_ = 3, 150, 200, 64
DIV = 255.0


@pytest.fixture(scope="module")
def world():
    g = torch.Generator().manual_seed(41)
    scene = torch.randint(1, 256, (C_, H_, W_), generator=g, dtype=torch.int64).to(U8).cuda()
    t = _truth(H_, W_, 10, U8, 41)
    return scene, t, torch.from_numpy(t).to(U8).cuda(), _model(C_, batch=64), _mlp()


def _check(out, ref_args, t, stride, pads, mask=None, ignore=()):
    probs, labels = ref_args
    assert torch.equal(out["labels"], labels) and torch.equal(out["probs"], probs)
    ref = confusion_ref(t, out["labels"].cpu().numpy(), 10, stride, (pads[0], pads[2]), mask=mask, ignore=ignore)
    assert np.array_equal(out["confusion"].cpu().numpy(), ref)
    assert int(out["confusion"].sum()) == H_ * W_ - (0 if mask is None else int(np.asarray(mask).sum()))
    m = eae_amd.confusion_metrics(ref)
    assert out["metrics"]["accuracy"] == m["accuracy"] and out["metrics"]["kappa"] == m["kappa"]
    assert out["metrics"]["area"].tolist() == m["area"].tolist() and out["metrics"]["total"] == m["total"]
    return ref


@pytest.mark.parametrize("border", [None, "reflect"])
@pytest.mark.parametrize("blend,stride", [(False, 64), (True, 32), (True, 16)])
def test_evaluate_scene(world, blend, stride, border):
    scene, t, truth, model, mlp = world
    kw = dict(divisor=DIV, stride=stride, batch=64, blend=blend, border=border, anchor="center")
    out = eae_amd.evaluate_scene(scene, model, mlp, truth, **kw)
    if border is None:
        pads = (0, 0, 0, 0)
    else:
        pads = eae_amd.border_grid(H_, W_, P_, stride)[2]
        assert pads[0] > 0 and pads[2] > 0
    ref = _check(out, eae_amd.classify_scene(scene, model, mlp, **kw), t, stride, pads)
    # without a border the pixels behind the grid's extent are not classified; with one every pixel is
    assert (ref[:, 10].sum() > 0) == (border is None)


def test_evaluate_scene_nodata_region_and_ignore(world):
    scene, t, truth, model, mlp = world
    holed = scene.clone()
    holed[:, :70, :90] = 0                                       # a nodata corner: its windows get label -1
    kw = dict(divisor=DIV, stride=32, batch=64, blend=True, nodata=0)
    out = eae_amd.evaluate_scene(holed, model, mlp, truth, **kw)
    assert bool((out["labels"] == -1).any()) and bool((out["labels"] >= 0).any())
    _check(out, eae_amd.classify_scene(holed, model, mlp, **kw), t, 32, (0, 0, 0, 0))
    # the validation region of a blocked split, and an ignored class
    n_h, n_w = eae_amd.window_grid(H_, W_, P_, 32)
    _, val, _ = eae_amd.block_split(n_h, n_w, P_, 32, 1, val_fraction=0.3, seed=2)
    region = eae_amd.footprint_mask(val, n_w, P_, 32, H_, W_, device="cuda")
    assert region.device.type == "cuda" and 0 < int(region.sum()) < H_ * W_
    kw = dict(divisor=DIV, stride=32, batch=64, blend=True, border="reflect")
    out = eae_amd.evaluate_scene(scene, model, mlp, truth, ignore=3, region=region, **kw)
    pads = eae_amd.border_grid(H_, W_, P_, 32)[2]
    ref = _check(out, eae_amd.classify_scene(scene, model, mlp, **kw), t, 32, pads, mask=~region.cpu().numpy(), ignore=(3,))
    assert ref[3].sum() == 0 and ref.sum() == int(region.sum())
