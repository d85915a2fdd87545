"""Scene borders on the device (eae_amd.scene, ``border=``): every scene function with border="constant" | "edge" | "reflect" is
compared, by torch.equal, with the same borderless function on numpy.pad(scene) uploaded to the device -- the one contract of the
feature.  Pixel-shaped outputs are compared with the oracle cropped to the real scene.

  case  scene                S   pads (centre)  windows  why
  A     3 x 100 x 150 uint8  32  14/14, 5/5     3 x 4    odd left pad (unaligned vector path), interior windows beside border ones
  B     13 x 70 x 64 uint16  64  29/29, 0/0     2 x 1    CP = 16, one padded axis only, a pad near P / 2
  C     1 x 40 x 200 fp32    48  12/12, 4/4     1 x 4    a scene lower than the patch, CP = 8, an even P - S for stitching
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eae_amd
import nodata_ref
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from scene_util import _scene, _divisor, _model, _mlp

pytestmark = pytest.mark.gpu

P = 64
FILL = 7
MODES = ("constant", "edge", "reflect")
CASES = {"A": (3, 100, 150, torch.uint8, 32, (3, 4), (14, 14, 5, 5)),
         "B": (13, 70, 64, torch.uint16, 64, (2, 1), (29, 29, 0, 0)),
         "C": (1, 40, 200, torch.float32, 48, (1, 4), (12, 12, 4, 4))}
RUNS = [(c, m, "center") for c in CASES for m in MODES] + [("A", m, "origin") for m in MODES]


def _np_pad(x, pads, mode, fill, lead=True):
    """numpy.pad of a [C,H,W] (or, lead=False, [H,W]) array: the oracle's padding."""
    pt, pb, pl, pr = pads
    width = ((0, 0),) * lead + ((pt, pb), (pl, pr))
    return np.pad(x, width, mode, **({"constant_values": fill} if mode == "constant" else {}))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene on the device, its host array, divisor, autoencoder, mlp) of a case: built once, never written."""
    c, h, w, dtype, s, _, _ = CASES[name]
    scene = _scene(c, h, w, dtype, seed=31 + c)
    model = _model(c, seed=5 + c, batch=16, all_halves=True)
    return scene, scene.cpu().numpy(), _divisor(c, dtype), model, _mlp()


@functools.lru_cache(maxsize=None)
def _run(name, mode, anchor):
    """(padded scene on the device, pads, grid) of a run, after the CPU checks that the comparison can fail: the grid and pads are
    those of the table, the three padded scenes differ from one another, and at least half of the windows touch padding."""
    c, h, w, dtype, s, grid, pads = CASES[name]
    n_h, n_w, got = eae_amd.border_grid(h, w, P, s, anchor)
    assert (n_h, n_w) == grid
    if anchor == "center":
        assert got == pads
    else:
        assert name == "A" and got == (0, 28, 0, 10)
    pt, pb, pl, pr = got
    host = _case(name)[1]
    padded = {m: _np_pad(host, got, m, FILL) for m in MODES}
    assert padded[mode].shape == (c, (n_h - 1) * s + P, (n_w - 1) * s + P)
    assert not np.array_equal(padded["constant"], padded["edge"]) and not np.array_equal(padded["edge"], padded["reflect"]) \
        and not np.array_equal(padded["constant"], padded["reflect"])
    touch = sum(1 for i in range(n_h) for j in range(n_w)
                if i * s < pt or i * s + P > pt + h or j * s < pl or j * s + P > pl + w)
    assert 2 * touch >= n_h * n_w
    return torch.from_numpy(padded[mode]).cuda(), got, (n_h, n_w)


def _kw(mode, anchor):
    return dict(border=mode, anchor=anchor, **({"fill": FILL} if mode == "constant" else {}))


@pytest.mark.parametrize("name,mode,anchor", RUNS)
def test_scene_windows_and_latents(name, mode, anchor):
    scene, _, div, model, _ = _case(name)
    padded, pads, (n_h, n_w) = _run(name, mode, anchor)
    s, kw = CASES[name][4], _kw(mode, anchor)
    ref = eae_amd.scene_windows(padded, div, P, s)
    got = eae_amd.scene_windows(scene, div, P, s, **kw)
    assert got.shape == (n_h * n_w, scene.shape[0], P, P) and torch.equal(got, ref)
    assert torch.equal(eae_amd.scene_windows(scene, div, P, s, first=n_h * n_w - 1, count=1, **kw), ref[-1:])
    z = eae_amd.encode_scene(scene, model, divisor=div, stride=s, batch=16, **kw)
    zr = eae_amd.encode_scene(padded, model, divisor=div, stride=s, batch=16)
    assert z.shape == (n_h * n_w, 64) and torch.isfinite(zr).all() and torch.equal(z, zr)


@pytest.mark.parametrize("name,mode,anchor", RUNS)
def test_classify_scene(name, mode, anchor):
    scene, _, div, model, mlp = _case(name)
    padded, pads, (n_h, n_w) = _run(name, mode, anchor)
    s, kw = CASES[name][4], _kw(mode, anchor)
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=16, **kw)
    rp, rl = eae_amd.classify_scene(padded, model, mlp, divisor=div, stride=s, batch=16)
    assert probs.shape == (10, n_h, n_w) and torch.equal(probs, rp) and torch.equal(labels, rl)
    if P % s == 0:
        k = P // s
        cp, cl = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=16, blend=True, **kw)
        rcp, rcl = eae_amd.classify_scene(padded, model, mlp, divisor=div, stride=s, batch=16, blend=True)
        assert cp.shape == (10, n_h + k - 1, n_w + k - 1) and torch.equal(cp, rcp) and torch.equal(cl, rcl)
    else:
        assert name == "C"


@pytest.mark.parametrize("name,mode,anchor", RUNS)
def test_reconstruction(name, mode, anchor):
    scene, _, div, model, _ = _case(name)
    padded, (pt, pb, pl, pr), (n_h, n_w) = _run(name, mode, anchor)
    c, h, w, _, s, _, _ = CASES[name]
    kw = _kw(mode, anchor)
    err, band = eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=s, batch=16, per_band=True, **kw)
    re_, rb = eae_amd.scene_reconstruction_error(padded, model, divisor=div, stride=s, batch=16, per_band=True)
    assert err.shape == (n_h, n_w) and band.shape == (c, n_h, n_w)
    assert torch.isfinite(re_).all() and torch.equal(err, re_) and torch.equal(band, rb)
    recon, res = eae_amd.reconstruct_scene(scene, model, divisor=div, stride=s, batch=16, residual=True, **kw)
    rr, rs = eae_amd.reconstruct_scene(padded, model, divisor=div, stride=s, batch=16, residual=True)
    assert recon.shape == (c, h, w) and res.shape == (h, w)
    assert torch.isfinite(rr).all() and torch.isfinite(rs).all()
    assert torch.equal(recon, rr[:, pt:pt + h, pl:pl + w]) and torch.equal(res, rs[pt:pt + h, pl:pl + w])


@pytest.mark.parametrize("mode", MODES)
def test_partial_batches_and_window_lists(mode):
    """Case A, 12 windows: batches of 5 (5 + 5 + 2) through every model-running function, and window lists that hold border windows,
    reversed and with a duplicate."""
    scene, _, div, _, mlp = _case("A")
    padded, (pt, pb, pl, pr), (n_h, n_w) = _run("A", mode, "center")
    model = _model(3, seed=9, batch=5, all_halves=True)
    kw = _kw(mode, "center")
    a = dict(divisor=div, stride=32, batch=5)
    assert n_h * n_w == 12
    assert torch.equal(eae_amd.encode_scene(scene, model, **a, **kw), eae_amd.encode_scene(padded, model, **a))
    for x, y in zip(eae_amd.classify_scene(scene, model, mlp, **a, **kw), eae_amd.classify_scene(padded, model, mlp, **a)):
        assert torch.equal(x, y)
    for x, y in zip(eae_amd.reconstruct_scene(scene, model, residual=True, **a, **kw),
                    eae_amd.reconstruct_scene(padded, model, residual=True, **a)):
        assert torch.equal(x, y[..., pt:pt + 100, pl:pl + 150])
    ids = torch.tensor([11, 8, 6, 5, 3, 0, 11], dtype=torch.int64, device="cuda")        # corners, an edge, an interior one
    assert torch.equal(eae_amd.encode_scene(scene, model, windows=ids, **a, **kw), eae_amd.encode_scene(padded, model, windows=ids, **a))
    for x, y in zip(eae_amd.classify_scene(scene, model, mlp, windows=ids, blend=True, **a, **kw),
                    eae_amd.classify_scene(padded, model, mlp, windows=ids, blend=True, **a)):
        assert torch.equal(x, y)
    e = eae_amd.scene_reconstruction_error(scene, model, windows=ids, **a, **kw)
    er = eae_amd.scene_reconstruction_error(padded, model, windows=ids, **a)
    assert torch.equal(torch.isnan(e), torch.isnan(er)) and int(torch.isnan(er).sum()) == 6
    assert torch.equal(torch.nan_to_num(e, nan=-1.0), torch.nan_to_num(er, nan=-1.0))
    rec = eae_amd.reconstruct_scene(scene, model, windows=ids, **a, **kw)
    rr = eae_amd.reconstruct_scene(padded, model, windows=ids, **a)[:, pt:pt + 100, pl:pl + 150]
    assert torch.isnan(rr).any() and not torch.isnan(rr).all()
    assert torch.equal(torch.isnan(rec), torch.isnan(rr)) and torch.equal(torch.nan_to_num(rec, nan=-1.0), torch.nan_to_num(rr, nan=-1.0))


def _counts_np(host, mask, pads, mode, fill, nodata, rule):
    """the border counts by NumPy alone (tests/nodata_ref.py): pad_ref, then the cumulative-sum counts -- no device in the oracle"""
    ps, pm = nodata_ref.pad_ref(host, mask, pads, mode, fill)
    return nodata_ref.counts_ref(nodata_ref.rows_ref(nodata_ref.invalid_ref(ps, nodata, rule, pm), P, 32), P, 32)


def _invalid_scene():
    """Case A's scene with a block of nodata (0 in every band) near the top-left corner and a mask block near the bottom-right one,
    both within pad distance (14 rows, 5 columns) of the border, so that reflect mirrors them, and both off the outermost row and
    column, so that edge does not replicate them: the three modes count differently."""
    host = _case("A")[1].copy()
    host[host == 0] = 1
    host[:, 3:30, 2:20] = 0
    mask = np.zeros((100, 150), dtype=np.uint8)
    mask[75:97, 125:148] = 1
    mask[97:100, 125:140] = 1               # a part that does reach the last row: edge replicates it, constant does not
    return host, mask


@pytest.mark.parametrize("mode", MODES)
def test_nodata_and_mask_counts_and_classification(mode):
    _, _, div, model, mlp = _case("A")
    host, mask = _invalid_scene()
    pads = eae_amd.border_grid(100, 150, P, 32)[2]
    scene, dmask = torch.from_numpy(host).cuda(), torch.from_numpy(mask).cuda()
    padded = torch.from_numpy(_np_pad(host, pads, mode, FILL)).cuda()
    pmask = torch.from_numpy(_np_pad(mask, pads, mode, 0, lead=False)).cuda()
    kw = _kw(mode, "center")
    ref = {m: eae_amd.window_invalid_counts(torch.from_numpy(_np_pad(host, pads, m, FILL)).cuda(), P, 32, nodata=0,
                                            mask=torch.from_numpy(_np_pad(mask, pads, m, 0, lead=False)).cuda()) for m in MODES}
    assert not torch.equal(ref["constant"], ref["edge"]) and not torch.equal(ref["edge"], ref["reflect"])
    for rule in ("all", "any"):
        got = eae_amd.window_invalid_counts(scene, P, 32, nodata=0, mask=dmask, rule=rule, **kw)
        assert got.shape == (3, 4) and torch.equal(got, eae_amd.window_invalid_counts(padded, P, 32, nodata=0, mask=pmask, rule=rule))
        assert np.array_equal(got.cpu().numpy(), _counts_np(host, mask, pads, mode, FILL, 0, rule))
    assert torch.equal(eae_amd.window_invalid_counts(scene, P, 32, nodata=0, mask=dmask, **kw), ref[mode])
    assert torch.equal(eae_amd.window_invalid_counts(scene, P, 32, mask=dmask.bool(), **kw),
                       eae_amd.window_invalid_counts(padded, P, 32, mask=pmask))
    assert np.array_equal(eae_amd.window_invalid_counts(scene, P, 32, mask=dmask.bool(), **kw).cpu().numpy(),
                          _counts_np(host, mask, pads, mode, FILL, None, "all"))
    np_ref = {m: _counts_np(host, mask, pads, m, FILL, 0, "all") for m in MODES}
    assert all(np.array_equal(ref[m].cpu().numpy(), np_ref[m]) for m in MODES)
    assert not np.array_equal(np_ref["constant"], np_ref["edge"]) and not np.array_equal(np_ref["edge"], np_ref["reflect"])
    ids = eae_amd.valid_windows(scene, P, 32, nodata=0, mask=dmask, max_invalid=0.1, **kw)
    assert torch.equal(ids, eae_amd.valid_windows(padded, P, 32, nodata=0, mask=pmask, max_invalid=0.1))
    for blend in (False, True):
        a = dict(divisor=div, stride=32, batch=16, nodata=0, max_invalid=0.1, blend=blend)
        probs, labels = eae_amd.classify_scene(scene, model, mlp, mask=dmask, **a, **kw)
        rp, rl = eae_amd.classify_scene(padded, model, mlp, mask=pmask, **a)
        assert (rl < 0).any() and (rl >= 0).any()                 # excluded and classified windows both occur
        assert torch.equal(probs, rp) and torch.equal(labels, rl)


def test_constant_fill_matching_nodata_is_invalid():
    host, mask = _invalid_scene()
    pads = eae_amd.border_grid(100, 150, P, 32)[2]
    scene = torch.from_numpy(host).cuda()
    got = eae_amd.window_invalid_counts(scene, P, 32, nodata=0, border="constant", fill=0)
    ref = eae_amd.window_invalid_counts(torch.from_numpy(_np_pad(host, pads, "constant", 0)).cuda(), P, 32, nodata=0)
    assert torch.equal(got, ref)
    assert np.array_equal(got.cpu().numpy(), _counts_np(host, None, pads, "constant", 0, 0, "all"))
    # window (0, 0) holds 50 x 59 real pixels: every other pixel of it is padding, and invalid
    assert int(got[0, 0]) >= P * P - 50 * 59
    other = eae_amd.window_invalid_counts(scene, P, 32, nodata=0, border="constant", fill=FILL)
    assert int(other[0, 0]) == int(got[0, 0]) - (P * P - 50 * 59)
    assert np.array_equal(other.cpu().numpy(), _counts_np(host, None, pads, "constant", FILL, 0, "all"))
    # fp32: NaN fill against a NaN nodata
    f = _case("C")[0]
    cnt = eae_amd.window_invalid_counts(f, P, 48, nodata=float("nan"), border="constant", fill=float("nan"))
    assert cnt.shape == (1, 4) and int(cnt[0, 1]) == P * P - 40 * P
    nan = float("nan")
    ps, _ = nodata_ref.pad_ref(f.cpu().numpy(), None, eae_amd.border_grid(40, 200, P, 48)[2], "constant", nan)
    assert np.array_equal(cnt.cpu().numpy(), nodata_ref.counts_ref(nodata_ref.rows_ref(nodata_ref.invalid_ref(ps, nan, "all", None), P, 48), P, 48))


def test_c_level_rejects():
    """eae_scene_check through the C ABI: each bad border descriptor is EAE_ERR_ARG (-2), and a good call afterwards still passes."""
    lib = _lib.load()
    scene, _, div, _, _ = _case("A")
    d = torch.tensor(div, dtype=torch.float32, device="cuda")
    out = torch.empty((1, 3, P, P), device="cuda")
    low = scene[:, :20].contiguous()

    def desc(x, border, pt, pb, pl, pr, fill=0.0, stride=32):
        return _lib.EaeScene(C.c_void_p(x.data_ptr()), C.c_void_p(d.data_ptr()), 0, 3, x.shape[1], x.shape[2], P, stride, border, pt, pb, pl,
                             pr, fill)

    bad = [desc(scene, 2, P, 0, 0, 0),               # pad = P
           desc(scene, 2, 0, 0, 0, P),
           desc(scene, 2, -1, 0, 0, 0),              # negative pad
           desc(scene, 1, 0, 0, -3, 0),
           desc(low, 3, 20, 24, 0, 0),               # reflect pad = H
           desc(low, 3, 24, 20, 0, 0),
           desc(scene, 4, 1, 1, 1, 1),               # border value 4
           desc(scene, -1, 0, 0, 0, 0),
           desc(scene, 0, 14, 14, 5, 5),             # pads without a border
           desc(scene, 0, 0, 0, 0, 1),
           desc(scene, 1, 1, 1, 1, 1, fill=256.0),   # fill outside uint8
           desc(scene, 1, 1, 1, 1, 1, fill=-1.0),
           desc(scene, 1, 1, 1, 1, 1, fill=0.5),
           desc(low, 2, 20, 23, 0, 0),               # virtual height 63 < P
           desc(low, 0, 0, 0, 0, 0)]                 # and without a border, as before
    for b in bad:
        rc = lib.eae_scene_windows(_stream(), C.byref(b), 0, 1, _ptr(out))
        assert rc == -2, (b.border, b.pad_top, b.pad_bottom, b.pad_left, b.pad_right, b.fill)
        with pytest.raises(_lib.EaeError):
            _lib.check(rc)
    rows, counts = torch.empty((P, 1), dtype=torch.int32, device="cuda"), torch.empty((1, 1), dtype=torch.int32, device="cuda")
    assert lib.eae_scene_invalid_counts(_stream(), C.byref(bad[0]), 1, 0.0, 0, None, _ptr(rows), _ptr(counts)) == -2
    # the good call: the last window of case A under edge, straight through the C ABI, and a low strip with the smallest legal pads
    padded, pads, (n_h, n_w) = _run("A", "edge", "center")
    _lib.check(lib.eae_scene_windows(_stream(), C.byref(desc(scene, 2, *pads)), n_h * n_w - 1, 1, _ptr(out)))
    assert torch.equal(out, eae_amd.scene_windows(padded, div, P, 32)[-1:])
    mid = scene[:, :40].contiguous()                  # reflect at its limit on the left: pad_left = 63 <= W - 1
    _lib.check(lib.eae_scene_windows(_stream(), C.byref(desc(mid, 3, 12, 12, 63, 0)), 1, 1, _ptr(out)))
    ref = torch.from_numpy(_np_pad(mid.cpu().numpy(), (12, 12, 63, 0), "reflect", 0)).cuda()
    assert torch.equal(out, eae_amd.scene_windows(ref, div, P, 32)[1:2])
    _lib.check(lib.eae_scene_windows(_stream(), C.byref(desc(low, 2, 19, 25, 0, 0)), 2, 1, _ptr(out)))
    ref = torch.from_numpy(_np_pad(low.cpu().numpy(), (19, 25, 0, 0), "edge", 0)).cuda()
    assert torch.equal(out, eae_amd.scene_windows(ref, div, P, 32)[2:3])
