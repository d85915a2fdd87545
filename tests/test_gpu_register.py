"""Co-registration on the device (eae_amd.register): `eae_match_tiles` and `eae_scene_resample` through the C ABI, bit for bit against
the NumPy definition (tests/register_ref.py), then `match_tiles`, `coregister`, `resample_scene` and their hand-over to
`detect_change`.  Every output is poisoned before a call.

Both kernels are exact (integers; float64 in a stated order), so every comparison through the C ABI is equality of bytes.  The Python
layer's matrix is compared with the reference pipeline's to 1e-9 (the host parts are float64 in both) and with the planted truth to
`register_ref.BOUND` = 0.25 px: twice the worst of the seven corner errors the reference pipeline gave on the CPU (0.0860 px), rounded
up to a power of two; the measurements are listed in tests/test_register_reference.py."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
import register_ref as R

pytestmark = pytest.mark.gpu

NP = R.NP
CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}
DIV = {"u8": 255.0, "u16": 1000.0, "f32": 0.7}          # u16 values above 1000 and f32 values outside [0, 0.7] exercise the clamps
POISON = -7
IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


def _scene(rng, kind, shape):
    if kind == "f32":
        return (0.35 + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    return rng.integers(0, 256 if kind == "u8" else 1400, shape).astype(NP[kind])


def _nodata(nd, rule):
    mode = 0 if nd is None else 2 if isinstance(nd, float) and np.isnan(nd) else 1
    return mode, 0.0 if mode != 1 else float(nd), {"all": 0, "any": 1}[rule]


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---------------------------------------------------------------------------------------------------- matching through the C ABI
def _c_match(a, b, bands, divs, tile, radius, oa, ob, nodata_a=None, rule_a="all", nodata_b=None, rule_b="all", mask_a=None, mask_b=None):
    """One call on a poisoned table: int64 [n, (2R + 1)^2, 6] as NumPy."""
    lib = _lib.load()
    n, nd = len(oa), 2 * radius + 1
    ta, tb = _dev(a), _dev(b)
    da = _dev(np.full(a.shape[0], divs[0], dtype=np.float32))
    db = _dev(np.full(b.shape[0], divs[1], dtype=np.float32))
    ma = _dev(None if mask_a is None else mask_a.astype(np.uint8))
    mb = _dev(None if mask_b is None else mask_b.astype(np.uint8))
    toa, tob = _dev(np.asarray(oa, dtype=np.int32)), _dev(np.asarray(ob, dtype=np.int32))
    sums = torch.full((n, nd * nd, 6), POISON, dtype=torch.int64, device="cuda")
    rc = lib.eae_match_tiles(_stream(), _ptr(ta), CODE[a.dtype], *a.shape, bands[0], _ptr(da), *_nodata(nodata_a, rule_a), _ptr(ma),
                             _ptr(tb), CODE[b.dtype], *b.shape, bands[1], _ptr(db), *_nodata(nodata_b, rule_b), _ptr(mb),
                             tile, radius, n, _ptr(toa), _ptr(tob), _ptr(sums))
    torch.cuda.synchronize()
    assert rc == 0, lib.eae_last_error()
    return sums.cpu().numpy()


def _ref_match(a, b, bands, divs, tile, radius, oa, ob, nodata_a=None, rule_a="all", nodata_b=None, rule_b="all", mask_a=None,
               mask_b=None):
    ua, ub = R.features(a[bands[0]], divs[0]), R.features(b[bands[1]], divs[1])
    va, vb = R.validity(a, nodata_a, rule_a, mask_a), R.validity(b, nodata_b, rule_b, mask_b)
    return R.tile_sums(ua, va, ub, vb, tile, radius, oa, ob)


def _origins(sa, sb, tile, radius):
    """Templates and windows inside, partly outside and wholly outside either raster, negative and extreme origins included."""
    (ha, wa), (hb, wb) = sa, sb
    big = 2 ** 31 - 1
    oa = [(0, 0), (ha - tile, wa - tile), (-(tile // 2), -3), (ha - 2, wa - 2), (-tile - 5, 0), (1, 2), (3, 5), (big, -big - 1), (2, 1)]
    ob = [(0, 0), (hb - tile, wb - tile), (2, -radius - 1), (hb - 1, wb - 1), (0, 0), (hb + radius + 1, 0), (4, 1), (-big - 1, big), (-1, 3)]
    return np.array(oa, dtype=np.int64), np.array(ob, dtype=np.int64)


GEOMETRIES = [(4, 0), (8, 1), (13, 3), (64, 16), (64, 0)]
#            scene A               scene B               bands
PAIRS = [((1, 16, 16), "u8", (1, 16, 16), "u8", (0, 0)),
         ((3, 40, 67), "u16", (3, 40, 67), "u16", (1, 2)),
         ((16, 70, 131), "f32", (16, 70, 131), "f32", (15, 15)),
         ((2, 90, 120), "u16", (5, 100, 97), "f32", (1, 3))]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "x".join(map(str, p[0])) + p[1] + "-" + "x".join(map(str, p[2])) + p[3])
@pytest.mark.parametrize("tile,radius", GEOMETRIES)
def test_match_tiles_bit_equal(pair, tile, radius):
    sa, ka, sb, kb, bands = pair
    rng = np.random.default_rng(tile * 100 + radius)
    a, b = _scene(rng, ka, sa), _scene(rng, kb, sb)
    b[bands[1], :sb[1] // 2, :sb[2] // 2] = (a[bands[0], :sb[1] // 2, :sb[2] // 2].astype(np.float64) * DIV[kb] / DIV[ka]).astype(NP[kb])
    oa, ob = _origins(sa[1:], sb[1:], tile, radius)
    args = (a, b, bands, (DIV[ka], DIV[kb]), tile, radius, oa, ob)
    got, want = _c_match(*args), _ref_match(*args)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want)
    assert (got[[4, 5, 7]] == 0).all() and got[0, :, 0].max() > 0          # wholly outside: every word written as zero
    assert got.max() < 2 ** 45


@pytest.mark.parametrize("tile,radius", [(8, 1), (13, 3)])
def test_match_tiles_nodata_rules_and_masks(tile, radius):
    rng = np.random.default_rng(21)
    a, b = _scene(rng, "u16", (3, 40, 67)), _scene(rng, "u8", (2, 45, 60))
    hole = rng.random((40, 67))
    a[:, hole < 0.1] = 0                                                   # all bands: nodata under both rules
    a[0][(hole >= 0.1) & (hole < 0.2)] = 0                                 # one band: nodata under "any" only
    hole = rng.random((45, 60))
    b[:, hole < 0.1] = 255
    b[1][(hole >= 0.1) & (hole < 0.2)] = 255
    mask_a, mask_b = rng.random((40, 67)) < 0.1, rng.random((45, 60)) < 0.1
    oa, ob = _origins((40, 67), (45, 60), tile, radius)
    seen = []
    for rule_a, rule_b in (("all", "any"), ("any", "all")):
        kw = dict(nodata_a=0, rule_a=rule_a, nodata_b=255, rule_b=rule_b, mask_a=mask_a, mask_b=mask_b)
        args = (a, b, (1, 0), (1000.0, 255.0), tile, radius, oa, ob)
        got = _c_match(*args, **kw)
        assert np.array_equal(got, _ref_match(*args, **kw))
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])
    only_a = _c_match(*args, mask_a=mask_a)
    assert np.array_equal(only_a, _ref_match(*args, mask_a=mask_a)) and not np.array_equal(only_a, _c_match(*args, mask_b=mask_b))


def test_match_tiles_float_nan_inf():
    rng = np.random.default_rng(22)
    a, b = _scene(rng, "f32", (4, 33, 50)), _scene(rng, "f32", (3, 33, 50))
    a[2, 5:9, 7:30] = np.nan                                               # not the matched band: the pixel is invalid all the same
    a[1, 20, :] = np.inf
    b[0, :, 10] = -np.inf
    b[:, 25:, 40:] = np.nan                                                # NaN as the nodata value as well
    b[1, 3, 3] = np.nan
    oa, ob = _origins((33, 50), (33, 50), 13, 3)
    for kw in (dict(), dict(nodata_b=float("nan"), rule_b="all"), dict(nodata_b=float("nan"), rule_b="any", nodata_a=0.5)):
        args = (a, b, (1, 2), (0.7, 1.0), 13, 3, oa, ob)
        assert np.array_equal(_c_match(*args, **kw), _ref_match(*args, **kw)), kw


def test_match_tiles_all_invalid_single_tile_and_grid_stride():
    rng = np.random.default_rng(23)
    a, b = _scene(rng, "u8", (1, 16, 16)), _scene(rng, "u8", (1, 16, 16))
    oa, ob = _origins((16, 16), (16, 16), 8, 1)
    args = (a, b, (0, 0), (255.0, 255.0), 8, 1)
    # a tile whose pairs are all invalid: all zeros, every word written
    assert (_c_match(*args, oa[:1], ob[:1], mask_a=np.ones((16, 16), dtype=bool)) == 0).all()
    # a single tile
    want = _ref_match(*args, oa, ob)
    for t in (0, 2, 6):
        assert np.array_equal(_c_match(*args, oa[t:t + 1], ob[t:t + 1]), want[t:t + 1])
    # more tiles than the launch grid (1024 workgroups): the origins repeated; twice, bit-equal
    idx = np.arange(2 * 1024 + 37) % len(oa)
    got = _c_match(*args, oa[idx], ob[idx])
    assert np.array_equal(got, want[idx])
    assert np.array_equal(got, _c_match(*args, oa[idx], ob[idx]))
    # the same for the largest footprint, where a tile's items outnumber the threads
    args = (a, b, (0, 0), (255.0, 255.0), 64, 16)
    got = _c_match(*args, oa, ob)
    assert np.array_equal(got, _c_match(*args, oa, ob))


# ---------------------------------------------------------------------------------------------------- resampling through the C ABI
def _c_resample(src, matrix, method, shape, nodata=None, rule="all", mask=None, fill=0.0, want_valid=True):
    """One call on poisoned outputs: (dst, valid or None) as NumPy."""
    lib = _lib.load()
    c, hs, ws = src.shape
    ts = _dev(src)
    tm = _dev(None if mask is None else mask.astype(np.uint8))
    dst = torch.empty((c,) + tuple(shape), dtype=ts.dtype, device="cuda")
    dst.view(torch.uint8).fill_(0xCD)
    valid = torch.full(tuple(shape), 0xCD, dtype=torch.uint8, device="cuda")
    m = np.ascontiguousarray(matrix, dtype=np.float64)
    rc = lib.eae_scene_resample(_stream(), _ptr(ts), CODE[src.dtype], c, hs, ws, *_nodata(nodata, rule), _ptr(tm), m.ctypes.data,
                                R.METHODS[method], float(fill), _ptr(dst), shape[0], shape[1], _ptr(valid) if want_valid else None)
    torch.cuda.synchronize()
    assert rc == 0, lib.eae_last_error()
    return dst.cpu().numpy(), valid.cpu().numpy() if want_valid else None


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _matrices(src_shape, dst_shape):
    (hs, ws), (hd, wd) = src_shape, dst_shape
    return {"identity": IDENT, "integer": [[1.0, 0.0, 3.0], [0.0, 1.0, -2.0]], "fraction": [[1.0, 0.0, 0.25], [0.0, 1.0, -1.5]],
            "rotation": R.rigid(0.7, 1.01, (0.3, -0.6), hd, wd), "partly": [[1.7, 0.0, -5.3], [0.0, 1.7, -4.1]],
            "outside": [[1.0, 0.0, ws + 10.0], [0.0, 1.0, 0.0]]}


SHAPES = [((1, 1, 1), (1, 1)), ((1, 1, 63), (1, 63)), ((3, 5, 67), (7, 50)), ((16, 33, 129), (33, 129)), ((2, 300, 520), (257, 511))]


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("src_shape,dst_shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scene_resample_bit_equal(src_shape, dst_shape, kind):
    rng = np.random.default_rng(31)
    src = _scene(rng, kind, src_shape)
    fill = 7.0 if kind != "f32" else -1.5
    for name, m in _matrices(src_shape[1:], dst_shape).items():
        for method in R.METHODS:
            got, gv = _c_resample(src, m, method, dst_shape, fill=fill)
            want, wv = R.resample_ref(src, m, dst_shape, method, fill=fill)
            assert _same(got, want) and _same(gv, wv), (name, method)
            if name == "outside":
                assert not gv.any() and (got == NP[kind](fill)).all()
            if name == "partly" and src_shape[1] >= 5:                     # a one-row source lies wholly above this map's image
                assert gv.any() and not gv.all()


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
def test_scene_resample_identity_and_integer_shift_are_copies(kind):
    rng = np.random.default_rng(32)
    src = _scene(rng, kind, (3, 37, 70))
    if kind == "f32":
        src[1, 4, 5] = -0.0
    for method in R.METHODS:
        got, gv = _c_resample(src, IDENT, method, (37, 70), fill=9.0)
        assert _same(got, src) and gv.all(), method
        got, gv = _c_resample(src, [[1.0, 0.0, -4.0], [0.0, 1.0, 6.0]], method, (37, 70), fill=9.0)
        want = np.full_like(src, 9)
        want[:, :31, 4:] = src[:, 6:, :66]
        assert _same(got, want) and gv[:31, 4:].all() and gv.sum() == 31 * 66, method


def test_scene_resample_nodata_mask_nan_and_fill():
    rng = np.random.default_rng(33)
    src = _scene(rng, "u16", (3, 33, 67))
    hole = rng.random((33, 67))
    src[:, hole < 0.05] = 0
    src[2][(hole >= 0.05) & (hole < 0.1)] = 0
    mask = rng.random((33, 67)) < 0.05
    m = R.rigid(0.7, 1.01, (0.3, -0.6), 40, 60)
    for method in R.METHODS:
        for rule in ("all", "any"):
            got, gv = _c_resample(src, m, method, (40, 60), nodata=0, rule=rule, mask=mask, fill=65535.0)
            want, wv = R.resample_ref(src, m, (40, 60), method, nodata=0, rule=rule, mask=mask, fill=65535.0)
            assert _same(got, want) and _same(gv, wv) and gv.any() and not gv.all(), (method, rule)
        got, gv = _c_resample(src, m, method, (40, 60), nodata=0, mask=mask, fill=3.0, want_valid=False)       # out_valid NULL
        assert gv is None and _same(got, R.resample_ref(src, m, (40, 60), method, nodata=0, mask=mask, fill=3.0)[0])
    f = _scene(rng, "f32", (2, 33, 67))
    f[0, 5:8, 10:20] = np.nan
    f[:, 20:, 50:] = np.nan
    f[1, 15, 30] = np.inf
    for method in R.METHODS:
        for kw in (dict(fill=float("nan")), dict(fill=float("nan"), nodata=float("nan"), rule="all"), dict(fill=-1.0, nodata=float("nan"), rule="any")):
            got, gv = _c_resample(f, m, method, (40, 60), **kw)
            want, wv = R.resample_ref(f, m, (40, 60), method, **kw)
            assert _same(gv, wv) and not gv.all() and gv.any()
            assert _same(got, want), (method, kw)
            assert np.isfinite(got[:, gv == 1]).all() and (np.isnan(got[:, gv == 0]).all() if np.isnan(kw["fill"]) else True)


def test_scene_resample_cubic_overshoot_is_clamped():
    rng = np.random.default_rng(34)
    for kind, hi in (("u8", 255), ("u16", 65535)):
        src = (rng.integers(0, 2, (2, 20, 40)) * hi).astype(NP[kind])      # steps between 0 and the maximum
        m = [[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]
        raw = R.resample_ref(src.astype(np.float32), m, (20, 40), "cubic")[0]
        assert (raw < 0).any() and (raw > hi).any()                        # the unclamped sums leave the range on both sides
        got, gv = _c_resample(src, m, "cubic", (20, 40))
        want, wv = R.resample_ref(src, m, (20, 40), "cubic")
        assert _same(got, want) and _same(gv, wv)
        assert (got[:, gv == 1][raw[:, gv == 1] < 0] == 0).all() and (got[:, gv == 1][raw[:, gv == 1] > hi] == hi).all()


# ---------------------------------------------------------------------------------------------------- the Python layer
CASES = R.CASES[:3]


@pytest.fixture(scope="module")
def planted_runs():
    """{seed: (a, b, div, truth, reference matrix, reference ok)} of the three planted pairs, the reference pipeline run once."""
    runs = {}
    for case in CASES:
        a, b, div, truth = R.planted_case(case)
        m, ok, _ = R.coregister_ref(a, b, divisor_a=div, divisor_b=div, **R.MATCH)
        runs[case[0]] = (a, b, div, truth, m, ok)
    return runs


def test_match_tiles_equals_the_reference(planted_runs):
    a, b, div, truth, _, _ = planted_runs[0]
    ca, pb, off, sub, sc, ok, sums = R.match_ref(a, b, divisor_a=div, divisor_b=div, **R.MATCH)
    got = eae_amd.match_tiles(_dev(a), _dev(b), divisor_a=div, divisor_b=div, keep_sums=True, **R.MATCH)
    assert np.array_equal(got.sums.cpu().numpy(), sums)
    assert np.array_equal(got.offsets, off) and np.array_equal(got.ok, ok) and got.offsets.dtype == np.int64 and got.ok.dtype == bool
    assert np.array_equal(got.centres, ca) and np.abs(got.points - pb).max() < 1e-9 and np.abs(got.scores - sc).max() < 1e-12
    assert got.geometry == eae_amd.TileGeometry(32, 32, 6, (6, 8), (192, 256))
    assert eae_amd.match_tiles(_dev(a), _dev(b), divisor_a=div, divisor_b=div, **R.MATCH).sums is None
    # a second pass from the truth finds every peak at the window's centre or next to it
    again = eae_amd.match_tiles(_dev(a), _dev(b), divisor_a=div, divisor_b=div, initial=truth, **R.MATCH)
    assert np.abs(again.offsets).max() <= 1 and again.ok.all()


@pytest.mark.parametrize("case", CASES, ids=[f"seed{c[0]}-{c[1]}" for c in CASES])
def test_coregister_planted(planted_runs, case):
    a, b, div, truth, ref_m, ref_ok = planted_runs[case[0]]
    b_on_a, valid, reg = eae_amd.coregister(_dev(a), _dev(b), divisor_a=div, divisor_b=div, **R.MATCH)
    err = R.corner_error(reg.matrix, truth, R.H, R.W)
    print("corner error %.4f px, %d of %d tiles inliers, |M - ref| %.3g" % (err, reg.inliers.sum(), reg.n_tiles, np.abs(reg.matrix - ref_m).max()))
    assert np.abs(reg.matrix - ref_m).max() < 1e-9
    assert err <= R.BOUND
    assert reg.n_tiles == 48 and np.isfinite(reg.residuals).sum() >= 36    # at most one quarter of the tiles rejected
    assert b_on_a.dtype == torch.from_numpy(b).dtype and tuple(b_on_a.shape) == a.shape and valid.dtype == torch.bool
    want, wv = R.resample_ref(b, reg.matrix, a.shape[1:], "bilinear")
    assert _same(b_on_a.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv.astype(bool))
    text = eae_amd.registration_table(reg, a.shape[1:])
    assert "inliers" in text and "of 48 tiles" in text and "scene centre" in text


def test_coregister_with_nodata_and_mask_then_detect_change():
    a, b, div, truth, mask_b = R.masked_case()
    ref_m, ref_ok, _ = R.coregister_ref(a, b, divisor_a=div, divisor_b=div, nodata_a=0, mask_b=mask_b, **R.MATCH)
    ta, tb = _dev(a), _dev(b)
    b_on_a, valid, reg = eae_amd.coregister(ta, tb, divisor_a=div, divisor_b=div, nodata_a=0, mask_b=_dev(mask_b), method="cubic", **R.MATCH)
    assert np.abs(reg.matrix - ref_m).max() < 1e-9 and R.corner_error(reg.matrix, truth, R.H, R.W) <= R.BOUND
    assert np.isfinite(reg.residuals).sum() == ref_ok.sum() >= 6
    want, wv = R.resample_ref(b, reg.matrix, a.shape[1:], "cubic", mask=mask_b)
    assert _same(b_on_a.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv.astype(bool))
    assert not valid.all() and valid.any()
    # the validity raster is what detect_change takes: NaN chi-square exactly on the invalid pixels (A's nodata strip included)
    res = eae_amd.detect_change(ta, b_on_a, divisor_a=div, divisor_b=div, nodata_a=0, mask=~valid, max_iter=3)
    bad = ~valid.cpu().numpy() | (a == 0).all(0)
    assert np.array_equal(np.isnan(res.chi2.cpu().numpy()), bad)


def test_resample_scene_nearest_of_a_class_map():
    rng = np.random.default_rng(35)
    cmap = rng.integers(0, 9, (50, 70)).astype(np.uint8)
    m = R.rigid(0.7, 1.01, (2.3, -1.6), 50, 70)
    out, valid = eae_amd.resample_scene(_dev(cmap), m, method="nearest", fill=255)
    want, wv = R.resample_ref(cmap[None], m, None, "nearest", fill=255.0)
    assert tuple(out.shape) == (50, 70) and out.dtype == torch.uint8 and valid.dtype == torch.bool
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(valid.cpu().numpy(), wv.astype(bool))
    assert set(np.unique(out.cpu().numpy())) <= set(range(9)) | {255}
    # fill defaults to the nodata value; a Registration is taken for its matrix; out_shape changes the grid
    reg = eae_amd.Registration(np.asarray(m), "affine", 0.0, np.ones(1, dtype=bool), 1, np.zeros(1))
    out, valid = eae_amd.resample_scene(_dev(cmap[None]), reg, out_shape=(20, 90), method="nearest", nodata=8)
    want, wv = R.resample_ref(cmap[None], m, (20, 90), "nearest", nodata=8, fill=8.0)
    assert tuple(out.shape) == (1, 20, 90) and np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), wv.astype(bool))
