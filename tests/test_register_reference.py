"""Co-registration (eae_amd.register; include/eae.h, "co-registration"): the two entry points in the header, the library and the
ctypes table; the argument errors of the C calls and of the four Python functions, all raised before a device is touched; and the
NumPy definition (tests/register_ref.py) itself: score, peak and parabola on hand-made tables, the trimmed fit on planted points,
resampling by the identity and by integer translations, and the reference pipeline on planted scene pairs.  No GPU needed.

The accuracy bound (`register_ref.BOUND`).  Measured with the reference pipeline on the CPU, tile 32, stride 32, radius 6, two passes, on the seven
`CASES` of `planted` at (2, 192, 256): the largest distance over the four corners of A between the fitted and the planted image of the
corner was 0.0448, 0.0260, 0.0192, 0.0203, 0.0348, 0.0860 and 0.0178 px (48 of 48 tiles accepted in every case); twice the worst,
0.172, rounded up to a power of two: 0.25 px."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd import register as G
import register_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eae_match_tiles", "eae_scene_resample")
PUBLIC = ("match_tiles", "fit_transform", "resample_scene", "coregister", "registration_table")
NP = R.NP

H, W, BOUND, CASES, MATCH, planted_case, masked_case = R.H, R.W, R.BOUND, R.CASES, R.MATCH, R.planted_case, R.masked_case


def test_symbols_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    assert "co-registration" in src
    for name in ("EAE_RESAMPLE_NEAREST 0", "EAE_RESAMPLE_BILINEAR 1", "EAE_RESAMPLE_CUBIC 2"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+"), src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.EXPORTS
    for name in PUBLIC:
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))
    for name in ("TileMatches", "Registration"):
        assert name in eae_amd.__all__ and getattr(eae_amd, name) is getattr(G, name)
    from eae_amd import build as B
    assert "eae_register.hip" in B.SOURCES


# ---------------------------------------------------------------------------------------------------- the C entry points
def _buf():
    buf = (C.c_longlong * 64)()
    return buf, C.cast(buf, C.c_void_p)


def _match_call(lib, a):
    return lib.eae_match_tiles(None, a["a"], a["dtype_a"], a["ca"], a["ha"], a["wa"], a["band_a"], a["div_a"], a["mode_a"], a["nd_a"],
                               a["rule_a"], None, a["b"], a["dtype_b"], a["cb"], a["hb"], a["wb"], a["band_b"], a["div_b"], a["mode_b"],
                               a["nd_b"], a["rule_b"], None, a["tile"], a["radius"], a["n"], a["oa"], a["ob"], a["sums"])


def test_match_tiles_rejects_bad_arguments():
    """The checks come before any device call, so they run without a device (the pointers are never dereferenced)."""
    lib = _lib.load()
    keep, p = _buf()
    odd = C.c_void_p(p.value + 1)
    ok = dict(a=p, dtype_a=1, ca=3, ha=40, wa=50, band_a=0, div_a=p, mode_a=0, nd_a=0.0, rule_a=0, b=p, dtype_b=2, cb=5, hb=30, wb=60,
              band_b=4, div_b=p, mode_b=0, nd_b=0.0, rule_b=0, tile=8, radius=2, n=4, oa=p, ob=p, sums=p)
    bad = [dict(a=None), dict(b=None), dict(div_a=None), dict(div_b=None), dict(oa=None), dict(ob=None), dict(sums=None),
           dict(dtype_a=3), dict(dtype_b=-1), dict(mode_a=3), dict(mode_b=-1), dict(rule_a=2), dict(rule_b=-1),
           dict(mode_a=2), dict(mode_a=1, nd_a=70000.0), dict(mode_a=1, nd_a=1.5),           # integer scene: no NaN, no such value
           dict(a=odd), dict(b=odd), dict(band_a=3), dict(band_a=-1), dict(band_b=5), dict(band_b=-1),
           dict(tile=3), dict(tile=65), dict(radius=-1), dict(radius=17), dict(n=0), dict(n=2 ** 20 + 1),
           dict(ca=0), dict(ca=17), dict(cb=0), dict(cb=17), dict(ha=0), dict(wa=0), dict(hb=0), dict(wb=0),
           dict(ha=2 ** 16, wa=2 ** 15), dict(hb=2 ** 16, wb=2 ** 15)]
    for change in bad:
        rc = _match_call(lib, dict(ok, **change))
        assert rc == -2 and b"match_tiles" in lib.eae_last_error(), change
    # the limits themselves pass their checks (and fail on the last one: a NULL table)
    for change in (dict(tile=4, radius=0, n=1), dict(tile=64, radius=16, n=2 ** 20), dict(ca=16, band_a=15), dict(ha=46340, wa=46340),
                   dict(mode_b=2), dict(mode_a=1, nd_a=65535.0)):
        rc = _match_call(lib, dict(ok, sums=None, **change))
        assert rc == -2 and b"NULL origin table or sums" in lib.eae_last_error(), change


def _resample_call(lib, a):
    m = None if a["matrix"] is None else (C.c_double * 6)(*a["matrix"])
    return lib.eae_scene_resample(None, a["src"], a["dtype"], a["c"], a["hs"], a["ws"], a["mode"], a["nd"], a["rule"], None, m,
                                  a["method"], a["fill"], a["dst"], a["hd"], a["wd"], None)


def test_scene_resample_rejects_bad_arguments():
    lib = _lib.load()
    keep, p = _buf()
    odd = C.c_void_p(p.value + 1)
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    ok = dict(src=p, dtype=1, c=3, hs=40, ws=50, mode=0, nd=0.0, rule=0, matrix=ident, method=1, fill=0.0, dst=p, hd=20, wd=30)
    bad = [dict(src=None), dict(dst=None), dict(matrix=None), dict(dtype=3), dict(dtype=-1), dict(method=3), dict(method=-1),
           dict(mode=3), dict(rule=2), dict(mode=2), dict(mode=1, nd=-1.0), dict(src=odd), dict(dst=odd), dict(c=0), dict(c=17),
           dict(hs=0), dict(ws=0), dict(hd=0), dict(wd=0), dict(hs=2 ** 16, ws=2 ** 15), dict(hd=2 ** 16, wd=2 ** 15),
           dict(matrix=[1.0, 0.0, float("nan"), 0.0, 1.0, 0.0]), dict(matrix=[1.0, 0.0, 0.0, float("inf"), 1.0, 0.0]),
           dict(fill=-1.0), dict(fill=65536.0), dict(fill=float("nan")), dict(dtype=0, fill=256.0)]
    for change in bad:
        rc = _resample_call(lib, dict(ok, **change))
        assert rc == -2 and b"scene_resample" in lib.eae_last_error(), change
    # what is allowed passes its check (and fails on the last one, the fill of an integer scene)
    for change in (dict(dtype=0, fill=256.0, method=0), dict(dtype=0, fill=256.0, method=2, c=16, hd=46340, wd=46340)):
        rc = _resample_call(lib, dict(ok, **change))
        assert rc == -2 and b"fill lies outside" in lib.eae_last_error(), change


# ---------------------------------------------------------------------------------------------------- the wrappers' host errors
def test_match_and_coregister_host_errors():
    a = torch.zeros((3, 40, 50), dtype=torch.uint8)
    b = torch.zeros((2, 45, 48), dtype=torch.float32)
    for f in (eae_amd.match_tiles, eae_amd.coregister):
        with pytest.raises(RuntimeError, match=r"planar tensor \[C,H,W\]"):
            f(a[0], b, tile=8)
        with pytest.raises(RuntimeError, match="scene dtype must be uint8, uint16 or float32"):
            f(a, b.to(torch.float64), tile=8)
        with pytest.raises(RuntimeError, match="bands must be in 1..16"):
            f(torch.zeros((17, 8, 8), dtype=torch.uint8), b, tile=8)
        with pytest.raises(RuntimeError, match="is empty"):
            f(a, b[:, :0], tile=8)
        with pytest.raises(RuntimeError, match="below 2\\^31"):
            f(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 2 ** 16, 2 ** 15), b, tile=8)
        for tile in (3, 65, 8.0, True):
            with pytest.raises(RuntimeError, match="tile must be an integer in 4..64"):
                f(a, b, tile=tile)
        for radius in (-1, 17, 2.0):
            with pytest.raises(RuntimeError, match="radius must be an integer in 0..16"):
                f(a, b, tile=8, radius=radius)
        with pytest.raises(RuntimeError, match="stride must be an integer"):
            f(a, b, tile=8, stride=0)
        with pytest.raises(RuntimeError, match="smaller than one 64 x 64 tile"):
            f(a, b, tile=64)
        with pytest.raises(RuntimeError, match="at most 2\\^20"):
            f(torch.zeros((1, 1, 1), dtype=torch.uint8).expand(1, 2000, 2000), b, tile=8, stride=1)
        for band in (3, -1, 1.0, (0, 2)):
            with pytest.raises(RuntimeError, match="band .* must be an integer"):
                f(a, b, tile=8, band=band)
        with pytest.raises(RuntimeError, match="divisor_b must have one value per band"):
            f(a, b, tile=8, divisor_b=[1.0, 2.0, 3.0])
        with pytest.raises(RuntimeError, match="nodata of a uint8 scene"):
            f(a, b, tile=8, nodata_a=300)
        with pytest.raises(RuntimeError, match="rule must be 'all' or 'any'"):
            f(a, b, tile=8, rule_b="some")
        with pytest.raises(RuntimeError, match=r"mask must be a \[H, W\]"):
            f(a, b, tile=8, mask_b=torch.zeros((40, 50), dtype=torch.bool))
        with pytest.raises(RuntimeError, match="mask dtype"):
            f(a, b, tile=8, mask_a=torch.zeros((40, 50), dtype=torch.int32))
        for mp in (0, 65, 2.5):
            with pytest.raises(RuntimeError, match="min_pairs must be an integer in 1..64"):
                f(a, b, tile=8, min_pairs=mp)
        for ms in ("x", float("nan"), True):
            with pytest.raises(RuntimeError, match="min_score must be a finite number"):
                f(a, b, tile=8, min_score=ms)
        for init in (np.eye(3), [[1.0, 0.0, float("inf")], [0.0, 1.0, 0.0]], "m"):
            with pytest.raises(RuntimeError, match="initial must"):
                f(a, b, tile=8, initial=init)
        with pytest.raises(RuntimeError, match="beyond the int32 range"):
            f(a, b, tile=8, initial=[[1.0, 0.0, 3e9], [0.0, 1.0, 0.0]])
        with pytest.raises(RuntimeError, match="HIP device"):              # everything is in order but the scenes are host tensors
            f(a, b, tile=8, radius=2, band=(2, 1), divisor_a=255.0, nodata_b=float("nan"), mask_a=torch.zeros((40, 50), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="keep_sums must be True or False"):
        eae_amd.match_tiles(a, b, tile=8, keep_sums=1)
    f = eae_amd.coregister
    for passes in (0, 17, 1.0):
        with pytest.raises(RuntimeError, match="passes must be an integer in 1..16"):
            f(a, b, tile=8, passes=passes)
    with pytest.raises(RuntimeError, match="model must be 'affine' or 'translation'"):
        f(a, b, tile=8, model="projective")
    with pytest.raises(RuntimeError, match="method must be 'nearest', 'bilinear' or 'cubic'"):
        f(a, b, tile=8, method="lanczos")
    with pytest.raises(RuntimeError, match="unknown argument 'tiles'"):
        f(a, b, tiles=8)
    with pytest.raises(RuntimeError, match="fill must be a number"):
        f(a, b, tile=8, fill="x")


def test_resample_scene_host_errors():
    f = eae_amd.resample_scene
    scene = torch.zeros((3, 40, 50), dtype=torch.uint16)
    ident = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]
    with pytest.raises(RuntimeError, match=r"planar tensor \[C,H,W\]"):
        f(torch.zeros((2, 3, 4, 5)), ident)
    with pytest.raises(RuntimeError, match="scene dtype must be uint8, uint16 or float32"):
        f(torch.zeros((40, 50), dtype=torch.int64), ident)                 # an int64 class map is out of scope
    with pytest.raises(RuntimeError, match="bands must be in 1..16"):
        f(torch.zeros((17, 4, 4)), ident)
    for m in (None, np.eye(2), [[1.0, 0.0, 0.0], [0.0, float("nan"), 0.0]], "m"):
        with pytest.raises(RuntimeError, match="matrix must"):
            f(scene, m)
    with pytest.raises(RuntimeError, match="method must be"):
        f(scene, ident, method="linear")
    for shape in ((0, 5), (4,), 7, (4.0, 5)):
        with pytest.raises(RuntimeError, match="out_shape"):
            f(scene, ident, out_shape=shape)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        f(scene, ident, out_shape=(2 ** 16, 2 ** 15))
    for fill in (-1, 65536, float("nan"), "x", True):
        with pytest.raises(RuntimeError, match="fill"):
            f(scene, ident, fill=fill)
    with pytest.raises(RuntimeError, match="nodata of a uint16 scene"):
        f(scene, ident, nodata=-1)
    with pytest.raises(RuntimeError, match="rule must be"):
        f(scene, ident, rule="none")
    with pytest.raises(RuntimeError, match=r"mask must be a \[H, W\]"):
        f(scene, ident, mask=torch.zeros((50, 40), dtype=torch.bool))
    for s in (scene, scene[0].to(torch.uint8), torch.zeros((2, 8, 8))):     # in order, but a host tensor
        with pytest.raises(RuntimeError, match="HIP device"):
            f(s, ident, method="nearest", fill=float("nan") if s.dtype == torch.float32 else 7)


def _matches(pa, pb, ok=None):
    n = len(pa)
    return G.TileMatches(np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64), np.zeros((n, 2), dtype=np.int64),
                         np.zeros((n, 2)), np.ones(n), np.ones(n, dtype=bool) if ok is None else ok,
                         G.TileGeometry(8, 8, 2, (1, n), (8, 8 * n)), None)


def test_fit_transform_host_errors():
    f = eae_amd.fit_transform
    pa = np.array([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0], [10.0, 10.0]])
    good = _matches(pa, pa + 1.0)
    with pytest.raises(RuntimeError, match="model must be"):
        f(good, model="rigid")
    for trim in (0.0, -1.0, float("inf"), "x"):
        with pytest.raises(RuntimeError, match="trim must be a finite number > 0"):
            f(good, trim=trim)
    with pytest.raises(RuntimeError, match="max_rounds must be an integer"):
        f(good, max_rounds=-1)
    for mp in (2, 0, 3.0):
        with pytest.raises(RuntimeError, match="min_points must be an integer in 3"):
            f(good, min_points=mp)
    with pytest.raises(RuntimeError, match="matches must be a TileMatches"):
        f((pa, pa))
    with pytest.raises(RuntimeError, match="4 of 4 tiles remain .* min_points is 5"):
        f(good, min_points=5)
    with pytest.raises(RuntimeError, match="0 of 4 tiles remain \\(0 were ok\\)"):
        f(_matches(pa, pa, np.zeros(4, dtype=bool)), model="translation")
    with pytest.raises(RuntimeError, match="2 of 4 tiles remain"):
        f(_matches(pa, pa, np.array([True, True, False, False])))
    line = np.stack([np.arange(6.0), 2.0 * np.arange(6.0) + 1.0], 1)
    with pytest.raises(RuntimeError, match="not on one line, 6 collinear remain"):
        f(_matches(line, line + 0.5))
    assert np.allclose(f(_matches(line, line + 0.5), model="translation").matrix, [[1, 0, 0.5], [0, 1, 0.5]])


# ---------------------------------------------------------------------------------------------------- score, peak, parabola
def _table(n, sa, sb, saa, sbb, sab):
    return np.array([n, sa, sb, saa, sbb, sab], dtype=np.int64)


def test_scores_on_hand_made_tables():
    # a = (1, 2, 3, 4), b = 2 a + 1: perfectly correlated; b' = (4, 3, 2, 1): -1; b'' = (1, 3, 1, 3): num = 4 * 22 - 10 * 8 = 8
    a = np.array([1, 2, 3, 4])
    rows = []
    for b in (2 * a + 1, a[::-1], np.array([1, 3, 1, 3])):
        rows.append(_table(4, a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum()))
    rows.append(_table(4, 8, 10, 16, 30, 20))                              # a constant: zero variance
    rows.append(_table(3, 6, 6, 14, 14, 14))                               # too few pairs
    rows.append(_table(0, 0, 0, 0, 0, 0))
    sc = R.scores(np.array(rows)[None], 4)[0]
    assert sc[0] == 1.0 and sc[1] == -1.0 and sc[2] == 8 / np.sqrt(20.0 * 16.0)
    assert np.isneginf(sc[3:]).all()
    # the largest sums the kernel can produce stay exact: 4096 pairs of 65535
    big = _table(4096, 4096 * 65535, 4096 * 65535, 4096 * 65535 ** 2, 4096 * 65535 ** 2, 4096 * 65535 ** 2)
    assert np.isneginf(R.scores(big[None, None], 1)).all() and 4096 * 4096 * 65535 ** 2 < 2 ** 57


def test_peaks_ties_border_and_parabola():
    radius, nd = 2, 5
    sc = np.full((6, nd, nd), 0.1)
    sc[0, 2, 3] = 0.9; sc[0, 2, 2] = 0.5; sc[0, 2, 4] = 0.7; sc[0, 1, 3] = 0.6; sc[0, 3, 3] = 0.6        # noqa: E702
    sc[1, 1, 1] = sc[1, 3, 2] = sc[1, 1, 3] = 0.8                          # a tie: the lowest entry wins
    sc[2, 0, 2] = 0.95                                                     # a peak on the border
    sc[3] = R.NEG                                                          # no score at all
    sc[4, 2, 2] = 0.69                                                     # below min_score
    sc[5, 2, 2] = 0.9; sc[5, 2, 1] = R.NEG; sc[5, 1, 2] = 0.9              # noqa: E702  a -inf neighbour; a flat top in y
    off, sub, s0, ok = R.peaks(sc.reshape(6, -1), radius, 0.7)
    assert off.tolist() == [[0, 1], [-1, -1], [-2, 0], [-2, -2], [0, 0], [-1, 0]]
    assert ok.tolist() == [True, True, False, False, False, True]
    assert s0[:3].tolist() == [0.9, 0.8, 0.95] and np.isneginf(s0[3]) and s0[4] == 0.69
    assert sub[0, 0] == 0.0 and sub[0, 1] == pytest.approx(0.5 * (0.5 - 0.7) / (0.5 - 1.8 + 0.7))
    assert sub[2, 0] == 0.0                                                # the neighbour above the border is missing
    assert (sub[3] == 0.0).all()
    # tile 5: the tie in y goes to the upper row (entry 7 before 12); its y parabola sees 0.1, 0.9, 0.9 and clamps to +0.5
    assert sub[5].tolist() == [0.5, pytest.approx(0.5 * (0.1 - 0.1) / (0.1 - 1.8 + 0.1))]
    # radius 0: the only entry is no border
    off, sub, s0, ok = R.peaks(np.array([[0.8], [0.2]]), 0, 0.7)
    assert off.tolist() == [[0, 0], [0, 0]] and ok.tolist() == [True, False] and (sub == 0.0).all()
    # the package's parabola is the reference's
    lo, mid, hi = np.array([0.5, R.NEG, 0.3, 0.3]), np.array([0.9, 0.9, 0.3, 0.9]), np.array([0.7, 0.2, 0.3, 0.9])
    assert np.array_equal(G._parabola(lo, mid, hi), R._parabola(lo, mid, hi))


# ---------------------------------------------------------------------------------------------------- the fit
def _grid_points(n=6):
    x, y = np.meshgrid(np.arange(n) * 32.0 + 15.5, np.arange(n) * 32.0 + 15.5)
    return np.stack([x.reshape(-1), y.reshape(-1)], 1)


def test_fit_recovers_a_planted_map():
    truth = R.rigid(0.5, 1.005, (3.4, -2.7), 192, 192)
    pa = _grid_points()
    pb = np.stack(R.apply(truth, pa[:, 0], pa[:, 1]), 1)
    for fit in (lambda: R.fit_transform_ref(pa, pb)[0], lambda: eae_amd.fit_transform(_matches(pa, pb)).matrix):
        assert np.abs(fit() - truth).max() < 1e-10
    reg = eae_amd.fit_transform(_matches(pa, pb))
    assert reg.inliers.all() and reg.n_tiles == 36 and reg.rmse < 1e-10 and reg.model == "affine"
    shift = np.array([[1.0, 0.0, -4.25], [0.0, 1.0, 7.5]])
    pb = np.stack(R.apply(shift, pa[:, 0], pa[:, 1]), 1)
    assert np.abs(eae_amd.fit_transform(_matches(pa, pb), model="translation").matrix - shift).max() < 1e-12
    assert np.abs(R.fit_transform_ref(pa, pb, "translation")[0] - shift).max() < 1e-12


def test_fit_rejects_a_fifth_of_outliers():
    truth = R.rigid(-0.4, 0.997, (-2.2, 5.1), 192, 192)
    pa = _grid_points()
    rng = np.random.default_rng(3)
    pb = np.stack(R.apply(truth, pa[:, 0], pa[:, 1]), 1) + 0.01 * rng.standard_normal((36, 2))
    out = rng.choice(36, 7, replace=False)
    pb[out] += rng.uniform(2.0, 6.0, (7, 2)) * rng.choice([-1.0, 1.0], (7, 2))
    ok = np.ones(36, dtype=bool)
    ok[5] = False                                                          # a tile that was not ok takes no part
    pb[5] += 100.0
    reg = eae_amd.fit_transform(_matches(pa, pb, ok))
    m, inl, res, rmse = R.fit_transform_ref(pa[ok], pb[ok])
    assert np.abs(reg.matrix - m).max() < 1e-12 and reg.rmse == pytest.approx(rmse)
    assert R.corner_error(reg.matrix, truth, 192, 192) < 0.03
    want = ok.copy()
    want[out] = False
    assert np.array_equal(reg.inliers, want) and np.isnan(reg.residuals[5]) and np.isfinite(reg.residuals[ok]).all()
    # without trimming rounds the outliers stay and the fit is off
    assert R.corner_error(eae_amd.fit_transform(_matches(pa, pb, ok), max_rounds=0).matrix, truth, 192, 192) > 0.5
    text = eae_amd.registration_table(reg, (192, 192))
    assert "inliers" in text and "28 of 36 tiles" in text and "rmse" in text and "affine" in text


# ---------------------------------------------------------------------------------------------------- resampling
def _scene(rng, kind, shape):
    if kind == "f32":
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, 256 if kind == "u8" else 65536, shape).astype(NP[kind])


@pytest.mark.parametrize("kind", ["u8", "u16", "f32"])
@pytest.mark.parametrize("method", ["nearest", "bilinear", "cubic"])
def test_resample_ref_identity_and_integer_shifts(kind, method):
    rng = np.random.default_rng(7)
    src = _scene(rng, kind, (3, 11, 17))
    if kind == "f32":
        src[0, 2, 3] = -0.0
    fill = 9.0
    out, valid = R.resample_ref(src, [[1, 0, 0], [0, 1, 0]], method=method, fill=fill)
    assert out.dtype == src.dtype and out.tobytes() == src.tobytes() and valid.all()
    for dx, dy in ((3, 0), (-2, 5), (0, -4), (20, 0)):
        out, valid = R.resample_ref(src, [[1, 0, dx], [0, 1, dy]], method=method, fill=fill)
        want = np.full_like(src, fill)
        wv = np.zeros((11, 17), dtype=np.uint8)
        ys, xs = np.arange(11), np.arange(17)
        iy, ix = (ys + dy >= 0) & (ys + dy < 11), (xs + dx >= 0) & (xs + dx < 17)
        if iy.any() and ix.any():
            want[:, iy[:, None] & ix[None, :]] = src[:, (ys + dy)[iy]][:, :, (xs + dx)[ix]].reshape(3, -1)
            wv[iy[:, None] & ix[None, :]] = 1
        assert out.tobytes() == want.tobytes() and np.array_equal(valid, wv), (dx, dy)


def test_resample_ref_weights_and_validity():
    src = np.array([[[0, 100, 0, 0], [0, 0, 0, 0], [0, 65535, 65535, 0]]], dtype=np.uint16)
    # half a pixel to the right in row 0: bilinear averages; cubic overshoots below 0 and is clamped
    out, valid = R.resample_ref(src, [[1, 0, 0.5], [0, 1, 0]], method="bilinear")
    assert out[0, 0].tolist() == [50, 50, 0, 0] and valid[0].tolist() == [1, 1, 1, 0]
    out, valid = R.resample_ref(src, [[1, 0, 0.5], [0, 1, 0]], method="cubic", out_shape=(3, 2))
    assert valid.tolist() == [[0, 1]] * 3 and out[0, 0, 1] == 56 and out[0, 2, 1] == 65535       # 9/16 * 100; 9/8 * 65535 clamped
    wts = R._axis(np.array([1.5]), "cubic")[1]
    assert [float(w[0]) for w in wts] == [-0.0625, 0.5625, 0.5625, -0.0625]
    # a nodata pixel under a non-zero weight invalidates the output; under a zero weight it does not
    out, valid = R.resample_ref(src, [[1, 0, 0.5], [0, 1, 0]], method="bilinear", nodata=100, fill=7)
    assert valid[0].tolist() == [0, 0, 1, 0] and out[0, 0].tolist() == [7, 7, 0, 7]
    out, valid = R.resample_ref(src, [[1, 0, 0], [0, 1, 0]], method="cubic", nodata=100, fill=7)
    assert valid[0].tolist() == [1, 0, 1, 1]


# ---------------------------------------------------------------------------------------------------- the reference pipeline
@pytest.fixture(scope="module")
def reference_runs():
    """The reference pipeline on every case, once: {seed: (matrix, ok, inliers, truth)}."""
    runs = {}
    for case in CASES:
        a, b, div, truth = planted_case(case)
        runs[case[0]] = R.coregister_ref(a, b, divisor_a=div, divisor_b=div, **MATCH) + (truth,)
    return runs


@pytest.mark.parametrize("case", CASES, ids=[f"seed{c[0]}-{c[1]}" for c in CASES])
def test_reference_pipeline_recovers_the_planted_map(reference_runs, case):
    m, ok, inl, truth = reference_runs[case[0]]
    print("corner error %.4f px, %d of %d tiles ok, %d inliers" % (R.corner_error(m, truth, H, W), ok.sum(), len(ok), inl.sum()))
    assert len(ok) == 48 and ok.sum() >= 36                                # at most one quarter of the tiles rejected
    assert R.corner_error(m, truth, H, W) <= BOUND


def test_reference_pipeline_with_nodata_and_mask():
    a, b, div, truth, mask_b = masked_case()
    m, ok, inl = R.coregister_ref(a, b, divisor_a=div, divisor_b=div, nodata_a=0, mask_b=mask_b, **MATCH)
    print("corner error %.4f px, %d of %d tiles ok, %d inliers" % (R.corner_error(m, truth, H, W), ok.sum(), len(ok), inl.sum()))
    assert ok.sum() >= 6 and not ok.reshape(6, 8)[:, 0].any()              # the tiles inside the nodata strip have no pairs
    assert R.corner_error(m, truth, H, W) <= BOUND
