"""Co-registration of two scenes of one place on the device: tie points, a robust affine fit, and resampling onto the other grid.

Two acquisitions are never aligned to the pixel, and every two-date function of this package (`change.detect_change`,
`change.class_transitions`, `change.invariant_regression`) reads a misalignment as change along every edge.  This module aligns scene
B to scene A's grid: the two kernels of the C library (include/eae.h, "co-registration") read the integer planar
[C, H, W] scenes in place, and the small tables between them are handled on the host in float64.

Conventions: pixel (y, x) has its centre at the point (x, y).  A transform is a float64 [2, 3] matrix M that maps a point of the
DESTINATION grid to the SOURCE: sx = M00 x + M01 y + M02, sy = M10 x + M11 y + M12; for co-registration the destination is A's grid
and the source is B, so M says where in B a pixel of A lies.  Points are (x, y), offsets and sub-pixel parts (dy, dx).

- `match_tiles`: zero-mean normalised cross-correlation of a grid of tiles of A with B over a search window; peak and sub-pixel part;
- `fit_transform`: trimmed least squares over the accepted tiles, host only;
- `resample_scene`: nearest, bilinear or cubic-convolution resampling through a matrix, with a validity raster;
- `coregister`: match, fit, match again from the fit, resample B onto A (`report.registration_table` prints the result).
"""
from __future__ import annotations

import inspect
import math
import numbers
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check
from ._args import _int_arg
from .engine import _ptr, _stream, _require_gpu

MAX_BANDS = 16
MIN_TILE, MAX_TILE, MAX_RADIUS, MAX_TILES = 4, 64, 16, 2 ** 20
METHODS = {"nearest": 0, "bilinear": 1, "cubic": 2}
MODELS = ("affine", "translation")
RESIDUAL_FLOOR = 0.05         # pixels: the trimming threshold never falls below this
_PIXEL_LIMIT = 2 ** 31
_IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


class TileGeometry(NamedTuple):
    """tile, stride, radius; grid = (tiles down, tiles across); shape = (H, W) of scene A."""
    tile: int
    stride: int
    radius: int
    grid: tuple
    shape: tuple


class TileMatches(NamedTuple):
    """All NumPy, one row per tile (row-major over the grid).  centres float64 [n, 2]: the tile's centre (x, y) in A; points float64
    [n, 2]: the matched point (x, y) in B; offsets int64 [n, 2] = (dy, dx) of the peak from the search window's centre; sub float64
    [n, 2] = (dy, dx) in [-0.5, 0.5]; scores float64 [n] (-inf: no score); ok bool [n]; geometry: `TileGeometry`; sums: the raw
    int64 [n, (2R + 1)^2, 6] table on the device with keep_sums=True, else None."""
    centres: np.ndarray
    points: np.ndarray
    offsets: np.ndarray
    sub: np.ndarray
    scores: np.ndarray
    ok: np.ndarray
    geometry: TileGeometry
    sums: object


class Registration(NamedTuple):
    """matrix float64 [2, 3] (a point of A -> its place in B); model; rmse of the inliers in pixels; inliers bool [n_tiles];
    n_tiles; residuals float64 [n_tiles] (NaN for a tile that was not ok)."""
    matrix: np.ndarray
    model: str
    rmse: float
    inliers: np.ndarray
    n_tiles: int
    residuals: np.ndarray


class _Args(NamedTuple):
    match: object
    fit: object
    resample: object


# ---------------------------------------------------------------------------------------------------- host-side validation
def _matrix_arg(matrix, name="matrix"):
    if isinstance(matrix, Registration):
        matrix = matrix.matrix
    if isinstance(matrix, torch.Tensor):
        matrix = matrix.detach().cpu().numpy()
    try:
        m = np.array(matrix, dtype=np.float64)
    except (TypeError, ValueError):
        raise RuntimeError(f"{name} must be a 2 x 3 matrix or a Registration") from None
    if m.shape != (2, 3) or not np.isfinite(m).all():
        raise RuntimeError(f"{name} must hold 2 x 3 finite numbers, got shape {list(m.shape)}")
    return m


def _real_arg(v, name, lo=None, lo_open=False):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)) \
            or (lo is not None and (float(v) <= lo if lo_open else float(v) < lo)):
        raise RuntimeError(f"{name} must be a finite number" + ("" if lo is None else f" {'>' if lo_open else '>='} {lo}") + f", got {v!r}")
    return float(v)


def _scene_arg(scene, name):
    from .scene import _check_scene
    _check_scene(scene)
    c, h, w = (int(v) for v in scene.shape)
    if not 1 <= c <= MAX_BANDS:
        raise RuntimeError(f"{name}: the number of bands must be in 1..16, got {c}")
    if h < 1 or w < 1:
        raise RuntimeError(f"{name} is empty: {[c, h, w]}")
    if h * w >= _PIXEL_LIMIT:
        raise RuntimeError(f"{name} has {h} x {w} pixels: H * W must be below 2^31")
    return c, h, w


def _host_args(match=None, fit=None, resample=None):
    """Every host-side check of the registration functions; no device is touched.  Each argument is None or the dict of one
    function's raw arguments; the result holds the checked form of each."""
    from .change import _divisor_arg
    from .scene import _mask_arg, _nodata_arg, _rule_arg, _INT_RANGE
    out = [None, None, None]
    if match is not None:
        a, b = match["a"], match["b"]
        ca, ha, wa = _scene_arg(a, "scene a")
        cb, hb, wb = _scene_arg(b, "scene b")
        if a.device != b.device:
            raise RuntimeError(f"scene a is on {a.device}, scene b on {b.device}")
        tile = _int_arg(match["tile"], "tile", MIN_TILE, MAX_TILE)
        stride = tile if match["stride"] is None else _int_arg(match["stride"], "stride", 1, 2 ** 31 - 1)
        radius = _int_arg(match["radius"], "radius", 0, MAX_RADIUS)
        band = match["band"]
        band_a, band_b = band if isinstance(band, (tuple, list)) and len(band) == 2 else (band, band)
        band_a, band_b = _int_arg(band_a, "band (scene a)", 0, ca - 1), _int_arg(band_b, "band (scene b)", 0, cb - 1)
        if tile > ha or tile > wa:
            raise RuntimeError(f"scene a ({ha} x {wa}) is smaller than one {tile} x {tile} tile")
        grid = ((ha - tile) // stride + 1, (wa - tile) // stride + 1)
        if grid[0] * grid[1] > MAX_TILES:
            raise RuntimeError(f"{grid[0]} x {grid[1]} tiles: at most 2^20 (raise stride)")
        min_pairs = tile * tile // 2 if match["min_pairs"] is None else _int_arg(match["min_pairs"], "min_pairs", 1, tile * tile)
        min_score = _real_arg(match["min_score"], "min_score")
        if not isinstance(match["keep_sums"], bool):
            raise RuntimeError(f"keep_sums must be True or False, got {match['keep_sums']!r}")
        initial = _IDENTITY if match["initial"] is None else _matrix_arg(match["initial"], "initial")
        ys, xs = np.arange(grid[0], dtype=np.int64) * stride, np.arange(grid[1], dtype=np.int64) * stride
        oa = np.stack(np.meshgrid(ys, xs, indexing="ij"), -1).reshape(-1, 2)
        half = (tile - 1) / 2.0
        cx, cy = oa[:, 1] + half, oa[:, 0] + half
        mx = (initial[0, 0] * cx + initial[0, 1] * cy) + initial[0, 2]
        my = (initial[1, 0] * cx + initial[1, 1] * cy) + initial[1, 2]
        ob = np.stack([np.rint(my - half), np.rint(mx - half)], 1)
        if np.abs(ob).max() > 2 ** 31 - 1 - MAX_TILE - MAX_RADIUS:
            raise RuntimeError("initial sends a tile beyond the int32 range")
        out[0] = dict(a=a, b=b, dims_a=(ca, ha, wa), dims_b=(cb, hb, wb), tile=tile, stride=stride, radius=radius, band_a=band_a,
                      band_b=band_b, div_a=_divisor_arg(match["divisor_a"], ca, "divisor_a"),
                      div_b=_divisor_arg(match["divisor_b"], cb, "divisor_b"),
                      nodata_a=_nodata_arg(a.dtype, match["nodata_a"]) + (_rule_arg(match["rule_a"]),),
                      nodata_b=_nodata_arg(b.dtype, match["nodata_b"]) + (_rule_arg(match["rule_b"]),),
                      mask_a=_mask_arg(a, match["mask_a"]), mask_b=_mask_arg(b, match["mask_b"]), min_pairs=min_pairs,
                      min_score=min_score, keep_sums=match["keep_sums"], grid=grid, origins_a=oa, origins_b=ob.astype(np.int64))
    if fit is not None:
        if fit["model"] not in MODELS:
            raise RuntimeError(f"model must be 'affine' or 'translation', got {fit['model']!r}")
        need = 3 if fit["model"] == "affine" else 1
        out[1] = dict(model=fit["model"], trim=_real_arg(fit["trim"], "trim", 0.0, lo_open=True),
                      max_rounds=_int_arg(fit["max_rounds"], "max_rounds", 0, 2 ** 31 - 1),
                      min_points=need if fit["min_points"] is None else _int_arg(fit["min_points"], "min_points", need, 2 ** 31 - 1))
        if "passes" in fit:
            out[1]["passes"] = _int_arg(fit["passes"], "passes", 1, 16)
    if resample is not None:
        scene = resample["scene"]
        flat = isinstance(scene, torch.Tensor) and scene.dim() == 2
        if flat:
            scene = scene.unsqueeze(0)
        c, h, w = _scene_arg(scene, "scene")
        if resample["method"] not in METHODS:
            raise RuntimeError(f"method must be 'nearest', 'bilinear' or 'cubic', got {resample['method']!r}")
        shape = resample["out_shape"]
        if shape is None:
            shape = (h, w)
        if not isinstance(shape, (tuple, list, torch.Size)) or len(shape) != 2:
            raise RuntimeError(f"out_shape must be (H, W), got {shape!r}")
        hd, wd = _int_arg(shape[0], "out_shape[0]", 1, 2 ** 31 - 1), _int_arg(shape[1], "out_shape[1]", 1, 2 ** 31 - 1)
        if hd * wd >= _PIXEL_LIMIT:
            raise RuntimeError(f"out_shape has {hd} x {wd} pixels: H * W must be below 2^31")
        nodata = _nodata_arg(scene.dtype, resample["nodata"]) + (_rule_arg(resample["rule"]),)
        fill = resample["fill"]
        if fill is None:
            fill = 0.0 if resample["nodata"] is None else float(resample["nodata"])
        if isinstance(fill, bool) or not isinstance(fill, numbers.Real):
            raise RuntimeError(f"fill must be a number, got {fill!r}")
        fill = float(fill)
        if scene.dtype in _INT_RANGE and not 0 <= fill <= _INT_RANGE[scene.dtype]:
            raise RuntimeError(f"fill of a {str(scene.dtype).replace('torch.', '')} scene must lie in 0..{_INT_RANGE[scene.dtype]}, "
                               f"got {fill!r}")
        matrix = None if resample["matrix"] is None else _matrix_arg(resample["matrix"])
        out[2] = dict(scene=scene, flat=flat, dims=(c, h, w), matrix=matrix, method=METHODS[resample["method"]], shape=(hd, wd),
                      nodata=nodata, mask=_mask_arg(scene, resample["mask"]), fill=fill)
    return _Args(*out)


# ---------------------------------------------------------------------------------------------------- matching
def _match(p):
    """One matching pass of checked arguments: `TileMatches`.  One launch, a handful of torch operations on the table, one read-back."""
    from .scene import _DTYPES
    a, b = p["a"], p["b"]
    dev = a.device
    _require_gpu(dev)
    lib = _lib.load()
    tile, radius = p["tile"], p["radius"]
    nd = 2 * radius + 1
    n = int(p["origins_a"].shape[0])
    with torch.cuda.device(dev):
        a, b = a.contiguous(), b.contiguous()
        div_a, div_b = p["div_a"].to(dev).contiguous(), p["div_b"].to(dev).contiguous()
        oa = torch.as_tensor(p["origins_a"].astype(np.int32), device=dev)
        ob = torch.as_tensor(p["origins_b"].astype(np.int32), device=dev)
        sums = torch.empty((n, nd * nd, 6), dtype=torch.int64, device=dev)
        check(lib.eae_match_tiles(_stream(), _ptr(a), _DTYPES[a.dtype], *p["dims_a"], p["band_a"], _ptr(div_a), *p["nodata_a"],
                                  _ptr(p["mask_a"]), _ptr(b), _DTYPES[b.dtype], *p["dims_b"], p["band_b"], _ptr(div_b), *p["nodata_b"],
                                  _ptr(p["mask_b"]), tile, radius, n, _ptr(oa), _ptr(ob), _ptr(sums)))
        # the score in float64 from exact int64 numerator and variances (all below 2^57)
        cnt, sa, sb, saa, sbb, sab = sums.unbind(-1)
        num, va, vb = cnt * sab - sa * sb, cnt * saa - sa * sa, cnt * sbb - sb * sb
        score = num.double() / torch.sqrt(va.double() * vb.double())
        score = torch.where((cnt < p["min_pairs"]) | (va <= 0) | (vb <= 0), float("-inf"), score)
        best = score.max(1).values
        entry = torch.arange(nd * nd, device=dev).expand(n, -1)
        flat = torch.where(score == best[:, None], entry, nd * nd).min(1).values              # the lowest entry on a tie
        pad = torch.nn.functional.pad(score.view(n, nd, nd), (1, 1, 1, 1), value=float("-inf"))
        t, py, px = torch.arange(n, device=dev), flat // nd, flat % nd
        small = torch.stack([flat.double(), pad[t, py + 1, px + 1], pad[t, py, px + 1], pad[t, py + 2, px + 1], pad[t, py + 1, px],
                             pad[t, py + 1, px + 2]], 1).cpu().numpy()
    flat = small[:, 0].astype(np.int64)
    py, px, s0 = flat // nd, flat % nd, small[:, 1]
    sub = np.stack([_parabola(small[:, 2], s0, small[:, 3]), _parabola(small[:, 4], s0, small[:, 5])], 1)
    border = (py == 0) | (py == nd - 1) | (px == 0) | (px == nd - 1)
    ok = np.isfinite(s0) & (s0 >= p["min_score"]) & ~(border & (radius > 0))
    off = np.stack([py - radius, px - radius], 1)
    half = (tile - 1) / 2.0
    oa, ob = p["origins_a"], p["origins_b"]
    centres = np.stack([oa[:, 1] + half, oa[:, 0] + half], 1)
    points = np.stack([ob[:, 1] + half + off[:, 1] + sub[:, 1], ob[:, 0] + half + off[:, 0] + sub[:, 0]], 1)
    geometry = TileGeometry(tile, p["stride"], radius, p["grid"], p["dims_a"][1:])
    return TileMatches(centres, points, off, sub, s0, ok, geometry, sums if p["keep_sums"] else None)


def _parabola(lo, mid, hi):
    """The vertex of the parabola through (-1, lo), (0, mid), (1, hi), clamped to +-0.5; 0 where a value is not finite or the
    denominator is 0."""
    with np.errstate(all="ignore"):
        den = lo - 2.0 * mid + hi
        sub = 0.5 * (lo - hi) / den
    bad = ~np.isfinite(lo) | ~np.isfinite(hi) | ~np.isfinite(mid) | (den == 0.0) | ~np.isfinite(sub)
    return np.where(bad, 0.0, np.clip(sub, -0.5, 0.5))


def match_tiles(a, b, tile=64, stride=None, radius=8, band=0, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask_a=None,
                mask_b=None, rule_a="all", rule_b="all", initial=None, min_pairs=None, min_score=0.7, keep_sums=False):
    """`TileMatches` between scene A and scene B ([C, H, W] uint8, uint16 or float32 on one device; shapes, dtypes and band counts
    may differ).  The tiles are the regular grid of ``tile`` x ``tile`` templates at ``stride`` (default: ``tile``) that lie wholly
    inside A.  Each is compared with B at every integer offset within ``radius`` of its search window's centre, which lies at the
    rounded image of the tile's centre under ``initial`` (a matrix or a `Registration`; None: the identity), so a second pass refines
    a first, and a known coarse offset larger than the radius can be given.

    One band of each scene is matched (``band``: an index, or a pair for the two scenes) as the 16-bit feature
    rint(65535 clip(v / divisor, 0, 1)); a pixel is invalid as in `change.joint_moments` (``nodata_*`` / ``rule_*`` over all bands of
    its scene, ``mask_*``, a non-finite float32 band, outside the raster) and a pair counts when both its pixels are valid.  The kernel
    returns exact integer sums; the score num / sqrt(va vb), num = n sum ab - sum a sum b, is formed from exact int64 terms in float64
    on the device and is -inf where fewer than ``min_pairs`` (default tile^2 / 2) pairs are valid or a variance is 0.  The peak is the
    argmax (the lowest entry on a tie); the sub-pixel part a parabola through the peak and its two neighbours per axis, clamped to
    +-0.5, and 0 where the denominator is 0 or a neighbour is -inf.  A tile is ``ok`` when its score is finite and >= ``min_score``
    and, for radius > 0, the peak is not on the border of the search window.

    Everything small comes back as NumPy: the call synchronises the host once, to read 6 numbers per tile."""
    p = _host_args(match=dict(a=a, b=b, tile=tile, stride=stride, radius=radius, band=band, divisor_a=divisor_a, divisor_b=divisor_b,
                              nodata_a=nodata_a, nodata_b=nodata_b, mask_a=mask_a, mask_b=mask_b, rule_a=rule_a, rule_b=rule_b,
                              initial=initial, min_pairs=min_pairs, min_score=min_score, keep_sums=keep_sums)).match
    return _match(p)


# ---------------------------------------------------------------------------------------------------- the fit
def _solve(pa, pb, model):
    if model == "affine":
        design = np.concatenate([pa, np.ones((len(pa), 1))], 1)
        sv = np.linalg.svd(design - design.mean(0), compute_uv=False) if len(pa) >= 3 else np.zeros(3)       # centred: rank 2 unless on a line
        if sv[1] <= 1e-9 * max(sv[0], 1.0):
            raise RuntimeError(f"fit_transform: an affine model needs 3 tiles that are not on one line, {len(pa)} "
                               f"{'collinear ' if len(pa) >= 3 else ''}remain")
        return np.linalg.lstsq(design, pb, rcond=None)[0].T.copy()
    if len(pa) < 1:
        raise RuntimeError("fit_transform: a translation needs 1 tile, none remains")
    d = (pb - pa).mean(0)
    return np.array([[1.0, 0.0, d[0]], [0.0, 1.0, d[1]]])


def _fit(matches, f):
    if not isinstance(matches, TileMatches):
        raise RuntimeError("matches must be a TileMatches (match_tiles)")
    ok = np.asarray(matches.ok, dtype=bool)
    pa, pb = np.asarray(matches.centres, dtype=np.float64)[ok], np.asarray(matches.points, dtype=np.float64)[ok]
    inl = np.ones(len(pa), dtype=bool)
    rounds = 0
    while True:
        if inl.sum() < f["min_points"]:
            raise RuntimeError(f"fit_transform: {int(inl.sum())} of {len(ok)} tiles remain ({int(ok.sum())} were ok), min_points is "
                               f"{f['min_points']}")
        m = _solve(pa[inl], pb[inl], f["model"])
        res = np.hypot((m[0, 0] * pa[:, 0] + m[0, 1] * pa[:, 1]) + m[0, 2] - pb[:, 0],
                       (m[1, 0] * pa[:, 0] + m[1, 1] * pa[:, 1]) + m[1, 2] - pb[:, 1])
        keep = inl & (res <= max(f["trim"] * 1.4826 * float(np.median(res[inl])), RESIDUAL_FLOOR))
        if rounds == f["max_rounds"] or keep.sum() == inl.sum():
            break
        inl, rounds = keep, rounds + 1
    inliers = np.zeros(len(ok), dtype=bool)
    inliers[np.flatnonzero(ok)[inl]] = True
    residuals = np.full(len(ok), np.nan)
    residuals[ok] = res
    return Registration(m, f["model"], float(np.sqrt((res[inl] ** 2).mean())), inliers, len(ok), residuals)


def fit_transform(matches, model="affine", trim=3.0, max_rounds=10, min_points=None):
    """`Registration` from `TileMatches`, on the host in float64: least squares points = M centres over the ``ok`` tiles ("affine":
    six parameters; "translation": the mean shift), then at most ``max_rounds`` times drop the tiles whose residual exceeds
    ``trim`` x 1.4826 x the median residual of the current inliers (not below 0.05 px) and refit, until nothing is dropped.
    Raises, naming the cause, when fewer than 3 tiles that are not on one line remain for "affine", fewer than 1 for "translation", or
    fewer than ``min_points``."""
    f = _host_args(fit=dict(model=model, trim=trim, max_rounds=max_rounds, min_points=min_points)).fit
    return _fit(matches, f)


# ---------------------------------------------------------------------------------------------------- resampling
def _resample(r, matrix):
    from .scene import _DTYPES
    scene = r["scene"]
    dev = scene.device
    _require_gpu(dev)
    lib = _lib.load()
    c, h, w = r["dims"]
    hd, wd = r["shape"]
    with torch.cuda.device(dev):
        scene = scene.contiguous()
        dst = torch.empty((c, hd, wd), dtype=scene.dtype, device=dev)
        valid = torch.empty((hd, wd), dtype=torch.uint8, device=dev)
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        check(lib.eae_scene_resample(_stream(), _ptr(scene), _DTYPES[scene.dtype], c, h, w, *r["nodata"], _ptr(r["mask"]),
                                     m.ctypes.data, r["method"], r["fill"], _ptr(dst), hd, wd, _ptr(valid)))
    return (dst[0] if r["flat"] else dst), valid.view(torch.bool)



def resample_scene(scene, matrix, out_shape=None, method="bilinear", nodata=None, mask=None, rule="all", fill=None):
    """(scene on the destination grid, valid bool [Hd, Wd]), both on the device: destination pixel (y, x) is taken from the source
    at (sx, sy) = ``matrix`` (x, y) (a [2, 3] matrix or a `Registration`) by ``method`` "nearest", "bilinear" or "cubic" (Catmull-Rom
    cubic convolution, which overshoots; integer dtypes round half to even and clamp).  ``out_shape``: (Hd, Wd), default the source's.
    The result has the source's dtype.  A destination pixel is valid when every tap with a non-zero weight is a valid source pixel
    (inside the raster, ``mask`` clear, ``nodata`` / ``rule`` silent, float32 finite); an invalid one gets ``fill`` (default: the
    nodata value where one is given, else 0; NaN is allowed for float32) in every band.  ``valid`` is what `change.detect_change`
    takes as ``mask=~valid``.  The arithmetic is float64 in a fixed order: the identity returns the source bit for bit.

    A [H, W] raster of the three dtypes is taken as one band and returned as [Hd, Wd], so that a class map stored as uint8 can be
    warped with method="nearest" (int64 class maps are out of scope).  No host synchronisation."""
    r = _host_args(resample=dict(scene=scene, matrix=matrix, out_shape=out_shape, method=method, nodata=nodata, mask=mask, rule=rule,
                                 fill=fill)).resample
    if r["matrix"] is None:
        raise RuntimeError("matrix must be a 2 x 3 matrix or a Registration")
    return _resample(r, r["matrix"])


def coregister(a, b, passes=2, model="affine", method="bilinear", trim=3.0, max_rounds=10, min_points=None, fill=None, **match_args):
    """(b_on_a, valid, registration): `match_tiles` and `fit_transform`, ``passes`` times, each pass starting from the fit before it
    (the second pass is what recovers rotation and scale: its search windows follow the first fit, so its tiles match near their
    centres); then `resample_scene` of B onto A's grid.  ``match_args`` are `match_tiles`' (``nodata_b``, ``mask_b`` and ``rule_b``
    also decide the validity of the resampled pixels).  One host synchronisation per pass."""
    defaults = {k: v.default for k, v in inspect.signature(match_tiles).parameters.items() if k not in ("a", "b")}
    for k in match_args:
        if k not in defaults:
            raise RuntimeError(f"coregister: unknown argument {k!r}")
    margs = dict(defaults, **match_args)
    p = _host_args(match=dict(a=a, b=b, **margs),
                   fit=dict(model=model, trim=trim, max_rounds=max_rounds, min_points=min_points, passes=passes),
                   resample=dict(scene=b, matrix=None, out_shape=tuple(a.shape[1:]) if isinstance(a, torch.Tensor) else None,
                                 method=method, nodata=margs["nodata_b"], mask=margs["mask_b"], rule=margs["rule_b"], fill=fill))
    reg = None
    for i in range(p.fit["passes"]):
        if i:
            p = p._replace(match=_host_args(match=dict(a=a, b=b, **dict(margs, initial=reg))).match)
        reg = _fit(_match(p.match), p.fit)
    b_on_a, valid = _resample(p.resample, reg.matrix)
    return b_on_a, valid, reg
