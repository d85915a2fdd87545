"""NumPy definition of co-registration (eae_amd.register; include/eae.h, "co-registration"): the matching
feature and validity, the brute-force correlation sums of a grid of tiles, score / peak / parabola, the trimmed least-squares fit, the
resampling in float64 in the header's order of operations (plain * and +, which NumPy never fuses), and the planted scene pairs the
tests share.

Coordinates: pixel (y, x) has its centre at the point (x, y); a matrix M [2, 3] maps a point of the destination grid (scene A) to the
source (scene B): sx = (M00 x + M01 y) + M02, sy = (M10 x + M11 y) + M12."""
import math

import numpy as np

NEG = -np.inf
METHODS = {"nearest": 0, "bilinear": 1, "cubic": 2}
INT_MAX = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535}


# ---------------------------------------------------------------------------------------------------- feature and validity
def features(band, divisor):
    """int64 [H, W]: u = rint(65535 * min(max(v / d, 0), 1)) in double, half to even, NaN -> 0."""
    with np.errstate(all="ignore"):
        p = band.astype(np.float64) / np.float64(np.float32(divisor))
        c = np.where(p > 0.0, np.where(p < 1.0, p, 1.0), 0.0)
        return np.rint(c * 65535.0).astype(np.int64)


def validity(scene, nodata=None, rule="all", mask=None):
    """bool [H, W]: the valid pixels of a scene [C, H, W] (the rule of change_ref.valid_pixels, for one scene)."""
    ok = np.ones(scene.shape[1:], dtype=bool)
    if nodata is not None:
        m = np.isnan(scene) if isinstance(nodata, float) and math.isnan(nodata) else scene == nodata
        ok &= ~(m.all(0) if rule == "all" else m.any(0))
    if scene.dtype == np.float32:
        ok &= np.isfinite(scene).all(0)
    if mask is not None:
        ok &= np.asarray(mask) == 0
    return ok


def _window(u, v, y0, x0, n):
    """(u, v) of the n x n window whose top-left pixel is (y0, x0); everything outside the raster is invalid (u = 0)."""
    h, w = u.shape
    wu, wv = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=bool)
    ys, xs = np.arange(y0, y0 + n), np.arange(x0, x0 + n)
    iy, ix = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if iy.any() and ix.any():
        sub = np.ix_(ys[iy], xs[ix])
        wu[np.ix_(iy, ix)] = u[sub]
        wv[np.ix_(iy, ix)] = v[sub]
    return wu * wv, wv


def tile_sums(ua, va, ub, vb, tile, radius, origins_a, origins_b):
    """int64 [n, (2R + 1)^2, 6] = (n, sum a, sum b, sum a^2, sum b^2, sum a b) over the pairs whose two pixels are valid, by brute
    force: a loop over the tiles and the offsets."""
    nd = 2 * radius + 1
    out = np.zeros((len(origins_a), nd * nd, 6), dtype=np.int64)
    for t, ((ay, ax), (by, bx)) in enumerate(zip(np.asarray(origins_a).tolist(), np.asarray(origins_b).tolist())):
        a, av = _window(ua, va, ay, ax, tile)
        win, wv = _window(ub, vb, by - radius, bx - radius, tile + 2 * radius)
        for dy in range(nd):
            for dx in range(nd):
                b, bv = win[dy:dy + tile, dx:dx + tile], wv[dy:dy + tile, dx:dx + tile]
                both = av & bv
                am, bm = a * both, b * both
                out[t, dy * nd + dx] = (both.sum(), am.sum(), bm.sum(), (am * am).sum(), (bm * bm).sum(), (am * bm).sum())
    return out


# ---------------------------------------------------------------------------------------------------- score, peak, parabola
def scores(sums, min_pairs):
    """float64 [n, O]: num / sqrt(va vb) with num = n sum ab - sum a sum b and the variances n sum a^2 - (sum a)^2 in int64 (exact);
    -inf where n < min_pairs or a variance is 0."""
    s = np.asarray(sums, dtype=np.int64)
    n, sa, sb, saa, sbb, sab = (s[..., k] for k in range(6))
    num, va, vb = n * sab - sa * sb, n * saa - sa * sa, n * sbb - sb * sb
    bad = (n < min_pairs) | (va <= 0) | (vb <= 0)
    with np.errstate(all="ignore"):
        sc = num.astype(np.float64) / np.sqrt(va.astype(np.float64) * vb.astype(np.float64))
    return np.where(bad, NEG, sc)


def _parabola(lo, mid, hi):
    with np.errstate(all="ignore"):
        den = lo - 2.0 * mid + hi
        sub = 0.5 * (lo - hi) / den
    bad = ~np.isfinite(lo) | ~np.isfinite(hi) | ~np.isfinite(mid) | (den == 0.0) | ~np.isfinite(sub)
    return np.where(bad, 0.0, np.clip(sub, -0.5, 0.5))


def peaks(score, radius, min_score):
    """(offsets int64 [n, 2] = (dy, dx), sub float64 [n, 2], peak score float64 [n], ok bool [n]) of a score table [n, (2R + 1)^2]:
    the argmax (the lowest entry on a tie), a parabola through the peak and its two neighbours per axis clamped to +-0.5 (0 where a
    neighbour is missing or -inf or the denominator is 0); ok: the score is finite and >= min_score and, for R > 0, the peak is not
    on the border of the search window."""
    nd = 2 * radius + 1
    sc = np.asarray(score, dtype=np.float64).reshape(-1, nd, nd)
    n = sc.shape[0]
    flat = sc.reshape(n, -1).argmax(1)
    py, px = flat // nd, flat % nd
    pad = np.full((n, nd + 2, nd + 2), NEG)
    pad[:, 1:-1, 1:-1] = sc
    t = np.arange(n)
    s0 = pad[t, py + 1, px + 1]
    sub = np.stack([_parabola(pad[t, py, px + 1], s0, pad[t, py + 2, px + 1]), _parabola(pad[t, py + 1, px], s0, pad[t, py + 1, px + 2])], 1)
    border = (py == 0) | (py == nd - 1) | (px == 0) | (px == nd - 1)
    ok = np.isfinite(s0) & (s0 >= min_score) & ~(border & (radius > 0))
    return np.stack([py - radius, px - radius], 1), sub, s0, ok


# ---------------------------------------------------------------------------------------------------- geometry and the fit
def tile_grid(h, w, tile, stride):
    """int64 [n, 2] = (y, x): the origins of the regular grid of tiles that lie wholly inside an H x W raster."""
    ys, xs = np.arange(0, h - tile + 1, stride), np.arange(0, w - tile + 1, stride)
    return np.stack(np.meshgrid(ys, xs, indexing="ij"), -1).reshape(-1, 2).astype(np.int64)


def apply(matrix, x, y):
    m = np.asarray(matrix, dtype=np.float64)
    return (m[0, 0] * x + m[0, 1] * y) + m[0, 2], (m[1, 0] * x + m[1, 1] * y) + m[1, 2]


def invert(matrix):
    """The inverse of an affine map [2, 3]."""
    m = np.asarray(matrix, dtype=np.float64)
    lin = np.linalg.inv(m[:, :2])
    return np.concatenate([lin, -(lin @ m[:, 2:])], 1)


def window_origins(origins_a, tile, matrix):
    """int64 [n, 2]: the zero-offset window of every tile, at the rounded image of the tile's centre."""
    half = (tile - 1) / 2.0
    mx, my = apply(matrix, origins_a[:, 1] + half, origins_a[:, 0] + half)
    return np.stack([np.rint(my - half), np.rint(mx - half)], 1).astype(np.int64)


def fit_transform_ref(pa, pb, model="affine", trim=3.0, max_rounds=10):
    """(matrix [2, 3], inliers bool [n], residuals [n], rmse): least squares pb = M pa over points [n, 2] = (x, y), then repeatedly
    drop the inliers whose residual exceeds max(trim * 1.4826 * median residual, 0.05) and refit until nothing is dropped."""
    pa, pb = np.asarray(pa, dtype=np.float64), np.asarray(pb, dtype=np.float64)
    inl = np.ones(len(pa), dtype=bool)
    rounds = 0
    while True:
        if model == "affine":
            design = np.concatenate([pa[inl], np.ones((int(inl.sum()), 1))], 1)
            m = np.linalg.lstsq(design, pb[inl], rcond=None)[0].T.copy()
        else:
            d = (pb[inl] - pa[inl]).mean(0)
            m = np.array([[1.0, 0.0, d[0]], [0.0, 1.0, d[1]]])
        fx, fy = apply(m, pa[:, 0], pa[:, 1])
        res = np.hypot(fx - pb[:, 0], fy - pb[:, 1])
        keep = inl & (res <= max(trim * 1.4826 * float(np.median(res[inl])), 0.05))
        if rounds == max_rounds or keep.sum() == inl.sum():
            break
        inl, rounds = keep, rounds + 1
    return m, inl, res, float(np.sqrt((res[inl] ** 2).mean()))


def match_ref(a, b, tile, stride, radius, band=0, divisor_a=1.0, divisor_b=1.0, nodata_a=None, nodata_b=None, mask_a=None, mask_b=None,
              rule_a="all", rule_b="all", initial=None, min_pairs=None, min_score=0.7):
    """(centres in A [n, 2] = (x, y), matched points in B [n, 2], offsets, sub, score, ok, sums): one matching pass."""
    da = np.broadcast_to(np.asarray(divisor_a, dtype=np.float32).reshape(-1), (a.shape[0],))
    db = np.broadcast_to(np.asarray(divisor_b, dtype=np.float32).reshape(-1), (b.shape[0],))
    ua, ub = features(a[band], da[band]), features(b[band], db[band])
    va, vb = validity(a, nodata_a, rule_a, mask_a), validity(b, nodata_b, rule_b, mask_b)
    oa = tile_grid(a.shape[1], a.shape[2], tile, stride)
    ob = window_origins(oa, tile, np.array([[1.0, 0, 0], [0, 1.0, 0]]) if initial is None else initial)
    sums = tile_sums(ua, va, ub, vb, tile, radius, oa, ob)
    off, sub, sc, ok = peaks(scores(sums, tile * tile // 2 if min_pairs is None else min_pairs), radius, min_score)
    half = (tile - 1) / 2.0
    ca = np.stack([oa[:, 1] + half, oa[:, 0] + half], 1)
    pb = np.stack([ob[:, 1] + half + off[:, 1] + sub[:, 1], ob[:, 0] + half + off[:, 0] + sub[:, 0]], 1)
    return ca, pb, off, sub, sc, ok, sums


def coregister_ref(a, b, passes=2, model="affine", **kw):
    """(matrix, ok of the last pass, inliers among the ok tiles): match, fit, and match again from the fit."""
    m = None
    for _ in range(passes):
        ca, pb, _, _, _, ok, _ = match_ref(a, b, initial=m, **kw)
        m, inl, _, _ = fit_transform_ref(ca[ok], pb[ok], model)
    return m, ok, inl


def corner_error(matrix, truth, h, w):
    """The largest distance over the four corners of an H x W grid between the two matrices' images of the corner."""
    x, y = np.array([0.0, w - 1.0, 0.0, w - 1.0]), np.array([0.0, 0.0, h - 1.0, h - 1.0])
    fx, fy = apply(matrix, x, y)
    tx, ty = apply(truth, x, y)
    return float(np.hypot(fx - tx, fy - ty).max())


# ---------------------------------------------------------------------------------------------------- resampling
def _axis(s, method):
    """(first tap's coordinate, weights): the header's expressions, one rounding per operation."""
    if method == "nearest":
        return np.floor(s + 0.5), [np.ones_like(s)]
    f = np.floor(s)
    t = s - f
    if method == "bilinear":
        return f, [1.0 - t, t]
    return f - 1.0, [((-0.5 * t + 1.0) * t - 0.5) * t, ((1.5 * t - 2.5) * t) * t + 1.0, ((-1.5 * t + 2.0) * t + 0.5) * t,
                     ((0.5 * t - 0.5) * t) * t]


def resample_ref(src, matrix, out_shape=None, method="bilinear", nodata=None, rule="all", mask=None, fill=0.0):
    """(dst [C, Hd, Wd] of src's dtype, valid uint8 [Hd, Wd]) of eae_scene_resample, bit for bit."""
    c, hs, ws = src.shape
    hd, wd = src.shape[1:] if out_shape is None else out_shape
    m = np.asarray(matrix, dtype=np.float64).reshape(2, 3)
    x, y = np.arange(wd, dtype=np.float64)[None, :], np.arange(hd, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        sx = (m[0, 0] * x + m[0, 1] * y) + m[0, 2]
        sy = (m[1, 0] * x + m[1, 1] * y) + m[1, 2]
        ok = np.isfinite(sx) & np.isfinite(sy)
        sx, sy = np.where(ok, sx, 0.0), np.where(ok, sy, 0.0)
        bx, wx = _axis(sx, method)
        by, wy = _axis(sy, method)
    srcv = validity(src, nodata, rule, mask)
    acc = np.zeros((c, hd, wd))
    started = np.zeros((hd, wd), dtype=bool)
    for r in range(len(wy)):
        for q in range(len(wx)):
            part = ok & (wy[r] != 0.0) & (wx[q] != 0.0)
            cy, cx = by + r, bx + q
            inside = (cy >= 0) & (cy <= hs - 1) & (cx >= 0) & (cx <= ws - 1)
            iy, ix = np.where(inside, cy, 0).astype(np.int64), np.where(inside, cx, 0).astype(np.int64)
            ok &= ~part | (inside & srcv[iy, ix])
            with np.errstate(all="ignore"):
                term = (wy[r] * wx[q]) * src[:, iy, ix].astype(np.float64)
                acc = np.where(part & ~started, term, np.where(part, acc + term, acc))
            started |= part
    if src.dtype == np.float32:
        with np.errstate(all="ignore"):
            out = acc.astype(np.float32)
        f = np.float32(fill)
    else:
        hi = INT_MAX[src.dtype]
        out = np.clip(np.rint(np.where(ok, acc, 0.0)), 0, hi).astype(src.dtype)
        f = src.dtype.type(np.rint(fill))
    return np.where(ok, out, f).astype(src.dtype), ok.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- planted pairs
SCALE = {np.dtype(np.uint8): (128.0, 100.0, 255.0), np.dtype(np.uint16): (2000.0, 1500.0, 4095.0),
         np.dtype(np.float32): (0.5, 0.4, 1.0)}          # (mean, amplitude, divisor)
WAVES = 40


def rigid(angle_deg, scale, shift, h, w):
    """The matrix of a rotation by angle_deg and a scale about the centre of an H x W grid, followed by a shift (x, y)."""
    t = math.radians(angle_deg)
    c, s = scale * math.cos(t), scale * math.sin(t)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    return np.array([[c, -s, cx - c * cx + s * cy + shift[0]], [s, c, cy - s * cx - c * cy + shift[1]]])


def _field(rng, c):
    """The closed form of a band-limited random field: per band WAVES sinusoids with wavelengths of 5 to 40 pixels."""
    wl = np.exp(rng.uniform(math.log(5.0), math.log(40.0), (c, WAVES)))
    ang = rng.uniform(0.0, 2.0 * math.pi, (c, WAVES))
    kx, ky = 2.0 * math.pi * np.cos(ang) / wl, 2.0 * math.pi * np.sin(ang) / wl
    ph = rng.uniform(0.0, 2.0 * math.pi, (c, WAVES))
    amp = rng.uniform(0.5, 1.0, (c, WAVES))
    amp /= np.sqrt((amp ** 2).sum(1, keepdims=True) / 2.0)           # unit variance of the sum; `planted` maps 3 sigma to the amplitude

    def f(x, y):
        return (amp[:, :, None, None] * np.sin(kx[:, :, None, None] * x + ky[:, :, None, None] * y + ph[:, :, None, None])).sum(1)
    return f


def planted(seed, dtype, shape, matrix):
    """(a, b, divisor): scene A is the closed form at the pixel centres scaled into the dtype; scene B is THE SAME CLOSED FORM at the
    coordinates mapped back through `matrix` (B at M p shows what A shows at p) (clipped at 3 sigma like A) with a per-band gain and offset and a little noise, so `matrix` is exact and no
    resampling enters."""
    dtype = np.dtype(dtype)
    c, h, w = shape
    rng = np.random.default_rng(seed)
    f = _field(rng, c)
    mean, amp, div = SCALE[dtype]
    y, x = np.mgrid[:h, :w].astype(np.float64)
    fa = np.clip(f(x, y) / 3.0, -1.0, 1.0)
    mx, my = apply(invert(matrix), x, y)                             # B(M p) = A(p): pixel q of B shows the field at M^-1 q
    fb = np.clip(f(mx, my) / 3.0, -1.0, 1.0)
    gain = (0.9 + 0.05 * np.arange(c))[:, None, None]
    a = mean + amp * fa
    b = mean + 0.05 * amp + gain * amp * fb + 0.01 * amp * rng.standard_normal((c, h, w))
    if dtype == np.float32:
        return a.astype(np.float32), b.astype(np.float32), div
    hi = INT_MAX[dtype]
    return np.clip(np.rint(a), 0, hi).astype(dtype), np.clip(np.rint(b), 0, hi).astype(dtype), div


# ---------------------------------------------------------------------------------------------------- the cases the tests share
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
H, W = 192, 256
BOUND = 0.25                   # pixels; measured with this file's pipeline on the CPU: tests/test_register_reference.py
#        seed, dtype, degrees, scale, shift (x, y)
CASES = [(0, "u8", 0.5, 1.005, (3.4, -2.7)), (1, "u16", -0.5, 0.995, (-3.4, 2.7)), (2, "f32", 0.3, 1.005, (3.4, 2.7)),
         (3, "u16", 0.5, 1.0, (0.0, 0.0)), (4, "u8", -0.25, 1.002, (-1.3, -2.7)), (5, "f32", 0.0, 1.0, (3.4, -2.7)),
         (6, "u16", 0.5, 1.005, (3.4, -2.7))]
MATCH = dict(tile=32, stride=32, radius=6)


def planted_case(case):
    seed, kind, angle, scale, shift = case
    truth = rigid(angle, scale, shift, H, W)
    a, b, div = planted(seed, NP[kind], (2, H, W), truth)
    return a, b, div, truth


def masked_case():
    """Case 6 with a nodata strip along A's left edge (both bands 0) and a masked block of B: (a, b, div, truth, mask_b)."""
    a, b, div, truth = planted_case(CASES[6])
    a = a.copy()
    a[:, :, :40] = 0
    mask_b = np.zeros((H, W), dtype=bool)
    mask_b[120:, 150:] = True
    return a, b, div, truth, mask_b
