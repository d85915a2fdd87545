"""Exact references for the 3x3 stride-2 conv / transposed-conv / weight-gradient kernels, and operands for which they are exact
(no torch, no GPU).

The references are fp64 loops over the nine taps on rectangular maps, with the index formulas of oracle/ae_numpy.py's docstrings.
The builders draw every stored tensor and coefficient from a coarse dyadic grid: the load transform of a source, every product and
every partial sum -- in ANY order -- is then exactly representable in fp32, so neither the accumulation order, nor the split into
tiles, slices and waves, nor fma contraction can change a bit of the kernels' accumulators.  A conv output must equal
bf16_round(exact sum + bias) and a weight gradient the exact sum, bit for bit.

Budget (from the formats, not from the code under test): conv products are multiples of 2^-7 (operand: multiples of 1/8, weight:
multiples of 1/16), weight-gradient products multiples of 2^-6 (1/8 x 1/8).  With S = sum |a||w| of one output, every partial sum
is a multiple of 2^-q of magnitude <= S, exact in fp32 as long as S * 2^q < 2^24.
"""
import itertools
import os

import numpy as np

Q_CONV, Q_WGRAD = 7, 6          # products are multiples of 2^-Q

# largest |operand value| a source mode can produce (builders below): stored k/4 with |k| <= 4; mode 1: 2*1 + 0.5; mode 2: 2*1 + 1*1 + 0.5
VMAX = {0: 1.0, 1: 2.5, 2: 3.5, 4: 1.0}
WMAX, BIASMAX = 1.0, 2.0


# ---------------------------------------------------------------------------------------------------------------
# fp64 references.  The "absolute" twins return S = the same sum over |a||w|.
# ---------------------------------------------------------------------------------------------------------------
def _pad1(x):
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + 2, w + 2), np.float64)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    return xp


def conv_s2(x, w):
    """y[n,co,oy,ox] = sum_{ci,ky,kx} x[n,ci,2oy-1+ky,2ox-1+kx] * w[co,ci,ky,kx];  x [N,Ci,H,W], w [Co,Ci,3,3] -> [N,Co,H/2,W/2]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, ci, h, wd = x.shape
    ho, wo = h // 2, wd // 2
    xp = _pad1(x)
    y = np.zeros((n, w.shape[0], ho, wo), np.float64)
    for ky in range(3):
        for kx in range(3):
            y += np.einsum("nchw,oc->nohw", xp[:, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2], w[:, :, ky, kx], optimize=True)
    return y


def deconv_s2(x, w):
    """y[n,co,oy,ox] = sum_{ci,ky,kx : oy = 2iy-1+ky, ox = 2ix-1+kx} x[n,ci,iy,ix] * w[ci,co,ky,kx];  x [N,Ci,H,W], w [Ci,Co,3,3]
    -> [N,Co,2H,2W]"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, ci, h, wd = x.shape
    yp = np.zeros((n, w.shape[1], 2 * h + 2, 2 * wd + 2), np.float64)          # index = oy + 1
    for ky in range(3):
        for kx in range(3):
            yp[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += np.einsum("nchw,co->nohw", x, w[:, :, ky, kx], optimize=True)
    return yp[:, :, 1:2 * h + 1, 1:2 * wd + 1].copy()


def wgrad_s2(small, big):
    """dw[cs,cb,ky,kx] = sum_{n,oy,ox} small[n,cs,oy,ox] * big[n,cb,2oy-1+ky,2ox-1+kx];  small [N,Cs,H,W], big [N,Cb,2H,2W]
    -> [Cs,Cb,3,3] (the weight gradient of a conv big -> small, and of a transposed conv small -> big)"""
    small, big = np.asarray(small, np.float64), np.asarray(big, np.float64)
    n, cs, h, wd = small.shape
    bp = _pad1(big)
    dw = np.zeros((cs, big.shape[1], 3, 3), np.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = np.einsum("nohw,nchw->oc", small, bp[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2], optimize=True)
    return dw


def conv_s2_abs(x, w):
    return conv_s2(np.abs(x), np.abs(w))


def deconv_s2_abs(x, w):
    return deconv_s2(np.abs(x), np.abs(w))


def wgrad_s2_abs(small, big):
    return wgrad_s2(np.abs(small), np.abs(big))


def assert_budget(S, q):
    """Every partial sum of terms that are multiples of 2^-q with sum of magnitudes <= S is exact in fp32."""
    smax = float(np.max(S))
    assert smax * 2.0 ** q < 2.0 ** 24, (smax, q)


def bf16_round(a):
    """fp32 -> bf16, round to nearest even, returned as fp32"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32).reshape(a.shape)


def exact_f32(a):
    """fp64 -> fp32, asserting that nothing is lost (what the budget promises)"""
    f = a.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), a)
    return f


# ---------------------------------------------------------------------------------------------------------------
# dyadic operands
# ---------------------------------------------------------------------------------------------------------------
def _quarters(rng, shape, kmax):
    return (rng.integers(-kmax, kmax + 1, shape) / 4.0).astype(np.float32)


def _pick(rng, values, n):
    return np.asarray(values, np.float32)[rng.integers(0, len(values), n)]


class DyadicSrc:
    """A source operand as a kernel materialises it on load.  `tensors`: the stored NCHW tensors (p0, p1 of eae_src), `coef`: the
    coefficient table ([rows][C] fp32) or None, `value`: the exact operand (fp64)."""

    def __init__(self, mode, shape, rng):
        c = shape[1]
        bc = lambda v: v[None, :, None, None].astype(np.float64)
        self.mode, self.coef = mode, None
        if mode in (0, 4):                                   # as stored
            y = _quarters(rng, shape, 4)
            self.tensors, self.value = [y], y.astype(np.float64)
        elif mode == 1:                                      # max(0, s*y + t)
            y = _quarters(rng, shape, 4)
            s, t = _pick(rng, (0.5, 1.0, 2.0), c), _quarters(rng, c, 2)
            self.tensors = [y]
            self.coef = np.stack([s, t, np.zeros(c, np.float32), np.ones(c, np.float32)])
            self.value = np.maximum(y * bc(s) + bc(t), 0.0)
        elif mode == 2:                                      # A*g + (B*y + C)
            g, y = _quarters(rng, shape, 4), _quarters(rng, shape, 4)
            a_, b_, c_ = _pick(rng, (0.5, 1.0, 2.0), c), _pick(rng, (-1.0, -0.5, 0.5, 1.0), c), _quarters(rng, c, 2)
            self.tensors = [g, y]
            self.coef = np.stack([a_, b_, c_])
            self.value = g * bc(a_) + (y * bc(b_) + bc(c_))
        else:
            raise ValueError(mode)
        assert np.abs(self.value).max() <= VMAX[mode] and np.array_equal(self.value * 8, np.round(self.value * 8))


def dyadic_weights(shape, rng):
    return (np.clip(np.round(0.3 * rng.standard_normal(shape) * 16), -16, 16) / 16).astype(np.float32)


def dyadic_bias(c, rng):
    return (rng.integers(-256, 257, c) / 128.0).astype(np.float32)


class DyadicPrev:
    """The mask epilogue's inputs: the previous layer's stored tensor and its coefficient rows (ps, pt, pm, pi).  `mask`: the exact
    decision yprev*ps + pt > 0 (it lands on 0 often: a zero gives 0, as torch's ReLU backward), `xhat` = yprev*pi - pm*pi, exact."""

    def __init__(self, shape, rng):
        c = shape[1]
        bc = lambda v: v[None, :, None, None].astype(np.float64)
        self.yprev = _quarters(rng, shape, 4)
        ps, pi = _pick(rng, (0.5, 1.0, 2.0), c), _pick(rng, (0.5, 1.0, 2.0), c)
        pt, pm = _quarters(rng, c, 4), _quarters(rng, c, 4)
        self.coef = np.stack([ps, pt, pm, pi])
        act = self.yprev * bc(ps) + bc(pt)
        self.mask = act > 0
        self.zeros = int((act == 0).sum())
        self.xhat = self.yprev * bc(pi) - bc(pm) * bc(pi)


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
# (kind, cin, cout, source mode, epilogue): the 14 instantiations eae_launch_conv_s2 / eae_launch_deconv_s2 list
IGEMM_INSTANCES = [
    (0, 32, 64, 1, 0), (0, 64, 128, 1, 0), (0, 128, 256, 1, 0),          # enc.conv2/3/4 forward
    (0, 32, 64, 2, 1), (0, 64, 128, 2, 1), (0, 128, 256, 2, 2),          # backward-data of dec.deconv3/2/1
    (0, 32, 64, 0, 0),                                                   # plain conv
    (1, 256, 128, 0, 0), (1, 128, 64, 1, 0), (1, 64, 32, 1, 0),          # dec.deconv1/2/3 forward
    (1, 256, 128, 2, 1), (1, 128, 64, 2, 1), (1, 64, 32, 2, 1),          # backward-data of enc.conv4/3/2
    (1, 64, 32, 0, 0),                                                   # plain transposed conv
]
# position grids (rows, columns, batch); conv kind: the output map, transposed kind: the input map
GRIDS = [
    (4, 4, 9),        # a last tile with one valid image, at 8 and at 4 images per tile
    (8, 8, 3),        # a last tile with one valid image at 2 images per tile
    (8, 16, 2),       # one 16x8 tile per image
    (16, 32, 1),      # 2x2 tiles: real halos in both directions
    (8, 32, 2),       # two tiles across only
    (24, 16, 1),      # three tiles down only
]
IGEMM_EXACT_CASES = [inst + grid for inst, grid in itertools.product(IGEMM_INSTANCES, GRIDS)]

# (cs, cb, small mode, big mode): the 13 instantiations of eae_launch_wgrad_s2
WGRAD_INSTANCES = [
    (64, 32, 2, 1), (128, 64, 2, 1), (256, 128, 2, 1),
    (64, 32, 1, 2), (128, 64, 1, 2), (256, 128, 0, 2),
    (64, 32, 0, 0),
    (64, 32, 4, 1), (128, 64, 4, 1), (256, 128, 4, 1),
    (64, 32, 1, 4), (128, 64, 1, 4), (256, 128, 0, 4),
]
# the small map's grids (rows, columns, batch)
WGRAD_GRIDS = [(4, 4, 9), (8, 8, 3), (8, 16, 1), (16, 32, 1), (8, 32, 2), (24, 16, 1)]
WGRAD_EXACT_CASES = [inst + grid for inst, grid in itertools.product(WGRAD_INSTANCES, WGRAD_GRIDS)] + [
    (256, 128, 2, 1, 4, 4, 70),       # 4x4x8 tiles: 9 tiles on 4 slices, 3 tiles per workgroup, then the slice reduction
    (64, 32, 1, 2, 16, 32, 3),        # 12 tiles of 16x8 on 12 slices (one tile per workgroup: 64 x 32 has 64 slices to give)
    (256, 128, 2, 1, 16, 32, 3),      # 16x8x1 tiles: 12 tiles on 4 slices, 3 per workgroup
    (128, 64, 1, 2, 16, 32, 5),       # 16x8x1 tiles: 20 tiles on 10 slices, 2 per workgroup
    (256, 128, 4, 1, 8, 8, 18),       # 8x8x2 tiles: 9 tiles on 3 slices, 3 per workgroup
]
# rows whose workgroups loop over several tiles (the double-buffered pipeline, the accumulator carried from tile to tile), per
# geometry: (case, tiles, slices, tiles per workgroup) under the launcher's default of 64 workgroups
WGRAD_MULTI_TILE = {
    (4, 4, 8): ((256, 128, 2, 1, 4, 4, 70), 9, 3, 3),
    (16, 8, 1): ((256, 128, 2, 1, 16, 32, 3), 12, 4, 3),
    (8, 8, 2): ((256, 128, 4, 1, 8, 8, 18), 9, 3, 3),
}


def igemm_budget_bound(kind, cin, cout, smode, epi, hp, wp, B):
    """S of any output by construction: 9 taps x cin channels (the transposed kind reaches at most 4 taps per output), plus the bias"""
    return 9 * cin * VMAX[smode] * WMAX + (BIASMAX if epi == 0 else 0.0)


def wgrad_budget_bound(cs, cb, smode, bmode, hs, ws, B):
    return B * hs * ws * VMAX[smode] * VMAX[bmode]


# ---------------------------------------------------------------------------------------------------------------
# the tile geometry a case is meant to hit: csrc/eae_conv_plan.h and the launcher of csrc/eae_wgrad_launch.hip as literal tables
# (the only copy in the tests: test_conv_plan.py compares the library's plan with this one)
# ---------------------------------------------------------------------------------------------------------------
WIDE = (16, 8, 1)                                                 # position grids that are multiples of 8 rows x 16 columns
NARROW = {(0, 8): ((8, 8, 2), (8, 8, 1)), (0, 4): ((4, 4, 8), (4, 4, 4)),      # (kind, side): (large tiles, small tiles)
          (1, 8): ((8, 8, 1), (8, 8, 1)), (1, 4): ((4, 4, 4), (4, 4, 4))}     # (transposed kind: small = narrower channel blocks)


def _cdiv(a, b):
    return -(-a // b)


def _tiles(geo, B, hp, wp):
    tw, th, ni = geo
    return _cdiv(B, ni) * (hp // th) * (wp // tw)


def ig_small_setting():
    """EAE_IG_SMALL as the library reads it (once per process): the mask, or None when unset"""
    v = os.environ.get("EAE_IG_SMALL")
    return None if v is None or int(v) < 0 else int(v)


def expected_geo(kind, cin, cout, hp, wp, B, ig_small=None):
    """(TW, TH, NI) of a (kind, cin, cout) layer on B position grids of hp x wp, None when the grid has no geometry.  ig_small: the
    EAE_IG_SMALL mask (bit 0: conv kind), None when unset: the small tiles while the large-tile grid has fewer than 256 workgroups."""
    if hp % 8 == 0 and wp % 16 == 0:                               # wide maps may be rectangular
        return WIDE
    if hp != wp or (kind, hp) not in NARROW:
        return None
    large, small = NARROW[kind, hp]
    takes_small = kind == 1 or cin >= 64                           # the conv kind has small tiles from 64 input channels on
    if ig_small is None:
        is_small = _tiles(large, B, hp, wp) * (cout // 64) < 256   # the large-tile grid leaves CUs empty
    else:
        is_small = (ig_small & (1 if kind == 0 else 2)) != 0
    return small if takes_small and is_small else large


def expected_ntiles(kind, cin, cout, hp, wp, B, ig_small=None):
    geo = expected_geo(kind, cin, cout, hp, wp, B, ig_small)
    return -1 if geo is None else _tiles(geo, B, hp, wp)


def wgrad_workgroups_setting(cs, smode):
    """the launcher's workgroup budget for a (cs, small mode) layer: 64, or what EAE_WGRAD_WGS=<one-block>[,<wide>[,<last>]] says"""
    one = wide = last = 64
    v = [int(t) for t in os.environ.get("EAE_WGRAD_WGS", "").split(",") if t.strip().lstrip("-").isdigit()]
    if v and v[0] > 0:
        one = v[0]
        wide = v[1] if len(v) >= 2 and v[1] > 0 else one
        last = v[2] if len(v) >= 3 and v[2] > 0 else one
    if cs == 64 and smode in (2, 4):                               # enc.conv2's weight gradient, the last one of the step
        return last
    return one if cs == 64 else wide                               # 64 x 32 is one 64 x 32 block


def expected_wgrad_launch(cs, cb, smode, hs, ws, B, scratch_floats):
    """((TW, TH, NI), tiles, slices, tiles per workgroup) of a weight-gradient launch: 16x8x1 tiles on wide small maps, 8x8x2 and
    4x4x8 on the narrow ones; the workgroup budget divided by the (cs/64)(cb/32) blocks gives the position slices, at most one per
    tile and no more than the scratch holds; a workgroup takes ceil(tiles / slices) consecutive tiles."""
    geo = WIDE if hs % 8 == 0 and ws % 16 == 0 else {8: (8, 8, 2), 4: (4, 4, 8)}[hs]
    assert geo == WIDE or hs == ws
    tiles = _tiles(geo, B, hs, ws)
    nblk, sz = (cs // 64) * (cb // 32), cs * cb * 9
    slices = min(max(wgrad_workgroups_setting(cs, smode) // nblk, 1), tiles)
    while slices * sz > scratch_floats and slices > 1:
        slices >>= 1
    per = _cdiv(tiles, slices)
    return geo, tiles, _cdiv(tiles, per), per
