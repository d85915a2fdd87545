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

The fp8 twins of the kernels (second half of this file) multiply QUANTISED operands: the same references, grids and budget, with S
taken from the quantised operands.  Measured on an MI355X (tests/test_gpu_fp8_exact.py): within this budget the four fp8 MFMA forms
(v_mfma_f32_16x16x32_{fp8,bf8}_{fp8,bf8}) accumulate exactly, as the bf16 form does -- eighths with up to 5 significant bits needed
no coarsening.
"""
import itertools
import os

import numpy as np

from oracle import ae_numpy as _O          # NumPy only: the fp8 conversion (fp8_round, _q8, fp8_bytes_e4m3)

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
# the tile geometry a case is meant to hit: csrc/eae_conv_plan.h and csrc/eae_wgrad_plan.h as literal tables
# (the only copy in the tests: test_conv_plan.py and test_wgrad_plan.py compare the C plans with this one)
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


def wgrad_workgroups_setting(cs, smode, wgs=None):
    """the launcher's workgroup budget for a (cs, small mode) layer: 64, or what EAE_WGRAD_WGS=<one-block>[,<wide>[,<last>]] says;
    wgs: the three budgets (one-block, wide, last) given outright instead of read from the environment"""
    one = wide = last = 64
    if wgs is not None:
        one, wide, last = wgs
    else:
        v = [int(t) for t in os.environ.get("EAE_WGRAD_WGS", "").split(",") if t.strip().lstrip("-").isdigit()]
        if v and v[0] > 0:
            one = v[0]
            wide = v[1] if len(v) >= 2 and v[1] > 0 else one
            last = v[2] if len(v) >= 3 and v[2] > 0 else one
    if cs == 64 and smode in (2, 4):                               # enc.conv2's weight gradient, the last one of the step
        return last
    return one if cs == 64 else wide                               # 64 x 32 is one 64 x 32 block


# what a weight-gradient launch is refused for (the launcher's three error texts), in the order the launcher checks
WGRAD_NO_GEOMETRY, WGRAD_SCRATCH, WGRAD_FP8_NARROW = "unsupported spatial size", "scratch too small", "fp8 needs 16-wide tiles"


def expected_wgrad_launch(cs, cb, smode, hs, ws, B, scratch_floats, mult=1, wgs=None, fp8=False):
    """((TW, TH, NI), tiles, slices, tiles per workgroup) of a weight-gradient launch: 16x8x1 tiles on wide small maps, 8x8x2 and
    4x4x8 on the narrow ones; the workgroup budget divided by the (cs/64)(cb/32) blocks gives the position slices, at most one per
    tile and no more than the scratch holds; a workgroup takes ceil(tiles / slices) consecutive tiles.  mult: the members of a
    grouped step (eae_set_geometry_mult) share the budget, down to 8 workgroups each; wgs: see wgrad_workgroups_setting.  One of the
    WGRAD_* strings instead when the launcher refuses: a map without geometry, a scratch below one partial, the fp8 variant on
    narrow tiles.  This is csrc/eae_wgrad_plan.h restated; test_wgrad_plan.py holds the two together without a GPU."""
    if hs % 8 == 0 and ws % 16 == 0:
        geo = WIDE
    elif hs == ws and hs in (8, 4):
        geo = {8: (8, 8, 2), 4: (4, 4, 8)}[hs]
    else:
        return WGRAD_NO_GEOMETRY
    tiles = _tiles(geo, B, hs, ws)
    nblk, sz = (cs // 64) * (cb // 32), cs * cb * 9
    budget = wgrad_workgroups_setting(cs, smode, wgs)
    if mult > 1:
        budget = max(budget // mult, 8)
    slices = min(max(budget // nblk, 1), tiles)
    while slices * sz > scratch_floats and slices > 1:
        slices >>= 1
    if slices * sz > scratch_floats:
        return WGRAD_SCRATCH
    if fp8 and geo != WIDE:
        return WGRAD_FP8_NARROW
    per = _cdiv(tiles, slices)
    return geo, tiles, _cdiv(tiles, per), per


# ---------------------------------------------------------------------------------------------------------------
# fp8 twins (igemm8_s2_kernel, wgrad8_s2_kernel): the same references on QUANTISED operands
#
# Every scale is a power of two, so scaling and unscaling move no bit: only the fp8 rounding of an operand changes a value, and
# oracle.ae_numpy.fp8_round / _q8 restate it.  Rounding only coarsens: a multiple of 1/8 with |v| <= 3.5 stays a multiple of 1/8
# (e4m3 at scales 2^-8 .. 2^8, e5m2 at 2^-16 .. 2^15; `quantised` asserts it for what it returns), the weights k/16 are e4m3 values at
# s_w = 2^-3 .. 2^8, and the budget above carries over with S taken from the quantised operands (the *_abs twins).
#
# The coarse DyadicSrc operands are fp8 values already at scale 1 in modes 0, 1 and 4 (nothing would be rounded): FineSrc stores
# eighths, so that a share of every operand is changed by the conversion, exact ties among them.
# ---------------------------------------------------------------------------------------------------------------
FP8_MAX = {"e4m3": 448.0, "e5m2": 57344.0}
FINE_VMAX = 3.5


def fp8_fmt(mode):
    """the format a source mode is converted to: the gradient operands (modes 2 and 4: QG / SG / BG of the kernels) go to e5m2"""
    return "e5m2" if mode in (2, 4) else "e4m3"


def _eighths(rng, shape, kmax):
    return (rng.integers(-kmax, kmax + 1, shape) / 8.0).astype(np.float32)


class FineSrc(DyadicSrc):
    """DyadicSrc on the 1/8 grid: stored tensors and coefficients are bf16- and fp32-exact, the materialised operand is a multiple
    of 1/8 with |v| <= 3.5 -- and, unlike DyadicSrc's, not an fp8 value throughout."""

    def __init__(self, mode, shape, rng):
        c = shape[1]
        bc = lambda v: v[None, :, None, None].astype(np.float64)
        self.mode, self.coef = mode, None
        if mode in (0, 4):                                   # as stored: k/8, |k| <= 28
            y = _eighths(rng, shape, 28)
            self.tensors, self.value = [y], y.astype(np.float64)
        elif mode == 1:                                      # max(0, s*y + t): |y| <= 3, s = +-1, |t| <= 1/2
            y = _eighths(rng, shape, 24)
            s, t = _pick(rng, (-1.0, 1.0), c), _eighths(rng, c, 4)
            self.tensors = [y]
            self.coef = np.stack([s, t, np.zeros(c, np.float32), np.ones(c, np.float32)])
            self.value = np.maximum(y * bc(s) + bc(t), 0.0)
        elif mode == 2:                                      # A*g + (B*y + C): |A g| <= 2, |B y| <= 1, |C| <= 1/2
            g, y = _quarters(rng, shape, 4), _eighths(rng, shape, 8)
            a_, b_, c_ = _pick(rng, (0.5, 1.0, 2.0), c), _pick(rng, (-1.0, 1.0), c), _quarters(rng, c, 2)
            self.tensors = [g, y]
            self.coef = np.stack([a_, b_, c_])
            self.value = g * bc(a_) + (y * bc(b_) + bc(c_))
        else:
            raise ValueError(mode)
        assert np.abs(self.value).max() <= FINE_VMAX and np.array_equal(self.value * 8, np.round(self.value * 8))


def quantised(src, scale, fmt):
    """_q8 of the bf16 operand (fp64): what the kernel multiplies.  Still on the 1/8 grid."""
    v32 = src.value.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), src.value) and np.array_equal(bf16_round(v32), v32)
    q = _O._q8(v32, scale, fmt).astype(np.float64)
    assert np.array_equal(q * 8, np.round(q * 8)) and np.abs(q).max() <= 4.0
    return q


def rounding_shares(value, scale, fmt):
    """What the conversion at `scale` does to an operand, from the oracle alone: shares of elements it changes, of exact ties (the
    two fp32 neighbours of the scaled value round to different fp8 values), of saturated and of flushed-to-zero elements."""
    x = (value * scale).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), value * scale)
    r = _O.fp8_round(x, fmt)
    lo, hi = _O.fp8_round(np.nextafter(x, np.float32(-np.inf)), fmt), _O.fp8_round(np.nextafter(x, np.float32(np.inf)), fmt)
    return {"changed": float((r != x).mean()), "ties": float(((lo != hi) & (r != x)).mean()),
            "saturated": float((np.abs(x) > FP8_MAX[fmt]).mean()), "flushed": float(((r == 0) & (x != 0)).mean())}


def fp8_round_variant(a, fmt, ties="even", saturate=True):
    """fp8 rounding with a switch for the tie rule and for the clamp: (even, True) is oracle.fp8_round; the others are the WRONG
    conversions the power checks of test_conv_reference.py hold the expected bits against."""
    mant, emin, maxv = (3, -6, 448.0) if fmt == "e4m3" else (2, -14, 57344.0)
    a = np.asarray(a, np.float64)
    m = np.abs(a)
    if saturate:
        m = np.minimum(m, maxv)
    q = np.exp2(np.maximum(np.floor(np.log2(np.maximum(m, 1e-300))), emin) - mant)
    r = (np.round(m / q) if ties == "even" else np.floor(m / q + 0.5)) * q
    if saturate:
        r = np.minimum(r, maxv)
    return np.sign(a) * r


# case tables: every instantiation on the four wide grids (the fp8 plan has the 16 x 8 x 1 geometry only, eae_s2_plan)
IGEMM8_EXACT_CASES = [inst + grid for inst, grid in itertools.product(IGEMM_INSTANCES, GRIDS[2:])]
WGRAD8_MULTI_TILE = {                                    # case: (tiles, slices, tiles per workgroup) under 64 workgroups
    (256, 128, 2, 1, 16, 32, 3): (12, 4, 3),
    (128, 64, 1, 2, 16, 32, 5): (20, 10, 2),
    (256, 128, 4, 1, 16, 32, 3): (12, 4, 3),             # SRC_RAWG: the form the train step launches
}
WGRAD8_EXACT_CASES = [inst + grid for inst, grid in itertools.product(WGRAD_INSTANCES, WGRAD_GRIDS[2:])] + [
    (256, 128, 2, 1, 16, 32, 3), (128, 64, 1, 2, 16, 32, 5), (64, 32, 1, 2, 16, 32, 3), (256, 128, 4, 1, 16, 32, 3)]
FP8_SETTINGS = ("regular", "edge")
REGULAR_SCALE = {"e4m3": 2.0 ** 4, "e5m2": 2.0 ** 12}
SATURATING_SCALE = {"e4m3": 2.0 ** 8, "e5m2": 2.0 ** 15}       # MAX / s = 1.75: about half of an operand clamps
FLUSHING_SCALE = {"e4m3": 2.0 ** -7, "e5m2": 2.0 ** -15}       # 1/8 is half of the smallest subnormal / a quarter of it
WEIGHT_SCALES = (2.0 ** -2, 2.0 ** 0, 2.0 ** 4, 2.0 ** 8)       # k/16 is an e4m3 value at every one of them


def edge_kind(idx):
    """the edge setting of case number idx: even rows saturate, odd rows reach the subnormals and flush.  The tables are instance-major
    with four grids each, so every instantiation (and with it every format, and both kinds of kernel) gets both."""
    return "saturating" if idx % 2 == 0 else "flushing"


def igemm8_scales(idx, setting, fmt):
    """(pixel scale, weight scale) of case number idx under a setting"""
    if setting == "regular":
        return REGULAR_SCALE[fmt], 2.0 ** 4
    return (SATURATING_SCALE if edge_kind(idx) == "saturating" else FLUSHING_SCALE)[fmt], WEIGHT_SCALES[(idx // 2) % 4]


def wgrad8_scales(idx, setting, fmt_s, fmt_b):
    """(small scale, big scale, the operand that has the edge scale or None): rows 4i, 4i+1 put it on the small operand, 4i+2, 4i+3
    on the big one"""
    s_s, s_b = REGULAR_SCALE[fmt_s], REGULAR_SCALE[fmt_b]
    if setting == "regular":
        return s_s, s_b, None
    table = SATURATING_SCALE if edge_kind(idx) == "saturating" else FLUSHING_SCALE
    if (idx // 2) % 2 == 0:
        return table[fmt_s], s_b, "small"
    return s_s, table[fmt_b], "big"


class Igemm8Case:
    """Row idx of IGEMM8_EXACT_CASES under a setting: operands, scales, the e4m3 weight bytes in the kernel's layout, the exact sum
    of the quantised operands (+ bias) with its S, and the expected stored output.  `quant` replaces the operand's conversion and
    `weights` / `operand` the exact sum's inputs: the power checks build wrong references with them."""

    def __init__(self, idx, setting):
        self.idx, self.setting = idx, setting
        self.case = kind, cin, cout, smode, epi, hp, wp, B = IGEMM8_EXACT_CASES[idx]
        rng = np.random.default_rng(41000 + idx)
        self.hin, self.win = (2 * hp, 2 * wp) if kind == 0 else (hp, wp)
        self.hout, self.wout = (hp, wp) if kind == 0 else (2 * hp, 2 * wp)
        self.fmt = fp8_fmt(smode)
        self.s_pix, self.s_w = igemm8_scales(idx, setting, self.fmt)
        self.src = FineSrc(smode, (B, cin, self.hin, self.win), rng)
        self.w = dyadic_weights((cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3), rng)
        w8 = self.w * np.float32(self.s_w)
        assert np.array_equal(_O.fp8_round(w8, "e4m3"), w8)                      # the pack holds the weights themselves
        # kernel layout [cout][9][cin]: conv weight [cout][cin][3][3]; transposed-conv weight [cin][cout][3][3]
        wk = w8.transpose(0, 2, 3, 1) if kind == 0 else w8.transpose(1, 2, 3, 0)
        self.w_bytes = _O.fp8_bytes_e4m3(np.ascontiguousarray(wk.reshape(cout, 9, cin)))
        self.bias = dyadic_bias(cout, rng) if epi == 0 else None
        self.prev = DyadicPrev((B, cout, self.hout, self.wout), rng) if epi == 1 else None
        self.qa = quantised(self.src, self.s_pix, self.fmt)
        self.amax = float(np.abs(self.src.value).max())                          # of the bf16 operand, before the conversion
        self.shares = rounding_shares(self.src.value, self.s_pix, self.fmt)
        self.exact = self.sum_of(self.qa, self.w)
        self.S = (conv_s2_abs if kind == 0 else deconv_s2_abs)(self.qa, self.w) + (0.0 if self.bias is None else
                                                                                   np.abs(self.bias)[None, :, None, None])

    def sum_of(self, operand, weights):
        kind = self.case[0]
        y = conv_s2(operand, weights) if kind == 0 else deconv_s2(operand, weights)
        return y if self.bias is None else y + self.bias[None, :, None, None].astype(np.float64)

    def stored(self, exact):
        """the bf16 tensor the kernel must store for an exact sum"""
        ref = bf16_round(exact_f32(exact))
        return ref if self.prev is None else ref * self.prev.mask               # a decision that lands on 0 gives 0

    def quant_variant(self, ties, saturate):
        sc = np.float64(self.s_pix)
        return fp8_round_variant(self.src.value * sc, self.fmt, ties, saturate) / sc


class Wgrad8Case:
    """Row idx of WGRAD8_EXACT_CASES under a setting"""

    def __init__(self, idx, setting):
        self.idx, self.setting = idx, setting
        self.case = cs, cb, smode, bmode, hs, ws, B = WGRAD8_EXACT_CASES[idx]
        rng = np.random.default_rng(42000 + idx)
        self.fmt_s, self.fmt_b = fp8_fmt(smode), fp8_fmt(bmode)
        self.s_s, self.s_b, self.edge_on = wgrad8_scales(idx, setting, self.fmt_s, self.fmt_b)
        self.small = FineSrc(smode, (B, cs, hs, ws), rng)
        self.big = FineSrc(bmode, (B, cb, 2 * hs, 2 * ws), rng)
        self.qs, self.qb = quantised(self.small, self.s_s, self.fmt_s), quantised(self.big, self.s_b, self.fmt_b)
        self.shares_s = rounding_shares(self.small.value, self.s_s, self.fmt_s)
        self.shares_b = rounding_shares(self.big.value, self.s_b, self.fmt_b)
        self.exact = wgrad_s2(self.qs, self.qb)
        self.S = wgrad_s2_abs(self.qs, self.qb)

    def quant_variant(self, which, ties, saturate):
        src, sc, fmt = (self.small, self.s_s, self.fmt_s) if which == "small" else (self.big, self.s_b, self.fmt_b)
        return fp8_round_variant(src.value * np.float64(sc), fmt, ties, saturate) / np.float64(sc)
