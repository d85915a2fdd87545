"""Exact references, operands and case tables for the two C-band edge layers, enc.conv1 and dec.deconv4 (no torch, no GPU).

The fp64 loops, the dyadic builders and the budget rule are conv_ref's (imported, not copied): every stored value is a coarse dyadic
number, so the load transform, every product and every partial sum -- in any order -- is exact in fp32, and the edge kernels must
give bf16_round(exact sum + bias) (conv1, deconv4's backward-data), the exact sum (the two weight gradients) and the exact
pre-sigmoid sum (deconv4 + loss) bit for bit.

The C-band operand is conv_ref.DyadicSrc(0, ...): multiples of 1/4 with |v| <= 1, exact in bf16, so conv1's fp32 -> bf16 rounding on
load changes nothing.  It is stored as an fp32 NCHW image (source kind 0) or as an NHWC-CP bf16 tensor whose bands >= C are zero
(source kind 1: what deconv4 + loss and sigmoid_bwd write).

Budgets, from the formats (S = sum of |a||w| of one output; partial sums are multiples of 2^-q of magnitude <= S, exact in fp32 while
S * 2^q < 2^24):
  conv1 / backward-data of deconv4: image 1/4 x weight 1/16 -> products are multiples of 2^-6; the fp32 bias is a multiple of 2^-7,
                                    so rows with a bias are budgeted at q = 7
  deconv4                         : 32-channel source 1/8 x weight 1/16 -> 2^-7, bias 2^-7
  edge weight gradients           : image 1/4 x side 1/8 -> 2^-5
"""
import itertools
import os

from types import SimpleNamespace

import numpy as np

from conv_ref import (BIASMAX, VMAX, WMAX, DyadicPrev, DyadicSrc, _cdiv, conv_s2, conv_s2_abs, deconv_s2, deconv_s2_abs, dyadic_bias,
                      dyadic_weights, wgrad_s2, wgrad_s2_abs)

Q_EDGE_CONV, Q_DECONV4, Q_EDGE_WGRAD, Q_BIAS = 6, 7, 5, 7

E_TH, E_TW = 4, 32                                   # a workgroup's tile: 4 x 32 positions of the 32-channel map


def edge_cp(c):
    """bands padded in LDS, in the weight packs and in the NHWC-CP gradient"""
    return 4 if c == 3 else 8 if c <= 8 else 16


def edge_kp(c):
    return (9 * edge_cp(c) + 31) // 32 * 32


def edge_nkc(c):
    """32-wide k chunks of the weight gradient's K = 9C"""
    return (9 * c + 31) // 32


def edge_lp_stride(c):
    """floats of a row of deconv4's loss partials: the squared error, C gradient sums, zero padding to whole float4s"""
    return (c + 4) // 4 * 4


def edge_tiles(h, w, b):
    return b * (h // 2 // E_TH) * (w // 2 // E_TW)


def to_nhwcp(value, c):
    """[B,C,H,W] -> [B,H,W,CP] fp32 with zero bands >= C"""
    b, _, h, w = value.shape
    out = np.zeros((b, h, w, edge_cp(c)), np.float32)
    out[..., :c] = value.transpose(0, 2, 3, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------
# CP = 4; CP = 8 partly and fully used; CP = 16 partly and fully used.  nkc = 1, 1, 2, 3, 3, 4, 5
EDGE_BANDS = [1, 3, 5, 8, 9, 13, 16]
# image grids (H, W, B)
EDGE_GRIDS = [
    (8, 64, 1),       # one tile: every halo is padding
    (8, 64, 3),       # one tile per image
    (16, 128, 1),     # 2x2 tiles
    (8, 192, 2),      # three across
    (24, 64, 2),      # three down
    (24, 192, 1),     # 3x3: a tile with four real neighbours
]
# (source kind, epilogue): the four edge_conv_kernel pairs eae_launch_edge_conv lists
EDGE_CONV_INSTANCES = [
    (0, 0),           # conv1 forward: fp32 image, + bias, statistics partials
    (1, 1),           # backward-data of deconv4: NHWC-CP gradient, ReLU mask, BatchNorm-backward partials
    (1, 2),           # plain, NHWC-CP source
    (0, 2),           # plain, fp32 image
]
# (source kind, side mode): the three edge_wgrad_kernel pairs of eae_launch_edge_wgrad
EDGE_WGRAD_INSTANCES = [
    (0, 2),           # conv1's weight gradient: fp32 image, BatchNorm-backward side
    (1, 1),           # deconv4's: NHWC-CP gradient, BatchNorm + ReLU side
    (0, 0),           # plain side
]
# source modes of deconv4_loss_kernel
DECONV4_INSTANCES = [1, 0]                            # BatchNorm + ReLU (the training step's), plain

EDGE_CONV_CASES = [i + (c,) + g for i, c, g in itertools.product(EDGE_CONV_INSTANCES, EDGE_BANDS, EDGE_GRIDS)]
# (kind, side mode, C, H, W, B, scratch in slices of 288*C floats or None for plenty)
EDGE_WGRAD_GRID_CASES = [i + (c,) + g + (None,) for i, c, g in itertools.product(EDGE_WGRAD_INSTANCES, EDGE_BANDS, EDGE_GRIDS)]
DECONV4_CASES = [(m, c) + g for m, c, g in itertools.product(DECONV4_INSTANCES, EDGE_BANDS, EDGE_GRIDS)]

# Rows whose workgroups loop over several tiles: case -> (tiles, workgroups, tiles per workgroup) under the launcher's default caps
EDGE_WGRAD_MULTI_TILE = {
    (0, 2, 3, 8, 64, 520, None): (520, 260, 2),       # main source above its cap of 512: every workgroup two tiles (two images)
    (1, 1, 3, 8, 64, 520, None): (520, 174, 3),       # side source above its cap of 256: three tiles, the last workgroup one
    (0, 2, 5, 16, 64, 5, 4): (10, 2, 5),              # scratch halving 10 -> 5 -> 2: the loop crosses an image boundary mid-way
    (1, 1, 8, 16, 64, 5, 4): (10, 2, 5),              # the same on the NHWC-CP source
    (0, 0, 16, 24, 64, 3, 2): (9, 2, 5),              # 9 -> 4 -> 2: 5 + 4, a short last workgroup; five k chunks rebuilt per tile
}
EDGE_WGRAD_CASES = EDGE_WGRAD_GRID_CASES + list(EDGE_WGRAD_MULTI_TILE)
EDGE_WGRAD_PLENTY = 2 * 1024 * 1024                   # floats of scratch where a row names none: more than any row's launch fills


def edge_conv_budget(kind, epi, c, h, w, b):
    """(S of any output by construction, q): nine taps x C bands, plus the bias under the forward epilogue"""
    return 9 * c * VMAX[0] * WMAX + (BIASMAX if epi == 0 else 0.0), Q_BIAS if epi == 0 else Q_EDGE_CONV


def deconv4_budget(smode, c, h, w, b):
    """an output pixel of a stride-2 transposed conv collects at most 2 x 2 of the nine taps, from 32 channels each"""
    return 4 * 32 * VMAX[smode] * WMAX + BIASMAX, Q_DECONV4


def edge_wgrad_budget(kind, smode, c, h, w, b, slices=None):
    """one term per position of the 32-channel map"""
    return b * (h // 2) * (w // 2) * VMAX[0] * VMAX[smode], Q_EDGE_WGRAD


def edge_wgrad_scratch_floats(case):
    c, slices = case[2], case[6]
    return EDGE_WGRAD_PLENTY if slices is None else slices * 288 * c


# ---------------------------------------------------------------------------------------------------------------
# the operands and the exact result of a row (seeded by the row: the CPU self-tests check the very references the GPU tests use)
# `exact`: the fp64 result, `S`: the same sum over magnitudes (what the budget is about)
# ---------------------------------------------------------------------------------------------------------------
def _bc(v):
    return v[None, :, None, None].astype(np.float64)


def edge_conv_case(kind, epi, c, H, W, B):
    """x: the C-band operand; w [32][C][3][3]; bias [32] under the forward epilogue, prev (DyadicPrev) under the mask epilogue"""
    rng = np.random.default_rng(41000 + 1000 * kind + 100 * epi + 10 * c + 3 * H + W + B)
    x = DyadicSrc(0, (B, c, H, W), rng)
    w = dyadic_weights((32, c, 3, 3), rng)
    exact, S = conv_s2(x.value, w), conv_s2_abs(x.value, w)
    bias = prev = None
    if epi == 0:
        bias = dyadic_bias(32, rng)
        exact, S = exact + _bc(bias), S + np.abs(_bc(bias))
    if epi == 1:
        prev = DyadicPrev((B, 32, H // 2, W // 2), rng)
    return SimpleNamespace(x=x, w=w, bias=bias, prev=prev, exact=exact, S=S)


def edge_wgrad_case(kind, smode, c, H, W, B, slices=None):
    """x: the C-band operand; side: the 32-channel map with its load transform; exact [32][C][3][3]"""
    rng = np.random.default_rng(42000 + 1000 * kind + 100 * smode + 10 * c + 3 * H + W + B)
    x = DyadicSrc(0, (B, c, H, W), rng)
    side = DyadicSrc(smode, (B, 32, H // 2, W // 2), rng)
    return SimpleNamespace(x=x, side=side, exact=wgrad_s2(side.value, x.value), S=wgrad_s2_abs(side.value, x.value))


def deconv4_case(smode, c, H, W, B):
    """a3: the 32-channel source; w [32][C][3][3] ([Cin][Cout]); bias [C]; exact: the pre-sigmoid sum with the bias; target: any
    fp32 in [0, 1); gscale: a power of two"""
    rng = np.random.default_rng(43000 + 100 * smode + 10 * c + 3 * H + W + B)
    a3 = DyadicSrc(smode, (B, 32, H // 2, W // 2), rng)
    w = dyadic_weights((32, c, 3, 3), rng)
    bias = dyadic_bias(c, rng)
    target = rng.random((B, c, H, W), dtype=np.float32)
    return SimpleNamespace(a3=a3, w=w, bias=bias, target=target, gscale=np.float32(2.0 ** -7),
                           exact=deconv_s2(a3.value, w) + _bc(bias), S=deconv_s2_abs(a3.value, w) + np.abs(_bc(bias)))


# ---------------------------------------------------------------------------------------------------------------
# the launch a weight-gradient case is meant to be: the edge plan of csrc/eae_wgrad_plan.h restated (test_wgrad_plan.py compares the two)
# ---------------------------------------------------------------------------------------------------------------
def edge_wgrad_cap_setting(kind):
    """the launcher's workgroup cap for a source kind (read once per process): 512 on the fp32 image or what EAE_EDGE_WGRAD_BLOCKS
    says, 256 on the NHWC-CP source (the launch beside the backward-data chain) or what EAE_EDGE_WGRAD_SIDE_BLOCKS says"""
    name, default = ("EAE_EDGE_WGRAD_SIDE_BLOCKS", 256) if kind == 1 else ("EAE_EDGE_WGRAD_BLOCKS", 512)
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        return int(v.strip())
    except ValueError:
        return 0                                                   # atoi of no number


def expected_edge_wgrad_launch(kind, C, H, W, B, scratch_floats, mult=1, caps=None):
    """(tiles, workgroups, tiles per workgroup): at most `cap` workgroups and one per tile, halved while their 288*C-float partials
    do not fit the scratch; a workgroup takes ceil(tiles / workgroups) consecutive tiles, and the workgroups that remain non-empty
    are launched.  mult: the members of a grouped step (eae_set_geometry_mult) share the cap, down to 32 workgroups each; caps: (fp32
    image, NHWC-CP source) given outright instead of read from the environment.  None when the launcher refuses: a scratch below
    one partial.  This is csrc/eae_wgrad_plan.h restated; test_wgrad_plan.py holds the two together without a GPU."""
    tiles, sl = edge_tiles(H, W, B), 32 * 9 * C
    cap = edge_wgrad_cap_setting(kind) if caps is None else caps[kind]
    if mult > 1:
        cap = max(cap // mult, 32)
    blocks = min(tiles, cap)
    while blocks * sl > scratch_floats and blocks > 1:
        blocks //= 2
    per = _cdiv(tiles, blocks)
    if _cdiv(tiles, per) * sl > scratch_floats:
        return None
    return tiles, _cdiv(tiles, per), per


# ---------------------------------------------------------------------------------------------------------------
# x_hat = 1 / (1 + exp(-s)) as deconv4 + loss computes it in fp32, from an exact s
# ---------------------------------------------------------------------------------------------------------------
SIG_A, SIG_B, SIG_C = 2.0, 1.25, 1.5


def sigmoid_bound(s):
    """(sigma, bound): the fp64 sigmoid of the exact pre-activation and the largest |x_hat - sigma| a correct kernel can show.

    The kernel evaluates  x_hat = fl(1 / fl(1 + e)),  e = exp2(fl(L * (-s))),  L = fl(log2 e) = 0x1.715476p+0: the fast exponential
    of the HIP headers (__expf: the hardware exp2 of the product with L), an fp32 add, and the correctly rounded fp32 division the
    compiler emits without fast-math.  With u = 2^-24:
      * L differs from log2(e) by 0.224 u relatively and the product rounds once (u): the argument of exp2 is off by at most
        1.224 u |s| log2(e), which the exponential turns into a RELATIVE error of e of 1.224 u |s| (ln 2 * log2 e = 1).  b = 1.25
        (the 2 % on top cover the second-order terms: the factors (1 + delta) multiplied out, and the curvature of 1 / (1 + e)).
      * the hardware exp2 (V_EXP_F32) is specified to 1 ulp by the instruction set manual: relative error of e at most 2^-23 = 2 u.
        a = 2.  It flushes denormal results: an absolute error of e below 2^-126, far below every other term.
      * d sigma / d e * e = -sigma (1 - sigma): a relative error delta of e moves sigma by sigma (1 - sigma) delta.
      * t = fl(1 + e) is off by half a unit in the last place of t, at most u t, which moves 1/t = sigma by at most sigma u, and
        for t in [1, 2) -- every sigma > 1/2 -- by sigma^2 u; the division rounds to half a unit of x_hat <= 1: at most u / 2.
        Neither shrinks with 1 - sigma, so they stand beside the first term: at most 1.5 u together.
      * where exp2 overflows (s < -88.7) x_hat is 0 and sigma < 2^-127: inside the constant term.
    Hence  |x_hat - sigma| <= sigma (1 - sigma) (2 + 1.25 |s|) 2^-24 + 1.5 * 2^-24."""
    s = np.asarray(s, np.float64)
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-s))
    one_minus = np.where(s > 0, 1.0 / (1.0 + np.exp(np.minimum(s, 700.0))), 1.0 - sig)     # 1 - sigma without cancellation
    return sig, sig * one_minus * (SIG_A + SIG_B * np.abs(s)) * 2.0 ** -24 + SIG_C * 2.0 ** -24
