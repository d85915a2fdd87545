"""Bit-exact tests of the fp8 hot path: igemm8_s2_kernel, wgrad8_s2_kernel, fp8_scales_kernel and the choice of the amax slot.

Operands come from tests/conv_ref.py (FineSrc: multiples of 1/8 within 3.5, weights k/16): every scale is a power of two, so only the
fp8 conversion of an operand changes a value, oracle.ae_numpy._q8 restates it, and the quantised operands are on the 1/8 grid again
-- every product and every partial sum of the kernels' fp32 accumulators is exact (budget: S * 2^Q < 2^24 with S from the quantised
operands, held for every row in tests/test_conv_reference.py).  A conv output must equal bf16_round(exact sum + bias), a weight
gradient the exact sum, compared with np.array_equal.  What wrong kernels would do to these expected bits (ties rounded away from
zero, no clamp, a dropped tap, a halo column from the wrong side of a tile seam) is shown on the references in
tests/test_conv_reference.py, never by breaking a kernel.

Instantiations and geometries
  test_igemm8_exact: all 14 instantiations of eae_launch_conv_s2 / eae_launch_deconv_s2 (the two plain ones included), each on the
    position grids 8x16x2 (one 16x8 tile per image), 16x32x1 (2x2 tiles: halos in both directions), 8x32x2 (two tiles across) and
    24x16x1 (three tiles down) -- the fp8 plan has the 16 x 8 x 1 tile only -- under two scale settings: 14 x 4 x 2 = 112 runs.
  test_wgrad8_exact: all 13 instantiations of eae_launch_wgrad_s2 (the six SRC_RAWG ones the train step launches included) on the
    small maps 8x16x1, 16x32x1, 8x32x2, 24x16x1, plus four rows of 16x32 maps with 3 or 5 images: (13 x 4 + 4) x 2 = 112 runs.
    Several tiles per workgroup (the accumulator carried from tile to tile, the double buffer), asserted against the launch
    prediction: 256x128 modes (2, 1) and (4, 1) on 3 images -- 12 tiles on 4 slices, 3 per workgroup -- and 128x64 modes (1, 2) on
    5 images -- 20 tiles on 10 slices, 2 per workgroup.  64x32 (1, 2) on 3 images has 12 slices of one tile.

Scale settings
  regular: pixel scale 2^4 (e4m3) / 2^12 (e5m2: source modes 2 and 4), s_w = 2^4.  The conversion changes 21 % of a mode-0 operand,
    8 % of mode 1 (all of them exact ties: odd eighths above 2), 20 % of mode 2 (17 % ties) and 46 % of mode 4 (24 % ties).
  edge, by the row's index: even rows saturate (2^8 / 2^15: MAX / s = 1.75; clamped: 49 % of modes 0 and 4, 20 % of mode 1, 12 % of
    mode 2), odd rows reach the subnormals and flush (2^-7 / 2^-15; flushed to zero: 3.5 % / 2 % / 17 % / 7 % of modes 0 / 1 / 2 / 4,
    e4m3: every odd eighth is a tie, e5m2: every k/8 with k = 2 mod 4); s_w rotates through 2^-2, 2^0, 2^4, 2^8.  For the weight gradient rows 4i, 4i+1 have the edge scale
    on the small operand and 4i+2, 4i+3 on the big one, the other operand keeps its regular scale.  (Shares computed by
    conv_ref.rounding_shares from the oracle, on (2, 64, 16, 32) operands.)
  The reported amax word is max |bf16 operand| BEFORE the conversion: above MAX / s in every saturating row.

test_fp8_scales_kernel runs fp8_scales_kernel on states built by eae_op_fp8_scales against floor(log2(MAX / (2 a))) computed exactly
(np.frexp), test_fp8_amax_slots the slot a reporting workgroup picks through eae_op_conv_s2_fp8_slots.

What the MI355X showed: every case is bit-equal and no kernel was changed.  The hardware agrees with oracle.fp8_round in the regimes
the probe values of test_fp8_rounding_matches_the_hardware_probe never recorded -- all of e5m2 (v_cvt_scalef32_pk_bf8_bf16), e4m3
ties (to even), subnormal results, the flush of a half and a quarter of the smallest subnormal, the clamp at +-MAX under
MODE.FP16_OVFL -- and the four fp8 MFMA forms (fp8/bf8 x fp8/bf8) add exactly whenever every partial sum is an fp32 value, as the
bf16 form does: the operand grid did not have to be coarsened.  log2f is exact at the power-of-two quotients of a = 7 * 2^k and
right for the bf16 neighbours and, for the weights' fp32 maxima, the fp32 neighbours of those values."""
import os

import numpy as np
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _upload(s):
    """DyadicSrc -> (eae_src, the device tensors it points to)"""
    import gpu_util as G
    keep = [G.to_nhwc_bf16(t) for t in s.tensors]
    cd = G.f32(s.coef) if s.coef is not None else None
    return G.src(s.mode, keep[0], keep[1] if len(keep) > 1 else None, cd), keep + [cd]


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} of {bad.size} differ, first at {idx[:8].tolist()}"


def _as_f32(words):
    return np.asarray(words.cpu().numpy()).view(np.uint32).view(np.float32)


_IG = [(i, s) for i in range(len(R.IGEMM8_EXACT_CASES)) for s in R.FP8_SETTINGS]
_WG = [(i, s) for i in range(len(R.WGRAD8_EXACT_CASES)) for s in R.FP8_SETTINGS]


def _id(table):
    return lambda v: "-".join(map(str, table[v])) if isinstance(v, int) else v


@pytest.mark.parametrize("idx,setting", _IG, ids=_id(R.IGEMM8_EXACT_CASES))
def test_igemm8_exact(lib, idx, setting):
    import gpu_util as G
    from eae_amd._lib import check
    k = R.Igemm8Case(idx, setting)
    kind, cin, cout, smode, epi, hp, wp, B = k.case
    nt = lib.eae_op_conv_s2_ntiles(kind, cin, B, k.hin, k.win)
    assert nt == R.expected_ntiles(kind, cin, cout, hp, wp, B, R.ig_small_setting()) == B * (hp // 8) * (wp // 16)
    R.assert_budget(k.S, R.Q_CONV)
    ref = k.stored(k.exact)

    sd, keep = _upload(k.src)
    wpk = torch.from_numpy(k.w_bytes).to(G.dev())
    bd = G.f32(k.bias) if epi == 0 else None
    yprev_d = pcoef_d = None
    if epi == 1:
        yprev_d, pcoef_d = G.to_nhwc_bf16(k.prev.yprev), G.f32(k.prev.coef)
    qs = G.f32(np.array([1.0 / k.s_pix, 1.0 / (k.s_pix * k.s_w)], np.float32))
    out = torch.full((B, k.hout, k.wout, cout), float("nan"), dtype=torch.bfloat16, device=G.dev())
    flat = torch.full((2 * cout * nt + 64,), float("nan"), dtype=torch.float32, device=G.dev())
    part, guard = flat[:2 * cout * nt].view(2, cout, nt), flat[2 * cout * nt:]
    amax = torch.zeros(1 + 64, dtype=torch.int32, device=G.dev())
    check(lib.eae_op_conv_s2_fp8(G.stream(), kind, sd, cin, cout, B, k.hin, k.win, G.ptr(wpk), G.ptr(bd), G.ptr(out),
                                 G.ptr(part) if epi != 2 else None, epi, G.ptr(yprev_d), G.ptr(pcoef_d), G.ptr(qs), G.ptr(amax)))
    torch.cuda.synchronize()
    got = G.from_nhwc(out)
    print(f"{k.case} {setting}: scales 2^{int(np.log2(k.s_pix))} 2^{int(np.log2(k.s_w))} {k.fmt}, shares {k.shares}, "
          f"{int((got != ref).sum())} of {ref.size} differ")
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    assert torch.isnan(guard).all()
    # the reported maximum: of the bf16 operand, before the conversion (bf16 bits in the high half of the word); one word written
    am = _as_f32(amax)
    assert am[0] == k.amax and not am[1:].any(), (am[0], k.amax)
    if setting == "edge" and R.edge_kind(idx) == "saturating":
        assert am[0] > R.FP8_MAX[k.fmt] / k.s_pix
    if epi == 2:
        assert torch.isnan(part).all()                         # the plain epilogue writes no partials
        return
    assert not torch.isnan(part).any()
    # partial totals against fp64 sums of the expected stored output: the kernels add bf16-exact values, or exact products of them,
    # in fp32 -- the plain summation bound, n terms inside the tiles and ntiles on top
    total = part.cpu().numpy().astype(np.float64).sum(2)
    r64 = ref.astype(np.float64)
    terms = [r64, r64 * r64] if epi == 0 else [r64, r64 * k.prev.xhat]
    n = B * k.hout * k.wout
    for col, t in enumerate(terms):
        want, mag = t.sum((0, 2, 3)), np.abs(t).sum((0, 2, 3))
        err = np.abs(total[col] - want)
        bound = (n + nt) * 2.0 ** -24 * mag
        print(f"partials column {col}: max err {err.max():.3e}, bound at that channel {bound[err.argmax()]:.3e}")
        assert np.all(err <= bound), (col, int(np.argmax(err - bound)), float(err.max()))


@pytest.mark.parametrize("idx,setting", _WG, ids=_id(R.WGRAD8_EXACT_CASES))
def test_wgrad8_exact(lib, idx, setting):
    import gpu_util as G
    from eae_amd._lib import check
    k = R.Wgrad8Case(idx, setting)
    cs, cb, smode, bmode, hs, ws, B = k.case
    R.assert_budget(k.S, R.Q_WGRAD)
    ref = R.exact_f32(k.exact)
    ss, keep_s = _upload(k.small)
    bs, keep_b = _upload(k.big)
    qs = G.f32(np.array([1.0 / k.s_s, 1.0 / k.s_b, 1.0 / (k.s_s * k.s_b)], np.float32))
    scratch = torch.full((6 * 1024 * 1024,), float("nan"), dtype=torch.float32, device=G.dev())
    dw = torch.full((cs, cb, 3, 3), float("nan"), dtype=torch.float32, device=G.dev())
    check(lib.eae_op_wgrad_s2_fp8(G.stream(), ss, bs, cs, cb, B, hs, ws, G.ptr(scratch), scratch.numel(), G.ptr(dw), G.ptr(qs)))
    torch.cuda.synchronize()
    got = dw.cpu().numpy()
    print(f"{k.case} {setting}: scales 2^{int(np.log2(k.s_s))} {k.fmt_s}, 2^{int(np.log2(k.s_b))} {k.fmt_b}, small {k.shares_s}, "
          f"big {k.shares_b}, {int((got != ref).sum())} of {ref.size} differ")
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    # several position slices leave one partial each at the head of the scratch (a single slice writes dw itself)
    geo, tiles, slices, per = R.expected_wgrad_launch(cs, cb, smode, hs, ws, B, scratch.numel())
    used = (slices if slices > 1 else 0) * cs * cb * 9
    assert geo == R.WIDE
    assert not torch.isnan(scratch[:used]).any() and torch.isnan(scratch[used:]).all(), (geo, tiles, slices, per)
    hit = R.WGRAD8_MULTI_TILE.get(k.case)
    if hit is not None and "EAE_WGRAD_WGS" not in os.environ:
        assert (tiles, slices, per) == hit and per > 1


# ---------------------------------------------------------------------------------------------------------------
# fp8_scales_kernel
# ---------------------------------------------------------------------------------------------------------------
SLOTS = 64                                    # FP8_AMAX_SLOTS (the op refuses nothing here: a wrong value shows as wrong maxima)
F32 = np.float32


def _bits(v):
    return int(np.asarray(v, F32).view(np.uint32))


def _scale_ref(bits, maxv, keep):
    """fp8_scale_from, exactly: MAX = 7 * 2^E and a = m * 2^ex with m in [1/2, 1) give MAX / (2 a) = (3.5 / m) * 2^(E - ex), and
    3.5 / m is in (3.5, 7]: its floor(log2) is 2 from m <= 7/8 down (the quotient is an exact power of two AT 7/8) and 1 above."""
    a = np.uint32(bits).view(F32)
    if not (a > 0) or not (a < F32(3.0e38)):
        return F32(keep)
    m, ex = np.frexp(np.float64(a))
    E = {448.0: 6, 57344.0: 13}[maxv]
    e = E - int(ex) + (2 if m <= 0.875 else 1)
    return F32(2.0 ** min(max(e, -60), 60))


def _bf16_neighbours(v):
    b = _bits(v)
    assert b & 0xFFFF == 0
    return [b - 0x10000, b, b + 0x10000]


def _scale_inputs(maxv, fp32_neighbours):
    """amax words of one kind of tensor: bf16 values (activations, gradients) or any fp32 (weights)"""
    vals = [0, 0x7F800000, 0x7FC00000, _bits(3.0e38), 0x7F620000, 0x7F7F0000,        # 0, +inf, NaN, 3e38 and bf16 values above it
            _bits(2.0 ** -100), _bits(2.0 ** 100), _bits(2.0 ** -66), _bits(2.0 ** 72), _bits(1.0), _bits(0.4375), _bits(3.0)]
    for k in (-20, -9, -3, 0, 4, 11, 30):
        vals += _bf16_neighbours(7.0 * 2.0 ** k)
        if fp32_neighbours:
            vals += [_bits(7.0 * 2.0 ** k) - 1, _bits(7.0 * 2.0 ** k) + 1]
    assert F32(3.0e38) <= np.uint32(0x7F620000).view(F32) and _bits(1e38) < _bits(3.0e38)
    return vals + [_bits(1e38)]


def test_fp8_scales_kernel(lib):
    import ctypes as C
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(77)
    maxv = (448.0, 57344.0, 448.0)                       # act, grad, w
    vals = [_scale_inputs(448.0, False), _scale_inputs(57344.0, False), _scale_inputs(448.0, True)]
    rounds = max(-(-len(v) // 6) for v in vals)
    seen = set()
    for r in range(rounds):
        amax = np.zeros((3, 6, SLOTS), np.uint32)
        peak = np.zeros((3, 6), np.uint32)
        s_in = np.zeros((3, 6), F32)
        for k in range(3):
            for i in range(6):
                a = vals[k][(r * 6 + i) % len(vals[k])]
                peak[k, i] = a
                s_in[k, i] = 2.0 ** (k * 6 + i + r + 1)                       # never 1: a kept scale is seen to be kept
                slot = (0, SLOTS - 1, 17 + i)[(r + i + k) % 3]
                if a and (r + i) % 2 == 0:                                    # smaller maxima in the other slots (bf16 bits)
                    lower = rng.integers(0, a >> 16, SLOTS).astype(np.uint32) << np.uint32(16)
                    amax[k, i] = np.minimum(lower, a)
                amax[k, i, slot] = a
                seen.add((k, slot))
        assert not (s_in == 1).any()
        s_out, qs, left = np.full((3, 6), np.nan, F32), np.full((6, 8), np.nan, F32), np.full((3, 6, SLOTS), 7, np.uint32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        check(lib.eae_op_fp8_scales(G.stream(), p(amax), p(s_in), p(s_out), p(qs), p(left)))
        want = np.array([[_scale_ref(peak[k, i], maxv[k], s_in[k, i]) for i in range(6)] for k in range(3)], F32)
        assert np.array_equal(s_out.view(np.uint32), want.view(np.uint32)), (r, [
            (k, i, hex(int(peak[k, i])), float(s_out[k, i]), float(want[k, i])) for k in range(3) for i in range(6) if s_out[k, i] != want[k, i]])
        sa, sg, sw = want
        one = F32(1)
        q_want = np.zeros((6, 8), F32)
        for i in range(6):
            ss, sb = (sg[i], sa[i]) if i < 3 else (sa[i], sg[i])              # conv layers: small = gradient; transposed: small = activation
            q_want[i] = [one / sa[i], one / F32(sa[i] * sw[i]), one / sg[i], one / F32(sg[i] * sw[i]),
                         one / ss, one / sb, one / F32(ss * sb), 0.0]
        assert np.isfinite(q_want).all() and (q_want[:, :7] > 0).all()
        assert np.array_equal(qs.view(np.uint32), q_want.view(np.uint32)), (r, qs, q_want)
        assert not left.any()                                                 # every maximum cleared for the next step
    assert seen >= {(k, s) for k in range(3) for s in (0, SLOTS - 1)}
    # the clamp acted in both directions, scales were kept, and the exact-power-of-two quotients were among the inputs
    assert _scale_ref(_bits(2.0 ** -100), 448.0, 3.0) == 2.0 ** 60 and _scale_ref(_bits(2.0 ** 100), 57344.0, 3.0) == 2.0 ** -60
    assert _scale_ref(0x7FC00000, 448.0, 3.0) == 3.0 and _scale_ref(0, 448.0, 3.0) == 3.0 and _scale_ref(_bits(3.0e38), 448.0, 3.0) == 3.0
    assert [_scale_ref(b, 448.0, 3.0) for b in _bf16_neighbours(7.0)] == [32.0, 32.0, 16.0]
    assert [_scale_ref(b, 57344.0, 3.0) for b in _bf16_neighbours(7.0 * 2 ** 11)] == [2.0, 2.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------
# the slot a reporting workgroup picks: (tile_id & amax_mask) * amax_stride
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,cin,cout", [(0, 32, 64), (1, 64, 32)])
def test_fp8_amax_slots(lib, kind, cin, cout):
    """Eight tiles (2 images of 2 x 2 tiles) report into 4 slots 32 words apart.  Every tile has its own peak, strictly inside the
    part of the operand only that tile reads (four positions from its border), over a background within 3.5."""
    import gpu_util as G
    from eae_amd._lib import check
    slots, stride, hp, wp, B = 4, 32, 16, 32, 2
    rng = np.random.default_rng(90 + kind)
    hin, win = (2 * hp, 2 * wp) if kind == 0 else (hp, wp)
    hout, wout = (hp, wp) if kind == 0 else (2 * hp, 2 * wp)
    src = R.FineSrc(0, (B, cin, hin, win), rng)
    x = src.tensors[0]
    peaks = 4.0 + 0.5 * rng.permutation(8)                                    # bf16 values, all different, all above the background
    tiles_y, tiles_x = hp // 8, wp // 16
    for t in range(8):
        img, tyb, txb = t // (tiles_y * tiles_x), (t // tiles_x) % tiles_y, t % tiles_x          # the kernel's tile order
        py, px = tyb * 8 + 4, txb * 16 + 8                                    # a position in the middle of the tile
        y0, x0 = (2 * py, 2 * px) if kind == 0 else (py, px)
        x[img, rng.integers(cin), y0, x0] = peaks[t] * (-1.0) ** t
    assert np.array_equal(R.bf16_round(x), x)
    assert lib.eae_op_conv_s2_ntiles(kind, cin, B, hin, win) == 8
    w = R.dyadic_weights((cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3), rng)
    w8 = w * F32(16)
    from oracle import ae_numpy as O
    wk = w8.transpose(0, 2, 3, 1) if kind == 0 else w8.transpose(1, 2, 3, 0)
    wpk = torch.from_numpy(O.fp8_bytes_e4m3(np.ascontiguousarray(wk.reshape(cout, 9, cin)))).to(G.dev())
    xd = G.to_nhwc_bf16(x)
    bd = G.f32(np.zeros(cout, F32))
    qs = G.f32(np.array([1.0 / 16, 1.0 / 256], F32))
    out = torch.zeros((B, hout, wout, cout), dtype=torch.bfloat16, device=G.dev())
    part = torch.zeros((2, cout, 8), dtype=torch.float32, device=G.dev())
    words = torch.zeros(slots * stride + 64, dtype=torch.int32, device=G.dev())
    check(lib.eae_op_conv_s2_fp8_slots(G.stream(), kind, G.src(0, xd), cin, cout, B, hin, win, G.ptr(wpk), G.ptr(bd), G.ptr(out),
                                       G.ptr(part), 0, None, None, G.ptr(qs), G.ptr(words), slots, stride))
    torch.cuda.synchronize()
    got = words.cpu().numpy().view(np.uint32)
    want = np.zeros_like(got)
    for s in range(slots):
        want[s * stride] = _bits(max(peaks[t] for t in range(8) if t & 3 == s))
    assert np.array_equal(got, want), (np.flatnonzero(got).tolist(), [hex(int(v)) for v in got[np.flatnonzero(got)]],
                                       [hex(int(v)) for v in want[::stride][:slots]])
    # and the launch computed the conv of the quantised operand all the same
    ref = R.bf16_round(R.exact_f32((R.conv_s2 if kind == 0 else R.deconv_s2)(O._q8(x, 16.0, "e4m3").astype(np.float64), w)))
    assert np.array_equal(G.from_nhwc(out), ref)
