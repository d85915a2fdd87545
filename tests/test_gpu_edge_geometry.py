"""Bit-exact tests of the C-band edge kernels -- enc.conv1, dec.deconv4 + loss, and their weight gradients -- on every geometry.

Every instantiation eae_edge_launch.hip lists runs at seven band counts (CP = 4, CP = 8 and 16 partly and fully used; one to five k
chunks of the weight gradient) on six image grids: a single 4x32 tile whose halos are all padding, one tile per image, 2x2 tiles,
three across, three down, and 3x3 with a tile that has four real neighbours.  The operands are dyadic (tests/edge_ref.py), so the
fp32 accumulators are exact: conv1 and deconv4's backward-data must give bf16_round(exact sum + bias), the weight gradients the exact
sum, and deconv4's x_hat the sigmoid of an exact pre-activation -- compared with np.array_equal, or for x_hat within a bound derived
from the fast exponential alone (edge_ref.sigmoid_bound).

The weight gradient runs in addition on rows whose workgroups loop over several tiles (edge_ref.EDGE_WGRAD_MULTI_TILE): above the
workgroup cap of each source kind, through the scratch-halving branch of the launcher, across an image boundary inside one
workgroup's loop, and with a short last workgroup.  The launch is observed in how much of a NaN-preset scratch it wrote.

Outputs are preset to NaN with a NaN guard band behind each: a skipped element and a store past the end both show."""
import os

import numpy as np
import pytest
import torch

import conv_ref as R
import edge_ref as E

pytestmark = pytest.mark.gpu

GUARD = 1024          # elements of NaN behind every output


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} of {bad.size} differ, first at {idx[:8].tolist()}"


def _nan(n, dtype):
    """n elements of NaN and a guard band behind them, in one allocation: (output, guard)"""
    import gpu_util as G
    flat = torch.full((n + GUARD,), float("nan"), dtype=dtype, device=G.dev())
    return flat[:n], flat[n:]


def _pack_edge(lib, w, c):
    """the engine's packs of a [32][C][3][3] weight (eae_op_pack_edge: pinned by test_gpu_pack.py)"""
    import gpu_util as G
    from eae_amd._lib import check
    wd = G.f32(w)
    both = torch.zeros(32 * E.edge_kp(c) + 4 * E.edge_cp(c) * 128, dtype=torch.bfloat16, device=G.dev())
    wpack, wjoint = both[:32 * E.edge_kp(c)], both[32 * E.edge_kp(c):]
    check(lib.eae_op_pack_edge(G.stream(), G.ptr(wd), c, G.ptr(wpack), G.ptr(wjoint)))
    return wpack, wjoint


def _upload_band_operand(kind, x, c):
    """the C-band operand as source kind 0 (fp32 NCHW) or 1 (bf16 NHWC-CP, bands >= C zero)"""
    import gpu_util as G
    if kind == 0:
        return G.f32(x.tensors[0])
    return G.f32(E.to_nhwcp(x.tensors[0], c)).to(torch.bfloat16)


def _upload_side(s):
    """DyadicSrc of the 32-channel map -> (eae_src, the device tensors it points to)"""
    import gpu_util as G
    keep = [G.to_nhwc_bf16(t) for t in s.tensors]
    cd = G.f32(s.coef) if s.coef is not None else None
    return G.src(s.mode, keep[0], keep[1] if len(keep) > 1 else None, cd), keep + [cd]


def _within_budget(S, bound, q):
    """the row's sums of magnitudes stay under the bound its table promises by construction, and that bound under 2^24 units"""
    assert S.max() <= bound
    R.assert_budget(bound, q)


def _summation_bound(n, nt, t):
    """fp32 sums of exactly representable terms, n inside the tiles and nt tiles on top, against the fp64 sum"""
    return (n + nt) * 2.0 ** -24 * np.abs(t)


@pytest.mark.parametrize("kind,epi,c,H,W,B", E.EDGE_CONV_CASES)
def test_edge_conv_exact(lib, kind, epi, c, H, W, B):
    import gpu_util as G
    from eae_amd._lib import check
    ho, wo = H // 2, W // 2
    nt = E.edge_tiles(H, W, B)
    k = E.edge_conv_case(kind, epi, c, H, W, B)
    _within_budget(k.S, *E.edge_conv_budget(kind, epi, c, H, W, B))
    ref = R.bf16_round(R.exact_f32(k.exact))
    bd = G.f32(k.bias) if epi == 0 else None
    prev, yprev_d, pcoef_d = k.prev, None, None
    if epi == 1:
        yprev_d, pcoef_d = G.to_nhwc_bf16(prev.yprev), G.f32(prev.coef)
        ref = ref * prev.mask                                  # a decision that lands on 0 gives 0
    wpack, _ = _pack_edge(lib, k.w, c)
    xd = _upload_band_operand(kind, k.x, c)
    out, out_guard = _nan(B * ho * wo * 32, torch.bfloat16)
    part, part_guard = _nan(2 * 32 * nt, torch.float32)
    check(lib.eae_op_edge_conv_c(G.stream(), kind, G.ptr(xd), c, B, H, W, G.ptr(wpack), G.ptr(bd), G.ptr(out), G.ptr(part), epi,
                                 G.ptr(yprev_d), G.ptr(pcoef_d)))
    torch.cuda.synchronize()
    got = G.from_nhwc(out.view(B, ho, wo, 32))
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    assert torch.isnan(out_guard).all() and torch.isnan(part_guard).all()
    if epi == 2:
        assert torch.isnan(part).all()                         # the plain epilogue writes no partials
        return
    assert not torch.isnan(part).any()
    total = part.view(2, 32, nt).cpu().numpy().astype(np.float64).sum(2)
    r64 = ref.astype(np.float64)
    terms = [r64, r64 * r64] if epi == 0 else [r64, r64 * prev.xhat]      # (sum y, sum y^2), or (sum g, sum g * xhat) under the mask
    n = B * ho * wo
    for col, t in enumerate(terms):
        want, bound = t.sum((0, 2, 3)), _summation_bound(n, nt, t).sum((0, 2, 3))
        err = np.abs(total[col] - want)
        print(f"partials column {col}: max err {err.max():.3e}, bound at that channel {bound[err.argmax()]:.3e}")
        assert np.all(err <= bound), (col, int(np.argmax(err - bound)), float(err.max()))


def _edge_wgrad_exact(lib, kind, smode, c, H, W, B, slices, mult=1):
    """one weight-gradient launch (as one of `mult` members of a grouped step) on a NaN-preset scratch: dw bit for bit, and the
    launch edge_ref.expected_edge_wgrad_launch says it is, which is returned"""
    import gpu_util as G
    from eae_amd._lib import check
    case = (kind, smode, c, H, W, B, slices)
    k = E.edge_wgrad_case(*case)
    _within_budget(k.S, *E.edge_wgrad_budget(*case))
    ref = R.exact_f32(k.exact)                                  # [32][C][3][3]
    xd = _upload_band_operand(kind, k.x, c)
    sd, keep = _upload_side(k.side)
    nsc = E.edge_wgrad_scratch_floats(case)
    scratch, scratch_guard = _nan(nsc, torch.float32)
    dw, dw_guard = _nan(32 * c * 9, torch.float32)
    check(lib.eae_set_geometry_mult(mult))
    try:
        check(lib.eae_op_edge_wgrad_c(G.stream(), kind, G.ptr(xd), c, B, H, W, sd, G.ptr(scratch), nsc, G.ptr(dw)))
    finally:
        check(lib.eae_set_geometry_mult(1))
    torch.cuda.synchronize()
    got = dw.cpu().numpy().reshape(32, c, 3, 3)
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    assert torch.isnan(dw_guard).all() and torch.isnan(scratch_guard).all()
    # the launch this row is meant to be: every workgroup leaves one partial of 288*C floats at the head of the scratch
    tiles, blocks, per = E.expected_edge_wgrad_launch(kind, c, H, W, B, nsc, mult)
    used = blocks * 288 * c
    assert used <= nsc
    written = ~torch.isnan(scratch)
    assert written[:used].all() and not written[used:].any(), (tiles, blocks, per, int(written.sum()), used)
    return tiles, blocks, per


def _caps_unset():
    return "EAE_EDGE_WGRAD_BLOCKS" not in os.environ and "EAE_EDGE_WGRAD_SIDE_BLOCKS" not in os.environ


@pytest.mark.parametrize("kind,smode,c,H,W,B,slices", E.EDGE_WGRAD_CASES)
def test_edge_wgrad_exact(lib, kind, smode, c, H, W, B, slices):
    case = (kind, smode, c, H, W, B, slices)
    tiles, blocks, per = _edge_wgrad_exact(lib, *case)
    if case in E.EDGE_WGRAD_MULTI_TILE and _caps_unset():
        assert (tiles, blocks, per) == E.EDGE_WGRAD_MULTI_TILE[case] and per > 1


def test_edge_wgrad_exact_as_a_member_of_a_grouped_step(lib):
    """The members of a grouped step share the workgroup cap (eae_set_geometry_mult): the row above the main source's cap, 260
    workgroups of 2 tiles alone, runs with two members under a cap of 512 / 2 = 256 -- 174 workgroups of 3 tiles, the last with one."""
    case = (0, 2, 3, 8, 64, 520, None)
    assert E.EDGE_WGRAD_MULTI_TILE[case] == (520, 260, 2)
    tiles, blocks, per = _edge_wgrad_exact(lib, *case, mult=2)
    if _caps_unset():
        assert (tiles, blocks, per) == (520, 174, 3)


@pytest.mark.parametrize("smode,c,H,W,B", E.DECONV4_CASES)
def test_deconv4_loss_exact(lib, smode, c, H, W, B):
    """x_hat against the fp64 sigmoid of the exact pre-activation within edge_ref.sigmoid_bound (derived there: the fast
    exponential, one add, one division); the gradient bit for bit from the kernel's own x_hat; the loss partials against fp64
    sums of what the kernel stored.  (On an MI355X the largest x_hat error over the table was 0.943 of the bound: 1.46 * 2^-24 at
    s = 5.086, sigma = 0.994 -- the roundings of 1 + e and of the division, which the bound's constant term 1.5 * 2^-24 is for.)"""
    import gpu_util as G
    from eae_amd._lib import check
    hin, win = H // 2, W // 2
    cp, lps, nt = E.edge_cp(c), E.edge_lp_stride(c), E.edge_tiles(H, W, B)
    k = E.deconv4_case(smode, c, H, W, B)
    _within_budget(k.S, *E.deconv4_budget(smode, c, H, W, B))
    s = R.exact_f32(k.exact)
    x, gscale = k.target, k.gscale
    assert x.dtype == np.float32 and 0.0 <= x.min() and x.max() < 1.0 and np.log2(float(gscale)) % 1 == 0
    _, wjoint = _pack_edge(lib, k.w, c)
    sd, keep = _upload_side(k.a3)
    bd, xd = G.f32(k.bias), G.f32(x)
    x_hat, xh_guard = _nan(B * c * H * W, torch.float32)
    g, g_guard = _nan(B * H * W * cp, torch.bfloat16)
    lp, lp_guard = _nan(nt * lps, torch.float32)
    check(lib.eae_op_deconv4_loss_c(G.stream(), sd, c, B, hin, win, G.ptr(wjoint), G.ptr(bd), G.ptr(xd), float(gscale), G.ptr(x_hat),
                                    G.ptr(g), G.ptr(lp)))
    torch.cuda.synchronize()
    assert torch.isnan(xh_guard).all() and torch.isnan(g_guard).all() and torch.isnan(lp_guard).all()
    xh = x_hat.cpu().numpy().reshape(B, c, H, W)
    assert not np.isnan(xh).any(), _where(np.isnan(xh))
    # 1. x_hat
    sig, bound = E.sigmoid_bound(s)
    err = np.abs(xh.astype(np.float64) - sig)
    worst = int(np.argmax(err / bound))
    print(f"x_hat: max |err| / bound = {(err / bound).max():.3f} (|err| {err.flat[worst]:.3e} at s = {s.flat[worst]})")
    assert np.all(err <= bound), _where(err > bound)
    # 2. the gradient: bf16(((gscale * d) * x_hat) * (1 - x_hat)), d = x_hat - x, every operation one fp32 rounding
    gr = g.view(B, H, W, cp).float().cpu().numpy()
    assert not np.isnan(gr).any(), _where(np.isnan(gr))
    d = xh - x
    g_ref = R.bf16_round(((gscale * d) * xh) * (np.float32(1.0) - xh))
    assert d.dtype == np.float32 and g_ref.dtype == np.float32
    got = gr[..., :c].transpose(0, 3, 1, 2)
    assert np.array_equal(got, g_ref), _where(got != g_ref)
    assert not gr[..., c:].any()
    # 3. loss partials: [tile][lps] = (sum d^2, sum g of band 0 .. C-1, zero padding)
    parts = lp.view(nt, lps).cpu().numpy()
    assert not np.isnan(parts).any()
    total = parts.astype(np.float64).sum(0)
    d2 = (xh.astype(np.float64) - x.astype(np.float64)) ** 2
    e0 = abs(total[0] - d2.sum())
    assert e0 <= _summation_bound(d2.size, nt, d2).sum(), (e0, d2.sum())
    g64 = g_ref.astype(np.float64)
    eg = np.abs(total[1:1 + c] - g64.sum((0, 2, 3)))
    assert np.all(eg <= _summation_bound(B * H * W, nt, g64).sum((0, 2, 3))), eg
    assert not parts[:, 1 + c:].any()
