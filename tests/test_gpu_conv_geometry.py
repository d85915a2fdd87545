"""Bit-exact tests of the stride-2 conv, transposed-conv and weight-gradient kernels on every tile geometry the plan can ask for.

Every instantiation of eae_conv_launch.hip / eae_wgrad_launch.hip runs on six position grids -- 4x4 and 8x8 (several images per
tile, a last tile with one valid image), one 16x8 tile per image, 2x2 tiles (real halos in both directions), two tiles across,
three tiles down (rectangular maps) -- on operands for which the fp32 accumulator is exact (tests/conv_ref.py): the output must be
bf16_round(exact sum + bias), the weight gradient the exact sum, compared with np.array_equal.  The launcher reads EAE_IG_SMALL and
EAE_IGEMM2 once per process, so the conv cases run again in one child process per setting (the last test).

What is asserted about the launch: for the conv kinds the tile count of the geometry a case names (nothing else is observable
through the C ABI: channel-block width and the choice of kernel are the plan's, read off csrc/eae_conv_plan.h); for the weight
gradient the number of position slices, seen in how much of a NaN-preset scratch the launch wrote, and with it the tiles each
workgroup loops over -- more than one on each of the three tile geometries (conv_ref.WGRAD_MULTI_TILE)."""
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
    """first differing elements, for the failure message: (image, channel, row, column)"""
    idx = np.argwhere(bad)
    return f"{len(idx)} of {bad.size} differ, first at (n, c, y, x) = {idx[:8].tolist()}"


@pytest.mark.parametrize("kind,cin,cout,smode,epi,hp,wp,B", R.IGEMM_EXACT_CASES)
def test_igemm_exact(lib, kind, cin, cout, smode, epi, hp, wp, B):
    import gpu_util as G
    from eae_amd._lib import check
    from test_gpu_ops_path import _pack
    rng = np.random.default_rng(31000 + 1000 * kind + 7 * cin + 100 * smode + 10 * epi + 3 * hp + wp)
    hin, win = (2 * hp, 2 * wp) if kind == 0 else (hp, wp)
    hout, wout = (hp, wp) if kind == 0 else (2 * hp, 2 * wp)
    # the geometry this case is meant to hit under this process's settings: a plan change fails here instead of emptying the case
    # (the tile count is all the library reports: 32- or 64-channel blocks of the transposed kind and the one-role or the
    #  wave-specialised kernel have the same count -- that the settings select them is read off csrc/eae_conv_plan.h, not asserted)
    nt = lib.eae_op_conv_s2_ntiles(kind, cin, B, hin, win)
    want = R.expected_ntiles(kind, cin, cout, hp, wp, B, R.ig_small_setting())
    assert nt == want, (nt, want, R.expected_geo(kind, cin, cout, hp, wp, B, R.ig_small_setting()))

    src = R.DyadicSrc(smode, (B, cin, hin, win), rng)
    if kind == 0:
        w = R.dyadic_weights((cout, cin, 3, 3), rng)
        buf, p1, p2 = _pack(lib, w)
        wpk, exact = p1, R.conv_s2(src.value, w)
    else:
        w = R.dyadic_weights((cin, cout, 3, 3), rng)
        buf, p1, p2 = _pack(lib, w)
        wpk, exact = p2, R.deconv_s2(src.value, w)
    R.assert_budget(R.igemm_budget_bound(kind, cin, cout, smode, epi, hp, wp, B), R.Q_CONV)
    bd = None
    if epi == 0:
        bias = R.dyadic_bias(cout, rng)
        bd = G.f32(bias)
        exact = exact + bias[None, :, None, None].astype(np.float64)
    ref = R.bf16_round(R.exact_f32(exact))
    prev = yprev_d = pcoef_d = None
    if epi == 1:
        prev = R.DyadicPrev((B, cout, hout, wout), rng)
        yprev_d, pcoef_d = G.to_nhwc_bf16(prev.yprev), G.f32(prev.coef)
        ref = ref * prev.mask                                  # a decision that lands on 0 gives 0

    sd, keep = _upload(src)
    out = torch.full((B, hout, wout, cout), float("nan"), dtype=torch.bfloat16, device=G.dev())
    flat = torch.full((2 * cout * nt + 64,), float("nan"), dtype=torch.float32, device=G.dev())
    part, guard = flat[:2 * cout * nt].view(2, cout, nt), flat[2 * cout * nt:]
    check(lib.eae_op_conv_s2(G.stream(), kind, sd, cin, cout, B, hin, win, G.ptr(wpk), G.ptr(bd), G.ptr(out),
                             G.ptr(part) if epi != 2 else None, epi, G.ptr(yprev_d), G.ptr(pcoef_d)))
    torch.cuda.synchronize()
    got = G.from_nhwc(out)
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    assert torch.isnan(guard).all()
    if epi == 2:
        assert torch.isnan(part).all()                         # the plain epilogue writes no partials
        return
    assert not torch.isnan(part).any()
    # partial totals against fp64 sums of the expected stored output: the kernels add bf16-exact values, or exact products of them,
    # in fp32 -- the plain summation bound, n terms inside the tiles and ntiles on top
    total = part.cpu().numpy().astype(np.float64).sum(2)
    r64 = ref.astype(np.float64)
    terms = [r64, r64 * r64] if epi == 0 else [r64, r64 * prev.xhat]
    n = B * hout * wout
    for col, t in enumerate(terms):
        want, mag = t.sum((0, 2, 3)), np.abs(t).sum((0, 2, 3))
        err = np.abs(total[col] - want)
        bound = (n + nt) * 2.0 ** -24 * mag
        print(f"partials column {col}: max err {err.max():.3e}, bound at that channel {bound[err.argmax()]:.3e}")
        assert np.all(err <= bound), (col, int(np.argmax(err - bound)), float(err.max()))


def _wgrad_exact(lib, cs, cb, smode, bmode, hs, ws, B, mult=1):
    """one weight-gradient launch (as one of `mult` members of a grouped step) on a NaN-preset scratch: dw bit for bit, and the
    launch conv_ref.expected_wgrad_launch says it is, which is returned"""
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(32000 + cs + 100 * smode + 10 * bmode + 3 * hs + ws + B)
    small = R.DyadicSrc(smode, (B, cs, hs, ws), rng)
    big = R.DyadicSrc(bmode, (B, cb, 2 * hs, 2 * ws), rng)
    R.assert_budget(R.wgrad_budget_bound(cs, cb, smode, bmode, hs, ws, B), R.Q_WGRAD)
    ref = R.exact_f32(R.wgrad_s2(small.value, big.value))
    ss, keep_s = _upload(small)
    bs, keep_b = _upload(big)
    scratch = torch.full((6 * 1024 * 1024,), float("nan"), dtype=torch.float32, device=G.dev())
    dw = torch.full((cs, cb, 3, 3), float("nan"), dtype=torch.float32, device=G.dev())
    check(lib.eae_set_geometry_mult(mult))
    try:
        check(lib.eae_op_wgrad_s2(G.stream(), ss, bs, cs, cb, B, hs, ws, G.ptr(scratch), scratch.numel(), G.ptr(dw)))
    finally:
        check(lib.eae_set_geometry_mult(1))
    torch.cuda.synchronize()
    got = dw.cpu().numpy()
    assert not np.isnan(got).any(), _where(np.isnan(got))
    assert np.array_equal(got, ref), _where(got != ref)
    # the launch this case is meant to be: several position slices leave one partial each at the head of the scratch (a single slice
    # writes dw itself), so the slice count shows there, and with the tile count of the geometry the tiles per workgroup follow
    geo, tiles, slices, per = R.expected_wgrad_launch(cs, cb, smode, hs, ws, B, scratch.numel(), mult)
    used = (slices if slices > 1 else 0) * cs * cb * 9
    assert not torch.isnan(scratch[:used]).any() and torch.isnan(scratch[used:]).all(), (geo, tiles, slices, per)
    return geo, tiles, slices, per


@pytest.mark.parametrize("cs,cb,smode,bmode,hs,ws,B", R.WGRAD_EXACT_CASES)
def test_wgrad_exact(lib, cs, cb, smode, bmode, hs, ws, B):
    geo, tiles, slices, per = _wgrad_exact(lib, cs, cb, smode, bmode, hs, ws, B)
    hit = R.WGRAD_MULTI_TILE.get(geo)
    if hit is not None and hit[0] == (cs, cb, smode, bmode, hs, ws, B) and "EAE_WGRAD_WGS" not in os.environ:
        assert (tiles, slices, per) == hit[1:] and per > 1


@pytest.mark.parametrize("mult,want", [(2, (12, 2, 6)), (8, (12, 1, 12))])
def test_wgrad_exact_as_a_member_of_a_grouped_step(lib, mult, want):
    """The members of a grouped step share the workgroup budget (eae_set_geometry_mult): the 16x8x1 multi-tile row, 4 slices of 3
    tiles alone, runs on 64 / 2 / 16 = 2 slices of 6, and with 8 members on the floor of 8 workgroups -- fewer than its 16 output
    blocks: one slice, which writes dw itself and leaves the whole scratch untouched.  The result stays the exact sum."""
    case = (256, 128, 2, 1, 16, 32, 3)
    assert R.WGRAD_MULTI_TILE[R.WIDE][0] == case
    geo, tiles, slices, per = _wgrad_exact(lib, *case, mult=mult)
    if "EAE_WGRAD_WGS" not in os.environ:
        assert geo == R.WIDE and (tiles, slices, per) == want


def test_exact_conv_cases_on_the_large_tiles_and_the_wave_specialised_kernel():
    """The default process gives the small tiles, the 32-channel blocks of the transposed kind and the wave-specialised kernel on
    transposed 256 -> 128 forward.  One child process per setting gives the large narrow tiles and the 64-channel blocks
    (EAE_IG_SMALL=0) with the wave-specialised kernel on every layer it exists for (EAE_IGEMM2=2) and on none (0)."""
    import subprocess
    import sys
    for mode in ("2", "0"):
        env = dict(os.environ, EAE_IGEMM2=mode, EAE_IG_SMALL="0")
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "igemm_exact",
                            "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"EAE_IGEMM2={mode}\n" + r.stdout[-3000:] + r.stderr[-2000:]
        assert f"{len(R.IGEMM_EXACT_CASES)} passed" in r.stdout, r.stdout[-1000:]
