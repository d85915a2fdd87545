"""tests/conv_ref.py pinned (CPU): the three fp64 references against torch in float64, the exactness budget of every row of the
case tables, and the premise of the bit-exact GPU tests shown on the CPU -- an fp32 accumulation in a shuffled order equals the fp64
result bit for bit.  Likewise tests/edge_ref.py for the two C-band edge layers: every row of its tables built and held to its budget,
its launch prediction, its references against oracle/ae_numpy.py, and the bound on x_hat."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
import edge_ref as E

MAPS = [(2, 5, 7, 8, 8), (3, 4, 6, 6, 14), (1, 3, 5, 12, 4)]          # (N, Cin, Cout, H, W) of the conv's input: square and rectangular


@pytest.mark.parametrize("n,ci,co,h,w", MAPS)
def test_references_match_torch_float64(n, ci, co, h, w):
    rng = np.random.default_rng(n * 100 + h)
    x = rng.standard_normal((n, ci, h, w))
    wc = rng.standard_normal((co, ci, 3, 3))
    xt, wt = torch.from_numpy(x), torch.from_numpy(wc).requires_grad_()
    y = F.conv2d(xt, wt, stride=2, padding=1)
    np.testing.assert_allclose(R.conv_s2(x, wc), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    dy = rng.standard_normal(tuple(y.shape))
    y.backward(torch.from_numpy(dy))
    np.testing.assert_allclose(R.wgrad_s2(dy, x), wt.grad.numpy(), rtol=1e-12, atol=1e-12)
    # transposed conv x [N,Ci,H,W] -> [N,Co,2H,2W]; its weight gradient has the small map = its input, the big map = dOut
    wd = rng.standard_normal((ci, co, 3, 3))
    wdt = torch.from_numpy(wd).requires_grad_()
    z = F.conv_transpose2d(xt, wdt, stride=2, padding=1, output_padding=1)
    assert tuple(z.shape) == (n, co, 2 * h, 2 * w)
    np.testing.assert_allclose(R.deconv_s2(x, wd), z.detach().numpy(), rtol=1e-12, atol=1e-12)
    dz = rng.standard_normal(tuple(z.shape))
    z.backward(torch.from_numpy(dz))
    np.testing.assert_allclose(R.wgrad_s2(x, dz), wdt.grad.numpy(), rtol=1e-12, atol=1e-12)


def test_absolute_twins_bound_the_sums():
    rng = np.random.default_rng(1)
    x, w = rng.standard_normal((2, 3, 8, 12)), rng.standard_normal((5, 3, 3, 3))
    assert np.all(np.abs(R.conv_s2(x, w)) <= R.conv_s2_abs(x, w) + 1e-12)
    wd = rng.standard_normal((3, 5, 3, 3))
    assert np.all(np.abs(R.deconv_s2(x, wd)) <= R.deconv_s2_abs(x, wd) + 1e-12)
    big = rng.standard_normal((2, 4, 16, 24))
    assert np.all(np.abs(R.wgrad_s2(x, big)) <= R.wgrad_s2_abs(x, big) + 1e-12)


def test_tables_are_the_products_the_kernels_instantiate():
    assert len(R.IGEMM_INSTANCES) == 14 and len(set(R.IGEMM_INSTANCES)) == 14
    assert len(R.IGEMM_EXACT_CASES) == 84
    assert len(R.WGRAD_INSTANCES) == 13 and len(set(R.WGRAD_INSTANCES)) == 13
    assert len(R.WGRAD_EXACT_CASES) == 13 * 6 + 5 and len(set(R.WGRAD_EXACT_CASES)) == 13 * 6 + 5


def test_weight_gradient_rows_reach_the_multi_tile_loop_on_every_geometry(monkeypatch):
    """With the launcher's default of 64 workgroups most rows give every workgroup ONE tile.  The rows named in WGRAD_MULTI_TILE
    are the ones whose workgroups loop over several tiles, one per tile geometry."""
    monkeypatch.delenv("EAE_WGRAD_WGS", raising=False)
    nsc = 6 * 1024 * 1024
    launch = {c: R.expected_wgrad_launch(c[0], c[1], c[2], c[4], c[5], c[6], nsc) for c in R.WGRAD_EXACT_CASES}
    assert set(R.WGRAD_MULTI_TILE) == {(16, 8, 1), (8, 8, 2), (4, 4, 8)}
    for geo, (case, tiles, slices, per) in R.WGRAD_MULTI_TILE.items():
        assert case in launch and launch[case] == (geo, tiles, slices, per) and per > 1 and slices > 1
    assert launch[(128, 64, 1, 2, 16, 32, 5)] == ((16, 8, 1), 20, 10, 2)
    assert launch[(64, 32, 1, 2, 16, 32, 3)] == ((16, 8, 1), 12, 12, 1)       # 64 slices to give: one tile per workgroup
    # a single slice writes the result itself (no reduction launch), several slices go through the scratch: both occur
    assert {1} < {l[2] for l in launch.values()}


def test_budget_of_every_row():
    """By construction, not by measurement: S <= terms * max |operand| * max |weight| (+ max |bias|)."""
    for case in R.IGEMM_EXACT_CASES:
        R.assert_budget(R.igemm_budget_bound(*case), R.Q_CONV)
    for case in R.WGRAD_EXACT_CASES:
        R.assert_budget(R.wgrad_budget_bound(*case), R.Q_WGRAD)
    with pytest.raises(AssertionError):
        R.assert_budget(2.0 ** 17, R.Q_CONV)


@pytest.mark.parametrize("mode", [0, 1, 2, 4])
def test_dyadic_sources_are_exact_in_bf16_and_differ_per_channel(mode):
    rng = np.random.default_rng(mode)
    s = R.DyadicSrc(mode, (2, 64, 4, 8), rng)
    v32 = s.value.astype(np.float32)
    assert np.array_equal(R.bf16_round(v32), v32) and np.array_equal(v32.astype(np.float64), s.value)
    for t in s.tensors:
        assert np.array_equal(R.bf16_round(t), t)
    if s.coef is not None:
        assert all(len(np.unique(row)) > 1 for row in s.coef[:2])
    # the fp32 arithmetic of the load, with and without contraction of the multiply-add, gives the same value
    if mode == 1:
        y, (sc, t) = s.tensors[0], (s.coef[0][None, :, None, None], s.coef[1][None, :, None, None])
        assert np.array_equal(np.maximum((y * sc).astype(np.float32) + t, np.float32(0)).astype(np.float64), s.value)


def test_mask_decision_lands_on_zero():
    p = R.DyadicPrev((2, 64, 8, 8), np.random.default_rng(3))
    assert p.zeros > 0.02 * p.yprev.size
    assert np.array_equal(p.xhat * 8, np.round(p.xhat * 8)) and np.abs(p.xhat).max() <= 4.0


def _f32_shuffled_conv(kind, x, w, rng):
    """fp32 accumulation, channels permuted and taps in a random order"""
    perm = rng.permutation(x.shape[1])
    x32 = np.ascontiguousarray(x[:, perm]).astype(np.float32)
    n, ci, h, wd = x32.shape
    if kind == 0:
        w32 = np.ascontiguousarray(w[:, perm]).astype(np.float32)
        ho, wo = h // 2, wd // 2
        xp = np.zeros((n, ci, h + 2, wd + 2), np.float32)
        xp[:, :, 1:h + 1, 1:wd + 1] = x32
        y = np.zeros((n, w.shape[0], ho, wo), np.float32)
        for tap in rng.permutation(9):
            ky, kx = divmod(int(tap), 3)
            y += np.einsum("nchw,oc->nohw", xp[:, :, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2], w32[:, :, ky, kx], optimize=True)
        return y
    w32 = np.ascontiguousarray(w[perm]).astype(np.float32)
    yp = np.zeros((n, w.shape[1], 2 * h + 2, 2 * wd + 2), np.float32)
    for tap in rng.permutation(9):
        ky, kx = divmod(int(tap), 3)
        yp[:, :, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] += np.einsum("nchw,co->nohw", x32, w32[:, :, ky, kx], optimize=True)
    return yp[:, :, 1:2 * h + 1, 1:2 * wd + 1]


def test_fp32_accumulation_in_any_order_is_exact_for_the_largest_conv_row():
    """The largest-K row of the conv table: transposed 256 -> 128 with the widest operand (mode 2) on the 16x32 grid."""
    kind, cin, cout, smode, epi, hp, wp, B = max(R.IGEMM_EXACT_CASES, key=lambda c: (c[1] * R.VMAX[c[3]], c[5] * c[6]))
    assert (kind, cin, smode, hp, wp) == (1, 256, 2, 16, 32)
    rng = np.random.default_rng(11)
    src = R.DyadicSrc(smode, (B, cin, hp, wp), rng)
    w = R.dyadic_weights((cin, cout, 3, 3), rng)
    S = R.deconv_s2_abs(src.value, w)
    R.assert_budget(S, R.Q_CONV)
    ref = R.deconv_s2(src.value, w)
    got = _f32_shuffled_conv(kind, src.value, w, rng)
    assert got.dtype == np.float32 and np.array_equal(got, R.exact_f32(ref))
    # the epilogue's rounding is exercised: a good share of the sums is not a bf16 value
    r32 = ref.astype(np.float32)
    assert (R.bf16_round(r32) != r32).mean() > 0.2


def test_fp32_accumulation_in_any_order_is_exact_for_conv_128_256():
    rng = np.random.default_rng(12)
    src = R.DyadicSrc(2, (1, 128, 32, 64), rng)
    w = R.dyadic_weights((256, 128, 3, 3), rng)
    R.assert_budget(R.conv_s2_abs(src.value, w), R.Q_CONV)
    assert np.array_equal(_f32_shuffled_conv(0, src.value, w, rng), R.exact_f32(R.conv_s2(src.value, w)))


def test_fp32_accumulation_in_any_order_is_exact_for_the_largest_wgrad_row():
    """The largest-K row of the weight-gradient table (K = positions summed over): 128 x 64 on 5 maps of 16 x 32."""
    cs, cb, smode, bmode, hs, ws, B = max(R.WGRAD_EXACT_CASES, key=lambda c: c[4] * c[5] * c[6])
    assert (cs, cb, B * hs * ws) == (128, 64, 2560)
    rng = np.random.default_rng(13)
    small, big = R.DyadicSrc(smode, (B, cs, hs, ws), rng), R.DyadicSrc(bmode, (B, cb, 2 * hs, 2 * ws), rng)
    R.assert_budget(R.wgrad_s2_abs(small.value, big.value), R.Q_WGRAD)
    ref = R.wgrad_s2(small.value, big.value)
    # fp32, positions in a shuffled order
    bp = np.zeros((B, cb, 2 * hs + 2, 2 * ws + 2), np.float32)
    bp[:, :, 1:-1, 1:-1] = big.value
    perm = rng.permutation(B * hs * ws)
    s2 = small.value.astype(np.float32).transpose(1, 0, 2, 3).reshape(cs, -1)[:, perm]
    got = np.zeros((cs, cb, 3, 3), np.float32)
    for ky in range(3):
        for kx in range(3):
            b2 = bp[:, :, ky:ky + 2 * hs:2, kx:kx + 2 * ws:2].transpose(1, 0, 2, 3).reshape(cb, -1)[:, perm]
            got[:, :, ky, kx] = np.ascontiguousarray(s2) @ np.ascontiguousarray(b2).T
    assert np.array_equal(got, R.exact_f32(ref))


# ---------------------------------------------------------------------------------------------------- the edge layers (edge_ref.py)
def test_edge_tables_are_the_products_the_kernels_instantiate():
    assert E.EDGE_BANDS == [1, 3, 5, 8, 9, 13, 16]
    assert [E.edge_cp(c) for c in E.EDGE_BANDS] == [8, 4, 8, 8, 16, 16, 16]
    assert [E.edge_nkc(c) for c in E.EDGE_BANDS] == [1, 1, 2, 3, 3, 4, 5]
    assert all(h % 8 == 0 and w % 64 == 0 for h, w, b in E.EDGE_GRIDS) and len(E.EDGE_GRIDS) == 6
    assert [(h // 8, w // 64, b) for h, w, b in E.EDGE_GRIDS] == [(1, 1, 1), (1, 1, 3), (2, 2, 1), (1, 3, 2), (3, 1, 2), (3, 3, 1)]
    assert len(set(E.EDGE_CONV_INSTANCES)) == 4 and len(set(E.EDGE_WGRAD_INSTANCES)) == 3 and len(set(E.DECONV4_INSTANCES)) == 2
    assert len(set(E.EDGE_CONV_CASES)) == 4 * 7 * 6 and len(set(E.DECONV4_CASES)) == 2 * 7 * 6
    assert len(set(E.EDGE_WGRAD_CASES)) == 3 * 7 * 6 + len(E.EDGE_WGRAD_MULTI_TILE)
    assert any(case[2] == 16 for case in E.EDGE_WGRAD_MULTI_TILE)             # five k chunks inside the tile loop


def test_edge_budget_of_every_row():
    """By construction: S <= terms * max |operand| * max |weight| (+ max |bias|); the 520-image rows are the tight ones."""
    for case in E.EDGE_CONV_CASES:
        R.assert_budget(*E.edge_conv_budget(*case))
    for case in E.DECONV4_CASES:
        R.assert_budget(*E.deconv4_budget(*case))
    for case in E.EDGE_WGRAD_CASES:
        R.assert_budget(*E.edge_wgrad_budget(*case))
    S, q = E.edge_wgrad_budget(0, 2, 3, 8, 64, 520)
    assert 2.0 ** 22 < S * 2.0 ** q < 2.0 ** 23                                   # 66560 positions x 3.5 x 2^5 = 7.5 M
    with pytest.raises(AssertionError):
        R.assert_budget(*E.edge_wgrad_budget(0, 2, 3, 8, 64, 1200))


def test_edge_wgrad_launch_prediction(monkeypatch):
    monkeypatch.delenv("EAE_EDGE_WGRAD_BLOCKS", raising=False)
    monkeypatch.delenv("EAE_EDGE_WGRAD_SIDE_BLOCKS", raising=False)
    for case, want in E.EDGE_WGRAD_MULTI_TILE.items():
        kind, smode, c, h, w, b, slices = case
        got = E.expected_edge_wgrad_launch(kind, c, h, w, b, E.edge_wgrad_scratch_floats(case))
        assert got == want and got[2] > 1, (case, got)
        tiles, blocks, per = got
        assert (blocks - 1) * per < tiles <= blocks * per
    # the last workgroup of the rows that are meant to have a short one
    assert 520 - 173 * 3 == 1 and 9 - 5 == 4
    # every grid row: one tile per workgroup
    for case in E.EDGE_WGRAD_GRID_CASES:
        kind, smode, c, h, w, b, slices = case
        tiles, blocks, per = E.expected_edge_wgrad_launch(kind, c, h, w, b, E.edge_wgrad_scratch_floats(case))
        assert tiles == E.edge_tiles(h, w, b) == blocks and per == 1
    # the benchmark's batch: 4096 tiles, 8 per workgroup on the main launch and 16 on the side launch
    assert E.expected_edge_wgrad_launch(0, 3, 64, 64, 512, 1 << 30) == (4096, 512, 8)
    assert E.expected_edge_wgrad_launch(1, 3, 64, 64, 512, 1 << 30) == (4096, 256, 16)
    # the two variables, each for its own source kind
    monkeypatch.setenv("EAE_EDGE_WGRAD_BLOCKS", "100")
    assert E.expected_edge_wgrad_launch(0, 3, 8, 64, 520, 1 << 30) == (520, 87, 6)
    assert E.expected_edge_wgrad_launch(1, 3, 8, 64, 520, 1 << 30) == (520, 174, 3)
    monkeypatch.setenv("EAE_EDGE_WGRAD_SIDE_BLOCKS", "1024")
    assert E.expected_edge_wgrad_launch(1, 3, 8, 64, 520, 1 << 30) == (520, 520, 1)


def _exact_within(k, bound, q):
    """the row's measured sums of magnitudes are under the bound promised by construction, that bound is within the fp32 budget, and
    the fp64 reference converts to fp32 without loss"""
    assert k.S.max() <= bound
    R.assert_budget(bound, q)
    R.assert_budget(k.S, q)
    assert np.all(np.abs(k.exact) <= k.S)
    return R.exact_f32(k.exact)


def test_every_edge_conv_row_is_exact_in_fp32():
    rounded = 0.0
    for case in E.EDGE_CONV_CASES:
        k = E.edge_conv_case(*case)
        y = _exact_within(k, *E.edge_conv_budget(*case))
        assert np.array_equal(k.x.value * 4, np.round(k.x.value * 4)) and np.abs(k.x.value).max() <= 1.0
        assert np.array_equal(R.bf16_round(k.x.tensors[0]), k.x.tensors[0])      # the fp32 image survives conv1's rounding on load
        assert np.array_equal(y * 128, np.round(y * 128))
        assert (k.bias is not None) == (case[1] == 0) and (k.prev is not None) == (case[1] == 1)
        if case[2] >= 3:
            rounded = max(rounded, float((R.bf16_round(y) != y).mean()))
        # the NHWC-CP form of the operand: bands >= C are zero
        c = case[2]
        p = E.to_nhwcp(k.x.tensors[0], c)
        assert p.shape[3] == E.edge_cp(c) and not p[..., c:].any() and np.array_equal(p[..., :c].transpose(0, 3, 1, 2), k.x.tensors[0])
    assert rounded > 0.2                                          # the epilogue's rounding is exercised


def test_every_edge_wgrad_row_is_exact_in_fp32():
    """Measured on the operands, not assumed: the 520-image rows sum 66560 positions."""
    for case in E.EDGE_WGRAD_CASES:
        k = E.edge_wgrad_case(*case)
        dw = _exact_within(k, *E.edge_wgrad_budget(*case))
        assert dw.shape == (32, case[2], 3, 3) and np.array_equal(dw * 32, np.round(dw * 32))
        assert k.side.mode == case[1]


def test_every_deconv4_row_is_exact_in_fp32():
    lo = hi = 0.0
    for case in E.DECONV4_CASES:
        k = E.deconv4_case(*case)
        s = _exact_within(k, *E.deconv4_budget(*case))
        assert np.array_equal(s * 128, np.round(s * 128))
        assert k.target.dtype == np.float32 and 0.0 <= k.target.min() and k.target.max() < 1.0
        assert np.log2(float(k.gscale)) % 1 == 0
        assert (np.abs(s) < 0.5).any()
        lo, hi = min(lo, float(s.min())), max(hi, float(s.max()))
    assert lo < -4.0 and hi > 4.0                                 # the sigmoid's slope and both of its shoulders


def test_edge_references_match_the_oracle():
    """One random non-dyadic case per kernel against oracle/ae_numpy.py.  Its backward functions accumulate in the dtype of the
    arrays they are given: fp64 operands give fp64 round-off.  Its forward functions accumulate the nine taps in an fp32 array
    whatever they are given: they agree to that array's own rounding, ten fp32 roundings of magnitude <= the sum of |terms|."""
    from oracle import ae_numpy as O
    rng = np.random.default_rng(77)
    c, b, h, w = 5, 2, 8, 12
    x = rng.standard_normal((b, c, h, w)).astype(np.float32).astype(np.float64)           # fp32 values: the oracle pads in fp32
    dy = rng.standard_normal((b, 32, h // 2, w // 2)).astype(np.float32).astype(np.float64)
    wc = rng.standard_normal((32, c, 3, 3))
    bias = rng.standard_normal(32)
    # conv1's weight gradient: conv_s2_bwd's dw
    _, dw, _ = O.conv_s2_bwd(x, np.zeros_like(wc), dy)
    np.testing.assert_allclose(R.wgrad_s2(dy, x), dw, rtol=1e-12, atol=1e-12)
    # deconv4's weight gradient ([32][C]: the small map is its input) and its backward-data (a conv of the gradient): deconv_s2_bwd
    dx, dwd, _ = O.deconv_s2_bwd(dy, wc, x)
    np.testing.assert_allclose(R.wgrad_s2(dy, x), dwd, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(R.conv_s2(x, wc), dx, rtol=1e-12, atol=1e-12)
    # conv1 forward
    y = O.conv_s2_fwd(x, wc, bias)
    tol = 10 * 2.0 ** -24 * (R.conv_s2_abs(x, wc) + np.abs(bias)[None, :, None, None])
    assert y.dtype == np.float32 and np.all(np.abs(R.conv_s2(x, wc) + bias[None, :, None, None] - y) <= tol)
    # deconv4 forward
    bc = rng.standard_normal(c)
    s = O.deconv_s2_fwd(dy, wc, bc)
    tol = 10 * 2.0 ** -24 * (R.deconv_s2_abs(dy, wc) + np.abs(bc)[None, :, None, None])
    assert s.dtype == np.float32 and np.all(np.abs(R.deconv_s2(dy, wc) + bc[None, :, None, None] - s) <= tol)


def test_sigmoid_bound_is_four_orders_below_the_old_tolerance_and_holds_for_an_fp32_evaluation():
    s = np.arange(-120 * 128, 120 * 128 + 1) / 128.0
    sig, bound = E.sigmoid_bound(s)
    assert 1.5 * 2.0 ** -24 <= bound.min() and bound.max() < 2.2 * 2.0 ** -24 < 2e-7       # the old tolerance was 1e-3 at the least
    # an fp32 evaluation with correctly rounded exp (numpy) is inside the bound everywhere
    s32 = s.astype(np.float32)
    with np.errstate(over="ignore"):
        xh = np.float32(1.0) / (np.float32(1.0) + np.exp(-s32))
    assert xh.dtype == np.float32 and np.all(np.abs(xh.astype(np.float64) - sig) <= bound)
    # and a relative error of exp of 2^-18 (a wrong constant, a half-precision path) is outside it
    bad = 1.0 / (1.0 + np.exp(-s) * (1 + 2.0 ** -18))
    assert np.any(np.abs(bad - sig) > bound)


def test_structured_errors_change_the_expected_bits():
    """Structured errors show in the expected bits: one 8-channel group missing from one tap of a 128-channel layer changes most
    outputs, and a tile whose halo column is zero padding where it should be the neighbour's pixel (two tiles across) changes the
    first output column of the second tile and nothing else."""
    rng = np.random.default_rng(14)
    src = R.DyadicSrc(2, (1, 128, 16, 64), rng)                       # output 8 x 32: two 16-wide tiles
    w = R.dyadic_weights((256, 128, 3, 3), rng)
    ref = R.bf16_round(R.exact_f32(R.conv_s2(src.value, w)))
    w_missing = w.copy()
    w_missing[:, 8:16, 1, 1] = 0
    bad = R.bf16_round(R.exact_f32(R.conv_s2(src.value, w_missing)))
    assert (bad != ref).mean() > 0.5
    halves = np.concatenate([R.conv_s2(src.value[..., :32], w), R.conv_s2(src.value[..., 32:], w)], axis=3)
    diff = R.bf16_round(R.exact_f32(halves)) != ref
    assert not diff[..., :16].any() and not diff[..., 17:].any() and diff[..., 16].mean() > 0.5


# ---------------------------------------------------------------------------------------------------- the fp8 twins (conv_ref.py)
def test_fp8_tables_cover_every_instantiation_setting_and_the_multi_tile_loop(monkeypatch):
    wide = [(8, 16), (16, 32), (8, 32), (24, 16)]
    assert len(R.IGEMM8_EXACT_CASES) == 14 * 4 and len(set(R.IGEMM8_EXACT_CASES)) == 56
    assert {c[:5] for c in R.IGEMM8_EXACT_CASES} == set(R.IGEMM_INSTANCES)
    assert all([c[5:7] for c in R.IGEMM8_EXACT_CASES if c[:5] == inst] == wide for inst in R.IGEMM_INSTANCES)
    assert [g[:2] for g in R.GRIDS[2:]] == wide and [g[:2] for g in R.WGRAD_GRIDS[2:]] == wide
    assert all(R.expected_geo(*c[:3], c[5], c[6], c[7]) == R.WIDE for c in R.IGEMM8_EXACT_CASES)
    assert len(R.WGRAD8_EXACT_CASES) == 13 * 4 + 4 and len(set(R.WGRAD8_EXACT_CASES)) == 56
    assert {c[:4] for c in R.WGRAD8_EXACT_CASES} == set(R.WGRAD_INSTANCES)
    assert all([c[4:6] for c in R.WGRAD8_EXACT_CASES[:52] if c[:4] == inst] == wide for inst in R.WGRAD_INSTANCES)
    assert set(R.WGRAD8_EXACT_CASES[52:]) < set(R.WGRAD_EXACT_CASES) | {(256, 128, 4, 1, 16, 32, 3)}
    # several tiles per workgroup, one row of them with SRC_RAWG (the form the train step launches)
    monkeypatch.delenv("EAE_WGRAD_WGS", raising=False)
    for case, (tiles, slices, per) in R.WGRAD8_MULTI_TILE.items():
        assert case in R.WGRAD8_EXACT_CASES
        assert R.expected_wgrad_launch(case[0], case[1], case[2], case[4], case[5], case[6], 6 << 20) == (R.WIDE, tiles, slices, per)
        assert per > 1 and slices > 1
    assert any(c[2] == 4 or c[3] == 4 for c in R.WGRAD8_MULTI_TILE)
    # both edge kinds for every instantiation (so for every format, and for both kernels); the weight scales rotate
    for i, c in enumerate(R.IGEMM8_EXACT_CASES):
        assert R.igemm8_scales(i, "regular", R.fp8_fmt(c[3])) == ({"e4m3": 16.0, "e5m2": 4096.0}[R.fp8_fmt(c[3])], 16.0)
    got = {(c[:5], R.edge_kind(i)) for i, c in enumerate(R.IGEMM8_EXACT_CASES)}
    assert got == {(inst, k) for inst in R.IGEMM_INSTANCES for k in ("saturating", "flushing")}
    assert {(R.fp8_fmt(c[3]), R.igemm8_scales(i, "edge", R.fp8_fmt(c[3]))[0]) for i, c in enumerate(R.IGEMM8_EXACT_CASES)} == {
        ("e4m3", 2.0 ** 8), ("e4m3", 2.0 ** -7), ("e5m2", 2.0 ** 15), ("e5m2", 2.0 ** -15)}
    assert {R.igemm8_scales(i, "edge", "e4m3")[1] for i in range(56)} == {0.25, 1.0, 16.0, 256.0}
    # the weight gradient: per instantiation the edge scale once on each operand, saturating and flushing
    got = set()
    for i, c in enumerate(R.WGRAD8_EXACT_CASES[:52]):
        fs, fb = R.fp8_fmt(c[2]), R.fp8_fmt(c[3])
        s_s, s_b, on = R.wgrad8_scales(i, "edge", fs, fb)
        assert R.wgrad8_scales(i, "regular", fs, fb) == (R.REGULAR_SCALE[fs], R.REGULAR_SCALE[fb], None)
        table = R.SATURATING_SCALE if R.edge_kind(i) == "saturating" else R.FLUSHING_SCALE
        assert (s_s, s_b) == ((table[fs], R.REGULAR_SCALE[fb]) if on == "small" else (R.REGULAR_SCALE[fs], table[fb]))
        got.add((c[:4], on, R.edge_kind(i)))
    assert got == {(inst, on, k) for inst in R.WGRAD_INSTANCES for on in ("small", "big") for k in ("saturating", "flushing")}


def _fp8_operand_scales():
    """every (mode, format, scale) the two tables use"""
    out = set()
    for setting in R.FP8_SETTINGS:
        for i, c in enumerate(R.IGEMM8_EXACT_CASES):
            out.add((c[3], R.fp8_fmt(c[3]), R.igemm8_scales(i, setting, R.fp8_fmt(c[3]))[0]))
        for i, c in enumerate(R.WGRAD8_EXACT_CASES):
            s_s, s_b, _ = R.wgrad8_scales(i, setting, R.fp8_fmt(c[2]), R.fp8_fmt(c[3]))
            out |= {(c[2], R.fp8_fmt(c[2]), s_s), (c[3], R.fp8_fmt(c[3]), s_b)}
    return sorted(out)


def test_fine_sources_stay_on_the_grid_and_are_really_rounded():
    """The conditions on the INPUTS, from the oracle alone: stored tensors bf16-exact, the operand a multiple of 1/8 within 3.5
    before and after the conversion at every scale the tables use; at scale 1 and at the regular scales at least 5 % of an operand
    is changed by the conversion, exact ties among them; the saturating scales clamp and the flushing scales flush a real share."""
    from oracle import ae_numpy as O
    used = _fp8_operand_scales()
    assert {(m, f) for m, f, _ in used} == {(0, "e4m3"), (1, "e4m3"), (2, "e5m2"), (4, "e5m2")}
    assert len(used) == 12                                                  # regular, saturating, flushing for each
    for mode, fmt in sorted({(m, f) for m, f, _ in used}):
        s = R.FineSrc(mode, (2, 64, 16, 32), np.random.default_rng(50 + mode))
        v32 = s.value.astype(np.float32)
        assert np.array_equal(R.bf16_round(v32), v32) and np.array_equal(v32.astype(np.float64), s.value)
        assert np.array_equal(s.value * 8, np.round(s.value * 8)) and np.abs(s.value).max() == 3.5
        for t in s.tensors:
            assert np.array_equal(R.bf16_round(t), t)
        if s.coef is not None:
            assert all(len(np.unique(row)) > 1 for row in s.coef[:2])
        if mode == 1:      # the fp32 arithmetic of the load without contraction gives the same value
            y, (sc, t) = s.tensors[0], (s.coef[0][None, :, None, None], s.coef[1][None, :, None, None])
            assert np.array_equal(np.maximum((y * sc).astype(np.float32) + t, np.float32(0)).astype(np.float64), s.value)
        for scale in [1.0] + [sc for m, f, sc in used if (m, f) == (mode, fmt)]:
            q = R.quantised(s, scale, fmt)                                  # asserts the grid
            assert np.array_equal(R.fp8_round_variant(s.value * scale, fmt) / scale, q)         # the variant's true setting IS the oracle
            sh = R.rounding_shares(s.value, scale, fmt)
            assert sh["changed"] == float((q != s.value).mean())
            if scale in (1.0, R.REGULAR_SCALE[fmt]):
                assert sh["changed"] >= 0.05 and sh["ties"] > 0 and sh["saturated"] == 0 and sh["flushed"] == 0, (mode, scale, sh)
            elif scale == R.SATURATING_SCALE[fmt]:
                assert sh["saturated"] >= 0.05 and np.abs(q).max() == 1.75 == R.FP8_MAX[fmt] / scale, (mode, scale, sh)
            else:
                assert scale == R.FLUSHING_SCALE[fmt] and sh["flushed"] >= 0.01 and sh["ties"] > 0, (mode, scale, sh)
                # subnormal results are in the operand: nonzero values below the smallest normal number
                assert ((q != 0) & (np.abs(q) * scale < (2.0 ** -6 if fmt == "e4m3" else 2.0 ** -14))).any()
    # the documented exception: e5m2 at 2^-16 rounds 3.5 UP to 4 (why S comes from the quantised operand, not from 3.5)
    assert O._q8(np.float32(3.5), 2.0 ** -16, "e5m2") == 4.0
    # the weights are e4m3 values at 2^-3 .. 2^8 and not at 2^9
    w = R.dyadic_weights((64, 32, 3, 3), np.random.default_rng(5))
    for e in range(-3, 9):
        assert np.array_equal(O.fp8_round(w * np.float32(2.0 ** e), "e4m3"), w * np.float32(2.0 ** e))
    assert not np.array_equal(O.fp8_round(w * np.float32(512), "e4m3"), w * np.float32(512))


def _edge_presence(value, q, scale, fmt, kind):
    """the quantised operand of an edge case really holds clamped values, or flushed ones"""
    lim = R.FP8_MAX[fmt] / scale
    if kind == "saturating":
        return bool(((np.abs(value) > lim) & (np.abs(q) == lim)).any())
    return bool(((value != 0) & (q == 0)).any())


@pytest.mark.parametrize("setting", R.FP8_SETTINGS)
def test_every_igemm8_case_is_exact_in_fp32_and_its_edge_is_reached(setting):
    for idx in range(len(R.IGEMM8_EXACT_CASES)):
        k = R.Igemm8Case(idx, setting)
        R.assert_budget(k.S, R.Q_CONV)
        assert np.all(np.abs(k.exact) <= k.S)
        y = R.exact_f32(k.exact)
        assert np.array_equal(y * 128, np.round(y * 128))
        assert k.w_bytes.shape == (k.case[2], 9, k.case[1]) and k.w_bytes.dtype == np.uint8
        if setting == "regular":
            assert k.shares["changed"] >= 0.05 and k.shares["ties"] > 0, (k.case, k.shares)
        else:
            assert _edge_presence(k.src.value, k.qa, k.s_pix, k.fmt, R.edge_kind(idx)), (k.case, k.shares)
            if R.edge_kind(idx) == "saturating":
                assert k.amax > R.FP8_MAX[k.fmt] / k.s_pix and k.shares["saturated"] > 0.05      # the reported maximum is the unclamped one
            else:
                assert k.shares["flushed"] > 0.01


@pytest.mark.parametrize("setting", R.FP8_SETTINGS)
def test_every_wgrad8_case_is_exact_in_fp32_and_its_edge_is_reached(setting):
    for idx in range(len(R.WGRAD8_EXACT_CASES)):
        k = R.Wgrad8Case(idx, setting)
        R.assert_budget(k.S, R.Q_WGRAD)
        assert np.all(np.abs(k.exact) <= k.S)
        dw = R.exact_f32(k.exact)
        assert dw.shape == k.case[:2] + (3, 3) and np.array_equal(dw * 64, np.round(dw * 64))
        for sh in (k.shares_s, k.shares_b):
            if setting == "regular":
                assert sh["changed"] >= 0.05 and sh["ties"] > 0, (k.case, sh)
        if setting == "edge":
            src, q, sc, fmt = (k.small, k.qs, k.s_s, k.fmt_s) if k.edge_on == "small" else (k.big, k.qb, k.s_b, k.fmt_b)
            assert _edge_presence(src.value, q, sc, fmt, R.edge_kind(idx)), (k.case, k.edge_on)


def _halo_swapped(x, kind):
    """the operand as a kernel would see it that takes the halo column between the first two tiles across from the wrong side of the
    seam: the conv kind's second tile reads input column 31 (its left halo), here a copy of column 30; the transposed kind's first
    tile reads input column 16 (its right halo), here a copy of its own last column 15"""
    x = x.copy()
    if kind == 0:
        x[..., 31] = x[..., 30]
    else:
        x[..., 16] = x[..., 15]
    return x


IGEMM8_POWER_SAMPLE = [i for i, c in enumerate(R.IGEMM8_EXACT_CASES) if c[6] == 32 and c[1] <= 128]      # two tiles across


@pytest.mark.parametrize("idx", IGEMM8_POWER_SAMPLE)
def test_wrong_conv_kernels_would_change_the_expected_bits(idx):
    """The power of test_igemm8_exact, shown on its references (never by breaking a kernel): each of four wrong kernels gives a
    stored output that differs from the expected one in at least one element.  Ties exist at the regular and the flushing scales (at
    a saturating scale the unclamped range has none on the 1/8 grid: MAX / s = 1.75 and below it the fp8 step is <= 1/8), clamped
    values at the saturating ones; a dropped tap and a wrong halo column show under every setting."""
    hit = set()
    for setting in R.FP8_SETTINGS:
        k = R.Igemm8Case(idx, setting)
        kind, cin, cout = k.case[:3]
        ref = k.stored(k.exact)
        differs = lambda operand, w: bool((k.stored(k.sum_of(operand, w)) != ref).any())
        assert not differs(k.quant_variant("even", True), k.w)
        if setting == "regular" or R.edge_kind(idx) == "flushing":
            assert differs(k.quant_variant("away", True), k.w)
            hit.add("away")
        if setting == "edge" and R.edge_kind(idx) == "saturating":
            assert differs(k.quant_variant("even", False), k.w)
            hit.add("unclamped")
        w = k.w.copy()                                       # one tap of one input channel out of 9 * cin
        if kind == 0:
            w[:, cin // 2, 2, 0] = 0
        else:
            w[cin // 2, :, 2, 0] = 0
        assert differs(k.qa, w)
        # the seam between the first two tiles across: only the outputs of the tile that reads the column as its halo change
        bad = k.stored(k.sum_of(_halo_swapped(k.qa, kind), k.w))
        seam = slice(16, None) if kind == 0 else slice(None, 32)
        mixed = ref.copy()
        mixed[..., seam] = bad[..., seam]
        d = mixed != ref
        col = 16 if kind == 0 else 31
        assert d[..., col].any() and not np.delete(d, col, axis=3).any()
    assert {"away"} <= hit


WGRAD8_POWER_SAMPLE = [i for i, c in enumerate(R.WGRAD8_EXACT_CASES[:52]) if c[5] == 32 and c[0] <= 128]


@pytest.mark.parametrize("idx", WGRAD8_POWER_SAMPLE)
def test_wrong_wgrad_kernels_would_change_the_expected_bits(idx):
    for setting in R.FP8_SETTINGS:
        k = R.Wgrad8Case(idx, setting)
        ref = R.exact_f32(k.exact)
        differs = lambda s, b: bool((R.wgrad_s2(s, b) != ref).any())
        assert not differs(k.quant_variant("small", "even", True), k.quant_variant("big", "even", True))
        flushing_on = k.edge_on if setting == "edge" and R.edge_kind(idx) == "flushing" else None
        for which in ("small", "big"):
            wrong = k.quant_variant(which, "away", True)
            if setting == "regular" or flushing_on == which or k.edge_on != which:      # (an operand at a saturating scale has no ties)
                assert differs(wrong, k.qb) if which == "small" else differs(k.qs, wrong)
        if setting == "edge" and R.edge_kind(idx) == "saturating":
            wrong = k.quant_variant(k.edge_on, "even", False)
            assert differs(wrong, k.qb) if k.edge_on == "small" else differs(k.qs, wrong)
        s = k.qs.copy()                                      # one position of one image dropped from the sum
        s[0, :, 3, 17] = 0
        assert differs(s, k.qb)
        # the second tile across reads big column 31 as its left halo: taken from column 30, only the kx = 0 taps change
        left, right = k.qs.copy(), k.qs.copy()
        left[..., 16:] = 0
        right[..., :16] = 0
        bad = R.wgrad_s2(left, k.qb) + R.wgrad_s2(right, _halo_swapped(k.qb, 0))
        d = bad != ref
        assert d[..., 0].any() and not d[..., 1:].any()
