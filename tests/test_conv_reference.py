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
