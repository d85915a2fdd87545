"""The NumPy reference of the nodata / mask kernels (tests/nodata_ref.py), checked without a device: the cumulative-sum counts
against a triple-loop brute force, the fp32 blend against a float64 box mean and the worked example of scene_blend_kernel's comment,
and every case of tests/test_gpu_nodata_kernels.py against the conditions that make its comparison able to fail.  The conditions are
facts of the reference alone (plan, alignment arithmetic, planted pixels): no device output enters them."""
import numpy as np
import pytest

import nodata_ref as R


# ---------------------------------------------------------------------------------------------------------------- the reference itself
def _counts_brute(inv, p, s):
    h, w = inv.shape
    n_h, n_w = (h - p) // s + 1, (w - p) // s + 1
    out = np.zeros((n_h, n_w), dtype=np.int64)
    for i in range(n_h):
        for j in range(n_w):
            out[i, j] = inv[i * s:i * s + p, j * s:j * s + p].sum()
    return out


@pytest.mark.parametrize("h,w,p,s", [(8, 8, 8, 8), (9, 17, 8, 8), (16, 24, 8, 8), (19, 23, 8, 3), (21, 40, 8, 1), (13, 13, 5, 5),
                                     (14, 31, 5, 2), (30, 11, 7, 4), (64, 70, 64, 20), (33, 29, 16, 16), (35, 50, 16, 5), (12, 12, 4, 3)])
def test_rows_and_counts_match_brute_force(h, w, p, s):
    """S < P, S = P, and extents that P and S do not divide"""
    inv = np.random.default_rng(h * 100 + w).random((h, w)) < 0.3
    rows = R.rows_ref(inv, p, s)
    n_h, n_w = (h - p) // s + 1, (w - p) // s + 1
    assert rows.dtype == np.int64 and rows.shape == ((n_h - 1) * s + p, n_w)
    for j in range(n_w):
        assert np.array_equal(rows[:, j], inv[:rows.shape[0], j * s:j * s + p].sum(1))
    counts = R.counts_ref(rows, p, s)
    assert counts.dtype == np.int64 and np.array_equal(counts, _counts_brute(inv, p, s))
    assert 0 < counts.max() <= p * p


def test_invalid_ref_rules_and_negative_zero():
    x = np.array([[[0.0, -0.0, 1.0, np.nan]], [[0.0, 2.0, -0.0, np.nan]]], dtype=np.float32)
    assert R.invalid_ref(x, 0.0, "all", None).tolist() == [[True, False, False, False]]
    assert R.invalid_ref(x, 0.0, "any", None).tolist() == [[True, True, True, False]]
    assert R.invalid_ref(x, R.NAN, "all", None).tolist() == [[False, False, False, True]]
    assert R.invalid_ref(x, None, "all", np.array([[0, 0, 9, 0]], dtype=np.uint8)).tolist() == [[False, False, True, False]]
    ps, pm = R.pad_ref(np.arange(6, dtype=np.uint8).reshape(1, 2, 3), np.ones((2, 3), np.uint8), (1, 0, 0, 2), "constant", 7)
    assert ps[0].tolist() == [[7, 7, 7, 7, 7], [0, 1, 2, 7, 7], [3, 4, 5, 7, 7]] and pm.tolist() == [[0] * 5, [1, 1, 1, 0, 0], [1, 1, 1, 0, 0]]
    ps, pm = R.pad_ref(np.arange(6, dtype=np.uint8).reshape(1, 2, 3), np.ones((2, 3), np.uint8), (1, 0, 0, 2), "reflect", 0)
    assert ps[0].tolist() == [[3, 4, 5, 4, 3], [0, 1, 2, 1, 0], [3, 4, 5, 4, 3]] and pm.min() == 1


def test_select_ref():
    c = np.array([[3, 0, 5], [1, 4096, 0]])
    assert R.select_ref(c, 0).tolist() == [1, 5] and R.select_ref(c, -1).tolist() == [] and R.select_ref(c, 4096).tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("n_h,n_w,k", [(2, 2, 1), (4, 4, 2), (7, 8, 4)])        # the grids of test_blend_is_the_box_mean (K = 6)
def test_blend_ref_is_the_box_mean(n_h, n_w, k):
    p = R.blend_probs(6, n_h, n_w, seed=k)
    for name, lab in [("plain", None)] + list(R.blend_label_maps(n_h, n_w, seed=k).items()):
        cell, cl = R.blend_ref(p, lab, k)
        assert cell.dtype == np.float32 and cell.shape == (6, n_h + k - 1, n_w + k - 1) and cl.dtype == np.int64
        ref = np.zeros(cell.shape)
        cnt = np.zeros(cell.shape[1:])
        for i in range(n_h):
            for j in range(n_w):
                if lab is None or lab[i, j] >= 0:
                    ref[:, i:i + k, j:j + k] += p[:, i:i + 1, j:j + 1].astype(np.float64)
                    cnt[i:i + k, j:j + k] += 1
        has = cnt > 0
        ref[:, has] /= cnt[has]
        assert np.abs(cell - ref).max() <= 1e-6, name
        assert (cl[~has] == -1).all() and (cell[:, ~has] == 0).all()
        assert np.array_equal(cl[has], cell.argmax(0)[has])
        if name == "none":
            plain = R.blend_ref(p, None, k)
            assert np.array_equal(cell, plain[0]) and np.array_equal(cl, plain[1])
        if k == 1 and lab is None:
            assert np.array_equal(cell, p)


def test_blend_ref_worked_example():
    """the 2 x 2 example of scene_blend_kernel's comment (csrc/eae_scene.hip): dyadic values, so every figure is exact"""
    p0 = np.array([[0.5, 0.25], [0.75, 1.0]], dtype=np.float32)
    p = np.stack([p0, 1 - p0])
    cell, lab = R.blend_ref(p, None, 2)
    assert cell[:, 0, 0].tolist() == [0.5, 0.5] and lab[0, 0] == 0
    assert cell[:, 0, 1].tolist() == [0.375, 0.625] and lab[0, 1] == 1
    assert cell[:, 1, 1].tolist() == [0.625, 0.375] and lab[1, 1] == 0
    cell, lab = R.blend_ref(p, np.array([[0, -1], [0, 0]]), 2)
    assert cell[:, 0, 2].tolist() == [0.0, 0.0] and lab[0, 2] == -1
    assert cell[:, 0, 1].tolist() == [0.5, 0.5] and lab[0, 1] == 0
    assert cell[:, 1, 1].tolist() == [0.75, 0.25] and lab[1, 1] == 0


# ---------------------------------------------------------------------------------------------------------------- a. count cases
def _check_plan(case, wv):
    n_w, J, nchunk = R.plan(case["P"], case["S"], wv)
    ch = R.chunks(case["P"], case["S"], wv)
    assert (nchunk, ch[-1][1]) == (case["nchunk"], case["last"]) and len(ch) == nchunk
    assert sum(c[1] for c in ch) == n_w and all((c[1] - 1) * case["S"] + case["P"] + 15 <= R.INV_SPAN for c in ch)
    assert case["split"] == (case["H"] * case["W"] * R.SIZE[case["dt"]] % 16 != 0)
    return n_w, J, ch


def _fit_rows(case, ch, rowoffs):
    """the (row, chunk) pairs whose workgroup fills pre[] to its last element: m = 15 and a span of INV_SPAN - 15"""
    e = R.SIZE[case["dt"]]
    return [(y, c) for c, (j0, jn, x0, x1) in enumerate(ch) if x1 - x0 + 15 == R.INV_SPAN
            for y, ro in rowoffs if R.shift(case.get("off", 0) * e, e, ro, x0) == 15]


def _boundaries_differ(a, ch):
    """the values change across every chunk boundary (columns j0 - 1 and j0), in some row"""
    return all((a[:, j0 - 1] != a[:, j0]).any() for j0, _, _, _ in ch[1:])


@pytest.mark.parametrize("case", R.COUNT_CASES, ids=lambda c: c["id"])
def test_count_case_conditions(case):
    P, S, H, W = case["P"], case["S"], case["H"], case["W"]
    n_w, J, ch = _check_plan(case, W)
    assert (n_w, J) == (case["nW"], case["J"])
    assert H == P + 2 * S or case["id"] in ("u8c1-p4032", "u8c3-one")
    n_h, _, hg, wg = R.grid(H, W, P, S)
    if case["fit"]:
        assert (min(J, n_w) - 1) * S + P + 15 == R.INV_SPAN
        assert _fit_rows(case, ch, [(y, y * W) for y in range(hg)])
    for nodata in case["nodata"]:
        x, m, ins, outs = R.count_scene(case, nodata)
        assert x.dtype == R.NP[case["dt"]] and x.shape == (case["C"], H, W) and len(ins) >= 4 * len(ch)
        maps = {}
        for nd, rule, um in R.count_variants(case, nodata):
            rows = R.rows_ref(R.invalid_ref(x, nd, rule, m if um else None), P, S)
            counts = maps[(nd is not None, rule, um)] = R.counts_ref(rows, P, S)
            assert rows.shape == (hg, n_w) and counts.shape == (n_h, n_w)
            if nd is None and not um:
                assert not counts.any()
                continue
            assert 0 < counts.max() <= P * P and (n_h * n_w == 1 or counts.min() < counts.max())
            assert _boundaries_differ(rows, ch) and _boundaries_differ(counts, ch)
        if case["C"] > 1:                                   # the rule matters, and so does the mask
            assert not np.array_equal(maps[(True, "all", False)], maps[(True, "any", False)])
        assert not np.array_equal(maps[(True, "all", False)], maps[(True, "all", True)])
        if case.get("zero_full"):
            c = maps[(True, "all", False)]
            assert c.min() == 0 and c.max() == P * P
        if nodata == 0.0 and case["dt"] == "f32":
            assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        # the pixels planted right of and below the extent exist wherever there is a remainder strip, and change nothing
        assert bool(outs) == (hg < H or wg < W)
        if outs:
            x0, m0, _, _ = R.count_scene(case, nodata, outside=False)
            assert not np.array_equal(x0, x, equal_nan=case["dt"] == "f32") and not np.array_equal(m0, m)
            c0 = R.counts_ref(R.rows_ref(R.invalid_ref(x0, nodata, "all", m0), P, S), P, S)
            assert np.array_equal(c0, maps[(True, "all", True)])


@pytest.mark.parametrize("case", R.POINTER_CASES, ids=lambda c: c["id"])
def test_pointer_case_conditions(case):
    P, S, H, W = case["P"], case["S"], case["H"], case["W"]
    e = R.SIZE[case["dt"]]
    assert H * W * e % 16 != 0 and W % 2 == 1
    x, m, ins, outs = R.pointer_scene(case)
    n_h, n_w, hg, wg = R.grid(H, W, P, S)
    assert (n_h, n_w) == (1, 4) and hg < H and wg < W and outs
    counts = {r: R.counts_ref(R.rows_ref(R.invalid_ref(x, case["nodata"], r, m), P, S), P, S) for r in ("all", "any")}
    assert counts["all"].min() < counts["all"].max() and not np.array_equal(counts["all"], counts["any"])
    # across the element offsets of the scene every shift m occurs, for band 0 and, differently, for the other bands
    for off in range(16 // e):
        ms = {R.shift(off * e, e, y * W, 0) for y in range(hg)}
        assert len(ms) == 16 // e


# ---------------------------------------------------------------------------------------------------------------- c. border cases
def _resolve(v, p, n, mode):
    s = v - p
    if 0 <= s < n:
        return s
    if mode == "edge":
        return 0 if s < 0 else n - 1
    if mode == "reflect":
        return -s if s < 0 else 2 * (n - 1) - s
    return -1


@pytest.mark.parametrize("case", R.BORDER_CASES, ids=lambda c: c["id"])
def test_border_case_conditions(case):
    P, S, H, W = case["P"], case["S"], case["H"], case["W"]
    pt, pb, pl, pr = case["pads"]
    n_w, J, ch = _check_plan(case, W + pl + pr)
    n_h, _, hg, wg = R.grid(H, W, P, S, case["pads"])
    assert all(0 <= p < P for p in case["pads"])
    for mode in R.MODES:                                    # reflect is allowed exactly where the pads stay below the scene
        ok = mode != "reflect" or (max(pt, pb) <= H - 1 and max(pl, pr) <= W - 1)
        assert ok == (mode in case["modes"])
    touch = sum(1 for i in range(n_h) for j in range(n_w) if i * S < pt or i * S + P > pt + H or j * S < pl or j * S + P > pl + W)
    assert 2 * touch >= n_h * n_w
    if case["fit"]:
        for mode in case["modes"]:
            sys_ = [(y, _resolve(y, pt, H, mode)) for y in range(hg)]
            assert _fit_rows(case, ch, [(y, max(sy, 0) * W - pl) for y, sy in sys_])
    nodata, rule = case["nodata"], case["rules"][0]
    x, m = R.border_scenes(case)[0]
    assert x.shape == (case["C"], H, W)
    maps = {mode: R.border_counts(x, m, case, mode, case["fills"][1], nodata, rule)[1] for mode in case["modes"]}
    names = list(maps)
    for a in range(len(names)):                             # the modes count differently
        assert maps[names[a]].shape == (n_h, n_w)
        for b in range(a + 1, len(names)):
            assert not np.array_equal(maps[names[a]], maps[names[b]]), (names[a], names[b])
    assert all(_boundaries_differ(c, ch) for c in maps.values())
    # a fill that matches nodata makes the padding invalid: window (0, 0) gains exactly its padding pixels that were not masked
    c_eq = R.border_counts(x, None, case, "constant", case["fills"][0], nodata, rule)[1]
    c_ne = R.border_counts(x, None, case, "constant", case["fills"][1], nodata, rule)[1]
    real = (min(pt + H, P) - pt) * (min(pl + W, P) - pl)
    assert c_eq[0, 0] - c_ne[0, 0] == P * P - real
    if "pixel" in case:
        full = R.border_counts(x, m, case, "edge", 0, nodata, rule)[1]
        assert full.tolist() == [[P * P]] and maps["constant"].tolist() == [[1]]
        x1, m1 = R.border_scenes(case)[1]
        assert R.border_counts(x1, m1, case, "edge", 0, nodata, rule)[1].tolist() == [[0]]


# ---------------------------------------------------------------------------------------------------------------- d, e
def test_select_and_blend_case_conditions():
    for n in R.SELECT_N:
        c = R.select_counts(n)
        assert c.dtype == np.int32 and c.min() >= 0 and c.max() <= 4096
        assert len(R.select_ref(c, -1)) == 0 and len(R.select_ref(c, 4096)) == n
        if n > 7:
            assert 0 < len(R.select_ref(c, 0)) < len(R.select_ref(c, 2048)) < n
    assert 8192 in R.SELECT_N and 8191 in R.SELECT_N and 8193 in R.SELECT_N
    p = R.blend_tie_probs()
    K, n_h, n_w, k = R.BLEND_TIE
    assert np.allclose(p.sum(0), 1.0)
    cell, lab = R.blend_ref(p, None, k)
    assert np.array_equal(cell[1], cell[2]) and np.array_equal(cell[0], cell[3])
    assert set(np.unique(lab)) <= {0, 1} and (lab == 0).any() and (lab == 1).any()      # never the higher class of a tie
    assert (cell[0] == cell[1]).any()                                                   # and a four-way tie somewhere
    for K, n_h, n_w, k in R.BLEND_SHAPES:
        maps = R.blend_label_maps(n_h, n_w, seed=K + n_w)
        pr = R.blend_probs(K, n_h, n_w, seed=K + n_h)
        assert np.abs(pr.sum(0) - 1).max() < 1e-5
        _, lb = R.blend_ref(pr, maps["block"], k)
        assert (lb == -1).any()                              # cells without a covering window (the block reaches the grid's corner)
        _, la = R.blend_ref(pr, maps["all"], k)
        assert (la == -1).all()
        if n_h * n_w > 20:
            assert (maps["some"] < 0).any() and (maps["some"] >= 0).any()
