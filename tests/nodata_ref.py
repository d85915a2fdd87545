"""NumPy reference of the nodata / mask path (csrc/eae_scene.hip: scene_invalid_rows_kernel, scene_invalid_windows_kernel,
scene_select_kernel, scene_blend_kernel<VALID>), the case tables of tests/test_gpu_nodata_kernels.py and the scenes they run on.

Nothing here touches a device or the library.  The counts are integers, so every comparison is np.array_equal; the blend is written
in the kernel's own order (fp32 adds over i, then j, one fp32 division), so it is compared with np.array_equal too.
tests/test_nodata_reference.py checks, on the CPU, this reference against brute force and every case against the conditions that
make its comparison able to fail (the plan it names, an exact fit, counts that change across a chunk boundary, ...)."""
import functools

import numpy as np

NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
SIZE = {"u8": 1, "u16": 2, "f32": 4}
MODES = ("constant", "edge", "reflect")
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- the plan, restated
# csrc/eae_scene.hip: INV_NT = 256 threads of 16 pixels, INV_SPAN = 4096 pixels of LDS per pass-1 workgroup, of which up to 15 are the
# alignment shift m; eae_scene_invalid_counts: J = (INV_SPAN - 15 - P) / S + 1 window columns per workgroup, nchunk = ceil(nW / J).
INV_SPAN = 4096


def plan(P, S, Wv):
    """(nW, J, nchunk) of a (virtual) scene width Wv"""
    n_w = (Wv - P) // S + 1
    J = (INV_SPAN - 15 - P) // S + 1
    return n_w, J, -(-n_w // J)


def chunks(P, S, Wv):
    """[(j0, jn, x0, x1)]: the window columns j0 .. j0 + jn - 1 and the pixels [x0, x1) of every pass-1 chunk (virtual coordinates)"""
    n_w, J, nchunk = plan(P, S, Wv)
    out = []
    for c in range(nchunk):
        j0 = c * J
        jn = min(J, n_w - j0)
        out.append((j0, jn, j0 * S, (j0 + jn - 1) * S + P))
    return out


def grid(H, W, P, S, pads=(0, 0, 0, 0)):
    """(nH, nW, Hg, Wg): the grid over the virtual scene and its extent"""
    hv, wv = H + pads[0] + pads[1], W + pads[2] + pads[3]
    n_h, n_w = (hv - P) // S + 1, (wv - P) // S + 1
    return n_h, n_w, (n_h - 1) * S + P, (n_w - 1) * S + P


def shift(base, elem, rowoff, x0):
    """m of scene_invalid_rows_kernel: the element misalignment of band 0's address base + (rowoff + x0) * elem"""
    return ((base + (rowoff + x0) * elem) % 16) // elem


# ---------------------------------------------------------------------------------------------------------------- the reference
def invalid_ref(scene, nodata, rule, mask):
    """bool [H, W]: a NaN nodata is isnan, a value nodata IEEE == (so -0.0 matches 0.0), over "all" or "any" of the bands; or mask != 0"""
    if nodata is None:
        inv = np.zeros(scene.shape[1:], dtype=bool)
    else:
        eq = np.isnan(scene) if isinstance(nodata, float) and np.isnan(nodata) else scene == nodata
        inv = eq.all(0) if rule == "all" else eq.any(0)
    if mask is not None:
        inv = inv | (mask != 0)
    return inv


def pad_ref(scene, mask, pads, mode, fill):
    """(padded scene, padded mask or None): np.pad by (top, bottom, left, right); constant pads the scene with fill, the mask with 0"""
    pt, pb, pl, pr = pads
    kw = {"constant_values": fill} if mode == "constant" else {}
    ps = np.pad(scene, ((0, 0), (pt, pb), (pl, pr)), mode, **kw)
    pm = None
    if mask is not None:
        pm = np.pad(mask, ((pt, pb), (pl, pr)), mode, **({"constant_values": 0} if mode == "constant" else {}))
    return ps, pm


def rows_ref(inv, P, S):
    """int64 [Hg, nW]: rows[y, j] = inv[y, j*S : j*S + P].sum(), by a cumulative sum along x"""
    n_h, n_w = (inv.shape[0] - P) // S + 1, (inv.shape[1] - P) // S + 1
    hg = (n_h - 1) * S + P
    cs = np.zeros((hg, inv.shape[1] + 1), dtype=np.int64)
    np.cumsum(inv[:hg], axis=1, dtype=np.int64, out=cs[:, 1:])
    j = np.arange(n_w) * S
    return cs[:, j + P] - cs[:, j]


def counts_ref(rows, P, S):
    """int64 [nH, nW]: counts[i, j] = rows[i*S : i*S + P, j].sum(), by a cumulative sum along y"""
    n_h = (rows.shape[0] - P) // S + 1
    cs = np.zeros((rows.shape[0] + 1, rows.shape[1]), dtype=np.int64)
    np.cumsum(rows, axis=0, dtype=np.int64, out=cs[1:])
    i = np.arange(n_h) * S
    return cs[i + P] - cs[i]


def select_ref(counts, t):
    return np.flatnonzero(counts.reshape(-1) <= t)


def blend_ref(probs, labels, k):
    """(cell fp32 [K, cH, cW], cell labels int64 [cH, cW]) of probs fp32 [K, nH, nW]; labels int64 [nH, nW] or None (every window
    valid).  Cell (ci, cj) sums its covering windows i in [ci-k+1, ci], j in [cj-k+1, cj] inside the grid in fp32, i ascending, then j
    ascending, invalid windows (label < 0) skipped, divides once by the fp32 count and takes the first class with the largest value."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    K, n_h, n_w = probs.shape
    ch, cw = n_h + k - 1, n_w + k - 1
    valid = np.ones((n_h, n_w), dtype=bool) if labels is None else np.asarray(labels) >= 0
    ci, cj = np.arange(ch)[:, None], np.arange(cw)[None, :]
    s = np.zeros((K, ch, cw), dtype=np.float32)
    nv = np.zeros((ch, cw), dtype=np.int64)
    for a in range(k):                        # i = ci - k + 1 + a ascends with a
        i = ci - k + 1 + a
        for b in range(k):
            j = cj - k + 1 + b
            use = (i >= 0) & (i < n_h) & (j >= 0) & (j < n_w)
            ic, jc = np.clip(i, 0, n_h - 1), np.clip(j, 0, n_w - 1)
            use = use & valid[ic, jc]
            q = probs[:, ic, jc]                                   # [K, ch, cw]
            s = np.where(use[None], (s + q).astype(np.float32), s)
            nv += use
    cell = np.zeros((K, ch, cw), dtype=np.float32)
    has = nv > 0
    cell[:, has] = (s[:, has] / nv[has].astype(np.float32)[None]).astype(np.float32)
    lab = np.zeros((ch, cw), dtype=np.int64)
    mx = cell[0].copy()
    for c in range(1, K):
        up = cell[c] > mx                     # strict: the lowest class wins a tie
        mx = np.where(up, cell[c], mx)
        lab = np.where(up, c, lab)
    lab[~has] = -1
    return cell, lab


# ---------------------------------------------------------------------------------------------------------------- planted pixels
def plant(scene, mask, P, S, pads, nodata):
    """Plant invalid pixels where the index arithmetic of pass 1 can go wrong, each in a row of its own as far as the rows last (the
    n-th one goes to real row (37 n + 5) mod the rows inside the extent, as _holey_scene of test_gpu_scene_nodata.py does):
    the virtual columns x0 - 1, x0, x1 - 1, x1 of every chunk (x1 in two rows), the first and last column and row of every window, the first and last
    real row and column; and, outside the extent (the remainder strips right of and below it), pixels that must not be counted.
    A pixel is planted as nodata in every band of ``scene`` (nodata not None) and as a non-zero byte of ``mask`` (not None) half the
    rows further down.  Returns (inside, outside): the real (y, x) of the pixels planted in the scene."""
    _, H, W = scene.shape
    pt, pb, pl, pr = pads
    n_h, n_w, hg, wg = grid(H, W, P, S, pads)
    rows_in, cols_in = min(H, hg - pt), min(W, wg - pl)          # real rows / columns inside the extent
    vcols = []
    for j0, jn, x0, x1 in chunks(P, S, W + pl + pr):
        vcols += [x0 - 1, x0, x1 - 1, x1, x1]          # x1 twice (two rows): the one at x0 - 1 of the next chunk cannot cancel it
    for j in range(n_w):
        vcols += [j * S, j * S + P - 1]
    vcols += [pl, pl + W - 1]
    vrows = [pt, pt + H - 1]
    for i in range(n_h):
        vrows += [i * S, i * S + P - 1]
    inside, outside = [], []
    for n, v in enumerate(vcols):
        x = v - pl
        if 0 <= x < cols_in:
            inside.append(((37 * n + 5) % rows_in, x))
    for n, v in enumerate(vrows):
        y = v - pt
        if 0 <= y < rows_in:
            inside.append((y, (53 * n + 3) % cols_in))
    for n, x in enumerate(sorted({cols_in, W - 1} if cols_in < W else ())):
        outside += [((37 * n + 5) % H, x), (H - 1 - (11 * n) % H, x)]
    for n, y in enumerate(sorted({rows_in, H - 1} if rows_in < H else ())):
        outside += [(y, (53 * n + 3) % W), (y, W - 1 - (13 * n) % W)]
    for y, x in inside + outside:
        if nodata is not None:
            scene[:, y, x] = nodata
    if mask is not None:
        for y, x in inside:
            mask[(y + rows_in // 2) % rows_in, x] = 1
        for y, x in outside:
            mask[y, x] = 1
    return inside, outside


def make_scene(dt, C, H, W, P, S, pads, nodata, seed, frac, full_window=None, planted=True, outside=True):
    """(scene [C, H, W], mask uint8 [H, W], inside, outside): a background without accidental nodata, then whole-pixel nodata at random
    (frac), single-band nodata at random (frac / 2: counts for rule "any" only), a random mask with arbitrary non-zero bytes and a small
    cloud, `plant`, and with full_window = (i, j) that window wholly nodata.  A value nodata of 0.0 is planted as -0.0 on every other
    planted pixel.  outside=False restores the background on the planted pixels outside the extent."""
    g = np.random.default_rng(seed)
    if dt == "f32":
        x = (g.random((C, H, W), dtype=np.float32) * 3.0 + 0.5).astype(np.float32)
    else:
        x = g.integers(1, np.iinfo(NP[dt]).max, (C, H, W)).astype(NP[dt])       # neither 0 nor the dtype's maximum
    back = x.copy()
    full = g.random((H, W)) < frac
    part = g.random((C, H, W)) < frac / 2
    x[part] = nodata
    x[:, full] = nodata
    mask = ((g.random((H, W)) < frac) * g.integers(1, 256, (H, W))).astype(np.uint8)
    if H >= 12 and W >= 16:
        mask[H // 3:H // 3 + 9, W // 2:W // 2 + 13] = 255        # a small cloud
    if full_window is not None:
        i, j = full_window
        x[:, i * S - pads[0]:i * S - pads[0] + P, j * S - pads[2]:j * S - pads[2] + P] = nodata
    ins, outs = [], []
    if planted:
        mask_back = mask.copy()
        ins, outs = plant(x, mask, P, S, pads, nodata)
        if dt == "f32" and nodata == 0.0:
            for n, (y, xx) in enumerate(ins + outs):
                if n % 2:
                    x[:, y, xx] = -0.0
        if not outside:
            for y, xx in outs:
                x[:, y, xx] = back[:, y, xx]
                mask[y, xx] = mask_back[y, xx]
    return x, mask, ins, outs


# ---------------------------------------------------------------------------------------------------------------- a. counts, no border
# H = P + 2 S unless the case says otherwise.  nodata: the values the case runs with (fp32: a NaN, then 0.0 planted as +0.0 and -0.0).
# nW, J, nchunk, last: the plan the case is there for (last = the window columns of the last chunk); fit: some row of a chunk has the
# shift m = 15 and a span (jn - 1) S + P + 15 of exactly INV_SPAN, so that pre[s0 + P] is the last element of pre.  off: the element
# offset of the scene in its device buffer (0: the allocation's own 16-byte aligned base).  The largest patch keeps its even width
# (every row of an even-width uint8 scene starts at an even address) and reaches m = 15 from an odd base, off = 1.
# split: H W sizeof(T) is no multiple of 16, so the bands of one 16-byte group take different load paths (the arithmetic decides
# this, case by case; the base-pointer cases of section b are all split).
COUNT_CASES = [
    dict(id="u8c1-fit", dt="u8", C=1, P=64, S=13, H=90, W=4081, nodata=(0,), nW=310, J=310, nchunk=1, last=310, fit=True, split=True),
    dict(id="u8c3-fit-1", dt="u8", C=3, P=64, S=13, H=90, W=4095, nodata=(0,), nW=311, J=310, nchunk=2, last=1, fit=True, split=True),
    dict(id="u8c1-s64", dt="u8", C=1, P=64, S=64, H=192, W=8128, nodata=(255,), nW=127, J=63, nchunk=3, last=1, fit=False, split=False,
         full_window=(1, 63), frac=0.0004, zero_full=True),
    dict(id="u8c2-s1", dt="u8", C=2, P=64, S=1, H=66, W=4200, nodata=(0,), nW=4137, J=4018, nchunk=2, last=119, fit=False, split=False,
         seed=1052),
    dict(id="u16c3", dt="u16", C=3, P=64, S=7, H=78, W=4100, nodata=(0,), nW=577, J=574, nchunk=2, last=3, fit=False, split=False),
    dict(id="f32c2", dt="f32", C=2, P=64, S=7, H=78, W=4100, nodata=(NAN, 0.0), nW=577, J=574, nchunk=2, last=3, fit=False, split=False),
    dict(id="u16c16-p128", dt="u16", C=16, P=128, S=20, H=168, W=4201, nodata=(65535,), nW=204, J=198, nchunk=2, last=6, fit=False,
         split=False),
    dict(id="u8c1-p4032", dt="u8", C=1, P=4032, S=49, H=4081, W=4130, nodata=(0,), nW=3, J=2, nchunk=2, last=1, fit=True, split=True,
         off=1, frac=0.0005),
    dict(id="u8c3-one", dt="u8", C=3, P=64, S=20, H=67, W=67, nodata=(0,), nW=1, J=201, nchunk=1, last=1, fit=False, split=True),
]


def count_variants(case, nodata):
    """(nodata, rule, use_mask) runs of a scene of a case: nodata under "all" (and "any" with several bands), the mask alone, both
    together, and neither (all zeros)"""
    v = [(nodata, "all", False)]
    if case["C"] > 1:
        v.append((nodata, "any", False))
    return v + [(None, "all", True), (nodata, "all", True), (nodata, "any", True), (None, "all", False)]


def _key(nodata):
    return "nan" if isinstance(nodata, float) and np.isnan(nodata) else nodata


@functools.lru_cache(maxsize=4)
def _count_scene(cid, key, outside):
    case = next(c for c in COUNT_CASES if c["id"] == cid)
    nodata = NAN if key == "nan" else key
    seed = case.get("seed", 1000 + 17 * COUNT_CASES.index(case)) + (0 if key == "nan" else int(key) % 7)
    x, m, ins, outs = make_scene(case["dt"], case["C"], case["H"], case["W"], case["P"], case["S"], (0, 0, 0, 0), nodata, seed,
                                 case.get("frac", 0.003), case.get("full_window"), outside=outside)
    x.setflags(write=False)
    m.setflags(write=False)
    return x, m, ins, outs


def count_scene(case, nodata, outside=True):
    """the (read-only, shared) scene, mask and planted pixels of a case of section a"""
    return _count_scene(case["id"], _key(nodata), outside)


# ---------------------------------------------------------------------------------------------------------------- b. base pointers
# the scene as a view at every element offset of a 16-byte group, the mask at byte offsets of its own; H W sizeof(T) % 16 != 0
POINTER_CASES = [dict(id="u8", dt="u8", C=3, P=64, S=20, H=70, W=131, nodata=0),
                 dict(id="u16", dt="u16", C=3, P=64, S=20, H=70, W=131, nodata=65535),
                 dict(id="f32", dt="f32", C=3, P=64, S=20, H=69, W=131, nodata=NAN)]
MASK_OFFSETS = (0, 1, 7, 15)


def pointer_scene(case):
    return make_scene(case["dt"], case["C"], case["H"], case["W"], case["P"], case["S"], (0, 0, 0, 0), case["nodata"],
                      2000 + POINTER_CASES.index(case), 0.004)


# ---------------------------------------------------------------------------------------------------------------- c. counts, border
# pads = (top, bottom, left, right).  modes: those the pads allow (a reflect pad is at most H - 1 / W - 1); the others are refused by
# eae_scene_check with EAE_ERR_ARG (-2), which the 1 x 1 case asserts.  fills: (a fill that matches nodata, one that does not).
# pixel: the 1 x 1 scene holds nodata, then another value.  fit / nchunk / last / split as in section a.
BORDER_CASES = [
    dict(id="u16c2-left0", dt="u16", C=2, H=70, W=131, P=64, S=20, pads=(5, 9, 0, 13), modes=MODES, nodata=65535, fills=(65535, 7),
         rules=("any", "all"), nchunk=1, last=5, fit=False, split=True),
    dict(id="f32c1-bottom0", dt="f32", C=1, H=41, W=97, P=64, S=16, pads=(23, 0, 7, 30), modes=MODES, nodata=NAN, fills=(NAN, 1.0),
         rules=("all",), nchunk=1, last=5, fit=False, split=True),
    dict(id="u8c1-1x1", dt="u8", C=1, H=1, W=1, P=64, S=64, pads=(31, 32, 40, 23), modes=MODES[:2], nodata=0, fills=(0, 7),
         rules=("all",), nchunk=1, last=1, fit=False, split=True, pixel=(0, 9)),
    dict(id="u8c3-narrow", dt="u8", C=3, H=64, W=5, P=64, S=1, pads=(0, 0, 30, 30), modes=MODES[:2], nodata=0, fills=(0, 7),
         rules=("all", "any"), nchunk=1, last=2, fit=False, split=False),
    dict(id="u8c3-reflect-max", dt="u8", C=3, H=33, W=33, P=64, S=1, pads=(32, 0, 0, 32), modes=MODES, nodata=0, fills=(0, 7),
         rules=("all", "any"), nchunk=1, last=2, fit=False, split=True),
    dict(id="u8c1-2chunks", dt="u8", C=1, H=40, W=4100, P=64, S=32, pads=(12, 12, 14, 14), modes=MODES, nodata=0, fills=(0, 7),
         rules=("all",), nchunk=2, last=2, fit=False, split=False),
    dict(id="u8c1-fit", dt="u8", C=1, H=40, W=4067, P=64, S=13, pads=(12, 12, 7, 7), modes=MODES, nodata=0, fills=(0, 7),
         rules=("all",), nchunk=1, last=310, fit=True, split=True),
    dict(id="u16c4-caseA", dt="u16", C=4, H=100, W=150, P=64, S=32, pads=(14, 14, 5, 5), modes=MODES, nodata=0, fills=(0, 7),
         rules=("all", "any"), nchunk=1, last=4, fit=False, split=False),
]


def border_scenes(case):
    """[(scene, mask)] of a border case: dense enough near the edges (2 % invalid) that the three modes count differently"""
    i = BORDER_CASES.index(case)
    if "pixel" in case:
        return [(np.full((1, 1, 1), v, dtype=NP[case["dt"]]), np.zeros((1, 1), dtype=np.uint8)) for v in case["pixel"]] + \
               [(np.full((1, 1, 1), case["pixel"][1], dtype=NP[case["dt"]]), np.ones((1, 1), dtype=np.uint8))]
    x, m, _, _ = make_scene(case["dt"], case["C"], case["H"], case["W"], case["P"], case["S"], case["pads"], case["nodata"], 3000 + i,
                            0.02)
    return [(x, m)]


def border_variants(case):
    """(mode, fill, rule, use_mask) runs: every allowed mode, in constant mode both fills, every rule, with and without the mask"""
    out = []
    for mode in case["modes"]:
        for fill in (case["fills"] if mode == "constant" else (0,)):
            for rule in case["rules"]:
                out += [(mode, fill, rule, True), (mode, fill, rule, False)]
    return out


def border_counts(x, m, case, mode, fill, nodata, rule):
    """(rows, counts) of the reference under a border: pad_ref, then the borderless reference"""
    ps, pm = pad_ref(x, m, case["pads"], mode, fill)
    rows = rows_ref(invalid_ref(ps, nodata, rule, pm), case["P"], case["S"])
    return rows, counts_ref(rows, case["P"], case["S"])


# ---------------------------------------------------------------------------------------------------------------- d. select
SELECT_N = (1, 7, 8191, 8192, 8193, 16384, 20001)            # 8192 windows per pass of scene_select_kernel
SELECT_T = (-1, 0, 1, 2048, 4096)


def select_counts(n):
    return np.random.default_rng(4000 + n).integers(0, 4097, n).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- e. blends
BLEND_SHAPES = [(1, 1, 1, 1), (6, 1, 1, 4), (6, 2, 9, 4), (64, 5, 3, 2), (10, 7, 300, 4), (3, 300, 2, 8), (10, 13, 17, 1)]   # K, nH, nW, k
BLEND_TIE = (4, 5, 6, 2)                                     # equal probabilities, constructed: argmax ties


def blend_probs(K, n_h, n_w, seed):
    """seeded softmax rows, fp32 [K, nH, nW]"""
    z = np.random.default_rng(seed).normal(size=(K, n_h, n_w)) * 2.0
    e = np.exp(z - z.max(0, keepdims=True))
    return (e / e.sum(0, keepdims=True)).astype(np.float32)


def blend_tie_probs():
    """[K, nH, nW] of BLEND_TIE with dyadic values: classes 1 and 2 are equal everywhere and the largest in half of the windows,
    classes 0 and 3 equal and the largest in the rest, so every cell's means tie exactly (sums of a few dyadic values are exact)"""
    K, n_h, n_w, _ = BLEND_TIE
    g = np.random.default_rng(5)
    hi = g.integers(0, 2, (n_h, n_w)).astype(bool)
    p = np.empty((K, n_h, n_w), dtype=np.float32)
    p[1] = p[2] = np.where(hi, 0.375, 0.125)
    p[0] = p[3] = np.where(hi, 0.125, 0.375)
    return p


def blend_label_maps(n_h, n_w, seed):
    """name -> int64 [nH, nW] window labels for the valid form: none invalid, about 30 % invalid, a wholly invalid 4 x 4 block (cells
    without a covering window wherever the block is at least k wide), all invalid"""
    g = np.random.default_rng(seed)
    base = g.integers(0, 3, (n_h, n_w)).astype(np.int64)
    some = base.copy()
    some[g.random((n_h, n_w)) < 0.3] = -1
    block = base.copy()
    block[:4, :4] = -1
    return {"none": base, "some": some, "block": block, "all": np.full((n_h, n_w), -1, dtype=np.int64)}


def where(bad, names="(y, x)"):
    """the number of differing elements and the first eight positions, for a failure message"""
    idx = np.argwhere(bad)
    return f"{len(idx)} of {bad.size} differ, first at {names} = {idx[:8].tolist()}"
