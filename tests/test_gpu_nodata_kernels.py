"""The kernels of the nodata / mask path (csrc/eae_scene.hip) by shape, through the C ABI, against the NumPy reference of
tests/nodata_ref.py: scene_invalid_rows_kernel and scene_invalid_windows_kernel (both outputs of eae_scene_invalid_counts: the rows
scratch and the counts) without and under a border, at every base-pointer alignment of the scene and the mask;
scene_select_kernel; scene_blend_kernel<VALID>.  The cases, what each reaches and the scenes are nodata_ref's;
tests/test_nodata_reference.py shows on the CPU that each case meets the conditions that let its comparison fail.

Every output is preset to -7 with a guard band of 64 elements behind it that must still hold -7 afterwards; every comparison is
np.array_equal (the counts are integers, the blend is fp32 adds in a stated order and one correctly rounded division: the build has
no fast-math flag); every call runs twice and must give the same bits.  Each case prints its plan and, per run, the number of
differing elements with the first eight positions, so a failure names the chunk, row alignment or pad it sits on."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpu_util as G
import nodata_ref as R
from eae_amd import _lib

pytestmark = pytest.mark.gpu

GUARD, PRESET = 64, -7
DTYPE_ID = {"u8": 0, "u16": 1, "f32": 2}                     # EAE_SCENE_U8 / U16 / F32
BORDER_ID = {None: 0, "constant": 1, "edge": 2, "reflect": 3}
RULE_ID = {"all": 0, "any": 1}
NODATA_NONE, NODATA_VALUE, NODATA_NAN = 0, 1, 2
ERR_ARG = -2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _upload(a, off_bytes=0):
    """(device address of a copy of array ``a`` that starts off_bytes behind a 16-byte boundary, the buffer that keeps it alive)"""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = torch.zeros(raw.size + 32, dtype=torch.uint8, device=G.dev())
    assert buf.data_ptr() % 16 == 0
    buf[off_bytes:off_bytes + raw.size].copy_(torch.from_numpy(raw))
    return buf.data_ptr() + off_bytes, buf


def _preset(n, dtype):
    return torch.full((n + GUARD,), PRESET, dtype=dtype, device=G.dev())


def _split(buf, n, what):
    """the first n elements of a preset buffer as NumPy, after checking the guard band behind them"""
    a = buf.cpu().numpy()
    assert (a[n:] == PRESET).all(), f"{what}: written behind the end, guard {R.where(a[n:] != PRESET, '(offset)')}"
    return a[:n]


def _nodata_arg(nodata):
    if nodata is None:
        return NODATA_NONE, 0.0
    return (NODATA_NAN, 0.0) if isinstance(nodata, float) and np.isnan(nodata) else (NODATA_VALUE, float(nodata))


def _invalid_counts(lib, geom, data, div, nodata, rule, mask, border=None, pads=(0, 0, 0, 0), fill=0.0):
    """eae_scene_invalid_counts on a scene at device address ``data`` (geom = dt, C, H, W, P, S), the mask at address ``mask`` (or
    None): (rc, rows [Hg, nW], counts [nH, nW]).  The descriptor is built as scene.py's _desc builds it, with any pads."""
    dt, c, h, w, p, s = geom
    n_h, n_w, hg, _ = R.grid(h, w, p, s, pads)
    rows, counts = _preset(hg * n_w, torch.int32), _preset(n_h * n_w, torch.int32)
    desc = _lib.EaeScene(C.c_void_p(data), G.ptr(div), DTYPE_ID[dt], c, h, w, p, s, BORDER_ID[border], *pads, float(fill))
    mode, value = _nodata_arg(nodata)
    rc = lib.eae_scene_invalid_counts(G.stream(), C.byref(desc), mode, value, RULE_ID[rule], C.c_void_p(mask or 0), G.ptr(rows),
                                      G.ptr(counts))
    torch.cuda.synchronize()
    if rc:
        assert (rows == PRESET).all() and (counts == PRESET).all()          # a refused call writes nothing
        return rc, None, None
    return 0, _split(rows, hg * n_w, "rows").reshape(hg, n_w), _split(counts, n_h * n_w, "counts").reshape(n_h, n_w)


def _check_counts(lib, tag, geom, data, div, nodata, rule, mask, ref_rows, ref_counts, **border):
    """two runs of the call against the reference, rows and counts; prints what differs before it asserts"""
    for run in (1, 2):
        rc, rows, counts = _invalid_counts(lib, geom, data, div, nodata, rule, mask, **border)
        assert rc == 0, (tag, rc, lib.eae_last_error())
        bad_r, bad_c = rows != ref_rows, counts != ref_counts
        print(f"{tag} run {run}: rows {R.where(bad_r, '(y, j)')}; counts {R.where(bad_c, '(i, j)')}")
        assert rows.shape == ref_rows.shape and not bad_r.any(), f"{tag} run {run}: rows {R.where(bad_r, '(y, j)')}"
        assert counts.shape == ref_counts.shape and not bad_c.any(), f"{tag} run {run}: counts {R.where(bad_c, '(i, j)')}"


def _plan_text(p, s, wv, elem, base):
    n_w, J, _ = R.plan(p, s, wv)
    return f"P {p} S {s} Wv {wv}: nW {n_w}, J {J}, chunks {R.chunks(p, s, wv)}, base % 16 = {base % 16}, elem {elem}"


# ---------------------------------------------------------------------------------------------------------------- a. counts, no border
@pytest.mark.parametrize("case", R.COUNT_CASES, ids=lambda c: c["id"])
def test_counts_by_shape(lib, case):
    dt, c, p, s, h, w = (case[k] for k in ("dt", "C", "P", "S", "H", "W"))
    geom, e = (dt, c, h, w, p, s), R.SIZE[dt]
    div = G.f32(np.ones(c))
    for nodata in case["nodata"]:
        x, m, _, _ = R.count_scene(case, nodata)
        data, keep = _upload(x, case.get("off", 0) * e)
        mask, keep_m = _upload(m)
        assert data % 16 == case.get("off", 0) * e           # the base the CPU conditions (shift m = 15 of the exact fits) assume
        print(f"{case['id']} nodata {nodata}: {_plan_text(p, s, w, e, data)}")
        for nd, rule, um in R.count_variants(case, nodata):
            inv = R.invalid_ref(x, nd, rule, m if um else None)
            ref_rows = R.rows_ref(inv, p, s)
            ref_counts = R.counts_ref(ref_rows, p, s)
            tag = f"{case['id']} nodata={nd} rule={rule} mask={um}"
            _check_counts(lib, tag, geom, data, div, nd, rule, mask if um else None, ref_rows, ref_counts)
            if nd is None and not um:
                assert not ref_counts.any()
        del keep, keep_m


# ---------------------------------------------------------------------------------------------------------------- b. base pointers
@pytest.mark.parametrize("case", R.POINTER_CASES, ids=lambda c: c["id"])
def test_counts_at_every_base_pointer(lib, case):
    dt, c, p, s, h, w, nodata = (case[k] for k in ("dt", "C", "P", "S", "H", "W", "nodata"))
    geom, e = (dt, c, h, w, p, s), R.SIZE[dt]
    assert h * w * e % 16 != 0                               # the bands of one group take different load paths
    div = G.f32(np.ones(c))
    x, m, _, _ = R.pointer_scene(case)
    ref = {}
    for rule in ("all", "any"):
        for um in (False, True):
            rows = R.rows_ref(R.invalid_ref(x, nodata, rule, m if um else None), p, s)
            ref[(rule, um)] = (rows, R.counts_ref(rows, p, s))
    masks = {mo: _upload(m, mo) for mo in R.MASK_OFFSETS}
    for off in range(16 // e):
        data, keep = _upload(x, off * e)
        assert data % 16 == off * e
        for n, mo in enumerate(R.MASK_OFFSETS):
            rule = ("all", "any")[(off + n) % 2]
            tag = f"{case['id']} scene +{off} elements, mask +{mo} bytes, rule={rule}"
            _check_counts(lib, tag, geom, data, div, nodata, rule, masks[mo][0], *ref[(rule, True)])
        _check_counts(lib, f"{case['id']} scene +{off} elements, no mask", geom, data, div, nodata, "all", None, *ref[("all", False)])
        del keep


# ---------------------------------------------------------------------------------------------------------------- c. counts, border
@pytest.mark.parametrize("case", R.BORDER_CASES, ids=lambda c: c["id"])
def test_counts_under_a_border(lib, case):
    dt, c, p, s, h, w, pads, nodata = (case[k] for k in ("dt", "C", "P", "S", "H", "W", "pads", "nodata"))
    geom, e = (dt, c, h, w, p, s), R.SIZE[dt]
    div = G.f32(np.ones(c))
    for n, (x, m) in enumerate(R.border_scenes(case)):
        data, keep = _upload(x)
        mask, keep_m = _upload(m)
        print(f"{case['id']} scene {n} pads {pads}: {_plan_text(p, s, w + pads[2] + pads[3], e, data)}")
        for mode in R.MODES:
            if mode not in case["modes"]:                    # a reflect pad above H - 1 / W - 1: refused, nothing written
                rc, _, _ = _invalid_counts(lib, geom, data, div, nodata, "all", mask, border=mode, pads=pads)
                assert rc == ERR_ARG, (case["id"], mode, rc)
        for mode, fill, rule, um in R.border_variants(case):
            ref_rows, ref_counts = R.border_counts(x, m if um else None, case, mode, fill, nodata, rule)
            tag = f"{case['id']} scene {n} {mode} fill={fill} rule={rule} mask={um}"
            _check_counts(lib, tag, geom, data, div, nodata, rule, mask if um else None, ref_rows, ref_counts, border=mode, pads=pads,
                          fill=fill)
        # the mask alone, and neither: padding is never invalid by itself
        for mode in case["modes"]:
            ref_rows, ref_counts = R.border_counts(x, m, case, mode, case["fills"][0], None, "all")
            _check_counts(lib, f"{case['id']} scene {n} {mode} mask only", geom, data, div, None, "all", mask, ref_rows, ref_counts,
                          border=mode, pads=pads, fill=case["fills"][0])
            zero = np.zeros_like(ref_counts)
            _check_counts(lib, f"{case['id']} scene {n} {mode} neither", geom, data, div, None, "all", None, np.zeros_like(ref_rows), zero,
                          border=mode, pads=pads, fill=case["fills"][0])
        del keep, keep_m


# ---------------------------------------------------------------------------------------------------------------- d. select
@pytest.mark.parametrize("n", R.SELECT_N)
def test_select_by_size(lib, n):
    counts = R.select_counts(n)
    dc = torch.from_numpy(counts).to(G.dev())
    seen = set()
    for t in R.SELECT_T:
        ref = R.select_ref(counts, t)
        seen.add(0 if len(ref) == 0 else 2 if len(ref) == n else 1)
        for run in (1, 2):
            ids, cnt = _preset(n, torch.int64), _preset(1, torch.int64)
            rc = lib.eae_scene_select(G.stream(), G.ptr(dc), n, t, G.ptr(ids), G.ptr(cnt))
            torch.cuda.synchronize()
            assert rc == 0, (rc, lib.eae_last_error())
            got, k = _split(ids, n, "ids"), int(_split(cnt, 1, "count")[0])
            print(f"select n {n} ({-(-n // 8192)} passes) t {t} run {run}: count {k} (reference {len(ref)})")
            assert k == len(ref)
            assert np.array_equal(got[:k], ref), R.where(got[:k] != ref, "(position)")
            assert (got[k:] == PRESET).all(), f"written behind ids[count): {R.where(got[k:] != PRESET, '(offset)')}"
    assert {0, 2} <= seen                                    # nothing selected, and everything


# ---------------------------------------------------------------------------------------------------------------- e. blends
def _blend(lib, probs, labels, k):
    """eae_scene_blend (labels None) or eae_scene_blend_valid: (cell [K, cH, cW], cell labels [cH, cW])"""
    K, n_h, n_w = probs.shape
    ch, cw = n_h + k - 1, n_w + k - 1
    dp = G.f32(probs)
    cell, lab = _preset(K * ch * cw, torch.float32), _preset(ch * cw, torch.int64)
    if labels is None:
        rc = lib.eae_scene_blend(G.stream(), G.ptr(dp), K, n_h, n_w, k, G.ptr(cell), G.ptr(lab))
    else:
        dl = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(G.dev())
        rc = lib.eae_scene_blend_valid(G.stream(), G.ptr(dp), G.ptr(dl), K, n_h, n_w, k, G.ptr(cell), G.ptr(lab))
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.eae_last_error())
    return _split(cell, K * ch * cw, "cell").reshape(K, ch, cw), _split(lab, ch * cw, "cell labels").reshape(ch, cw)


def _check_blend(lib, tag, probs, labels, k):
    ref_cell, ref_lab = R.blend_ref(probs, labels, k)
    out = None
    for run in (1, 2):
        cell, lab = _blend(lib, probs, labels, k)
        bad_c, bad_l = cell.view(np.uint32) != ref_cell.view(np.uint32), lab != ref_lab
        print(f"{tag} run {run}: cell {R.where(bad_c, '(class, ci, cj)')}; labels {R.where(bad_l, '(ci, cj)')}")
        assert not bad_c.any(), f"{tag} run {run}: cell {R.where(bad_c, '(class, ci, cj)')}"
        assert not bad_l.any(), f"{tag} run {run}: labels {R.where(bad_l, '(ci, cj)')}"
        out = (cell, lab)
    return out


@pytest.mark.parametrize("K,n_h,n_w,k", R.BLEND_SHAPES + [R.BLEND_TIE])
def test_blends_bit_for_bit(lib, K, n_h, n_w, k):
    tie = (K, n_h, n_w, k) == R.BLEND_TIE
    probs = R.blend_tie_probs() if tie else R.blend_probs(K, n_h, n_w, seed=K + n_h)
    tag = f"blend K {K} grid {n_h} x {n_w} k {k}" + (" (ties)" if tie else "")
    plain = _check_blend(lib, tag + " plain", probs, None, k)
    if tie:
        assert (plain[1] == 1).any() and (plain[1] == 0).any() and set(np.unique(plain[1])) <= {0, 1}
    for name, labels in R.blend_label_maps(n_h, n_w, seed=K + n_w).items():
        cell, lab = _check_blend(lib, f"{tag} valid form, {name} invalid", probs, labels, k)
        if name == "none":                                   # no label negative: the plain form's bits
            assert np.array_equal(cell.view(np.uint32), plain[0].view(np.uint32)) and np.array_equal(lab, plain[1])
        if name == "all":
            assert (lab == -1).all() and not cell.any()
        if name == "block":
            assert (lab == -1).any()
