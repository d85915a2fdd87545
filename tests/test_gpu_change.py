"""Change detection on the device (eae_amd.change): `eae_change_moments` / `eae_change_variates` through the C ABI by shape and dtype
against the NumPy float64 restatement (tests/change_ref.py), then `joint_moments`, `mad_fit`, `detect_change`,
`invariant_regression` and `class_transitions`.

Bounds (derived in change_ref's docstring, not measured): a moment within (chunk + 2) 2^-24 sum w |d_i d_j| of the float64 sum of the
same fp32 differences; a variate within (2C + 1) 2^-24 sum_j |T_ji d_j|, chi2 from that; prob within the closed form's evaluation
bound of the float64 closed form at the fp32 chi2 the kernel wrote.  Symmetry, run-to-run equality, the invalid pixels' values and
the independence of the requested outputs are exact.  Every output is poisoned before a call and the workspace is filled with 0xFF.
The two end-to-end bounds (`mad_fit`, `invariant_regression`) are 8 x the first run's measurement, rounded up to a power of two."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
import change_ref as R

pytestmark = pytest.mark.gpu

#          (C, H, W)
SHAPES = [(1, 1, 1), (1, 1, 63), (3, 5, 67), (4, 64, 64), (16, 33, 129), (13, 70, 300),
          (2, 600, 1100)]              # 2579 chunks for 2048 waves: more than one grid round
DTYPES = [("u8", "u8"), ("u16", "u16"), ("f32", "f32"), ("u16", "f32")]
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
CODE = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}
POISON = -7.0


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _scene(rng, kind, c, h, w):
    if kind == "f32":
        return (300.0 + 100.0 * rng.standard_normal((c, h, w))).astype(np.float32)
    return rng.integers(0, 256 if kind == "u8" else 4096, (c, h, w)).astype(NP[kind])


def _pair(shape, kinds, seed):
    """(a, b, div_a, div_b): b follows a loosely, so the cross moments are not noise; some divisors are 1 (no division)."""
    c, h, w = shape
    rng = np.random.default_rng(seed)
    a, b = _scene(rng, kinds[0], c, h, w), _scene(rng, kinds[1], c, h, w)
    b = (0.5 * b + 0.5 * a.astype(np.float64) * (float(b.max()) + 1) / (float(a.max()) + 1)).astype(NP[kinds[1]])
    div_a = np.where(np.arange(c) % 2 == 0, 1.0, 255.0 if kinds[0] == "u8" else 1000.0).astype(np.float32)
    div_b = np.where(np.arange(c) % 3 == 0, 1.0, 3.0).astype(np.float32)
    return a, b, div_a, div_b


def _nodata(nd, rule):
    mode = 0 if nd is None else 2 if isinstance(nd, float) and np.isnan(nd) else 1
    return mode, 0.0 if mode != 1 else float(nd), {"all": 0, "any": 1}[rule]


def _head(a, b, div_a, div_b, nodata_a, rule_a, nodata_b, rule_b, mask, shape=None, null=()):
    """Device copies and the scene arguments the two calls share."""
    c, h, w = a.shape if shape is None else shape
    t = dict(a=torch.from_numpy(a).cuda(), b=torch.from_numpy(b).cuda(), div_a=torch.from_numpy(div_a).cuda(),
             div_b=torch.from_numpy(div_b).cuda(), mask=None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda())
    p = {k: None if k in null else _ptr(v) for k, v in t.items()}
    return t, (p["a"], p["b"], CODE[a.dtype], CODE[b.dtype], c, h, w, p["div_a"], p["div_b"], *_nodata(nodata_a, rule_a),
               *_nodata(nodata_b, rule_b), p["mask"])


def _c_moments(a, b, div_a, div_b, pivot, weights=None, nodata_a=None, rule_a="all", nodata_b=None, rule_b="all", mask=None,
               ws_bytes=None, ws_null=False, null=(), shape=None):
    """One moments call on poisoned outputs and a 0xFF workspace: (rc, moments float64, count)."""
    lib = _lib.load()
    c, h, w = a.shape if shape is None else shape
    keep, head = _head(a, b, div_a, div_b, nodata_a, rule_a, nodata_b, rule_b, mask, shape, null)
    need = lib.eae_change_moments_workspace_bytes(*a.shape)
    assert need > 0
    nb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(nb, 1),), 0xFF, dtype=torch.uint8, device="cuda")        # NaN bit patterns: every partial read must have been written
    t = dict(weights=None if weights is None else torch.from_numpy(weights.astype(np.float32)).cuda(),
             pivot=torch.from_numpy(np.asarray(pivot, dtype=np.float32)).cuda(),
             out=torch.full((1 + 2 * a.shape[0] + 4 * a.shape[0] ** 2,), POISON, dtype=torch.float64, device="cuda"),
             count=torch.full((1,), int(POISON), dtype=torch.int64, device="cuda"))
    p = {k: None if k in null else _ptr(v) for k, v in t.items()}
    rc = lib.eae_change_moments(_stream(), *head, p["weights"], p["pivot"], p["out"], p["count"], None if ws_null else _ptr(ws), nb)
    torch.cuda.synchronize()
    del keep
    return rc, t["out"].cpu().numpy(), int(t["count"].cpu()[0])


def _c_variates(a, b, div_a, div_b, mean, tm, dof, nodata_a=None, rule_a="all", nodata_b=None, rule_b="all", mask=None,
                outputs=("chi2", "prob", "var"), null=(), shape=None):
    """One variates call on poisoned outputs: (rc, chi2, prob, variates) as NumPy, None for an output that was not asked for."""
    lib = _lib.load()
    c, h, w = a.shape
    keep, head = _head(a, b, div_a, div_b, nodata_a, rule_a, nodata_b, rule_b, mask, shape, null)
    t = dict(mean=torch.from_numpy(np.asarray(mean, dtype=np.float32)).cuda(),
             T=torch.from_numpy(np.ascontiguousarray(tm, dtype=np.float32)).cuda())
    out = dict(chi2=torch.full((h, w), POISON, dtype=torch.float32, device="cuda") if "chi2" in outputs else None,
               prob=torch.full((h, w), POISON, dtype=torch.float32, device="cuda") if "prob" in outputs else None,
               var=torch.full((c, h, w), POISON, dtype=torch.float32, device="cuda") if "var" in outputs else None)
    p = {k: None if k in null else _ptr(v) for k, v in t.items()}
    rc = lib.eae_change_variates(_stream(), *head, p["mean"], p["T"], dof, _ptr(out["chi2"]), _ptr(out["prob"]), _ptr(out["var"]))
    torch.cuda.synchronize()
    del keep
    return (rc,) + tuple(None if out[k] is None else out[k].cpu().numpy() for k in ("chi2", "prob", "var"))


def _check_moments(a, b, div_a, div_b, pivot, weights=None, **inv):
    """A moments call against the reference: within the bound, the count exact, S bitwise symmetric.  Returns (moments, count)."""
    c = a.shape[0]
    rc, mom, count = _c_moments(a, b, div_a, div_b, pivot, weights, **inv)
    assert rc == 0, _lib.load().eae_last_error()
    v = R.pixel_vectors(a, b, div_a, div_b)
    valid = R.valid_pixels(a, b, inv.get("nodata_a"), inv.get("rule_a", "all"), inv.get("nodata_b"), inv.get("rule_b", "all"),
                           inv.get("mask"), weights)
    ref, n, bound = R.moments_ref(v, valid, pivot, weights, R.chunk_pixels(*a.shape))
    assert count == n
    assert np.isfinite(mom).all() and (np.abs(mom - ref) <= bound).all(), float((np.abs(mom - ref) / np.maximum(bound, 1e-300)).max())
    s = mom[1 + 2 * c:].reshape(2 * c, 2 * c)
    assert np.array_equal(_bits(s), _bits(s.T.copy()))
    return mom, count


def _pivot(a, b, div_a, div_b, shift=0.0):
    with np.errstate(all="ignore"):
        v = R.pixel_vectors(a, b, div_a, div_b).astype(np.float64)
    v = np.where(np.isfinite(v), v, 0.0)
    return (v.mean(1) + shift).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("kinds", DTYPES, ids=["-".join(k) for k in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_moments_by_shape(shape, kinds):
    a, b, div_a, div_b = _pair(shape, kinds, 1)
    pivot = _pivot(a, b, div_a, div_b)
    mom, count = _check_moments(a, b, div_a, div_b, pivot)
    assert count == shape[1] * shape[2] and mom[0] == count                       # N of unit weights is exact
    w = np.random.default_rng(2).random(shape[1:]).astype(np.float32)
    _check_moments(a, b, div_a, div_b, pivot, w)


INVALID_SHAPES = [(4, 64, 64), (13, 70, 300)]


@pytest.mark.parametrize("shape", INVALID_SHAPES, ids=[str(s) for s in INVALID_SHAPES])
def test_moments_weights_zero_negative_nan(shape):
    a, b, div_a, div_b = _pair(shape, ("u16", "u8"), 3)
    rng = np.random.default_rng(4)
    w = rng.random(shape[1:]).astype(np.float32)
    pick = rng.random(shape[1:])
    w[pick < 0.1] = 0.0
    w[(pick >= 0.1) & (pick < 0.2)] = -1.0
    w[(pick >= 0.2) & (pick < 0.3)] = np.nan
    w[(pick >= 0.3) & (pick < 0.35)] = np.inf
    _, count = _check_moments(a, b, div_a, div_b, _pivot(a, b, div_a, div_b), w)
    assert count == int((pick < 0.1).sum() + (pick >= 0.35).sum())                # a zero weight leaves the pixel valid


@pytest.mark.parametrize("rule", ["all", "any"])
@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("shape", INVALID_SHAPES, ids=[str(s) for s in INVALID_SHAPES])
def test_moments_nodata(shape, side, rule):
    a, b, div_a, div_b = _pair(shape, ("u16", "u8"), 5)
    rng = np.random.default_rng(6)
    s, nd = (a, 4095) if side == "a" else (b, 0)
    s[:, rng.random(shape[1:]) < 0.1] = nd                                        # every band: fires under both rules
    s[0][rng.random(shape[1:]) < 0.1] = nd                                        # one band: fires under "any" (and "all" when C = 1)
    kw = {f"nodata_{side}": nd, f"rule_{side}": rule}
    _, count = _check_moments(a, b, div_a, div_b, _pivot(a, b, div_a, div_b), **kw)
    assert 0 < count < shape[1] * shape[2]


@pytest.mark.parametrize("shape", INVALID_SHAPES, ids=[str(s) for s in INVALID_SHAPES])
def test_moments_mask_and_nonfinite_floats(shape):
    a, b, div_a, div_b = _pair(shape, ("f32", "f32"), 7)
    rng = np.random.default_rng(8)
    mask = rng.random(shape[1:]) < 0.2
    a[1 % shape[0]][rng.random(shape[1:]) < 0.05] = np.nan
    b[0][rng.random(shape[1:]) < 0.05] = np.inf
    b[-1][rng.random(shape[1:]) < 0.05] = -np.inf
    a[:, rng.random(shape[1:]) < 0.05] = -9999.0
    pivot = _pivot(a, b, div_a, div_b)
    _check_moments(a, b, div_a, div_b, pivot, mask=mask)
    _check_moments(a, b, div_a, div_b, pivot, mask=mask, nodata_a=-9999.0, nodata_b=float("nan"), rule_b="any")
    _check_moments(a, b, div_a, div_b, pivot, np.where(mask, np.nan, 0.5).astype(np.float32))


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 67), (2, 600, 1100)], ids=str)
def test_moments_all_invalid(shape):
    a, b, div_a, div_b = _pair(shape, ("u8", "u16"), 9)
    for kw in (dict(mask=np.ones(shape[1:], dtype=bool)), dict(weights=np.full(shape[1:], -1.0, dtype=np.float32))):
        rc, mom, count = _c_moments(a, b, div_a, div_b, np.zeros(2 * shape[0]), **kw)
        assert rc == 0 and count == 0 and np.array_equal(_bits(mom), _bits(np.zeros_like(mom)))


@pytest.mark.parametrize("shape,kinds", [((3, 5, 67), ("u8", "u8")), ((16, 33, 129), ("u16", "f32")), ((2, 600, 1100), ("u16", "u16"))],
                         ids=str)
def test_moments_run_to_run(shape, kinds):
    a, b, div_a, div_b = _pair(shape, kinds, 10)
    pivot = _pivot(a, b, div_a, div_b)
    w = np.random.default_rng(11).random(shape[1:]).astype(np.float32)
    first, second = _c_moments(a, b, div_a, div_b, pivot, w), _c_moments(a, b, div_a, div_b, pivot, w)
    assert first[0] == 0 and first[2] == second[2] and np.array_equal(_bits(first[1]), _bits(second[1]))


@pytest.mark.parametrize("shape", [(4, 64, 64), (2, 600, 1100)], ids=str)
def test_moments_two_pivots_agree(shape):
    """Integer scenes, divisor 1, integer pivots: v - p is exact, so the moments about p1 convert to those about p2 exactly in
    float64 (s2 = s1 + N e, S2 = S1 + s1 e^T + e s1^T + N e e^T, e = p1 - p2) and the two calls must agree within the sum of their
    bounds, the first one's carried through the same conversion."""
    c = shape[0]
    a, b, _, _ = _pair(shape, ("u16", "u16"), 12)
    one = np.ones(c, dtype=np.float32)
    v = R.pixel_vectors(a, b).astype(np.float64)
    valid = np.ones(v.shape[1], dtype=bool)
    p1, p2 = np.rint(v.mean(1)), np.rint(v.mean(1) + 37.0)
    chunk = R.chunk_pixels(*shape)
    (rc1, m1, _), (rc2, m2, _) = _c_moments(a, b, one, one, p1), _c_moments(a, b, one, one, p2)
    assert rc1 == 0 and rc2 == 0
    _, _, b1 = R.moments_ref(v.astype(np.float32), valid, p1, None, chunk)
    _, _, b2 = R.moments_ref(v.astype(np.float32), valid, p2, None, chunk)
    n2, e = 2 * c, p1 - p2
    split = lambda m: (m[0], m[1:1 + n2], m[1 + n2:].reshape(n2, n2))
    (n, s, cov), (bn, bs, bc) = split(m1), split(b1)
    conv = np.concatenate([[n], s + n * e, (cov + np.outer(s, e) + np.outer(e, s) + n * np.outer(e, e)).reshape(-1)])
    ae = np.abs(e)
    cb = np.concatenate([[bn], bs + bn * ae, (bc + np.outer(bs, ae) + np.outer(ae, bs) + bn * np.outer(ae, ae)).reshape(-1)])
    assert (np.abs(conv - m2) <= cb + b2).all()


# ---------------------------------------------------------------------------------------------------- variates
def _model_for(a, b, div_a, div_b, seed):
    """(mean fp32 [2C], T fp32 [2C, C]): variates of order 1 for these scenes."""
    c = a.shape[0]
    with np.errstate(all="ignore"):
        v = R.pixel_vectors(a, b, div_a, div_b).astype(np.float64)
    v = np.where(np.isfinite(v), v, 0.0)
    t = np.random.default_rng(seed).standard_normal((2 * c, c)) / (np.sqrt(2 * c) * (v.std(1)[:, None] + 1e-3))
    return v.mean(1).astype(np.float32), t.astype(np.float32)


def _check_variates(got, ref, dof):
    rc, chi2, prob, var = got
    m, z, _, bm, bz = ref
    assert rc == 0
    valid = ~np.isnan(z)
    if var is not None:
        var = var.reshape(m.shape)
        assert np.isnan(var[:, ~valid]).all() and (np.abs(var[:, valid] - m[:, valid]) <= bm[:, valid]).all()
    if chi2 is not None:
        chi2 = chi2.reshape(-1)
        assert np.isnan(chi2[~valid]).all() and (np.abs(chi2[valid] - z[valid]) <= bz[valid]).all()
    if prob is not None:
        prob = prob.reshape(-1)
        assert (prob[~valid] == 0).all()
        if chi2 is not None:
            zk = chi2[valid].astype(np.float64)
            assert (np.abs(prob[valid] - R.chi2_sf(dof, zk)) <= R.prob_bound(dof, zk)).all()
            assert (prob[valid] >= 0).all() and (prob[valid] <= 1 + 2.0 ** -20).all()


@pytest.mark.parametrize("kinds", DTYPES, ids=["-".join(k) for k in DTYPES])
@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_variates_by_shape(shape, kinds):
    c = shape[0]
    a, b, div_a, div_b = _pair(shape, kinds, 13)
    rng = np.random.default_rng(14)
    mask = rng.random(shape[1:]) < 0.1
    inv = dict(mask=mask)
    if kinds[0] == "f32":
        a[0][rng.random(shape[1:]) < 0.05] = np.nan
        b[-1][rng.random(shape[1:]) < 0.05] = np.inf
    else:
        a[:, rng.random(shape[1:]) < 0.05] = 17
        inv.update(nodata_a=17, rule_a="all")
    mean, tm = _model_for(a, b, div_a, div_b, 15)
    valid = R.valid_pixels(a, b, inv.get("nodata_a"), "all", None, "all", mask)
    ref = R.variates_ref(R.pixel_vectors(a, b, div_a, div_b), valid, mean, tm, c)
    _check_variates(_c_variates(a, b, div_a, div_b, mean, tm, c, **inv), ref, c)


@pytest.mark.parametrize("dof", range(1, 17))
def test_prob_for_every_dof(dof):
    """One band: T = [[1], [0]] and a zero mean make chi2 = a^2 exactly where a^2 is an fp32 number, so the closed form is driven over
    0 .. 300 (past the cut at 256), through tiny values and up to an overflowing square."""
    r = np.sqrt(np.concatenate([np.linspace(0.0, 300.0, 3000), [1e-30, 1e-12, 1e-6, 255.99, 256.0, 256.01, 1e4]]))
    a = np.concatenate([r, [1e30]]).astype(np.float32).reshape(1, 1, -1)
    b = np.zeros_like(a)
    one = np.ones(1, dtype=np.float32)
    rc, chi2, prob, _ = _c_variates(a, b, one, one, np.zeros(2), np.array([[1.0], [0.0]]), dof, outputs=("chi2", "prob"))
    assert rc == 0
    z = chi2.reshape(-1).astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(chi2.reshape(-1), (a * a).reshape(-1)) and np.isinf(z[-1])
    assert (np.abs(prob.reshape(-1) - R.chi2_sf(dof, z)) <= R.prob_bound(dof, np.minimum(z, 1e300))).all()
    assert prob.reshape(-1)[0] == 1.0 and (prob.reshape(-1)[z > 256.0] == 0.0).all()


@pytest.mark.parametrize("shape,kinds", [((3, 5, 67), ("u8", "u16")), ((13, 70, 300), ("f32", "f32"))], ids=str)
def test_variates_outputs_in_turn(shape, kinds):
    c = shape[0]
    a, b, div_a, div_b = _pair(shape, kinds, 16)
    mask = np.random.default_rng(17).random(shape[1:]) < 0.1
    mean, tm = _model_for(a, b, div_a, div_b, 18)
    full = _c_variates(a, b, div_a, div_b, mean, tm, c, mask=mask)
    assert full[0] == 0
    for outputs in (("chi2",), ("prob",), ("var",), ("chi2", "var"), ("prob", "var"), ()):
        got = _c_variates(a, b, div_a, div_b, mean, tm, c, mask=mask, outputs=outputs)
        assert got[0] == 0
        for name, x, y in zip(("chi2", "prob", "var"), got[1:], full[1:]):
            assert (x is None) == (name not in outputs)
            assert x is None or np.array_equal(_bits(x), _bits(y))               # NaN equals itself


# ---------------------------------------------------------------------------------------------------- error codes
def test_error_codes():
    lib = _lib.load()
    shape = (3, 5, 67)
    a, b, div_a, div_b = _pair(shape, ("u8", "u16"), 19)
    pivot = np.zeros(6)
    need = lib.eae_change_moments_workspace_bytes(*shape)
    mean, tm = _model_for(a, b, div_a, div_b, 20)

    def bad(rc, word):
        assert rc == -2 and word.encode() in lib.eae_last_error(), (rc, lib.eae_last_error())

    for c in (0, 17):
        bad(lib.eae_change_moments_workspace_bytes(c, 5, 67), "bands")
        bad(_c_moments(a, b, div_a, div_b, pivot, shape=(c, 5, 67))[0], "bands")
        bad(_c_variates(a, b, div_a, div_b, mean, tm, 3, shape=(c, 5, 67))[0], "bands")
    for h, w in ((65536, 32768), (0, 67), (5, -1)):
        word = "2^31" if h > 0 and w > 0 else "empty"
        bad(lib.eae_change_moments_workspace_bytes(3, h, w), word)
        bad(_c_moments(a, b, div_a, div_b, pivot, shape=(3, h, w))[0], word)
        bad(_c_variates(a, b, div_a, div_b, mean, tm, 3, shape=(3, h, w))[0], word)
    bad(_c_moments(a, b, div_a, div_b, pivot, ws_bytes=need - 1)[0], "workspace")
    bad(_c_moments(a, b, div_a, div_b, pivot, ws_null=True)[0], "workspace")
    for name in ("a", "b", "div_a", "div_b", "pivot", "out", "count"):
        rc, mom, count = _c_moments(a, b, div_a, div_b, pivot, null=(name,))
        bad(rc, "NULL")
        assert (mom == POISON).all() and count == int(POISON)                     # nothing was launched
    for name in ("a", "b", "div_a", "div_b", "mean", "T"):
        rc, chi2, prob, var = _c_variates(a, b, div_a, div_b, mean, tm, 3, null=(name,))
        bad(rc, "NULL")
        assert (chi2 == POISON).all() and (prob == POISON).all() and (var == POISON).all()
    for dof in (0, 17):
        bad(_c_variates(a, b, div_a, div_b, mean, tm, dof)[0], "dof")
    bad(_c_moments(a, b, div_a, div_b, pivot, nodata_a=256)[0], "nodata")
    bad(_c_moments(a, b, div_a, div_b, pivot, nodata_b=float("nan"))[0], "NaN nodata")
    bad(_c_variates(a, b, div_a, div_b, mean, tm, 3, nodata_b=65536)[0], "nodata")
    head = _head(a, b, div_a, div_b, None, "all", None, "all", None)
    args = list(head[1])
    args[2] = 3                                                                    # no such dtype
    out = torch.zeros(64, dtype=torch.float64, device="cuda")
    bad(lib.eae_change_variates(_stream(), *args, _ptr(out), _ptr(out), 3, _ptr(out), None, None), "dtype")
    args[2], args[11] = 0, 2                                                       # no such rule (scene a)
    bad(lib.eae_change_variates(_stream(), *args, _ptr(out), _ptr(out), 3, _ptr(out), None, None), "rule")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the Python layer
def _planted_dev(seed, dtype):
    a, b, changed = R.planted(seed, dtype)
    return a, b, changed, torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()


def test_joint_moments_mean_and_pivot():
    a, b, _, ta, tb = _planted_dev(1, np.uint16)
    v = R.pixel_vectors(a, b).astype(np.float64)
    auto = eae_amd.joint_moments(ta, tb)
    far = eae_amd.joint_moments(ta, tb, pivot=v.mean(1) + 200.0)
    assert auto.n == auto.count == far.count == 96 * 96
    mean, cov = v.mean(1), np.cov(v, bias=True)
    # |d| <= reach = 4000 for both pivots (values up to about 3600, pivots inside the data or 200 above its mean).  s / N is then
    # within (chunk + 2) 2^-24 reach, S / N within (chunk + 2) 2^-24 reach^2, and (s / N)(s / N)^T within twice that: 3 in all
    unit = (R.chunk_pixels(4, 96, 96) + 2) * R.U
    for m in (auto, far):
        assert np.abs(m.mean - mean).max() <= unit * 4000.0
        assert np.array_equal(m.cov, m.cov.T)
        assert np.abs(m.cov - cov).max() <= 3 * unit * 4000.0 ** 2
    assert np.abs(auto.cov - far.cov).max() <= 6 * unit * 4000.0 ** 2             # the pivot matters no more than rounding
    empty = eae_amd.joint_moments(ta, tb, mask=torch.ones((96, 96), dtype=torch.bool, device="cuda"))
    assert empty.n == 0 and empty.count == 0 and np.isnan(empty.mean).all()


RHO_BOUND = 2.0 ** -19           # 8 x 1.458e-07 = 1.17e-06, rounded up to a power of two
CHI2_BOUND = 2.0 ** -11          # 8 x 4.330e-05 = 3.46e-04, rounded up to a power of two


def test_mad_fit_against_reference():
    """`mad_fit(tol=0, max_iter=5)` on planted(0, uint16) against the float64 `irmad_ref`: max |rho - rho_ref| over the five
    iterations, and max |chi2 - chi2_ref| / max(chi2_ref, 1) of `mad_transform` under the final model.  Measured on the first run on
    an MI355X: 1.458e-07 and 4.330e-05 (max |prob - prob_ref| 1.405e-05); the bounds are 8 x that, rounded up to a power of two: 2^-19
    and 2^-11.  A |d rho| above 1e-3 would be a defect to find, not a tolerance to adopt."""
    a, b, _, ta, tb = _planted_dev(0, np.uint16)
    model = eae_amd.mad_fit(ta, tb, tol=0.0, max_iter=5)
    history, z, prob, _ = R.irmad_ref(a, b, 5)
    assert model.iterations == 5 and len(model.history) == 5
    d_rho = max(float(np.abs(h - r).max()) for h, r in zip(model.history, history))
    chi2, gp, var = eae_amd.mad_transform(ta, tb, model, variates=True)
    chi2 = chi2.cpu().numpy().reshape(-1).astype(np.float64)
    d_chi2 = float((np.abs(chi2 - z) / np.maximum(z, 1.0)).max())
    d_prob = float(np.abs(gp.cpu().numpy().reshape(-1) - prob).max())
    print(f"mad_fit measured: max |d rho| = {d_rho:.3e}, max rel d chi2 = {d_chi2:.3e}, max |d prob| = {d_prob:.3e}")
    assert var.shape == (4, 96, 96) and np.array_equal(model.rho, model.history[-1])
    assert d_rho <= RHO_BOUND
    assert d_chi2 <= CHI2_BOUND
    # max_iter = 1 is plain MAD: the first iteration's rho
    plain = eae_amd.mad_fit(ta, tb, max_iter=1)
    assert plain.iterations == 1 and np.array_equal(plain.rho, model.history[0])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("seed", range(5))
def test_detect_change_finds_the_planted_block(seed, dtype):
    a, b, changed, ta, tb = _planted_dev(seed, dtype)
    res = eae_amd.detect_change(ta, tb, max_iter=10, tol=0.0, alpha=0.01)
    change = res.change.cpu().numpy()
    assert change.dtype == bool and res.model.iterations == 10 and res.scale > 1.0
    assert change[changed].mean() >= 0.99
    assert change[~changed].mean() <= 0.02
    raw = eae_amd.detect_change(ta, tb, max_iter=10, tol=0.0, alpha=0.01, calibrate=False)
    assert raw.scale == 1.0 and raw.change.cpu().numpy()[~changed].mean() > 0.2   # why the calibration exists
    assert torch.equal(raw.chi2, res.chi2)


GAIN_BOUND = 2.0 ** -24          # 8 x 6.704e-09 = 5.36e-08, rounded up to a power of two
OFFSET_BOUND = 2.0 ** -13        # 8 x 1.391e-05 = 1.11e-04, rounded up to a power of two


def test_invariant_regression_against_reference():
    """gain and offset of planted(0, uint16) from the pixels with prob > 0.95 against the float64 `orthogonal_regression_ref` over
    the same pixels (62 of them).  Measured on the first run on an MI355X: max |d gain| = 6.704e-09, max |d offset| = 1.391e-05; the
    bounds are 8 x that, rounded up to a power of two: 2^-24 and 2^-13."""
    a, b, _, ta, tb = _planted_dev(0, np.uint16)
    res = eae_amd.detect_change(ta, tb, max_iter=10, tol=0.0)
    gain, offset, count = eae_amd.invariant_regression(ta, tb, res.prob)
    sel = res.prob.cpu().numpy() > 0.95
    assert count == int(sel.sum()) and count >= 30
    ref = np.array([R.orthogonal_regression_ref(a[c][sel].astype(np.float64), b[c][sel].astype(np.float64)) for c in range(4)])
    d_gain, d_off = float(np.abs(gain - ref[:, 0]).max()), float(np.abs(offset - ref[:, 1]).max())
    print(f"invariant_regression measured: max |d gain| = {d_gain:.3e}, max |d offset| = {d_off:.3e}; gain {gain}, offset {offset}, "
          f"count {count}")
    assert d_gain <= GAIN_BOUND and d_off <= OFFSET_BOUND
    # the planted line, loosely: B's noise (sigma 15; the selection's bands spread by 100 or more) biases a total-least-squares slope
    # by up to gain * 15^2 / var(x) <= 0.0225, the few dozen selected pixels add a sampling error of about 15 / (100 sqrt(30)) =
    # 0.027, and the offset moves by the slope's error times the mean (about 2000)
    assert np.abs(gain - R.GAINS).max() <= 0.05 and np.abs(offset - (100.0 + 30.0 * np.arange(4))).max() <= 100.0


def test_class_transitions_equal_bincount():
    rng = np.random.default_rng(21)
    k, shape = 5, (37, 53)
    ma, mb = rng.integers(-1, k + 1, shape), rng.integers(-1, k + 1, shape)
    mask = rng.random(shape) < 0.2
    ra, rb = np.where((ma >= 0) & (ma < k), ma, k), np.where((mb >= 0) & (mb < k), mb, k)
    for dt in (torch.int64, torch.int32, torch.uint8):
        src = np.where(ma < 0, k, ma) if dt == torch.uint8 else ma
        got = eae_amd.class_transitions(torch.from_numpy(src).to(dt).cuda(), torch.from_numpy(mb).cuda(), k,
                                        mask=torch.from_numpy(mask).cuda())
        want = np.bincount((ra * (k + 1) + rb)[~mask], minlength=(k + 1) ** 2).reshape(k + 1, k + 1)
        assert np.array_equal(got.cpu().numpy(), want)
    got = eae_amd.class_transitions(torch.from_numpy(ma).cuda(), torch.from_numpy(mb).cuda(), k, ignore=2)
    ri = np.where(ra == 2, k, ra)
    assert np.array_equal(got.cpu().numpy(), np.bincount((ri * (k + 1) + rb).ravel(), minlength=(k + 1) ** 2).reshape(k + 1, k + 1))
