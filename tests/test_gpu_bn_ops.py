"""The stand-alone BatchNorm finalize kernels (eae_misc.hip: bn_finalize_kernel, bn_eval_coef_kernel, bn_bwd_finalize_kernel)
through eae_op_bn_finalize / eae_op_bn_eval_coef / eae_op_bn_bwd_finalize.  The default train step folds these finalizes into
the conv kernels; the stand-alone ones run in eval mode and under EAE_NO_FOLD_FWD / EAE_NO_FOLD_BWD, which the suite
otherwise never enters.

The partial sums come from a real y [N][C] cut into `ntiles` unequal row chunks (tests/ops_ref.py) and the fp64 reference is
given the SAME fp32 partials, so what is left is the kernel's own arithmetic: an fp64 reduction (order-dependent at the 1e-16
level) and fewer than ten fp32 operations per coefficient.

Bounds, in units of u = 2^-23 (the largest relative spacing of fp32; a correctly rounded operation errs by at most 0.5 u; sqrtf
and the division need not be correctly rounded: up to 3 u and 2.5 u, the limits of the fast forms):
  mean     (float) of the fp64 mean: 0.5 u                                                               -> 1 u |mean|
  invstd   1 / sqrtf((float)var + eps): the conversion and the sum give 0.5 u each on the radicand, halved by the inverse
           square root (0.5 u), sqrtf 3 u, division 2.5 u: 6 u                                              -> 8 u |invstd|
  s        gamma * invstd: 6.5 u                                                                         -> 8 u |s|
  t        beta - (float)mean * s: the product carries 0.5 + 6.5 + 0.5 = 7.5 u of |mean * s|, the difference adds 0.5 u of
           at most |beta| + |mean * s|                                                                  -> 8 u (|beta| + |mean*s|)
  running  (1 - m) * r + m * (float)stat: 1 - m, two products, one conversion, one sum: at most 2.5 u on either term
                                                                                                        -> 4 u (|(1-m) r| + |m stat|)
  dgamma / dbeta   one rounding of the fp64 sum (half an fp32 ulp) plus the order of the fp64 reduction  -> 2^-24 |ref| + 1e-13 sum|partials|
  A        gamma * invstd from fp32 inputs: 0.5 u                                                        -> 1 u |A|
  B        -A * invstd * dgamma / count: 0.5 (A) + 0.5 + 0.5 (dgamma) + 0.5 + 2.5 (division) = 4.5 u        -> 6 u |B|
  C        -A * dbeta / count - B * mean: 4 u of the first term, 5 u of the second, 0.5 u of the difference -> 8 u (|A dbeta / count| + |B mean|)
Largest errors observed on an MI355X over all cases of this module, same units (every check prints its figure as a
`BNERR <coefficient> <multiple of u>` line, pytest -s): mean 0.50, invstd 0.98, s 1.30, t 1.52, running mean / var 0.99 / 0.99;
A 0.49, B 1.42, C 1.28; eval coefficients invstd 0.73, s 1.07, t 1.09; composed dy 3.10 (bound 16); dgamma / dbeta never above
half an ulp."""
import numpy as np
import pytest
import torch

import ops_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
MOM, EPS = float(np.float32(0.1)), float(np.float32(1e-5))      # the values the kernels receive (C floats)
GUARD = 16
WIDTHS = (32, 64, 128, 256)
NTILES = (1, 5, 255, 256, 257, 1000)       # the 256-thread stride loop: below, at and above one round, and several rounds with a tail

# multiples of u (derivation above)                   largest observed on MI355X
K_MEAN, K_INVSTD, K_S, K_T, K_RUN = 1, 8, 8, 8, 4      # 0.50, 0.98, 1.30, 1.52, 0.99
K_A, K_B, K_C = 1, 6, 8                                 # 0.49, 1.42, 1.28


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _worst(name, err, scale):
    """largest err / (u * scale) over the channels (what the K_* multiples bound); printed for the record"""
    r = float((np.abs(err) / np.maximum(U * np.abs(scale), 1e-300)).max())
    print(f"BNERR {name} {r:.3f}")
    return r


def _nanbuf(n):
    import gpu_util as G
    return torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=G.dev())


def _guarded(init):
    """device copy of a host vector followed by GUARD NaNs"""
    t = _nanbuf(len(init))
    t[:len(init)] = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).to(t.device)
    return t


def _split(t, n):
    a = t.cpu().numpy()
    assert np.isnan(a[n:]).all(), "guard behind the logical end was written"
    assert np.isfinite(a[:n]).all(), "an output element was not written (or is not finite)"
    return a[:n].astype(np.float64)


def _data(C, ntiles, seed):
    rng = np.random.default_rng(seed)
    n = 2 * ntiles + 3
    y = (rng.standard_normal((n, C)) * rng.uniform(0.3, 3.0, C) + rng.uniform(-2.0, 2.0, C)).astype(np.float32)
    g = (rng.standard_normal((n, C)) * rng.uniform(0.1, 1.0, C)).astype(np.float32)
    p = {"gamma": rng.uniform(0.5, 1.5, C), "beta": rng.standard_normal(C) * 0.3,
         "rm": rng.standard_normal(C) * 0.5, "rv": rng.uniform(0.3, 3.0, C)}
    p = {k: v.astype(np.float32) for k, v in p.items()}
    return rng, n, y, g, p, R.splits_for(n, ntiles, rng)


def _finalize(lib, part, count, p, running=True, nbt0=41):
    """eae_op_bn_finalize on NaN-filled / guarded buffers -> coef [4][C] (fp64 view), running mean / var, nbt"""
    import gpu_util as G
    from eae_amd._lib import check
    _, C, nt = part.shape
    pd, gd, bd = G.f32(part), G.f32(p["gamma"]), G.f32(p["beta"])
    coef = _nanbuf(4 * C)
    rm, rv = _guarded(p["rm"]), _guarded(p["rv"])
    nbt = torch.tensor([nbt0, -5], dtype=torch.int64, device=G.dev())
    check(lib.eae_op_bn_finalize(G.stream(), G.ptr(pd), nt, C, count, G.ptr(gd), G.ptr(bd), G.ptr(rm) if running else None,
                                 G.ptr(rv) if running else None, G.ptr(nbt) if running else None, MOM, EPS, G.ptr(coef)))
    torch.cuda.synchronize()
    return _split(coef, 4 * C).reshape(4, C), _split(rm, C), _split(rv, C), nbt.cpu().numpy()


def _check_fwd_coef(coef, ref, p, tag):
    beta = p["beta"].astype(np.float64)
    e = [_worst(tag + "mean", coef[2] - ref["mean"], ref["mean"]), _worst(tag + "invstd", coef[3] - ref["invstd"], ref["invstd"]),
         _worst(tag + "s", coef[0] - ref["s"], ref["s"]), _worst(tag + "t", coef[1] - ref["t"], np.abs(beta) + np.abs(ref["mean"] * ref["s"]))]
    assert e[0] <= K_MEAN and e[1] <= K_INVSTD and e[2] <= K_S and e[3] <= K_T, e


def _check_running(rm, rv, ref, p, count, tag):
    unb = ref["var"] * (count / (count - 1.0)) if count > 1 else ref["var"]
    e = [_worst(tag + "running_mean", rm - ref["running_mean"], np.abs((1 - MOM) * p["rm"]) + np.abs(MOM * ref["mean"])),
         _worst(tag + "running_var", rv - ref["running_var"], np.abs((1 - MOM) * p["rv"]) + np.abs(MOM * unb))]
    assert max(e) <= K_RUN, e


@pytest.mark.parametrize("ntiles", NTILES)
@pytest.mark.parametrize("C", WIDTHS)
def test_bn_finalize(lib, C, ntiles):
    rng, n, y, g, p, sp = _data(C, ntiles, 1000 * C + ntiles)
    part = R.partials(y, sp)
    mean, var = R.moments_from_partials(part, n)
    ref = R.bn_from_moments(mean, var, n, p["gamma"], p["beta"], p["rm"], p["rv"], MOM, EPS)
    coef, rm, rv, nbt = _finalize(lib, part, n, p)
    _check_fwd_coef(coef, ref, p, "fin ")
    _check_running(rm, rv, ref, p, n, "fin ")
    assert nbt.tolist() == [42, -5]
    # without running statistics: the same coefficients, nothing else touched
    coef2, rm2, rv2, nbt2 = _finalize(lib, part, n, p, running=False)
    assert np.array_equal(coef2, coef)
    assert np.array_equal(rm2, p["rm"].astype(np.float64)) and np.array_equal(rv2, p["rv"].astype(np.float64)) and nbt2.tolist() == [41, -5]


def test_bn_finalize_edge_channels(lib):
    """In one call: channel 0 constant (its variance from the fp32 partials comes out NEGATIVE in fp64: the clamp must give
    invstd = 1/sqrt(eps)), channel 1 with mean 100 and std 0.5 (the cancellation in E[y^2] - mean^2 has to happen in fp64).
    Then count = 1: one element per channel, biased variance into the running variance."""
    C, ntiles = 32, 5
    rng, n, y, g, p, sp = _data(C, ntiles, 77)
    n = 700
    y = (rng.standard_normal((n, C)) + 0.5).astype(np.float32)
    sp = R.splits_for(n, ntiles, rng)
    y[:, 1] = (100.0 + 0.5 * rng.standard_normal(n)).astype(np.float32)
    for const in (0.1, 0.3, 0.7, 1.1, 1.3, 3.3, 5.7, 9.9):      # the first constant whose rounded partials give a negative variance
        y[:, 0] = np.float32(const)
        part = R.partials(y, sp)
        raw = part.astype(np.float64).sum(2)
        if raw[1, 0] / n - (raw[0, 0] / n) ** 2 < 0:
            break
    else:
        raise AssertionError("no constant with a negative raw variance: the case does not reach the clamp")
    mean, var = R.moments_from_partials(part, n)
    assert var[0] == 0.0 and abs(var[1] - 0.25) < 0.05
    ref = R.bn_from_moments(mean, var, n, p["gamma"], p["beta"], p["rm"], p["rv"], MOM, EPS)
    coef, rm, rv, nbt = _finalize(lib, part, n, p)
    _check_fwd_coef(coef, ref, p, "edge ")
    _check_running(rm, rv, ref, p, n, "edge ")
    assert abs(coef[3, 0] - 1.0 / np.sqrt(EPS)) <= K_INVSTD * U / np.sqrt(EPS)
    # count = 1
    y1 = y[:1]
    part1 = R.partials(y1, np.zeros(1, np.int64))
    mean1, var1 = R.moments_from_partials(part1, 1)
    ref1 = R.bn_from_moments(mean1, var1, 1, p["gamma"], p["beta"], p["rm"], p["rv"], MOM, EPS)
    coef, rm, rv, nbt = _finalize(lib, part1, 1, p)
    _check_fwd_coef(coef, ref1, p, "count1 ")
    _check_running(rm, rv, ref1, p, 1, "count1 ")
    assert nbt.tolist() == [42, -5]


def _bwd_finalize(lib, part, count, gamma, coef_fwd, want_grads=True):
    import gpu_util as G
    from eae_amd._lib import check
    _, C, nt = part.shape
    pd, gd, cf = G.f32(part), G.f32(gamma), G.f32(coef_fwd)
    dg, db, cb = _nanbuf(C), _nanbuf(C), _nanbuf(3 * C)
    check(lib.eae_op_bn_bwd_finalize(G.stream(), G.ptr(pd), nt, C, count, G.ptr(gd), G.ptr(cf), G.ptr(dg) if want_grads else None,
                                     G.ptr(db) if want_grads else None, G.ptr(cb)))
    torch.cuda.synchronize()
    if not want_grads:
        assert np.isnan(dg.cpu().numpy()).all() and np.isnan(db.cpu().numpy()).all()
        return None, None, _split(cb, 3 * C).reshape(3, C)
    return _split(dg, C), _split(db, C), _split(cb, 3 * C).reshape(3, C)


def _fwd_coef32(y, p):
    """[4][C] fp32 forward coefficients (s, t, mean, invstd) of y, as the forward finalize would leave them"""
    r = R.bn_train_ref(y, p["gamma"], p["beta"], None, None, MOM, EPS)
    return np.stack([r["s"], r["t"], r["mean"], r["invstd"]]).astype(np.float32)


def _check_bwd_coef(cb, part, count, gamma, cf, tag):
    sums = part.astype(np.float64).sum(2)
    # the kernel rounds the two sums to fp32 (they are its dgamma / dbeta outputs) before it forms B and C
    db32, dg32 = sums[0].astype(np.float32), sums[1].astype(np.float32)
    A, B, Cc = R.bn_bwd_coef_ref(db32, dg32, count, gamma, cf[2], cf[3])
    e = [_worst(tag + "A", cb[0] - A, A), _worst(tag + "B", cb[1] - B, B),
         _worst(tag + "C", cb[2] - Cc, np.abs(A * db32.astype(np.float64) / count) + np.abs(B * cf[2].astype(np.float64)))]
    assert e[0] <= K_A and e[1] <= K_B and e[2] <= K_C, e
    return A, B, Cc


@pytest.mark.parametrize("ntiles", NTILES)
@pytest.mark.parametrize("C", WIDTHS)
def test_bn_bwd_finalize(lib, C, ntiles):
    rng, n, y, g, p, sp = _data(C, ntiles, 2000 * C + ntiles)
    cf = _fwd_coef32(y, p)
    xhat = (y.astype(np.float64) - cf[2].astype(np.float64)) * cf[3].astype(np.float64)
    part = R.partials2(g, g.astype(np.float64) * xhat, sp)
    dg, db, cb = _bwd_finalize(lib, part, n, p["gamma"], cf)
    sums, asum = part.astype(np.float64).sum(2), np.abs(part.astype(np.float64)).sum(2)
    # one fp32 rounding of the fp64 sum (+ the order of the fp64 reduction)
    assert (np.abs(db - sums[0]) <= 2.0 ** -24 * np.abs(sums[0]) + 1e-13 * asum[0]).all()
    assert (np.abs(dg - sums[1]) <= 2.0 ** -24 * np.abs(sums[1]) + 1e-13 * asum[1]).all()
    _check_bwd_coef(cb, part, n, p["gamma"], cf, "bwd ")
    # without dgamma / dbeta: the same coefficients
    _, _, cb2 = _bwd_finalize(lib, part, n, p["gamma"], cf, want_grads=False)
    assert np.array_equal(cb2, cb)


@pytest.mark.parametrize("C", WIDTHS)
def test_bn_bwd_finalize_eval_count(lib, C):
    """count = 2^40 is how the eval-mode backward asks for dy = A*g alone: B and C must vanish against A."""
    rng, n, y, g, p, sp = _data(C, 5, 3000 + C)
    cf = _fwd_coef32(y, p)
    xhat = (y.astype(np.float64) - cf[2].astype(np.float64)) * cf[3].astype(np.float64)
    part = R.partials2(g, g.astype(np.float64) * xhat, sp)
    dg, db, cb = _bwd_finalize(lib, part, 1 << 40, p["gamma"], cf)
    A, B, Cc = _check_bwd_coef(cb, part, float(1 << 40), p["gamma"], cf, "eval ")
    assert (np.abs(cb[1]) * np.abs(y).max(0) + np.abs(cb[2]) <= 2.0 ** -24 * np.abs(cb[0]) * np.abs(g).max(0)).all()


@pytest.mark.parametrize("C", WIDTHS)
def test_bn_forward_then_backward_finalize_gives_the_input_gradient(lib, C):
    """finalize -> backward finalize on one y, g; dy = A*g + B*y + C evaluated in fp64 from the KERNELS' coefficients against the
    exact BatchNorm input gradient.  Beyond the coefficient bounds above (at most 8 u each) the statistics now come from fp32
    partials while the reference's come from y itself: each partial is rounded once (0.5 u), which moves mean, invstd, dbeta / N and
    dgamma / N by at most ~1 u of the sums of magnitudes they are made of; they enter dy linearly.  Bound: 16 u of the
    largest |A g| + |B y| + |C| of the channel (with mean and std of order 1, as here, the sums of magnitudes are of that size)."""
    rng, n, y, g, p, sp = _data(C, 13, 4000 + C)
    part = R.partials(y, sp)
    coef, _, _, _ = _finalize(lib, part, n, p)
    cf = coef.astype(np.float32)
    xhat = (y.astype(np.float64) - coef[2]) * coef[3]
    partb = R.partials2(g, g.astype(np.float64) * xhat, sp)
    dg, db, cb = _bwd_finalize(lib, partb, n, p["gamma"], cf)
    g64, y64 = g.astype(np.float64), y.astype(np.float64)
    got = cb[0] * g64 + cb[1] * y64 + cb[2]
    exact = R.bn_train_ref(y, p["gamma"], p["beta"], None, None, MOM, EPS)
    ref = R.bn_bwd_ref(g, y, p["gamma"], exact["mean"], exact["invstd"])
    scale = (np.abs(cb[0] * g64) + np.abs(cb[1] * y64) + np.abs(cb[2])).max(0)
    e = _worst("composed dy", np.abs(got - ref["dy"]).max(0), scale)
    assert e <= 16, e                                                                       # observed on MI355X: 3.10
    assert (np.abs(dg - ref["dgamma"]) <= 16 * U * np.abs(g64 * ref["xhat"]).sum(0)).all()
    assert (np.abs(db - ref["dbeta"]) <= 16 * U * np.abs(g64).sum(0)).all()


@pytest.mark.parametrize("C", WIDTHS + (3, 100))
def test_bn_eval_coef(lib, C):
    """64 threads per block: C = 3 and C = 100 end inside a block (the tail guard).  invstd = 1 / sqrtf(rv + eps): 0.5 u of the sum
    halved, sqrtf 3 u, division 2.5 u -> within the 8 u of the training form; s and t as there; the mean is copied."""
    import gpu_util as G
    from eae_amd._lib import check
    rng, n, y, g, p, sp = _data(C, 1, 5000 + C)
    coef = _nanbuf(4 * C)
    d = [G.f32(p[k]) for k in ("gamma", "beta", "rm", "rv")]
    check(lib.eae_op_bn_eval_coef(G.stream(), C, *[G.ptr(t) for t in d], EPS, G.ptr(coef)))
    torch.cuda.synchronize()
    got = _split(coef, 4 * C).reshape(4, C)
    ref = R.bn_eval_ref(p["gamma"], p["beta"], p["rm"], p["rv"], EPS)
    assert np.array_equal(got[2], p["rm"].astype(np.float64))
    e = [_worst("eval invstd", got[3] - ref["invstd"], ref["invstd"]), _worst("eval s", got[0] - ref["s"], ref["s"]),
         _worst("eval t", got[1] - ref["t"], np.abs(p["beta"].astype(np.float64)) + np.abs(ref["mean"] * ref["s"]))]
    assert e[0] <= K_INVSTD and e[1] <= K_S and e[2] <= K_T, e                              # observed on MI355X: 0.73, 1.07, 1.09
