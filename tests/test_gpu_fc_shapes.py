"""The latent-projection kernels (eae_fc.hip.h) by shape, through eae_op_fc_splitk / eae_op_fc_bias_bf16 / eae_op_fc_wgrad.

test_gpu_ops.py::test_fc_ops runs them at B = 37, L = 64, Pn = 16 only.  Here: a second M tile and M = 1, N up to 256, more
than 64 K-slices in the split-K reduction (its `k0 += 64` loop takes a second and a partial third round), the raw source with an
addend (dec.fc backward-data), up to six 64-row batch chunks in the weight-gradient kernel (its register ring of four is re-issued
from the fifth chunk on) and Pn = 64 (the 4-position column tiles of the enc.fc weight gradient).

Operands are exact bf16 values; the reference is O.linear_fwd / O.linear_bwd in fp64 on the same rounded values.  Layouts and
packing as in test_fc_ops: activations NHWC-flattened (k' = p*256 + c), weights permuted to match.  Every output is NaN-filled with
guard rows behind its end: it must be finite afterwards (each element written) and the guard still NaN (no row past the end).
Bounds: fp32 outputs from exact operands relmax < 1e-4 (test_wgrad_instantiation's bound for exact operands); BN+ReLU operands
2e-3 / 3e-3 / 1e-2 (test_fc_ops: the kernel's fp32 fma can land one bf16 ulp from the NumPy value); bf16 outputs
2^-7 * max|ref| + 1e-3."""
import numpy as np
import pytest
import torch

from oracle import ae_numpy as O

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float("nan")
HW = {16: (4, 4), 64: (8, 8), 80: (8, 10)}       # Pn -> map of 256 channels


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _bf(rng, shape, scale=1.0):
    return O.bf16_round((rng.standard_normal(shape) * scale).astype(np.float32))


def _raw_src(rng, M, Pn):
    """bf16 tensor [M][256][h][w] as stored (source mode 0) -> (eae_src, keep-alive, value [M][K] in the reference's c*Pn+p order)"""
    import gpu_util as G
    x = _bf(rng, (M, 256) + HW[Pn])
    d = G.to_nhwc_bf16(x)
    return G.src(0, d), [d], x.reshape(M, 256 * Pn).astype(np.float64)


def _bnrelu_src(rng, M, Pn):
    """source mode 1: relu(s*y + t) in fp32 (one fma), rounded to bf16 on load"""
    import gpu_util as G
    y = _bf(rng, (M, 256) + HW[Pn])
    s = (1.0 + 0.1 * rng.standard_normal(256)).astype(np.float32); t = (0.1 * rng.standard_normal(256)).astype(np.float32)
    coef = np.stack([s, t, np.zeros(256, np.float32), np.ones(256, np.float32)])
    d, cd = G.to_nhwc_bf16(y), G.f32(coef)
    pre = (y.astype(np.float64) * s[None, :, None, None] + t[None, :, None, None]).astype(np.float32)
    act = O.bf16_round(np.maximum(pre, 0.0))
    return G.src(1, d, None, cd), [d, cd], act.reshape(M, 256 * Pn).astype(np.float64)


def _pack_cols(w_ref, Pn):
    """[R][K] with k = c*Pn + p -> k' = p*256 + c"""
    r = w_ref.shape[0]
    return np.ascontiguousarray(w_ref.reshape(r, 256, Pn).transpose(0, 2, 1).reshape(r, 256 * Pn))


def _pack_rows(w_ref, Pn):
    """[K][L] with k = c*Pn + p -> rows k' = p*256 + c"""
    k, l = w_ref.shape
    return np.ascontiguousarray(w_ref.reshape(256, Pn, l).transpose(1, 0, 2).reshape(k, l))


def _out(rows, cols, dtype=torch.float32):
    import gpu_util as G
    return torch.full((rows + GUARD, cols), NAN, dtype=dtype, device=G.dev())


def _take(t, rows):
    a = t.float().cpu().numpy()
    assert np.isnan(a[rows:]).all(), "rows behind the logical end were written"
    assert np.isfinite(a[:rows]).all(), "an output element was not written"
    return a[:rows].astype(np.float64)


# ---------------------------------------------------------------------------------------------------- eae_op_fc_splitk
SPLITK = ([(1, "b", m, n, 16) for m in (1, 37, 128, 129, 200) for n in (64, 256)] +           # 32 slices: M tiles and tails
          [(1, "b", 37, n, 64) for n in (64, 128, 192, 256)] +                                  # 128 slices: two full rounds of the reduction
          [(1, "b", 9, 64, 80)] +                                                               # 160 slices: a partial third round
          [(0, "a", m, n, pn) for m in (37, 129) for n in (64, 256) for pn in (16, 64)] +       # raw source + addend, no bias
          [(0, "ba", 5, 128, 16)])                                                              # bias + addend


@pytest.mark.parametrize("mode,extra,M,N,Pn", SPLITK)
def test_fc_splitk(lib, mode, extra, M, N, Pn):
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(mode * 7 + M * 1000 + N + Pn * 100003)
    K = 256 * Pn
    src, keep, a = (_bnrelu_src if mode == 1 else _raw_src)(rng, M, Pn)
    w = _bf(rng, (N, K), 0.02)
    bias = rng.standard_normal(N).astype(np.float32) if "b" in extra else None
    addend = rng.standard_normal((M, N)).astype(np.float32) if "a" in extra else None
    wd = G.f32(_pack_cols(w, Pn)).to(torch.bfloat16)
    bd, ad = (None if bias is None else G.f32(bias)), (None if addend is None else G.f32(addend))
    need = (K // 128) * M * N
    scratch = torch.full((need,), NAN, dtype=torch.float32, device=G.dev())
    out = _out(M, N)
    check(lib.eae_op_fc_splitk(G.stream(), src, G.ptr(wd), M, N, K, G.ptr(bd), G.ptr(ad), G.ptr(scratch), need, G.ptr(out)))
    torch.cuda.synchronize()
    got = _take(out, M)
    ref = a @ w.astype(np.float64).T
    if bias is not None:
        ref = ref + bias
    if addend is not None:
        ref = ref + addend
    err = G.relmax(got, ref)
    print(f"splitk mode {mode} {extra} M {M} N {N} Pn {Pn}: relmax {err:.2e}")
    assert err < (2e-3 if mode == 1 else 1e-4), err


def test_fc_splitk_scratch_one_float_short_is_refused(lib):
    import gpu_util as G
    rng = np.random.default_rng(3)
    M, N, Pn = 5, 64, 16
    K = 256 * Pn
    src, keep, a = _raw_src(rng, M, Pn)
    wd = G.f32(_pack_cols(_bf(rng, (N, K), 0.02), Pn)).to(torch.bfloat16)
    need = (K // 128) * M * N
    scratch = torch.full((need,), NAN, dtype=torch.float32, device=G.dev())
    out = _out(M, N)
    rc = lib.eae_op_fc_splitk(G.stream(), src, G.ptr(wd), M, N, K, None, None, G.ptr(scratch), need - 1, G.ptr(out))
    torch.cuda.synchronize()
    assert rc == -2                                                          # EAE_ERR_ARG
    assert np.isnan(out.cpu().numpy()).all() and np.isnan(scratch.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------- eae_op_fc_bias_bf16
@pytest.mark.parametrize("M,L,Pn", [(1, 64, 16), (37, 128, 64), (129, 192, 16), (129, 256, 64), (37, 256, 16)])
def test_fc_bias_bf16(lib, M, L, Pn):
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(M * 1000 + L + Pn * 100003)
    K = 256 * Pn
    z = rng.standard_normal((M, L)).astype(np.float32)
    w = _bf(rng, (K, L), 0.1)                                                 # reference [K][L], K = c*Pn + p
    b = rng.standard_normal(K).astype(np.float32)
    wd = G.f32(_pack_rows(w, Pn)).to(torch.bfloat16)
    bd = G.f32(b.reshape(256, Pn).T.reshape(K))
    zd = G.f32(z)
    out = _out(M, K, torch.bfloat16)
    check(lib.eae_op_fc_bias_bf16(G.stream(), G.ptr(zd), G.ptr(wd), M, K, L, G.ptr(bd), G.ptr(out)))
    torch.cuda.synchronize()
    got = _take(out, M).reshape(M, Pn, 256).transpose(0, 2, 1).reshape(M, K)
    ref = O.linear_fwd(O.bf16_round(z).astype(np.float64), w.astype(np.float64), b)
    assert np.abs(got - ref).max() <= 2 ** -7 * np.abs(ref).max() + 1e-3, G.relmax(got, ref)


# ---------------------------------------------------------------------------------------------------- eae_op_fc_wgrad
# (Bt, L, Pn): 1, 1, 1, 2, 4, 5 and 6 batch chunks of 64 rows
WGRAD = [(1, 64, 16), (63, 64, 64), (64, 256, 16), (65, 64, 16), (256, 256, 16), (257, 64, 64), (321, 256, 64)]


@pytest.mark.parametrize("Bt,L,Pn", WGRAD)
def test_fc_wgrad_dec(lib, Bt, L, Pn):
    """mode 0 (dec.fc): dW[K][L] = g^T . z with rows permuted back to c*Pn + p, db = sum g; exact operands"""
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(Bt * 1000 + L + Pn * 100003)
    K = 256 * Pn
    gsrc, keep, g = _raw_src(rng, Bt, Pn)
    z = rng.standard_normal((Bt, L)).astype(np.float32)
    zd = G.f32(z)
    dw, db = _out(K, L), _out(1, K)
    check(lib.eae_op_fc_wgrad(G.stream(), 0, gsrc, G.src(3, zd), Bt, K, L, Pn, G.ptr(dw), G.ptr(db)))
    torch.cuda.synchronize()
    _, refw, refb = O.linear_bwd(O.bf16_round(z).astype(np.float64), np.zeros((K, L)), g)
    ew, eb = G.relmax(_take(dw, K), refw), G.relmax(_take(db, 1)[0], refb)
    print(f"wgrad dec Bt {Bt} L {L} Pn {Pn}: relmax dw {ew:.2e} db {eb:.2e}")
    assert ew < 1e-4 and eb < 1e-4, (ew, eb)


@pytest.mark.parametrize("Bt,L,Pn", WGRAD)
def test_fc_wgrad_enc(lib, Bt, L, Pn):
    """mode 1 (enc.fc): dW[L][K] = dz^T . relu(BN(y4)) with columns permuted back, db = sum dz"""
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(Bt * 1000 + L + Pn * 100003 + 1)
    K = 256 * Pn
    asrc, keep, act = _bnrelu_src(rng, Bt, Pn)
    dz = rng.standard_normal((Bt, L)).astype(np.float32)
    dzd = G.f32(dz)
    dw, db = _out(L, K), _out(1, L)
    check(lib.eae_op_fc_wgrad(G.stream(), 1, G.src(3, dzd), asrc, Bt, L, K, Pn, G.ptr(dw), G.ptr(db)))
    torch.cuda.synchronize()
    _, refw, refb = O.linear_bwd(act, np.zeros((L, K)), O.bf16_round(dz).astype(np.float64))
    ew, eb = G.relmax(_take(dw, L), refw), G.relmax(_take(db, 1)[0], refb)
    print(f"wgrad enc Bt {Bt} L {L} Pn {Pn}: relmax dw {ew:.2e} db {eb:.2e}")
    assert ew < 3e-3 and eb < 1e-2, (ew, eb)


@pytest.mark.parametrize("mode", [0, 1])
def test_fc_wgrad_without_colsum(lib, mode):
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(17 + mode)
    Bt, L, Pn = 65, 64, 16
    K = 256 * Pn
    f = rng.standard_normal((Bt, L)).astype(np.float32)
    fd = G.f32(f)
    if mode == 0:
        s, keep, v = _raw_src(rng, Bt, Pn)
        dw = _out(K, L)
        check(lib.eae_op_fc_wgrad(G.stream(), 0, s, G.src(3, fd), Bt, K, L, Pn, G.ptr(dw), None))
        _, ref, _ = O.linear_bwd(O.bf16_round(f).astype(np.float64), np.zeros((K, L)), v)
        rows, bound = K, 1e-4
    else:
        s, keep, v = _bnrelu_src(rng, Bt, Pn)
        dw = _out(L, K)
        check(lib.eae_op_fc_wgrad(G.stream(), 1, G.src(3, fd), s, Bt, L, K, Pn, G.ptr(dw), None))
        _, ref, _ = O.linear_bwd(v, np.zeros((L, K)), O.bf16_round(f).astype(np.float64))
        rows, bound = L, 3e-3
    torch.cuda.synchronize()
    assert G.relmax(_take(dw, rows), ref) < bound
