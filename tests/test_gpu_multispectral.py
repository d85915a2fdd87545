"""Multispectral inputs (in_channels = C bands, 1..16) through the fused engine: forward, all 38 gradients, Adam, autograd, the
grouped step and the C-band edge ops.

The reference hard-codes RGB (R.md:292 `Conv2d(3, ...)`), so parity at C != 3 is against the bf16-emulating NumPy oracle only, which is
channel-generic; the tolerances are those of test_gpu_ae.py::test_image128_forward_and_gradients_vs_oracle.  At C = 3 the C-band ops
are checked bitwise against the RGB ops they generalise.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from helpers import load_state_np
from oracle import ae_numpy as O
from stage_ref import stage_ref as _stage_ref

pytestmark = pytest.mark.gpu

PRE_BN_BIAS = {f"enc.encoder.{i}.bias" for i in (0, 3, 6, 9)} | {f"dec.decoder.{i}.bias" for i in (1, 4, 7)}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _model(c, seed=5, size=64, latent=64):
    import eae_amd
    torch.manual_seed(seed)
    m = eae_amd.SupervisedAutoencoder(latent_dim=latent, num_classes=10, image_size=size, in_channels=c)
    p = gu.perturb_bn({k: v.detach().numpy().copy() for k, v in m.state_dict().items()})
    load_state_np(m, p)
    return m.to("cuda"), p


def _engine(m, max_batch=8):
    from eae_amd.engine import engine_for
    return engine_for(m, max_batch=max_batch)


def _images(b, c, seed, size=64):
    rng = np.random.default_rng(seed)
    return rng.random((b, c, size, size), dtype=np.float32), rng.integers(0, 10, b).astype(np.int64)


def _cos(a, b):
    a, b = a.ravel().astype(np.float64), b.ravel().astype(np.float64)
    return float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("c,b,size", [(1, 8, 64), (4, 2, 64), (4, 8, 64), (13, 2, 64), (13, 8, 64), (16, 8, 64), (13, 2, 128)])
def test_fused_forward_and_gradients_vs_oracle(c, b, size):
    m, p = _model(c, size=size)
    x, y = _images(b, c, 10 + c, size)
    eng = _engine(m, max_batch=b)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    torch.cuda.synchronize()
    assert xh.shape == (b, c, size, size)
    out = O.ae_forward(p, x, train=True, quant="bf16")
    assert np.abs(z.cpu().numpy() - out["z"]).max() <= 6e-3 * np.abs(out["z"]).max()
    assert np.abs(lg.cpu().numpy() - out["logits"]).max() <= 6e-3 * np.abs(out["logits"]).max()
    d = np.abs(xh.cpu().numpy() - out["x_hat"])
    assert d.max() <= 1.5e-2 and d.mean() <= 1.5e-3, (d.max(), d.mean())
    m2, _ = _model(c, size=size)
    load_state_np(m2, p)
    eng2 = _engine(m2, max_batch=b)
    eng2.grad_step(_cuda(x), _cuda(y), 35.0)
    torch.cuda.synchronize()
    loss = float(eng2.loss_last[0])
    ref_loss, _, _ = O.ae_loss(out, x, y, 35.0)
    assert abs(loss - ref_loss) <= 1e-2 * abs(ref_loss), (loss, ref_loss)
    eng2.expose_grads()
    gq = O.ae_backward(p, out, x, y, 35.0, quant="bf16")
    bad = []
    names = [n for n, _ in m2.named_parameters()]
    assert len(names) == 38
    for name, prm in m2.named_parameters():
        got = prm.grad.cpu().numpy()
        ref = gq[name]
        assert got.shape == ref.shape, name
        if name in PRE_BN_BIAS:
            assert np.abs(got).max() == 0.0, name
            continue
        if not _cos(got, ref) > 0.995:
            bad.append((name, _cos(got, ref)))
    assert not bad, bad


def test_five_adam_steps_vs_oracle_c13():
    c, lr, alpha = 13, 5e-3, 35.0
    m, p = _model(c)
    eng = _engine(m)
    po = {k: v.copy() for k, v in p.items()}
    so = O.new_adam_state()
    losses, ref = [], []
    for step in range(5):
        x, y = _images(8, c, 300 + step)
        eng.train_step(_cuda(x), _cuda(y), alpha, lr)
        torch.cuda.synchronize()
        losses.append(float(eng.loss_last[0]))
        ref.append(O.ae_train_step(po, so, x, y, alpha, lr, quant="bf16")[0])
    np.testing.assert_allclose(losses[:3], ref[:3], rtol=1e-2)
    np.testing.assert_allclose(losses[3], ref[3], rtol=5e-2)
    np.testing.assert_allclose(losses[4], ref[4], rtol=0.2)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    bad = []
    for name, _ in m.named_parameters():
        if name in PRE_BN_BIAS:
            continue
        dmax = float(np.abs(sd[name] - po[name]).max())
        if dmax > 2 * 5 * lr + 1e-3:
            bad.append((name, dmax))
    assert not bad, bad
    assert int(sd["enc.encoder.1.num_batches_tracked"]) == 5


def test_autograd_drop_in_matches_fused_step_c13():
    c, alpha = 13, 35.0
    x, y = _images(8, c, 77)
    xd, yd = _cuda(x), _cuda(y)
    m1, p = _model(c)
    e1 = _engine(m1)
    e1.grad_step(xd, yd, alpha)
    torch.cuda.synchronize()
    e1.expose_grads()
    want = {n: q.grad.detach().clone() for n, q in m1.named_parameters()}
    m2, _ = _model(c)
    load_state_np(m2, p)
    m2.train()
    opt = torch.optim.Adam(m2.parameters(), lr=1e-3)
    opt.zero_grad()
    x_hat, logits, z = m2(xd)
    assert x_hat.shape == (8, c, 64, 64)
    loss = alpha * torch.nn.functional.mse_loss(x_hat, xd) + torch.nn.functional.cross_entropy(logits, yd)
    loss.backward()
    for n, q in m2.named_parameters():
        a, b = want[n].cpu().numpy(), q.grad.detach().cpu().numpy()
        scale = max(1e-12, np.abs(a).max())
        # as test_gpu_ae.py::test_autograd_drop_in_loop_matches_fused_step: the same kernels, only sigmoid / MSE / CE run in torch
        assert np.abs(a - b).max() <= 2e-2 * scale, (n, np.abs(a - b).max() / scale)
    opt.step()


def test_determinism_c13():
    outs = []
    for _ in range(2):
        m, _p = _model(13)
        eng = _engine(m)
        for s in range(2):
            x, y = _images(8, 13, 500 + s)
            eng.train_step(_cuda(x), _cuda(y), 35.0, 5e-3)
        torch.cuda.synchronize()
        outs.append(eng.params.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])


def test_grouped_step_c13_is_bitwise_each_member_alone():
    from eae_amd import _lib
    from eae_amd.engine import AEEngine
    lib = _lib.load()
    n, c = 4, 13
    alphas = [35.0 + 3.0 * k for k in range(n)]
    lrs = [1e-3 * (1 + k % 3) for k in range(n)]
    data = [tuple(_cuda(t) for t in _images(8, c, 700 + k)) for k in range(n)]

    def fresh():
        return [(m, _engine(m)) for m in (_model(c, seed=40 + k)[0] for k in range(n))]

    def snap(e, xd, yd, a):
        xh, lg, z = e.forward(xd, labels=yd, train=False, alpha=a)
        torch.cuda.synchronize()
        return [t.clone() for t in (e.params, e.adam_m, e.adam_v, e.bn_running, e.loss_accum, xh, lg, z)]

    grouped = fresh()
    for _ in range(3):
        AEEngine.group_train_step([e for _, e in grouped], [d[0] for d in data], [d[1] for d in data], alphas, lrs)
    torch.cuda.synchronize()
    got = [snap(e, data[k][0], data[k][1], alphas[k]) for k, (_, e) in enumerate(grouped)]
    del grouped
    alone = fresh()
    _lib.check(lib.eae_set_geometry_mult(n))
    try:
        for k, (_, e) in enumerate(alone):
            for _ in range(3):
                e.train_step(data[k][0], data[k][1], alphas[k], lrs[k])
    finally:
        _lib.check(lib.eae_set_geometry_mult(1))
    want = [snap(e, data[k][0], data[k][1], alphas[k]) for k, (_, e) in enumerate(alone)]
    for k in range(n):
        for a, w in zip(got[k], want[k]):
            assert torch.equal(a, w), k
    assert not torch.equal(got[0][0], got[1][0])


def test_group_of_mixed_band_counts_is_rejected():
    from eae_amd import _lib
    from eae_amd.engine import AEEngine
    ms = [_model(13, seed=1)[0], _model(4, seed=2)[0]]
    es = [_engine(m) for m in ms]
    xs = [_cuda(_images(8, c, 9)[0]) for c in (13, 4)]
    ys = [_cuda(_images(8, c, 9)[1]) for c in (13, 4)]
    with pytest.raises(_lib.EaeError, match="in_channels"):
        AEEngine.group_train_step(es, xs, ys, [35.0, 35.0], [1e-3, 1e-3])


def test_fit_autoencoder_c13_equals_stepping_by_hand():
    from eae_amd import train
    c = 13
    batches = [tuple(torch.from_numpy(t) for t in _images(8, c, 900 + i)) for i in range(3)]
    m1, p = _model(c)
    r = train.fit_autoencoder(batches, batches[:1], alpha=35.0, lr=1e-3, num_epochs=1, model=m1, verbose=False, log=lambda *a: None)
    m2, _ = _model(c)
    load_state_np(m2, p)
    eng = _engine(m2)
    for xb, yb in batches:
        eng.train_step(xb.cuda(), yb.cuda(), 35.0, 1e-3)
    torch.cuda.synchronize()
    s1, s2 = r["model"].state_dict(), m2.state_dict()
    for k in s1:
        assert torch.equal(s1[k].cpu(), s2[k].cpu()), k
    from eae_amd.engine import engine_for
    z = engine_for(m2).encoder(batches[0][0].cuda(), train=False)
    m2.eval()
    with torch.no_grad():
        z2 = m2.enc(batches[0][0].cuda())
    assert torch.equal(z, z2)


# ---------------------------------------------------------------------------------------------------- op level
BANDS = [1, 3, 4, 8, 13, 16]
EB, EH, EW = 2, 16, 128          # two tiles across: the halo column of the second one is a real pixel


def _lib():
    from eae_amd import _lib as L
    return L.load(), L


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cp(c):
    return 4 if c == 3 else 8 if c <= 8 else 16


def _pack_edge(lib, w, c):
    cp = _cp(c)
    kp = (9 * cp + 31) // 32 * 32
    wd = _cuda(w.astype(np.float32))
    wpack = torch.zeros(32 * kp, dtype=torch.bfloat16, device="cuda")
    wjoint = torch.zeros(4 * cp * 128, dtype=torch.bfloat16, device="cuda")
    assert lib.eae_op_pack_edge(_st(), _p(wd), c, _p(wpack), _p(wjoint)) == 0, lib.eae_last_error()
    return wpack, wjoint, cp


def _bf(a):
    return O.bf16_round(np.asarray(a, dtype=np.float32))


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _nhwc_bf16(a):            # [B,C,H,W] -> bf16 NHWC device tensor
    return _cuda(np.ascontiguousarray(a.transpose(0, 2, 3, 1))).to(torch.bfloat16)


def _edge_source(kind, c, rng):
    """(device tensor, bf16-rounded NCHW value) of a C-band edge operand: fp32 NCHW image, or the NHWC-CP bf16 gradient with zero
    bands >= C (what deconv4 + loss and sigmoid_bwd write)."""
    if kind == 0:
        x = rng.random((EB, c, EH, EW), dtype=np.float32)
        return _cuda(x), _bf(x)
    g = _bf(rng.standard_normal((EB, c, EH, EW)) * 0.5)
    pad = np.zeros((EB, _cp(c), EH, EW), np.float32)
    pad[:, :c] = g
    pad[:, c:] = 7.0                # must never be read: the kernels take only bands < C
    d = _nhwc_bf16(pad)
    d.view(EB, EH, EW, _cp(c))[..., c:] = 0.0
    return d, g


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("c", BANDS)
def test_edge_conv_op_vs_oracle(c, kind):
    """kind 0: conv1 forward (fp32 NCHW, +bias, statistics partials); kind 1: deconv4 backward-data (NHWC-CP bf16, ReLU mask of
    (yprev, prev_coef), BatchNorm-backward partials)."""
    lib, L = _lib()
    rng = np.random.default_rng(10 * c + kind)
    src, val = _edge_source(kind, c, rng)
    w = _bf(rng.standard_normal((32, c, 3, 3)) * 0.2)
    bias = (rng.standard_normal(32) * 0.1).astype(np.float32)
    wpack, _, _ = _pack_edge(lib, w, c)
    bd = _cuda(bias) if kind == 0 else None
    ho, wo = EH // 2, EW // 2
    out = torch.zeros((EB, ho, wo, 32), dtype=torch.bfloat16, device="cuda")
    nt = EB * (ho // 4) * (wo // 32)
    part = torch.zeros((2, 32, nt), dtype=torch.float32, device="cuda")
    bc = lambda v: v[None, :, None, None].astype(np.float64)
    yprev_d = coef_d = None
    if kind == 1:
        yprev = _bf(rng.standard_normal((EB, 32, ho, wo)))
        ps, pt = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32), (0.3 * rng.standard_normal(32)).astype(np.float32)
        pm, pi = (0.1 * rng.standard_normal(32)).astype(np.float32), (1.0 + 0.2 * rng.random(32)).astype(np.float32)
        yprev_d, coef_d = _nhwc_bf16(yprev), _cuda(np.stack([ps, pt, pm, pi]))
    rc = lib.eae_op_edge_conv_c(_st(), kind, _p(src), c, EB, EH, EW, _p(wpack), _p(bd), _p(out), _p(part), kind, _p(yprev_d), _p(coef_d))
    assert rc == 0, lib.eae_last_error()
    torch.cuda.synchronize()
    got = out.float().cpu().numpy().transpose(0, 3, 1, 2)
    ref = O.conv_s2_fwd(val, w, bias if kind == 0 else None)
    tol = 2 ** -7 * np.abs(ref).max() + 1e-3
    s = part.cpu().numpy().sum(2)
    g64 = got.astype(np.float64)
    if kind == 0:
        assert np.abs(got - ref).max() <= tol, np.abs(got - ref).max()
        np.testing.assert_allclose(s[0], g64.sum((0, 2, 3)), rtol=2e-4, atol=2e-2)
        np.testing.assert_allclose(s[1], (g64 ** 2).sum((0, 2, 3)), rtol=2e-4, atol=2e-2)
    else:
        act = _f32(yprev.astype(np.float64) * bc(ps) + bc(pt))
        mask, clear = act > 0, np.abs(act) > 1e-5
        assert np.abs(got - ref * mask)[clear].max() <= tol
        assert np.all(got[clear & ~mask] == 0.0)
        xhat = _f32(yprev.astype(np.float64) * bc(pi) + bc(-pm * pi))
        np.testing.assert_allclose(s[0], g64.sum((0, 2, 3)), rtol=2e-4, atol=2e-2)
        np.testing.assert_allclose(s[1], (g64 * xhat).sum((0, 2, 3)), rtol=2e-4, atol=2e-2)
    if c == 3:       # the C-band op at C = 3 is bitwise the RGB op
        out3, part3 = torch.zeros_like(out), torch.zeros_like(part)
        rc = lib.eae_op_edge_conv(_st(), kind, _p(src), EB, EH, EW, _p(wpack), _p(bd), _p(out3), _p(part3), kind, _p(yprev_d), _p(coef_d))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out3, out) and torch.equal(part3, part)


@pytest.mark.parametrize("kind,side_mode", [(0, 0), (0, 2), (1, 1)])
@pytest.mark.parametrize("c", BANDS)
def test_edge_wgrad_op_vs_oracle(c, kind, side_mode):
    """(0, 2): conv1's weight gradient (fp32 image, BatchNorm-backward side); (1, 1): deconv4's (NHWC-CP gradient, BN+ReLU side);
    (0, 0): plain side.  dw [32][C][3][3] vs the oracle on the values the kernel loads."""
    lib, L = _lib()
    rng = np.random.default_rng(100 + 10 * c + side_mode)
    src, val = _edge_source(kind, c, rng)
    shp = (EB, 32, EH // 2, EW // 2)
    bc = lambda v: v[None, :, None, None].astype(np.float64)
    keep = []
    if side_mode == 0:
        dy = _bf(rng.standard_normal(shp) * 0.1)
        d = _nhwc_bf16(dy)
        keep, side = [d], L.EaeSrc(d.data_ptr(), None, None, 0)
    elif side_mode == 1:
        y = _bf(rng.standard_normal(shp))
        s_, t_ = (1.0 + 0.2 * rng.standard_normal(32)).astype(np.float32), (0.3 * rng.standard_normal(32)).astype(np.float32)
        coef = np.stack([s_, t_, np.zeros(32, np.float32), np.ones(32, np.float32)])
        d, cd = _nhwc_bf16(y), _cuda(coef)
        keep, side = [d, cd], L.EaeSrc(d.data_ptr(), None, cd.data_ptr(), 1)
        dy = _bf(np.maximum(_f32(y.astype(np.float64) * bc(s_) + bc(t_)), 0.0))
    else:
        g = _bf(rng.standard_normal(shp) * 0.1)
        y = _bf(rng.standard_normal(shp))
        a_, b_, c_ = (1.0 + 0.1 * rng.standard_normal(32)).astype(np.float32), (0.1 * rng.standard_normal(32)).astype(np.float32), \
            (0.05 * rng.standard_normal(32)).astype(np.float32)
        gd, yd, cd = _nhwc_bf16(g), _nhwc_bf16(y), _cuda(np.stack([a_, b_, c_]))
        keep, side = [gd, yd, cd], L.EaeSrc(gd.data_ptr(), yd.data_ptr(), cd.data_ptr(), 2)
        inner = _f32(y.astype(np.float64) * bc(b_) + bc(c_))
        dy = _bf(_f32(g.astype(np.float64) * bc(a_) + inner.astype(np.float64)))
    scratch = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    dw = torch.zeros(32 * c * 9, dtype=torch.float32, device="cuda")
    rc = lib.eae_op_edge_wgrad_c(_st(), kind, _p(src), c, EB, EH, EW, side, _p(scratch), 1 << 20, _p(dw))
    assert rc == 0, lib.eae_last_error()
    torch.cuda.synchronize()
    _, ref, _ = O.conv_s2_bwd(val, np.zeros((32, c, 3, 3), np.float32), dy)
    got = dw.cpu().numpy().reshape(32, c, 3, 3)
    assert np.abs(got - ref).max() < 1e-4 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()
    if c == 3:
        dw3 = torch.zeros_like(dw)
        rc = lib.eae_op_edge_wgrad(_st(), kind, _p(src), EB, EH, EW, side, _p(scratch), 1 << 20, _p(dw3))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(dw3, dw)
    del keep


@pytest.mark.parametrize("c", BANDS)
def test_deconv4_loss_op_vs_oracle(c):
    lib, L = _lib()
    rng = np.random.default_rng(80 + c)
    Hin, Win = EH // 2, EW // 2
    a3 = _bf(np.maximum(rng.standard_normal((EB, 32, Hin, Win)), 0))
    w = _bf(rng.standard_normal((32, c, 3, 3)) * 0.2)
    bias = (rng.standard_normal(c) * 0.1).astype(np.float32)
    x = rng.random((EB, c, EH, EW), dtype=np.float32)
    _, wjoint, cp = _pack_edge(lib, w, c)
    a3d = _nhwc_bf16(a3)
    bd, xd = _cuda(bias), _cuda(x)
    x_hat = torch.zeros((EB, c, EH, EW), dtype=torch.float32, device="cuda")
    g = torch.full((EB, EH, EW, cp), 7.0, dtype=torch.bfloat16, device="cuda")
    ntiles = EB * (Hin // 4) * (Win // 32)
    lps = (c + 4) // 4 * 4
    lp = torch.zeros(ntiles * lps, dtype=torch.float32, device="cuda")
    numel = EB * c * EH * EW
    gscale = 2.0 * 35.0 / numel
    src = L.EaeSrc(a3d.data_ptr(), None, None, 0)
    rc = lib.eae_op_deconv4_loss_c(_st(), src, c, EB, Hin, Win, _p(wjoint), _p(bd), _p(xd), C.c_float(gscale), _p(x_hat), _p(g), _p(lp))
    assert rc == 0, lib.eae_last_error()
    torch.cuda.synchronize()
    s = O.deconv_s2_fwd(a3, w, bias)
    xh_ref = O.sigmoid(s)
    xh = x_hat.cpu().numpy()
    assert np.abs(xh - xh_ref).max() <= 2 ** -7 * 0.25 * np.abs(s).max() + 1e-3
    gr = g.float().cpu().numpy()
    assert np.all(gr[..., c:] == 0)
    g_ref = (gscale * (xh - x) * xh * (1 - xh)).transpose(0, 2, 3, 1)      # from the kernel's own x_hat: bf16 rounding only
    assert np.abs(gr[..., :c] - g_ref).max() <= 2 ** -8 * np.abs(g_ref).max()
    parts = lp.cpu().numpy().reshape(ntiles, lps).astype(np.float64).sum(0)
    np.testing.assert_allclose(parts[0], ((xh.astype(np.float64) - x) ** 2).sum(), rtol=1e-4)
    np.testing.assert_allclose(parts[1:1 + c], gr[..., :c].astype(np.float64).sum((0, 1, 2)), rtol=1e-4, atol=1e-9)
    assert np.all(parts[1 + c:] == 0)
    if c == 3:
        x_hat3, g3, lp3 = torch.zeros_like(x_hat), torch.full_like(g, 7.0), torch.zeros_like(lp)
        rc = lib.eae_op_deconv4_loss(_st(), src, EB, Hin, Win, _p(wjoint), _p(bd), _p(xd), C.c_float(gscale), _p(x_hat3), _p(g3), _p(lp3))
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(x_hat3, x_hat) and torch.equal(g3, g) and torch.equal(lp3, lp)


@pytest.mark.parametrize("c", BANDS)
def test_sigmoid_bwd_op_vs_numpy(c):
    lib, L = _lib()
    rng = np.random.default_rng(300 + c)
    B, H, W = 3, 64, 64
    xh = rng.random((B, c, H, W), dtype=np.float32)
    dxh = (rng.standard_normal((B, c, H, W)) * 1e-3).astype(np.float32)
    cp = _cp(c)
    g = torch.full((B, H, W, cp), 7.0, dtype=torch.bfloat16, device="cuda")
    db = torch.zeros(c, dtype=torch.float32, device="cuda")
    nblk = (B * H * W + 255) // 256
    scratch = torch.zeros(nblk * ((c + 4) // 4 * 4), dtype=torch.float32, device="cuda")
    xhd, dxhd = _cuda(xh), _cuda(dxh)
    assert lib.eae_op_sigmoid_bwd_c(_st(), _p(xhd), _p(dxhd), c, B, H, W, _p(g), _p(db), _p(scratch)) == 0, lib.eae_last_error()
    torch.cuda.synchronize()
    ref = _bf(_f32(dxh * xh * (np.float32(1.0) - xh))).transpose(0, 2, 3, 1)
    gr = g.float().cpu().numpy()
    assert np.array_equal(gr[..., :c], ref) and np.all(gr[..., c:] == 0)
    np.testing.assert_allclose(db.cpu().numpy(), ref.astype(np.float64).sum((0, 1, 2)), rtol=1e-5, atol=1e-9)


# ---------------------------------------------------------------------------------------------------- staging
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_stage_bands_exact_with_explicit_draws_c13(dtype):
    from eae_amd.augment import stage_bands
    rng = np.random.default_rng(21)
    N, c, B = 7, 13, 5
    hi = 10000 if dtype == np.uint16 else 255
    data = rng.integers(0, hi + 1, (N, c, 64, 64)).astype(dtype)
    idx = np.array([6, 0, 3, 3, 1], np.int64)
    div = (np.linspace(2000, 12000, c) if dtype == np.uint16 else np.full(c, 255.0)).astype(np.float32)
    params = np.stack([rng.integers(0, 2, B), rng.integers(0, 9, B), rng.integers(0, 9, B)], 1).astype(np.int32)
    params[0] = (1, 0, 8)
    noise = rng.standard_normal((B, c, 64, 64)).astype(np.float32)
    t = torch.from_numpy(data.astype(np.int32)).to(torch.uint16 if dtype == np.uint16 else torch.uint8).cuda()
    got = stage_bands(t, div, index=torch.from_numpy(idx).cuda(), params=torch.from_numpy(params), noise=torch.from_numpy(noise))
    ref = _stage_ref(data, idx, div, params, noise, 0.03)
    assert got.shape == (B, c, 64, 64)
    assert np.array_equal(got.cpu().numpy(), ref)
    ev = stage_bands(t, div, index=torch.from_numpy(idx).cuda(), train=False)
    assert np.array_equal(ev.cpu().numpy(), _stage_ref(data, idx, div, [(0, 4, 4)] * B, None, 0.0))


def test_stage_bands_rgb_is_augment_batch():
    from eae_amd.augment import augment_batch, stage_bands
    rng = np.random.default_rng(5)
    B = 6
    u8 = rng.integers(0, 256, (B, 64, 64, 3)).astype(np.uint8)
    params = torch.from_numpy(np.stack([rng.integers(0, 2, B), rng.integers(0, 9, B), rng.integers(0, 9, B)], 1).astype(np.int32))
    noise = torch.from_numpy(rng.standard_normal((B, 3, 64, 64)).astype(np.float32))
    a = augment_batch(torch.from_numpy(u8).cuda(), train=True, params=params, noise=noise)
    chw = torch.from_numpy(np.ascontiguousarray(u8.transpose(0, 3, 1, 2))).cuda()
    b = stage_bands(chw, 255.0, params=params, noise=noise)
    assert torch.equal(a, b)


def test_stage_bands_rng_mode_c13():
    from eae_amd.augment import stage_bands
    N, c = 64, 13
    data = torch.full((N, c, 64, 64), 5000, dtype=torch.int32).to(torch.uint16).cuda()
    div = torch.full((c,), 10000.0)
    a = stage_bands(data, div, seed=3, step=7)
    b = stage_bands(data, div, seed=3, step=7)
    d = stage_bands(data, div, seed=3, step=8)
    assert torch.equal(a, b) and not torch.equal(a, d)
    interior = a[:, :, 8:56, 8:56] - 0.5          # away from the crop padding: pure noise around 0.5
    assert abs(float(interior.std()) - 0.03) <= 5e-4 and abs(float(interior.mean())) <= 5e-4
    assert bool(torch.isfinite(a).all())


# ---------------------------------------------------------------------------------------------------- loops, DP, stand-alone halves
def test_fit_functions_pass_in_channels_on():
    from eae_amd import train
    c = 4
    batches = [tuple(torch.from_numpy(t) for t in _images(8, c, 950 + i)) for i in range(2)]
    r = train.fit_autoencoder(batches, batches[:1], alpha=35.0, lr=1e-3, num_epochs=1, verbose=False, log=lambda *a: None,
                              in_channels=c)
    assert r["model"].in_channels == c and np.isfinite(r["best_val_loss"])
    rs = train.fit_autoencoder_group(batches, batches[:1], [(35.0, 1e-3), (30.0, 2e-3)], num_epochs=1, verbose=False, in_channels=c)
    assert [m["model"].in_channels for m in rs] == [c, c] and all(np.isfinite(m["best_val_loss"]) for m in rs)
    seen = []

    def fit_fn(tl, vl, alpha, lr, **kw):
        seen.append(kw.get("in_channels"))
        return train.fit_autoencoder(tl, vl, alpha, lr, **kw)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        train.grid_search_autoencoder(batches, batches[:1], alpha_values=(35,), lr_values=(1e-3,), num_epochs=1, out_dir=d,
                                      verbose=False, fit_fn=fit_fn, in_channels=c)
        sd = torch.load(os.path.join(d, "AE_GLOBAL_BEST.pt"))
    assert seen == [c] and tuple(sd["enc.encoder.0.weight"].shape) == (32, c, 3, 3)


def test_stand_alone_halves_match_the_engine_c13():
    """Stand-alone Decoder / Encoder autograd at C = 13: repeatable bitwise, deconv4's bias gradient equal to the NumPy sigmoid + MSE
    backward of the kernel's own x_hat, conv1's weight gradient of shape [32,13,3,3], and the input check names [B,13,H,W]."""
    import eae_amd
    c = 13
    torch.manual_seed(3)
    dec = eae_amd.Decoder(64, out_channels=c).cuda()
    z = torch.randn(4, 64, device="cuda", requires_grad=True)
    target = torch.rand(4, c, 64, 64, device="cuda")
    x_hat = dec(z)
    assert x_hat.shape == (4, c, 64, 64)
    torch.nn.functional.mse_loss(x_hat, target).backward()
    g1 = {n: q.grad.clone() for n, q in dec.named_parameters()}
    dz1 = z.grad.clone()
    for q in dec.parameters():
        q.grad = None
    z.grad = None
    x_hat = dec(z)
    torch.nn.functional.mse_loss(x_hat, target).backward()
    for n, q in dec.named_parameters():          # deterministic: the same forward + backward twice
        assert torch.equal(q.grad, g1[n]), n
    assert torch.equal(z.grad, dz1)
    # against the oracle: the decoder half of ae_forward / ae_backward on an encoder-free parameter dict
    p = {k: v.detach().cpu().numpy() for k, v in dec.state_dict().items()}
    assert dec.decoder[10].bias.grad.shape == (c,)
    # d/d bias of deconv4 = sum over pixels of dL/ds: equals the sigmoid backward of the kernel's own x_hat
    xh = x_hat.detach().cpu().numpy()
    dl = 2.0 * (xh - target.cpu().numpy()) / xh.size
    ref_db = (dl * xh * (1 - xh)).sum((0, 2, 3))
    got_db = dec.decoder[10].bias.grad.cpu().numpy()
    assert _cos(got_db, ref_db) > 0.999 and np.abs(got_db - ref_db).max() <= 2e-2 * np.abs(ref_db).max()
    enc = eae_amd.Encoder(64, in_channels=c).cuda()
    x = torch.rand(4, c, 64, 64, device="cuda")
    zz = enc(x)
    assert zz.shape == (4, 64)
    zz.sum().backward()
    assert enc.encoder[0].weight.grad.shape == (32, c, 3, 3) and enc.encoder[0].weight.grad.abs().max() > 0
    with pytest.raises(RuntimeError, match=r"\[B,13,64,64\]"):
        enc(torch.zeros(2, 3, 64, 64, device="cuda"))
    del p


def test_data_parallel_world1_rccl_c13():
    """A world-1 native RCCL step at C = 13 equals the plain step bitwise (as test_gpu_ae.py's RGB test)."""
    import torch.distributed as dist
    from eae_amd import dp
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29900 + os.getpid() % 90))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        x, y = _images(8, 13, 61)
        xd, yd = _cuda(x), _cuda(y)
        ma, p = _model(13)
        ea = _engine(ma)
        for _ in range(2):
            ea.train_step(xd, yd, 35.0, 5e-3)
        torch.cuda.synchronize()
        mb, _ = _model(13)
        load_state_np(mb, p)
        eb = _engine(mb)
        tr = dp.DataParallelTrainer(eb, native=True)
        assert tr.native and tr.rccl_ranks() == 1
        tr.broadcast_parameters()
        for _ in range(2):
            tr.train_step(xd, yd, 35.0, 5e-3)
        torch.cuda.synchronize()
        assert torch.equal(ea.params, eb.params) and torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.bn_running, eb.bn_running)
    finally:
        if created:
            dist.destroy_process_group()
