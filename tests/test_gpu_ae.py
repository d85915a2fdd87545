"""End-to-end parity of the fused autoencoder path (C ABI: eae_ae_forward / eae_ae_grad_step / eae_ae_train_step).

Two references per quantity:
  (1) the golden vectors produced by the reference's own fp32 classes (tests/golden/*.npz) -- tolerances for the bf16
      path from SURVEY.md 8c: x_hat <= 3e-2 max-abs and <= 3e-3 mean-abs, logits / z <= 2 % of the tensor's abs-max;
  (2) the NumPy oracle with bf16 storage emulation (same rounding points as the kernels) -- tight tolerances.
"""
import os

import numpy as np
import pytest
import torch

import golden_util as gu
from helpers import ae_state_np, load_state_np
from oracle import ae_numpy as O

pytestmark = pytest.mark.gpu


def _model(latent=64, sd=None):
    import eae_amd
    torch.manual_seed(gu.AE_SEED)
    m = eae_amd.SupervisedAutoencoder(latent_dim=latent, num_classes=10)
    load_state_np(m, sd if sd is not None else ae_state_np(latent))
    return m.to("cuda")


def _engine(m, max_batch=64):
    from eae_amd.engine import engine_for
    return engine_for(m, max_batch=max_batch)


def _cuda(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _check_fwd(x_hat, logits, z, g, prefix=""):
    xh = g[prefix + "x_hat"]
    d = np.abs(x_hat - xh)
    assert d.max() <= 3e-2 and d.mean() <= 3e-3, (d.max(), d.mean())
    assert np.abs(logits - g[prefix + "logits"]).max() <= 0.02 * np.abs(g[prefix + "logits"]).max()
    assert np.abs(z - g[prefix + "z"]).max() <= 0.02 * np.abs(g[prefix + "z"]).max()


@pytest.mark.parametrize("b", [2, 8])
def test_forward_train_and_eval_vs_golden(golden, b):
    g = golden(f"ae_fwd_bwd_b{b}.npz")
    m = _model()
    eng = _engine(m)
    x = _cuda(g["x"])
    xh, lg, z = eng.forward(x, train=False)
    _check_fwd(xh.cpu().numpy(), lg.cpu().numpy(), z.cpu().numpy(), g, "eval_")
    xh, lg, z = eng.forward(x, labels=_cuda(g["labels"]), train=True, alpha=float(g["alpha"]))
    torch.cuda.synchronize()
    _check_fwd(xh.cpu().numpy(), lg.cpu().numpy(), z.cpu().numpy(), g)
    last = eng.loss_last.cpu().numpy()
    assert abs(last[0] - g["loss"]) <= 0.02 * abs(g["loss"]), (last, g["loss"])
    assert abs(last[1] - g["loss_recon"]) <= 0.02 * g["loss_recon"]
    assert abs(last[2] - g["loss_class"]) <= 0.02 * g["loss_class"]
    # running statistics after one training-mode forward (BatchNorm momentum update)
    sd = m.state_dict()
    for k in g.files:
        if k.startswith("buf/"):
            name = k[4:]
            if name.endswith("num_batches_tracked"):
                assert int(sd[name]) == int(g[k]), name
            else:
                np.testing.assert_allclose(sd[name].cpu().numpy(), g[k], rtol=2e-2, atol=2e-3, err_msg=name)


def test_forward_vs_bf16_oracle():
    p = ae_state_np()
    x, y = gu.make_images(8, 100)
    out = O.ae_forward(p, x, train=True, quant="bf16")
    m = _model()
    eng = _engine(m)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    torch.cuda.synchronize()
    assert np.abs(z.cpu().numpy() - out["z"]).max() <= 4e-3 * np.abs(out["z"]).max()
    assert np.abs(lg.cpu().numpy() - out["logits"]).max() <= 4e-3 * np.abs(out["logits"]).max()
    # sigmoid output: a handful of bf16 rounding flips upstream move single pixels by a few 1e-3
    d = np.abs(xh.cpu().numpy() - out["x_hat"])
    assert d.max() <= 1.2e-2 and d.mean() <= 1.5e-3, (d.max(), d.mean())


def _rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b)))


def _norm_ratio(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64)) / max(1e-30, np.linalg.norm(np.asarray(b, np.float64))))


def test_gradients_vs_golden_and_oracle(golden):
    """All 38 gradients at b=8, per tensor, against the bf16-emulating oracle (same rounding points: what is left is summation
    order and the rounding ties it flips) and against the reference's fp32 gradients.
    Bounds = measured on MI355X (tools/measure_parity.py, round 2) + margin: vs the oracle the worst tensor had relmax 0.18
    (dec.decoder.1.weight; the oracle itself sits 0.10-0.36 from the fp32 golden in relmax: bf16 noise of this network, not of
    the kernels), norm ratio 0.986-1.007, cosine >= 0.9958.  The NORM RATIO is the scale check (a wrong 1/B, 1/count or
    BatchNorm-backward coefficient moves it by far more than 3 %); border taps / phases are pinned op by op in
    tests/test_gpu_ops_path.py at 1e-3."""
    import gpu_util as G
    g = golden("ae_fwd_bwd_b8.npz")
    p = ae_state_np()
    x, y = g["x"], g["labels"]
    alpha = float(g["alpha"])
    m = _model()
    eng = _engine(m)
    eng.grad_step(_cuda(x), _cuda(y), alpha)
    torch.cuda.synchronize()
    eng.expose_grads()
    out = O.ae_forward(p, x, train=True, quant="bf16")
    gq = O.ae_backward(p, out, x, y, alpha, quant="bf16")
    report = []
    bad = []
    for name, prm in m.named_parameters():
        got = prm.grad.cpu().numpy()
        ref32 = g[f"grad/{name}"]
        if np.abs(ref32).max() < 1e-6:          # bias in front of BatchNorm: identically zero here
            assert np.abs(got).max() == 0.0, name
            continue
        refq = gq[name]
        r_q, c_q, c_32 = G.relmax(got, refq), G.cosine(got, refq), G.cosine(got, ref32)
        l2_q, nr_q, nr_32 = _rel_l2(got, refq), _norm_ratio(got, refq), _norm_ratio(got, ref32)
        report.append(f"{name:28s} vs-bf16-oracle relmax {r_q:.3e} relL2 {l2_q:.3e} norm {nr_q:.4f} cos {c_q:.5f} | vs-fp32-golden norm {nr_32:.4f} cos {c_32:.5f}")
        ok = (c_q > 0.995 and c_32 > 0.97 and r_q <= 0.25 and l2_q <= 0.12 and 0.97 <= nr_q <= 1.03 and 0.95 <= nr_32 <= 1.05)
        if not ok:
            bad.append(name)
    print("\n".join(report))
    assert not bad, bad


@pytest.mark.parametrize("b", [2, 32, 48, 56])
def test_gradient_digests_at_other_batch_sizes(golden, b):
    """The gradd/* digests of ae_fwd_bwd_b{2,32,48,56}.npz (reference fp32 gradients: l2 norm + every 97th element), incl. the
    short last batches of the reference's loaders (48, 56: images past the batch inside 2- and 8-image tiles).
    Measured on MI355X: l2 ratio 0.971-1.031 over all tensors and batch sizes; sample cosine >= 0.982 on the tensors with
    >= 100 samples."""
    import gpu_util as G
    g = golden(f"ae_fwd_bwd_b{b}.npz")
    x, y = gu.make_images(b, int(g["seed"]))
    m = _model()
    eng = _engine(m)
    eng.grad_step(_cuda(x), _cuda(y), float(g["alpha"]))
    torch.cuda.synchronize()
    eng.expose_grads()
    bad = []
    for name, prm in m.named_parameters():
        got = prm.grad.cpu().numpy()
        dg, smp = g[f"gradd/{name}/digest"], g[f"gradd/{name}/sample"]
        if dg[1] < 1e-6:
            assert np.abs(got).max() == 0.0, name
            continue
        d, s = gu.tensor_digest(got)
        ratio = d[1] / dg[1]
        cos = G.cosine(s, smp) if smp.size >= 100 else 1.0
        if not (0.95 <= ratio <= 1.05 and cos > 0.975):
            bad.append((name, round(ratio, 4), round(cos, 4)))
    assert not bad, bad


@pytest.mark.parametrize("b", [32, 48, 56])
def test_big_and_short_batches(golden, b):
    g = golden(f"ae_fwd_bwd_b{b}.npz")
    x, y = gu.make_images(b, int(g["seed"]))
    m = _model()
    eng = _engine(m)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=float(g["alpha"]))
    torch.cuda.synchronize()
    d = np.abs(xh.cpu().numpy().ravel()[::7] - g["x_hat"])
    assert d.max() <= 3e-2 and d.mean() <= 3e-3
    assert np.abs(lg.cpu().numpy() - g["logits"]).max() <= 0.02 * np.abs(g["logits"]).max()
    assert abs(eng.loss_last.cpu().numpy()[0] - g["loss"]) <= 0.02 * abs(g["loss"])


def test_eval_b1_and_latent128(golden):
    g = golden("ae_eval_b1.npz")
    m = _model()
    xh, lg, z = _engine(m).forward(_cuda(g["x"]), train=False)
    assert np.abs(xh.cpu().numpy() - g["eval_x_hat"]).max() <= 3e-2
    assert np.abs(lg.cpu().numpy() - g["eval_logits"]).max() <= 0.02 * np.abs(g["eval_logits"]).max()
    g = golden("ae_latent128_b8.npz")
    m = _model(128)
    xh, lg, z = _engine(m).forward(_cuda(g["x"]), train=True)
    assert np.abs(xh.cpu().numpy() - g["x_hat"]).max() <= 3e-2
    assert np.abs(z.cpu().numpy() - g["z"]).max() <= 0.02 * np.abs(g["z"]).max()


@pytest.mark.parametrize("latent", [48])
def test_latent_width_not_a_multiple_of_64_vs_golden(golden, latent):
    """The reference takes any latent_dim (R.md:309, 365, 423); the engine pads the latent width to a multiple of 64 inside its
    packs and workspaces.  ae_latent48_b8.npz (reference run): forward, loss, gradient digests of every parameter, parameters
    after one Adam step; plus the encoder -> decoder entry points and the autograd path with caller-side [B][48] latents."""
    import gpu_util as G
    g = golden(f"ae_latent{latent}_b8.npz")
    x, y = gu.make_images(8, int(g["seed"]))
    m = _model(latent)
    eng = _engine(m)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=float(g["alpha"]))
    torch.cuda.synchronize()
    assert tuple(z.shape) == (8, latent)
    d = np.abs(xh.cpu().numpy().ravel()[::7] - g["x_hat"])
    assert d.max() <= 3e-2 and d.mean() <= 3e-3
    assert np.abs(z.cpu().numpy() - g["z"]).max() <= 0.02 * np.abs(g["z"]).max()
    assert np.abs(lg.cpu().numpy() - g["logits"]).max() <= 0.02 * np.abs(g["logits"]).max()
    assert abs(eng.loss_last.cpu().numpy()[0] - g["loss"]) <= 0.02 * abs(g["loss"])
    # encoder / decoder entry points with the caller's unpadded latent
    z2 = eng.encoder(_cuda(x), train=False)
    xh2 = eng.decoder(z2, train=False)
    xh3, _, z3 = eng.forward(_cuda(x), train=False)
    torch.cuda.synchronize()
    assert torch.equal(z2, z3) and torch.equal(xh2, xh3)
    # gradients
    eng.grad_step(_cuda(x), _cuda(y), float(g["alpha"]))
    torch.cuda.synchronize()
    eng.expose_grads()
    bad = []
    for name, prm in m.named_parameters():
        got = prm.grad.cpu().numpy()
        dg, smp = g[f"grad/{name}/digest"], g[f"grad/{name}/sample"]
        if dg[1] < 1e-6:
            assert np.abs(got).max() == 0.0, name
            continue
        dd, s = gu.tensor_digest(got)
        ratio = dd[1] / dg[1]
        cos = G.cosine(s, smp) if smp.size >= 100 else 1.0
        if not (0.95 <= ratio <= 1.05 and cos > 0.975):
            bad.append((name, round(ratio, 4), round(cos, 4)))
    assert not bad, bad
    # one Adam step: -lr * sign(g) elementwise (as test_one_adam_step_elementwise_vs_golden)
    m = _model(latent)
    eng = _engine(m)
    lr = float(g["lr"])
    eng.train_step(_cuda(x), _cuda(y), float(g["alpha"]), lr)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    for k in g.files:
        if not (k.startswith("final/") and k.endswith("/sample")):
            continue
        name = k[6:-7]
        if "running" in name or "num_batches" in name or gu.is_prebn_bias(name):
            continue
        _, s = gu.tensor_digest(sd[name])
        err = np.abs(s - g[k])
        assert err.max() <= 2 * lr + 1e-4 and (s.size < 50 or float(np.mean(err < 1e-4)) >= 0.90), (name, float(err.max()))


def test_num_classes_other_than_10_vs_oracle():
    """The reference takes any num_classes (R.md:417, 426); the head kernel holds up to 64.  37 classes, latent 48, B=8 against the
    oracle (the head is fp32 end to end: logits and the classifier gradients are tight)."""
    import eae_amd
    import gpu_util as G
    torch.manual_seed(11)
    m = eae_amd.SupervisedAutoencoder(latent_dim=48, num_classes=37)
    p = gu.perturb_bn({k: v.detach().numpy().copy() for k, v in m.state_dict().items()})
    load_state_np(m, p)
    m = m.to("cuda")
    x, _ = gu.make_images(8, 321)
    y = np.random.default_rng(5).integers(0, 37, 8).astype(np.int64)
    eng = _engine(m, max_batch=8)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    eng.grad_step(_cuda(x), _cuda(y), 35.0)
    torch.cuda.synchronize()
    eng.expose_grads()
    out = O.ae_forward(p, x, train=True, quant="bf16")
    assert tuple(lg.shape) == (8, 37)
    assert np.abs(lg.cpu().numpy() - out["logits"]).max() <= 0.02 * np.abs(out["logits"]).max()
    loss, l_r, l_c = O.ae_loss(out, x, y, 35.0)
    got = eng.loss_last.cpu().numpy()
    assert abs(got[2] - l_c) <= 2e-2 * abs(l_c) and abs(got[1] - l_r) <= 2e-2 * l_r, (got, l_r, l_c)
    gq = O.ae_backward(p, out, x, y, 35.0, quant="bf16")
    for name in ("classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias", "enc.encoder.13.weight"):
        got_g = dict(m.named_parameters())[name].grad.cpu().numpy()
        assert got_g.shape == gq[name].shape
        assert G.cosine(got_g, gq[name]) > 0.995, (name, G.cosine(got_g, gq[name]))
        if name.startswith("classifier"):
            # the head is fp32 end to end: its gradients differ from the oracle's only through the bf16 rounding of z upstream, so
            # a wrong SCALE (1/B, a missed class) must show: elementwise and in the norm (cosine alone is scale-blind)
            nr = np.linalg.norm(got_g.ravel().astype(np.float64)) / np.linalg.norm(gq[name].ravel().astype(np.float64))
            assert G.relmax(got_g, gq[name]) <= 2e-2 and 0.99 <= nr <= 1.01, (name, G.relmax(got_g, gq[name]), nr)
    with pytest.raises(Exception, match="num_classes"):
        _engine(eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=65).cuda(), max_batch=4)


@pytest.mark.parametrize("tag,head", [("joint", True), ("recon", False)])
def test_adam_trajectory_vs_golden(golden, tag, head):
    g = golden(f"ae_adam5_{tag}_b8.npz")
    m = _model()
    eng = _engine(m)
    alpha = float(g["alpha"]) if head else 1.0
    lr = float(g["lr"])
    losses = []
    for step in range(5):
        x, y = gu.make_images(8, 200 + step)
        eng.train_step(_cuda(x), _cuda(y), alpha, lr, head=head)
        losses.append(float(eng.loss_last.cpu().numpy()[0]))
    # Adam's sign-like first steps at lr=5e-3 make the trajectory chaotic: the NumPy oracle with bf16 storage emulation
    # itself drifts from the fp32 golden by 0.2 % / 0.2 % / 0.9 % / 5.7 % over steps 2..5 (measured), so the bound
    # widens with the step index.  (Two builds of this engine that differ only in a tile geometry, i.e. in fp32 summation
    # order, measured 1.8 % at step 4 and 9 % / 12 % at step 5.)
    np.testing.assert_allclose(np.array(losses)[:3], g["losses"][:3], rtol=1e-2)
    np.testing.assert_allclose(np.array(losses)[3], g["losses"][3], rtol=5e-2)
    np.testing.assert_allclose(np.array(losses)[4], g["losses"][4], rtol=0.2)
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    assert int(sd["enc.encoder.1.num_batches_tracked"]) == 5
    # How far does the SAME arithmetic with bf16 storage drift from the fp32 reference on this trajectory?  The NumPy oracle with bf16
    # emulation is run through the same five steps here (2 s of CPU) and its own per-buffer deviation from the golden is the yardstick
    # for the running statistics below (the bound is justified by a measured spread, not by a constant).
    po = {k: v.copy() for k, v in ae_state_np().items()}
    so = O.new_adam_state()
    for step in range(5):
        x, y = gu.make_images(8, 200 + step)
        O.ae_train_step(po, so, x, y, alpha, lr, quant="bf16", head=head)
    spread = {k[4:]: float(np.abs(po[k[4:]] - g[k]).max()) for k in g.files if k.startswith("buf/") and "running" in k}
    # final/* weights and BatchNorm buffers of the reference after the 5 steps.  Every step moves a weight by about +-lr, so two
    # runs that disagree on the sign of a near-zero gradient differ by up to 2*5*lr there (measured max 0.041 = 8.3 lr); what
    # the bound catches is a wrong update size, a missed tensor or a wrong buffer, not bf16 noise.
    bad = []
    for k in g.files:
        if not (k.startswith("final/") and k.endswith("/digest")):
            continue
        name = k[6:-7]
        dg, smp = g[k], g[f"final/{name}/sample"]
        d, s = gu.tensor_digest(sd[name])
        if name.endswith("num_batches_tracked"):
            ok = int(sd[name]) == 5
        elif "running" in name:            # measured: mean |d| <= 0.11, var <= 12 % of its max (8x8x8 samples per channel at b=8);
            # 19 % on single channels of one layer with another tile geometry (the trajectory is chaotic, see above): the
            # per-channel bound is loose, and the norm of the whole buffer is held to 15 % (measured up to 8.4 %)
            # Bound per buffer: twice the oracle's own drift (floor: 2 % of the buffer's max + 0.01).  Measured drift of the oracle after
            # 5 steps: up to 0.78 (22 % of max) on dec.decoder.2.running_var, 0.12 (33 %) on enc.encoder.10.running_mean, < 1 % on
            # the first layers -- the old flat 25 %-of-max bound was looser than this on 11 of the 14 buffers.
            full = np.abs(sd[name] - g[f"buf/{name}"]).max()
            ok = full <= max(2.0 * spread[name], 0.02 * np.abs(g[f"buf/{name}"]).max() + 0.01) and 0.85 <= d[1] / max(dg[1], 1e-30) <= 1.15
        elif gu.is_prebn_bias(name) or (not head and name.startswith("classifier")):
            ok = True                      # zero-gradient biases: the reference random-walks them, the engine keeps them
        else:
            # (the norm of a tensor with a few dozen elements moves by several % with a handful of +-lr sign flips: big tensors only)
            ok = np.abs(s - smp).max() <= 2 * 5 * lr + 1e-3 and (sd[name].size < 1024 or 0.97 <= d[1] / dg[1] <= 1.03)
        if not ok:
            bad.append((name, float(np.abs(s - smp).max()), float(d[1] / max(dg[1], 1e-30))))
    assert not bad, bad


def test_one_adam_step_elementwise_vs_golden(golden):
    """After ONE step Adam has moved every weight by -lr*sign(g) (m_hat/sqrt(v_hat) = g/|g|), so the reference's parameters
    (ae_adam1_joint_b8.npz) are reproduced ELEMENTWISE except where a near-zero gradient changes sign under bf16: the fraction
    of sampled elements off by more than 1e-4 must stay small (a wrong gradient sign pattern, a skipped tensor or a wrong step
    size fails everywhere).  Measured on MI355X: see the bound's comment."""
    g = golden("ae_adam1_joint_b8.npz")
    m = _model()
    eng = _engine(m)
    x, y = gu.make_images(8, int(g["seed"]))
    lr = float(g["lr"])
    eng.train_step(_cuda(x), _cuda(y), float(g["alpha"]), lr)
    torch.cuda.synchronize()
    assert abs(float(eng.loss_last[0]) - float(g["loss"])) <= 0.02 * float(g["loss"])
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    rep, bad = [], []
    for k in g.files:
        if not (k.startswith("final/") and k.endswith("/sample")):
            continue
        name = k[6:-7]
        if "running" in name or "num_batches" in name or gu.is_prebn_bias(name):
            continue
        _, s = gu.tensor_digest(sd[name])
        err = np.abs(s - g[k])
        frac = float(np.mean(err < 1e-4))
        rep.append(f"{name:28s} same {frac:.3f} max {err.max():.2e}")
        # a sign flip moves an element by exactly 2*lr; nothing may move further
        if err.max() > 2 * lr + 1e-4 or (s.size >= 50 and frac < 0.90):
            bad.append((name, frac, float(err.max())))
    print("\n".join(rep))
    assert not bad, bad


def test_epoch_accounting_vs_golden(golden):
    """a6 (R.md:642-684): the reference's training epoch (batches 64, 64, 48, Adam) and eval-mode validation epoch (64, 56)
    through AEStepper: the device-side sample-weighted accumulators (loss, mse, ce, n, #correct) against the epoch means the
    reference's own loop produced (tests/golden/ae_epoch.npz).  bf16 path: means within 2 %, counts exact."""
    from eae_amd.train import AEStepper
    g = golden("ae_epoch.npz")
    m = _model()
    st = AEStepper(m, float(g["alpha"]), float(g["lr"]), max_batch=64)
    m.train()
    st.begin()
    per_batch = []
    for i, b in enumerate(g["train_batches"]):
        x, y = gu.make_images(int(b), int(g["train_seed0"]) + i)
        st.train_step(_cuda(x), _cuda(y))
        per_batch.append(st.eng.loss_last.cpu().numpy().copy())
    loss, mse, ce, n, _ = st.eng.read_loss()
    assert n == int(g["n_train"])
    assert abs(loss - g["train_epoch_loss"]) <= 0.02 * g["train_epoch_loss"], (loss, g["train_epoch_loss"])
    w = g["train_batches"] / g["train_batches"].sum()
    assert abs(mse - float((g["train_mse"] * w).sum())) <= 0.02 * float((g["train_mse"] * w).sum())
    assert abs(ce - float((g["train_ce"] * w).sum())) <= 0.03 * float((g["train_ce"] * w).sum())
    for i in range(3):
        assert abs(per_batch[i][0] - g["train_losses"][i]) <= 0.03 * g["train_losses"][i], (i, per_batch[i], g["train_losses"][i])
    assert st.end()[0] == loss
    m.eval()
    st.begin()
    for i, b in enumerate(g["val_batches"]):
        x, y = gu.make_images(int(b), int(g["val_seed0"]) + i)
        st.eval_step(_cuda(x), _cuda(y))
    loss, mse, ce, n, correct = st.eng.read_loss()
    assert n == int(g["n_val"])
    assert abs(loss - g["val_epoch_loss"]) <= 0.02 * g["val_epoch_loss"], (loss, g["val_epoch_loss"])
    wv = g["val_batches"] / g["val_batches"].sum()
    assert abs(mse - float((g["val_mse"] * wv).sum())) <= 0.02 * float((g["val_mse"] * wv).sum())
    assert abs(ce - float((g["val_ce"] * wv).sum())) <= 0.03 * float((g["val_ce"] * wv).sum())
    assert abs(correct - int(g["val_correct"])) <= 2      # argmax near-ties may flip under bf16 (120 samples, 10 classes at init)
    # and the eval-mode loss of ONE batch against the oracle with bf16 emulation (tight)
    p = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    x, y = gu.make_images(56, int(g["val_seed0"]) + 1)
    st.begin()
    st.eval_step(_cuda(x), _cuda(y))
    loss, mse, ce, n, correct = st.eng.read_loss()
    out = O.ae_forward(p, x, train=False, quant="bf16")
    rl, rm, rc = O.ae_loss(out, x, y, float(g["alpha"]))
    assert n == 56 and abs(loss - rl) <= 3e-3 * rl and abs(mse - rm) <= 3e-3 * rm and abs(ce - rc) <= 5e-3 * rc, (loss, rl, mse, rm, ce, rc)
    assert abs(correct - int((out["logits"].argmax(1) == y).sum())) <= 1


def test_determinism():
    x, y = gu.make_images(8, 100)
    outs = []
    for _ in range(2):
        m = _model()
        eng = _engine(m)
        for s in range(2):
            eng.train_step(_cuda(x), _cuda(y), 35.0, 5e-3)
        torch.cuda.synchronize()
        assert eng.gate_timeouts() == 0
        outs.append(eng.params.cpu().numpy().copy())
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("n,b", [(3, 16), (8, 64), (10, 8)])
def test_grouped_step_is_bitwise_each_configuration_alone(n, b):
    """eae_group_train_step (R.md:599-711: the grid's configurations share the architecture, not alpha / lr / weights / batches): n engines
    stepped by ONE sequence of grouped launches.  Every member ends bitwise where it ends when it is stepped alone with the same tile
    geometries (eae_set_geometry_mult(n): the launchers then choose grids as the grouped step does) -- parameters, Adam moments,
    BatchNorm buffers, the device-side loss sums, and the next eval forward.  n = 10 > 8: more members than one launch carries."""
    from eae_amd import _lib
    from eae_amd.engine import AEEngine
    lib = _lib.load()
    alphas = [35.0 + 3.0 * k for k in range(n)]
    lrs = [1e-3 * (1 + k % 3) for k in range(n)]
    data = [tuple(_cuda(t) for t in gu.make_images(b, 200 + k)) for k in range(n)]

    def fresh():
        out = []
        for k in range(n):
            m = _model()
            g = torch.Generator(device="cuda").manual_seed(900 + k)
            with torch.no_grad():
                for p_ in m.parameters():          # own weights per member
                    p_.add_(0.02 * p_.abs().mean() * torch.randn(p_.shape, device="cuda", generator=g))
            out.append((m, _engine(m, max_batch=64)))
        return out

    def snap(e, xd, yd, a):
        xh, lg, z = e.forward(xd, labels=yd, train=False, alpha=a)
        torch.cuda.synchronize()
        return [t.clone() for t in (e.params, e.adam_m, e.adam_v, e.bn_running, e.loss_accum, e.loss_last, xh, lg, z)]

    grouped = fresh()
    for _ in range(3):
        AEEngine.group_train_step([e for _, e in grouped], [d[0] for d in data], [d[1] for d in data], alphas, lrs)
    torch.cuda.synchronize()
    assert all(e.gate_timeouts() == 0 for _, e in grouped)
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
    # (and the members are different trainings: not one result n times)
    assert not torch.equal(got[0][0], got[1][0])


def test_data_parallel_trainer_world1_rccl():
    """The DP step (grad_step -> bucketed all-reduce over RCCL -> adam_step) on a 1-rank NCCL group equals the fused
    single-GPU train_step bit for bit (the multi-rank arithmetic is covered on CPU by tests/test_dp_gloo.py)."""
    import os
    import torch.distributed as dist
    from eae_amd import dp
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29400 + os.getpid() % 500))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
        created = True
    try:
        x, y = gu.make_images(8, 100)
        xd, yd = _cuda(x), _cuda(y)
        ma = _model()
        ea = _engine(ma)
        for _ in range(2):
            ea.train_step(xd, yd, 35.0, 5e-3)
        torch.cuda.synchronize()
        # (1) the engine-owned RCCL communicator (eae_dp_init / eae_ae_dp_train_step), overlapped and serial; (2) torch.distributed
        for native, overlap in ((True, "1"), (True, "0"), (False, "0")):
            os.environ["EAE_DP_OVERLAP"] = overlap
            mb = _model()
            eb = _engine(mb)
            tr = dp.DataParallelTrainer(eb, native=native)
            assert tr.native == native and tr.rccl_ranks() == (1 if native else 0)
            tr.broadcast_parameters()
            for _ in range(2):
                tr.train_step(xd, yd, 35.0, 5e-3)
            torch.cuda.synchronize()
            assert eb.gate_timeouts() == 0
            assert torch.equal(ea.params, eb.params), (native, overlap)
            assert torch.equal(ea.adam_m, eb.adam_m) and torch.equal(ea.bn_running, eb.bn_running)
            if native:       # the bucket entry point by itself: a 1-rank sum leaves the arena untouched
                from eae_amd._lib import check
                import gpu_util as G
                g0 = eb.grads.clone()
                check(eb.lib.eae_dp_allreduce_bucket(eb.ctx, G.stream(), eb.poff[18], eb.poff[38] - eb.poff[18]))
                torch.cuda.synchronize()
                assert torch.equal(g0, eb.grads)
            # the refusal switch travels through the exchange: a step whose input is non-finite sets the step-wide word on
            # this rank; the word is max-reduced over the ranks (here: one) and the optimizer leaves every parameter untouched
            p0, m0 = eb.params.clone(), eb.adam_m.clone()
            xbad = xd.clone()
            xbad[3, 1, 10, 10] = float("inf")
            tr.train_step(xbad, yd, 35.0, 5e-3)
            torch.cuda.synchronize()
            assert torch.equal(p0, eb.params) and torch.equal(m0, eb.adam_m), (native, overlap)
            tr.train_step(xd, yd, 35.0, 5e-3)      # ... and the next clean step updates again (the word is per step)
            torch.cuda.synchronize()
            assert not torch.equal(p0, eb.params) and bool(torch.isfinite(eb.params).all())
    finally:
        os.environ.pop("EAE_DP_OVERLAP", None)
        if created:
            dist.destroy_process_group()


def test_autograd_drop_in_loop_matches_fused_step(golden):
    """The reference's own loop shape (R.md:646-654): torch losses + loss.backward() + torch.optim.Adam on the module
    shells.  Gradients must equal the fused eae_ae_grad_step path (same kernels; only sigmoid/MSE/CE run in torch)."""
    import torch.nn as nn
    g = golden("ae_fwd_bwd_b8.npz")
    x, y = _cuda(g["x"]), _cuda(g["labels"])
    alpha = float(g["alpha"])
    m1, m2 = _model(), _model()
    e1 = _engine(m1)
    e1.grad_step(x, y, alpha)
    e1.expose_grads()
    m2.train()
    opt = torch.optim.Adam(m2.parameters(), lr=5e-3)
    opt.zero_grad()
    x_hat, logits, _ = m2(x)
    loss = alpha * nn.MSELoss()(x_hat, x) + nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    assert abs(float(loss) - float(g["loss"])) <= 0.02 * abs(float(g["loss"]))
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        a, b = p1.grad.cpu().numpy(), p2.grad.cpu().numpy()
        scale = max(1e-12, np.abs(a).max())
        # the fused path rounds the loss gradient to bf16 at the same point; tiny differences come from fp32 sigmoid/MSE in torch
        assert np.abs(a - b).max() <= 2e-2 * scale, (n1, np.abs(a - b).max() / scale)
    w0 = m2.enc.encoder[0].weight.detach().clone()
    opt.step()
    assert not torch.equal(w0, m2.enc.encoder[0].weight)
    with torch.no_grad():          # parameters were changed by a torch optimizer: the next forward repacks them
        m2.eval()
        xh2, _, _ = m2(x)
    assert torch.isfinite(xh2).all()


@pytest.mark.skipif(bool(os.environ.get("EAE_NO_FOLD_BWD")), reason="the eval-mode backward is built on the folded BatchNorm-backward finalize")
def test_autograd_through_an_eval_mode_model_vs_torch_cpu_port(golden):
    """`model.eval(); loss.backward()` (fine-tuning with frozen BatchNorm statistics): BatchNorm normalises with the running
    statistics and is differentiated as the per-channel affine map it then is.  Gradients against torch autograd of the torch-CPU
    port of the reference graph (oracle/ae_torch_cpu.py, itself pinned by the goldens) in eval mode; buffers untouched."""
    import torch.nn as nn
    import gpu_util as G
    from oracle import ae_torch_cpu as T
    g = golden("ae_fwd_bwd_b8.npz")
    x, y = g["x"], g["labels"]
    alpha = float(g["alpha"])
    sd = ae_state_np()
    p = T.build(state=sd)
    m = _model()
    m.eval()
    rv_before = m.enc.encoder[1].running_var.detach().clone()
    xh, lg, z = m(_cuda(x))
    loss = alpha * nn.MSELoss()(xh, _cuda(x)) + nn.CrossEntropyLoss()(lg, _cuda(y))
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(rv_before, m.enc.encoder[1].running_var) and int(m.enc.encoder[1].num_batches_tracked) == 0
    # reference: the same graph in torch on the CPU, eval mode
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    xr, lr_, _ = T.forward(p, xt, train=False)
    lref = alpha * nn.functional.mse_loss(xr, xt) + nn.functional.cross_entropy(lr_, yt)
    lref.backward()
    assert abs(float(loss) - float(lref)) <= 0.02 * abs(float(lref))
    assert np.abs(xh.detach().cpu().numpy() - xr.detach().numpy()).max() <= 3e-2
    bad = []
    for name, prm in m.named_parameters():
        ref = p[name].grad.numpy()
        got = prm.grad.cpu().numpy()
        # (in eval mode a bias in front of a BatchNorm DOES get a gradient: the normalisation no longer removes it)
        c = G.cosine(got, ref)
        ratio = np.linalg.norm(got) / max(np.linalg.norm(ref), 1e-30)
        if not (c > 0.97 and 0.9 <= ratio <= 1.1):
            bad.append((name, round(c, 4), round(float(ratio), 3)))
    assert not bad, bad
    # a SECOND eval-mode backward right behind the first (fine-tuning with an external optimizer: no engine-side Adam in between that
    # would clear the BatchNorm-backward accumulators): the same gradients, bit for bit -- the sums of the first pass must not pile up
    first = {name: prm.grad.detach().clone() for name, prm in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    xh2, lg2, _ = m(_cuda(x))
    (alpha * nn.MSELoss()(xh2, _cuda(x)) + nn.CrossEntropyLoss()(lg2, _cuda(y))).backward()
    torch.cuda.synchronize()
    for name, prm in m.named_parameters():
        assert torch.equal(prm.grad, first[name]), name
    # a train-mode gradient step afterwards: the biases in front of the BatchNorms have an identically zero gradient again
    eng = _engine(m)
    eng.grad_step(_cuda(x), _cuda(y), alpha)
    torch.cuda.synchronize()
    eng.expose_grads()
    for name, prm in m.named_parameters():
        if gu.is_prebn_bias(name):
            assert float(prm.grad.abs().max()) == 0.0, name


def test_autograd_through_stand_alone_encoder_and_decoder(golden):
    """The notebook defines Encoder and Decoder as modules of their own (R.md:287, 361).  A plain autoencoder composed by hand,
    `x_hat = dec(enc(x))` with an MSE loss and loss.backward(), must give the gradients of the fused reconstruction-only step
    (head=False, alpha=1) of a SupervisedAutoencoder holding the same weights: same kernels, only the loss gradient comes from torch."""
    import torch.nn as nn
    import eae_amd
    g = golden("ae_fwd_bwd_b8.npz")
    x = _cuda(g["x"])
    sd = ae_state_np()
    m = _model()
    e = _engine(m)
    e.grad_step(x, _cuda(g["labels"]), 1.0, head=False)
    e.expose_grads()
    ref = {n: p.grad.clone() for n, p in m.named_parameters()}
    enc, dec = eae_amd.Encoder(latent_dim=64), eae_amd.Decoder(latent_dim=64)
    load_state_np(enc, {k[4:]: v for k, v in sd.items() if k.startswith("enc.")})
    load_state_np(dec, {k[4:]: v for k, v in sd.items() if k.startswith("dec.")})
    enc, dec = enc.cuda().train(), dec.cuda().train()
    z = enc(x)
    assert z.requires_grad and tuple(z.shape) == (8, 64)
    x_hat = dec(z)
    loss = nn.MSELoss()(x_hat, x)
    loss.backward()
    torch.cuda.synchronize()
    for mod, prefix in ((enc, "enc."), (dec, "dec.")):
        for n, p in mod.named_parameters():
            a, b = ref[prefix + n].cpu().numpy(), p.grad.cpu().numpy()
            scale = max(1e-12, np.abs(a).max())
            assert np.abs(a - b).max() <= 2e-2 * scale, (prefix + n, np.abs(a - b).max() / scale)
    # a second forward before the backward invalidates the first one's activations: raises instead of differentiating the wrong batch
    z1 = enc(x)
    _ = enc(x)
    with pytest.raises(Exception, match="later forward"):
        z1.sum().backward()
    # no-grad / eval use is unchanged (extract_features' call shape, R.md:2504)
    enc.eval()
    with torch.no_grad():
        z2 = enc(x)
    assert not z2.requires_grad and torch.isfinite(z2).all()


def test_autograd_temporary_noncontiguous_input_and_stale_forward(golden):
    """The backward reads the input batch again (conv1's weight gradient).  It must be the autograd node's own saved copy: a
    temporary (`model(imgs + noise)`) or a non-contiguous input is gone when backward runs, and the allocator hands its memory
    to the next tensor.  A second forward before the backward replaces the resident activations: that must raise, not
    silently differentiate the wrong batch."""
    import torch.nn as nn
    g = golden("ae_fwd_bwd_b8.npz")
    x, y = _cuda(g["x"]), _cuda(g["labels"])
    alpha = float(g["alpha"])
    m1 = _model()
    e1 = _engine(m1)
    e1.grad_step(x, y, alpha)
    e1.expose_grads()
    ref = {n: p.grad.clone() for n, p in m1.named_parameters()}
    for variant in ("temporary", "channels_last"):
        m2 = _model()
        m2.train()
        if variant == "temporary":
            x_hat, logits, _ = m2(x + 0.0)                     # nothing but the autograd node holds this tensor
        else:
            xin = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            assert not xin.is_contiguous()
            x_hat, logits, _ = m2(xin)
            del xin
        loss = alpha * nn.MSELoss()(x_hat, x) + nn.CrossEntropyLoss()(logits, y)
        junk = [torch.full_like(x, 7.0) for _ in range(4)]      # recycle whatever the forward's temporaries freed
        torch.cuda.synchronize()
        loss.backward()
        del junk
        for n, p in m2.named_parameters():
            a, b = ref[n].cpu().numpy(), p.grad.cpu().numpy()
            assert np.abs(a - b).max() <= 2e-2 * max(1e-12, np.abs(a).max()), (variant, n)
    m3 = _model()
    m3.train()
    out1 = m3(x)
    out2 = m3(x)
    with pytest.raises(RuntimeError, match="later forward"):
        (out1[0].sum()).backward()
    (out2[0].sum()).backward()                                  # the resident forward still differentiates


def test_graph_replay_equals_eager():
    """With EAE_GRAPH=1, from the third call with the same buffers the train step is replayed from a captured hipGraph;
    the result must be bit-identical to the eager launch sequence."""
    import os
    x, y = gu.make_images(8, 100)
    xd, yd = _cuda(x), _cuda(y)
    res = []
    for no_graph in (False, True):
        if no_graph:
            os.environ.pop("EAE_GRAPH", None)
        else:
            os.environ["EAE_GRAPH"] = "1"
        try:
            m = _model()
            eng = _engine(m)
            for s in range(7):
                eng.train_step(xd, yd, 35.0, 5e-3)
            torch.cuda.synchronize()
            res.append((eng.params.cpu().numpy().copy(), eng.bn_running.cpu().numpy().copy(), eng.loss_accum.cpu().numpy().copy(),
                        int(m.state_dict()["enc.encoder.1.num_batches_tracked"])))
        finally:
            os.environ.pop("EAE_GRAPH", None)
    assert np.array_equal(res[0][0], res[1][0]), np.abs(res[0][0] - res[1][0]).max()
    assert np.array_equal(res[0][1], res[1][1]), np.abs(res[0][1] - res[1][1]).max()
    assert np.array_equal(res[0][2], res[1][2]), (res[0][2], res[1][2])
    assert res[0][3] == res[1][3] == 7
    assert np.isfinite(res[0][0]).all()


def test_ce_mse_ratio_probe_vs_oracle():
    """R.md:501-519: fresh latent-128 models, train-mode forward under no_grad, ratio CE/MSE; each trial's parameters are
    captured and replayed through the bf16-emulating oracle.  BN running statistics must have been updated (Appendix A.9)."""
    import eae_amd
    x, y = gu.make_images(16, 321)
    states = []

    def grab(i, model):
        states.append({k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})

    torch.manual_seed(77)
    ratios = eae_amd.ce_mse_ratio_probe([(torch.from_numpy(x), torch.from_numpy(y))], n_models=3, on_model=grab)
    assert len(ratios) == 3 and len(states) == 3
    assert not np.array_equal(states[0]["enc.encoder.0.weight"], states[1]["enc.encoder.0.weight"])       # re-drawn every trial
    assert int(states[1]["enc.encoder.1.num_batches_tracked"]) == 0                                     # and BN buffers reset
    for r, sd in zip(ratios, states):
        out = O.ae_forward(sd, x, train=True, quant="bf16")
        _, l_r, l_c = O.ae_loss(out, x, y, 1.0)
        assert abs(r - float(l_c) / float(l_r)) <= 1e-2 * float(l_c) / float(l_r), (r, l_c, l_r)
        assert 5.0 < r < 100.0           # the reference's histogram sits around 25-38 for real images (R.md:532)


def test_ce_mse_ratio_probe_concurrent_trials_vs_oracle():
    """SURVEY 8f N4 with concurrent=K: K model + engine pairs on K streams, the parameter draws still one sequence in trial order (a
    turnstile hands torch's generator from trial to trial).  Every trial's captured parameters replayed through the bf16 oracle; the
    trials are captured in order; a second run with the same seed gives the same ratios (the forwards overlap, the draws do not)."""
    import eae_amd
    x, y = gu.make_images(16, 321)
    runs = []
    for _ in range(2):
        states, order = [], []

        def grab(i, model):
            order.append(i)
            states.append({k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})

        torch.manual_seed(78)
        ratios = eae_amd.ce_mse_ratio_probe([(torch.from_numpy(x), torch.from_numpy(y))], n_models=7, on_model=grab, concurrent=3)
        assert order == list(range(7)) and len(ratios) == 7
        runs.append((ratios, states))
    assert runs[0][0] == runs[1][0]
    for r, sd in zip(*runs[0]):
        out = O.ae_forward(sd, x, train=True, quant="bf16")
        _, l_r, l_c = O.ae_loss(out, x, y, 1.0)
        assert abs(r - float(l_c) / float(l_r)) <= 1e-2 * float(l_c) / float(l_r), (r, l_c, l_r)
    assert len({s["enc.encoder.0.weight"].tobytes() for s in runs[0][1]}) == 7          # seven different draws


PRE_BN_BIAS = {f"enc.encoder.{i}.bias" for i in (0, 3, 6, 9)} | {f"dec.decoder.{i}.bias" for i in (1, 4, 7)}


def test_image128_forward_and_gradients_vs_oracle():
    """Runtime spatial size: a 128x128 input (fc over 256*8*8 features; towards BASELINE config 5).  The reference has no
    such case (parity unpinned by it); checked against the bf16-emulating oracle only."""
    import eae_amd
    import gpu_util as G
    torch.manual_seed(5)
    m = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=10, image_size=128)
    p = gu.perturb_bn({k: v.detach().numpy().copy() for k, v in m.state_dict().items()})
    load_state_np(m, p)
    m = m.to("cuda")
    rng = np.random.default_rng(9)
    x = rng.random((3, 3, 128, 128)).astype(np.float32)
    y = rng.integers(0, 10, 3).astype(np.int64)
    eng = _engine(m, max_batch=4)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    torch.cuda.synchronize()
    out = O.ae_forward(p, x, train=True, quant="bf16")
    assert np.abs(z.cpu().numpy() - out["z"]).max() <= 6e-3 * np.abs(out["z"]).max()
    assert np.abs(lg.cpu().numpy() - out["logits"]).max() <= 6e-3 * np.abs(out["logits"]).max()
    d = np.abs(xh.cpu().numpy() - out["x_hat"])
    assert d.max() <= 1.5e-2 and d.mean() <= 1.5e-3, (d.max(), d.mean())
    m2 = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=10, image_size=128)
    load_state_np(m2, p)
    m2 = m2.to("cuda")
    eng2 = _engine(m2, max_batch=4)
    eng2.grad_step(_cuda(x), _cuda(y), 35.0)
    torch.cuda.synchronize()
    eng2.expose_grads()
    gq = O.ae_backward(p, out, x, y, 35.0, quant="bf16")
    bad = []
    for name, prm in m2.named_parameters():
        got = prm.grad.cpu().numpy()
        ref = gq[name]
        if name in PRE_BN_BIAS:                 # analytically zero gradient: the engine writes exact zeros
            assert np.abs(got).max() == 0.0 and np.abs(ref).max() <= 1e-3 * max(1.0, np.abs(gq[name.replace("bias", "weight")]).max()), name
            continue
        if not G.cosine(got, ref) > 0.995:
            bad.append((name, G.cosine(got, ref)))
    assert not bad, bad


def test_config5_shape_256px_latent256_vs_oracle():
    """BASELINE config 5's shape (256x256 inputs, 256-d latent) in bf16 (its fp8 MFMA variant is not built): forward, losses
    and all gradients against the bf16-emulating oracle.  The reference holds no vector for this shape (parity unpinned by it)."""
    import eae_amd
    import gpu_util as G
    torch.manual_seed(6)
    m = eae_amd.SupervisedAutoencoder(latent_dim=256, num_classes=10, image_size=256)
    p = gu.perturb_bn({k: v.detach().numpy().copy() for k, v in m.state_dict().items()})
    load_state_np(m, p)
    m = m.to("cuda")
    rng = np.random.default_rng(10)
    x = rng.random((2, 3, 256, 256)).astype(np.float32)
    y = rng.integers(0, 10, 2).astype(np.int64)
    eng = _engine(m, max_batch=2)
    eng.grad_step(_cuda(x), _cuda(y), 35.0)
    torch.cuda.synchronize()
    eng.expose_grads()
    out = O.ae_forward(p, x, train=True, quant="bf16")
    loss, l_r, l_c = O.ae_loss(out, x, y, 35.0)
    got_loss = eng.loss_last.cpu().numpy()
    assert abs(got_loss[1] - l_r) <= 2e-2 * l_r and abs(got_loss[2] - l_c) <= 2e-2 * abs(l_c), (got_loss, l_r, l_c)
    gq = O.ae_backward(p, out, x, y, 35.0, quant="bf16")
    bad = []
    for name, prm in m.named_parameters():
        got = prm.grad.cpu().numpy()
        if name in PRE_BN_BIAS:
            assert np.abs(got).max() == 0.0, name
            continue
        c = G.cosine(got, gq[name])
        if not c > 0.99:
            bad.append((name, c))
    assert not bad, bad


def test_full_size_batch512_properties():
    """BASELINE config c3 size (B=512), where the oracle is too slow: size-independent properties instead.
    (1) eval-mode forward is per-image: one B=512 call == eight B=64 calls, bitwise;
    (2) the gradient is affine in alpha (loss = alpha*MSE + CE): g(35)-g(20) == 1.5*(g(30)-g(20)) within bf16 noise;
    (3) two identical gradient steps from the same state are bitwise equal (no atomics anywhere)."""
    import gpu_util as G
    x, y = gu.make_images(512, 777)
    xd, yd = _cuda(x), _cuda(y)
    m = _model()
    m.eval()
    eng = _engine(m, max_batch=512)
    xh, lg, z = eng.forward(xd, labels=yd, train=False, alpha=35.0)
    torch.cuda.synchronize()
    for k in range(0, 512, 64):
        xh_k, lg_k, z_k = eng.forward(xd[k:k + 64].contiguous(), labels=yd[k:k + 64].contiguous(), train=False, alpha=35.0)
        torch.cuda.synchronize()
        assert torch.equal(z_k, z[k:k + 64]) and torch.equal(lg_k, lg[k:k + 64]) and torch.equal(xh_k, xh[k:k + 64]), k
    grads = {}
    for alpha in (20.0, 30.0, 35.0, 35.0):
        m2 = _model()
        e2 = _engine(m2, max_batch=512)
        e2.grad_step(xd, yd, alpha)
        torch.cuda.synchronize()
        g = e2.grads.cpu().numpy().copy()
        if alpha in grads:
            assert np.array_equal(grads[alpha], g)              # (3)
        grads[alpha] = g
    d35, d30 = grads[35.0] - grads[20.0], grads[30.0] - grads[20.0]
    assert G.cosine(d35, 1.5 * d30) > 0.999 and G.relmax(d35, 1.5 * d30) < 3e-2, (G.cosine(d35, 1.5 * d30), G.relmax(d35, 1.5 * d30))


def test_encoder_decoder_alone_in_train_mode_repeatable():
    """Encoder.forward / Decoder.forward on their own in TRAIN mode (batch statistics): the folded BatchNorm accumulators must
    be clean for every call, whatever ran before -- the same call twice (running stats restored in between) gives the same
    bits, and it agrees with the full forward's z / x_hat."""
    x, y = gu.make_images(8, 55)
    xd, yd = _cuda(x), _cuda(y)
    m = _model()
    m.train()
    eng = _engine(m)
    bn0 = eng.bn_running.clone(); nbt0 = eng.bn_nbt.clone()
    xh_f, lg_f, z_f = eng.forward(xd, labels=yd, train=True, alpha=35.0)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        eng.bn_running.copy_(bn0); eng.bn_nbt.copy_(nbt0)
        z = eng.encoder(xd, train=True)
        xh = eng.decoder(z, train=True)
        torch.cuda.synchronize()
        outs.append((z.clone(), xh.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][0], z_f) and torch.equal(outs[0][1], xh_f)


def test_non_finite_input_poisons_the_step_like_the_reference():
    """A diverged run must look diverged (the reference's grid contains learning rates that blow up, R.md:2447-2450): a
    non-finite activation has to reach the loss through the fixed-point BatchNorm statistics as NaN, not as a finite number."""
    x, y = gu.make_images(8, 11)
    x = x.copy()
    x[3, 1, 10, 10] = np.inf
    m = _model()
    eng = _engine(m)
    xh, lg, z = eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    torch.cuda.synchronize()
    assert not np.isfinite(eng.loss_last.cpu().numpy()[0])
    # (z itself may come out finite: the packed-bf16 ReLU is an integer max, which sends negative-signed NaNs to 0 where
    #  torch.relu keeps them -- DESIGN.md section 5, deviations; a diverged PARAMETER always reaches the loss)
    # and the next, finite batch is unaffected by what the poisoned one left in the accumulators
    x2, y2 = gu.make_images(8, 100)
    m2 = _model()
    e2 = _engine(m2)
    ref = [t.clone() for t in e2.forward(_cuda(x2), labels=_cuda(y2), train=True, alpha=35.0)]
    eng.bn_running.copy_(e2.bn_running); eng.bn_nbt.copy_(e2.bn_nbt)
    m3 = _model()
    e3 = _engine(m3)
    e3.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0)
    load_state_np(m3, ae_state_np())
    e3.params_changed()
    got = e3.forward(_cuda(x2), labels=_cuda(y2), train=True, alpha=35.0)
    torch.cuda.synchronize()
    assert torch.equal(got[2], ref[2]) and torch.equal(got[0], ref[0])


def test_nan_exact_switch_reproduces_what_a_diverged_step_does_to_the_reference_model(golden, monkeypatch):
    """EAE_NAN_EXACT=1 (parity gap 6c): after a non-finite step the reference's model is NaN in EVERY parameter and both
    Adam moments (tests/golden/ae_nan_step_b8.npz, generated by driving the reference's own classes through one step of R.md:646-654
    with x[3, 1, 10, 10] = inf); with the switch the engine's replica is too.  Default (switch off): the optimizer refuses the update
    and parameters and moments keep their last finite values -- the documented deviation of DESIGN.md section 5."""
    g = golden("ae_nan_step_b8.npz")
    assert np.isnan(float(g["loss"]))
    pf = {k.split("/", 1)[1]: float(g[k]) for k in g.files if k.startswith("nan_frac/") and "running" not in k and "num_batches" not in k}
    assert len(pf) == 38 and all(v == 1.0 for v in pf.values())           # what the reference does: everything is NaN
    assert all(float(g[k]) == 1.0 for k in g.files if k.startswith("nan_frac_m/") or k.startswith("nan_frac_v/"))
    x, y = gu.make_images(8, int(g["seed"]))
    x = x.copy()
    x[3, 1, 10, 10] = np.inf
    for exact in ("1", "0"):
        monkeypatch.setenv("EAE_NAN_EXACT", exact)
        m = _model()
        eng = _engine(m)
        p0 = eng.params.clone()
        eng.train_step(_cuda(x), _cuda(y), float(g["alpha"]), float(g["lr"]))
        torch.cuda.synchronize()
        assert not np.isfinite(eng.loss_last.cpu().numpy()[0])
        if exact == "1":
            for name, prm in m.named_parameters():
                assert bool(torch.isnan(prm).all()), name                 # the module's parameters are views of the arena
            assert bool(torch.isnan(eng.adam_m).all()) and bool(torch.isnan(eng.adam_v).all())
        else:
            assert torch.equal(p0, eng.params) and bool((eng.adam_m == 0).all())


def _stall(seconds):
    """Keep the CURRENT stream busy for about `seconds`: many short torch.cuda._sleep kernels (it spins for a number of shader-clock
    ticks: one long count overflows its 32-bit counter, and a single calibration taken on an idle, down-clocked GPU is several times
    too long -- the probe is timed three times after a warm-up and the SHORTEST is used, so the stall is at least as long as asked)."""
    probe = 20_000_000
    torch.cuda._sleep(probe); torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); torch.cuda._sleep(probe); e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    per_probe = max(min(times), 1e-4)
    for _ in range(min(int(seconds / per_probe) + 1, 20000)):
        torch.cuda._sleep(probe)


def test_caller_stream_stalled_for_seconds_in_front_of_a_step_is_waited_for():
    """the side-stream gates used to give up after ~2 s and let the weight-gradient kernels run before the kernels
    they depend on.  The spin is now bounded by 30 s of wall clock: a step enqueued behind a 2.6 s stall of the caller's stream
    (a late data-parallel peer, a long copy; > 2 s, the old bound) produces the same gradients, bit for bit, as an unstalled one."""
    x, y = gu.make_images(8, 321)
    ma, mb = _model(), _model()
    ea, eb = _engine(ma), _engine(mb)
    xd, yd = _cuda(x), _cuda(y)           # (device copies BEFORE the stall: a pageable H2D copy would wait for the stalled stream on the host)
    ea.grad_step(xd, yd, 35.0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _stall(3.0)
    eb.grad_step(xd, yd, 35.0)
    e1.record()
    torch.cuda.synchronize()
    assert e0.elapsed_time(e1) > 2100.0     # the step really was enqueued behind a stall longer than the old 2 s bound
    assert eb.gate_timeouts() == 0
    assert torch.equal(ea.grads, eb.grads)


@pytest.mark.skipif(bool(os.environ.get("EAE_NO_SIDE_STREAM") or os.environ.get("EAE_FORK_EVENTS")), reason="event hand-overs / no side streams: nothing is gated")
def test_a_gate_timeout_is_loud(monkeypatch):
    """... and a gate that does time out (bound lowered to 100 ms for this context) cannot go unnoticed: the sticky word makes the
    optimizer kernel leave the parameters untouched and write NaN losses, check_gates() / AEStepper.end() raise."""
    from eae_amd._lib import EaeError
    from eae_amd.train import AEStepper
    monkeypatch.setenv("EAE_GATE_TIMEOUT_MS", "100")
    x, y = gu.make_images(8, 321)
    m = _model()
    eng = _engine(m)
    monkeypatch.delenv("EAE_GATE_TIMEOUT_MS")
    xd, yd = _cuda(x), _cuda(y)
    eng.train_step(xd, yd, 35.0, 5e-3)          # a normal step first
    torch.cuda.synchronize()
    assert eng.gate_timeouts() == 0 and np.isfinite(float(eng.loss_last[0]))
    p0 = eng.params.clone()
    _stall(0.8)
    eng.train_step(xd, yd, 35.0, 5e-3)
    torch.cuda.synchronize()
    assert eng.gate_timeouts() != 0
    assert torch.equal(eng.params, p0)                       # no update from gradients that may be stale
    assert np.isnan(float(eng.loss_last[0]))
    with pytest.raises(EaeError):
        eng.check_gates()
    st = AEStepper(m, 35.0, 5e-3, max_batch=64)
    st.begin()
    with pytest.raises(EaeError):
        st.end()
    eng.clear_gate_timeouts()
    eng.train_step(xd, yd, 35.0, 5e-3)
    torch.cuda.synchronize()
    assert eng.gate_timeouts() == 0 and not torch.equal(eng.params, p0) and np.isfinite(float(eng.loss_last[0]))


def test_autograd_half_guards():
    """(1) an Encoder whose INPUT requires grad must not silently return no input gradient; (2) dec(enc(x)) on the two
    halves of one SupervisedAutoencoder (one shared engine workspace) is refused at forward time with a pointer to model(x)."""
    import eae_amd
    x, y = gu.make_images(4, 5)
    enc = eae_amd.Encoder(64).cuda().train()
    xi = _cuda(x).requires_grad_(True)
    with pytest.raises(RuntimeError, match="does not compute dL/dx"):
        enc(xi)
    m = _model(); m.train()
    z = m.enc(_cuda(x))
    with pytest.raises(RuntimeError, match="call model"):
        m.dec(z)
    # the resident encoder forward is still differentiable after the refused call
    z.sum().backward()
    assert m.enc.encoder[0].weight.grad is not None and torch.isfinite(m.enc.encoder[0].weight.grad).all()


@pytest.mark.parametrize("b", [64, 512])
def test_nan_parameter_poisons_the_statistics_at_any_batch_size(b):
    """non-finite partials used to travel INSIDE the wrapping fixed-point sums (2^61 each): a power-of-two number of poisoned
    workgroups per accumulator copy cancelled mod 2^64 and the statistics came out finite (mean 0, var 0).  They now set a sticky
    per-channel flag: a NaN weight of enc.conv2 gives NaN running statistics for exactly its channel, at every batch size.  What the
    NaN DATA does downstream is not reliable (the packed-bf16 ReLU of the consumers is an integer max: a negative-signed NaN becomes 0 --
    measured: every later layer stayed finite), so the consumer that finds a flagged channel also sets a step-wide word: the losses
    read NaN like the reference's, and the optimizer kernel leaves the parameters untouched (a diverged configuration of the grid,
    R.md:2447, stays visibly diverged instead of training on garbage)."""
    x, y = gu.make_images(b, 12)
    m = _model()
    eng = _engine(m, max_batch=b)
    with torch.no_grad():
        m.enc.encoder[3].weight[5, 0, 0, 0] = float("nan")
    eng.params_changed()
    eng.forward(_cuda(x), labels=_cuda(y), train=True, alpha=35.0, want=())
    torch.cuda.synchronize()
    assert np.isnan(eng.loss_last.cpu().numpy()[:3]).all()
    rv, rm = m.enc.encoder[4].running_var, m.enc.encoder[4].running_mean
    assert bool(torch.isnan(rv[5])) and bool(torch.isnan(rm[5]))
    assert bool(torch.isfinite(rv[:5]).all()) and bool(torch.isfinite(rv[6:]).all())      # like the reference: only that channel
    # a full train step on the poisoned model: NaN losses, no update
    before = eng.params.clone()
    eng.train_step(_cuda(x), _cuda(y), 35.0, 1e-3)
    torch.cuda.synchronize()
    assert np.isnan(eng.loss_last.cpu().numpy()[:3]).all()
    same = (eng.params == before) | (torch.isnan(eng.params) & torch.isnan(before))
    assert bool(same.all())
    # ... and the word is per step: the repaired model trains again
    load_state_np(m, ae_state_np())
    eng.params_changed()
    eng.train_step(_cuda(x), _cuda(y), 35.0, 1e-3)
    torch.cuda.synchronize()
    assert np.isfinite(eng.loss_last.cpu().numpy()[:3]).all() and not torch.equal(eng.params, before)


def test_two_adam_steps_running_statistics_vs_golden(golden):
    """BatchNorm running statistics at a TIGHT tolerance, before the Adam trajectory turns chaotic.  Reference run:
    two joint steps at B=32 with every buffer recorded after each (tests/golden/ae_adam2_bn_b32.npz, tools/make_golden.py --round3).
    After step 1 the buffers only depend on the forward: momentum 0.1, UNBIASED variance, num_batches_tracked -- held to 5e-3 of the
    buffer's max (the bf16-emulating oracle measures 8.7e-4).  After step 2 the weights have moved by +-lr: the bf16 oracle itself is
    5.9e-2 off on its worst buffer, so each buffer is held to max(2e-2, 2 x the oracle's own deviation measured here) of its max."""
    g = golden("ae_adam2_bn_b32.npz")
    alpha, lr = float(g["alpha"]), float(g["lr"])
    m = _model()
    eng = _engine(m)
    po = {k: v.copy() for k, v in ae_state_np().items()}
    so = O.new_adam_state()
    for step in (1, 2):
        x, y = gu.make_images(32, 800 + step - 1)
        eng.train_step(_cuda(x), _cuda(y), alpha, lr)
        torch.cuda.synchronize()
        O.ae_train_step(po, so, x, y, alpha, lr, quant="bf16")
        assert abs(float(eng.loss_last[0]) - float(g["losses"][step - 1])) <= 1e-2 * float(g["losses"][step - 1])
        sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        bad = []
        for k in g.files:
            if not k.startswith(f"step{step}/"):
                continue
            name = k.split("/", 1)[1]
            if name.endswith("num_batches_tracked"):
                assert int(sd[name]) == step == int(g[k])
                continue
            ref = g[k]
            scale = np.abs(ref).max()
            dev = np.abs(sd[name] - ref).max() / scale
            odev = np.abs(po[name] - ref).max() / scale
            tol = 5e-3 if step == 1 else max(2e-2, 2.0 * odev)
            if not dev <= tol:
                bad.append((name, float(dev), float(odev), tol))
        assert not bad, (step, bad)


def test_config2_batch256_reconstruction_only_properties_and_torch_cpu_port():
    """BASELINE configs[1] at its FULL size (B=256, encoder + decoder, MSE only; bench.py's `configs.c2`): the reference holds a
    golden for this mode at b=8 only (ae_adam5_recon_b8.npz), so at 256: (1) eval forward is per-image (one call == four B=64 calls,
    bitwise); (2) the gradient of alpha*MSE is linear in alpha; (3) two identical gradient steps are bitwise equal and the classifier
    receives exactly zero gradient; (4) loss, x_hat and every gradient against the torch-CPU port of the reference graph
    (oracle/ae_torch_cpu.py, fp32) at the same size -- one CPU step of 256 images is cheap enough."""
    import gpu_util as G
    from oracle import ae_torch_cpu as T
    x, y = gu.make_images(256, 4242)
    xd, yd = _cuda(x), _cuda(y)
    m = _model()
    eng = _engine(m, max_batch=256)
    m.eval()
    xh, _, z = eng.forward(xd, train=False, head=False, want=("x_hat", "z"))
    torch.cuda.synchronize()
    for k in range(0, 256, 64):
        xh_k, _, z_k = eng.forward(xd[k:k + 64].contiguous(), train=False, head=False, want=("x_hat", "z"))
        torch.cuda.synchronize()
        assert torch.equal(z_k, z[k:k + 64]) and torch.equal(xh_k, xh[k:k + 64]), k
    grads = {}
    for alpha in (1.0, 2.0, 1.0):
        m2 = _model()
        e2 = _engine(m2, max_batch=256)
        x_hat = torch.empty_like(xd)
        e2.grad_step(xd, yd, alpha, head=False, x_hat=x_hat)
        torch.cuda.synchronize()
        gnp = e2.grads.cpu().numpy().copy()
        if alpha in grads:
            assert np.array_equal(grads[alpha][0], gnp)                                  # (3)
        grads[alpha] = (gnp, float(e2.loss_last[1]), x_hat.cpu().numpy(), e2)
    g1, g2 = grads[1.0][0], grads[2.0][0]
    assert G.cosine(g2, 2.0 * g1) > 0.9995 and G.relmax(g2, 2.0 * g1) < 3e-2, (G.cosine(g2, 2.0 * g1), G.relmax(g2, 2.0 * g1))   # (2)
    e2 = grads[1.0][3]
    assert float(e2.grads[e2.poff[34]:e2.poff[38]].abs().max()) == 0.0                   # (3) head untouched
    # (4) the torch-CPU port (fp32) on the same batch
    pt = T.build(latent_dim=64, state=ae_state_np())
    xt = torch.from_numpy(x)
    out = T.forward(pt, xt, train=True, head=False)
    xh_ref = out[0] if isinstance(out, tuple) else out
    loss = torch.nn.functional.mse_loss(xh_ref, xt)
    loss.backward()
    assert abs(grads[1.0][1] - float(loss)) <= 2e-2 * float(loss), (grads[1.0][1], float(loss))
    d = np.abs(grads[1.0][2] - xh_ref.detach().numpy())
    assert d.max() <= 3e-2 and d.mean() <= 3e-3, (d.max(), d.mean())
    slot_of = {id(q): j for q, j in e2._slots}
    bad = []
    for name, prm in e2.root_ref().named_parameters():
        if name.startswith("classifier") or name in PRE_BN_BIAS:
            continue
        i = slot_of[id(prm)]
        got = g1[e2.poff[i]: e2.poff[i] + prm.numel()].reshape(tuple(prm.shape))
        ref = pt[name].grad.numpy()
        c = G.cosine(got, ref)
        nr = np.linalg.norm(got.ravel().astype(np.float64)) / max(np.linalg.norm(ref.ravel().astype(np.float64)), 1e-30)
        # BatchNorm affine parameters (sums of g and g*xhat over 256 x H x W bf16 values against an fp32 run) are the noisiest tensors:
        # measured worst case here enc.encoder.1.weight at cosine 0.967 / norm ratio 1.095; the 3x3 and FC weights sit at > 0.99 / 0.98-1.02
        lo_c, lo_n, hi_n = (0.95, 0.88, 1.12) if prm.ndim == 1 else (0.97, 0.93, 1.07)
        if not (c > lo_c and lo_n <= nr <= hi_n):
            bad.append((name, c, nr))
    assert not bad, bad


def test_full_size_batch512_joint_step_vs_torch_cpu_port():
    """BASELINE configs[2] -- the configuration the headline metric is quoted on (B=512, joint alpha*MSE + CE) -- against the torch-CPU
    port of the reference graph (oracle/ae_torch_cpu.py, fp32, pinned by the goldens) on the SAME batch: loss, mse, ce, x_hat, logits,
    z and every one of the 38 gradients (cosine + norm ratio per tensor).  test_full_size_batch512_properties covers the
    size-independent properties; this is the direct comparison VERDICT r3 asked for (one CPU step of 512 images is ~1 s)."""
    import gpu_util as G
    from oracle import ae_torch_cpu as T
    x, y = gu.make_images(512, 777)
    xd, yd = _cuda(x), _cuda(y)
    alpha = 35.0
    m = _model()
    eng = _engine(m, max_batch=512)
    x_hat = torch.empty_like(xd)
    eng.grad_step(xd, yd, alpha, x_hat=x_hat)
    torch.cuda.synchronize()
    g1 = eng.grads.cpu().numpy().copy()
    got_loss = [float(v) for v in eng.loss_last[:3]]
    pt = T.build(latent_dim=64, state=ae_state_np())
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    xh_ref, lg_ref, z_ref = T.forward(pt, xt, train=True, head=True)
    mse = torch.nn.functional.mse_loss(xh_ref, xt)
    ce = torch.nn.functional.cross_entropy(lg_ref, yt)
    loss = alpha * mse + ce
    loss.backward()
    assert abs(got_loss[0] - float(loss)) <= 2e-2 * float(loss), (got_loss, float(loss))
    assert abs(got_loss[1] - float(mse)) <= 2e-2 * float(mse) and abs(got_loss[2] - float(ce)) <= 2e-2 * float(ce), (got_loss, float(mse), float(ce))
    d = np.abs(x_hat.cpu().numpy() - xh_ref.detach().numpy())
    assert d.max() <= 3e-2 and d.mean() <= 3e-3, (d.max(), d.mean())
    slot_of = {id(q): j for q, j in eng._slots}
    bad = []
    for name, prm in eng.root_ref().named_parameters():
        if name in PRE_BN_BIAS:
            continue
        i = slot_of[id(prm)]
        got = g1[eng.poff[i]: eng.poff[i] + prm.numel()].reshape(tuple(prm.shape))
        ref = pt[name].grad.numpy()
        c = G.cosine(got, ref)
        nr = np.linalg.norm(got.ravel().astype(np.float64)) / max(np.linalg.norm(ref.ravel().astype(np.float64)), 1e-30)
        # same bounds as at B=256 (BatchNorm affine parameters are sums over B x H x W bf16 values against an fp32 run: the noisiest)
        lo_c, lo_n, hi_n = (0.95, 0.88, 1.12) if prm.ndim == 1 else (0.97, 0.93, 1.07)
        if not (c > lo_c and lo_n <= nr <= hi_n):
            bad.append((name, c, nr))
    assert not bad, bad


def test_config5_benchmarked_geometry_b128_properties():
    """bench.py times BASELINE configs[4]'s per-GPU shape at B=128 (256x256 inputs, 256-d latent); the oracle checks of that shape
    run at B=2 / 8 (a different igemm grid geometry: the small-tile rule of eae_conv_launch.hip depends on the batch).  At the
    benchmarked geometry: (1) eval forward per image (one B=128 call == two B=64 calls, bitwise); (2) two gradient steps from the
    same state are bitwise equal, bf16 and fp8; (3) the fp8 variant's gradients stay close to the bf16 ones (cosine, norm) and are
    not identical to them.  No reference vector exists for this shape (R.md:309): parity unpinned by the reference."""
    import eae_amd
    import gpu_util as G
    from eae_amd.engine import AEEngine
    g = torch.Generator(device="cuda"); g.manual_seed(99)
    x = torch.rand((128, 3, 256, 256), generator=g, device="cuda")
    y = torch.randint(0, 10, (128,), generator=g, device="cuda")

    def make(quant):
        torch.manual_seed(6)
        m = eae_amd.SupervisedAutoencoder(latent_dim=256, num_classes=10, image_size=256).cuda().train()
        return m, AEEngine(m, max_batch=128, quant=quant)

    m, eng = make("bf16")
    m.eval()
    xh, lg, z = eng.forward(x, labels=y, train=False, alpha=35.0)
    torch.cuda.synchronize()
    for k in (0, 64):
        xh_k, lg_k, z_k = eng.forward(x[k:k + 64].contiguous(), labels=y[k:k + 64].contiguous(), train=False, alpha=35.0)
        torch.cuda.synchronize()
        assert torch.equal(z_k, z[k:k + 64]) and torch.equal(lg_k, lg[k:k + 64]) and torch.equal(xh_k, xh[k:k + 64]), k
    del eng, m
    got = {}
    for quant in ("bf16", "fp8"):
        runs = []
        for _ in range(2):
            m, eng = make(quant)
            if quant == "fp8":
                eng.fp8_calibrate(x, y, 35.0)
            eng.grad_step(x, y, 35.0)
            torch.cuda.synchronize()
            assert eng.gate_timeouts() == 0
            runs.append((eng.grads.cpu().numpy().copy(), float(eng.loss_last[0])))
            del eng, m
            torch.cuda.empty_cache()
        assert np.array_equal(runs[0][0], runs[1][0]), quant                            # (2)
        assert np.isfinite(runs[0][1])
        got[quant] = runs[0]
    gb, gf = got["bf16"][0], got["fp8"][0]
    assert not np.array_equal(gb, gf)
    nr = np.linalg.norm(gf.astype(np.float64)) / np.linalg.norm(gb.astype(np.float64))
    assert G.cosine(gf, gb) > 0.95 and 0.88 <= nr <= 1.12, (G.cosine(gf, gb), nr)         # (3)
    assert abs(got["fp8"][1] - got["bf16"][1]) <= 3e-2 * abs(got["bf16"][1])


def test_training_curve_tracks_the_torch_cpu_port_over_120_steps():
    """Training DYNAMICS, not one step: 120 joint steps (4 batches of 64 learnable images cycled 30 times, alpha 35, lr 1e-3) on the
    engine and on the fp32 torch-CPU port of the reference graph from the same initial weights.  Per-step trajectories of a bf16 and an
    fp32 run diverge element-wise (chaos), the LOSS curves must not: the mean loss of every 20-step window within 4 % of the port's,
    both fall by more than a third, and the final validation loss (eval mode: running statistics) of the two models within 5 %."""
    from oracle import ae_torch_cpu as T
    rng = np.random.default_rng(2024)
    # learnable structure: class-dependent smooth patterns + noise (labels are predictable from the image)
    yy, xx = np.meshgrid(np.linspace(0, 1, 64, dtype=np.float32), np.linspace(0, 1, 64, dtype=np.float32), indexing="ij")
    def batch(n):
        y = rng.integers(0, 10, size=n)
        base = np.stack([np.stack([0.5 + 0.4 * np.sin(2 * np.pi * ((k % 5 + 1) * xx + (k // 5) * yy) + c) for c in range(3)]) for k in y])
        x = np.clip(base + 0.05 * rng.standard_normal(base.shape), 0, 1).astype(np.float32)
        return x, y.astype(np.int64)
    train = [batch(64) for _ in range(4)]
    xv, yv = batch(64)
    alpha, lr = 35.0, 1e-3
    m = _model()
    eng = _engine(m, max_batch=64)
    p = T.build(state=ae_state_np())
    opt = T.make_adam(p, lr)
    le, lp = [], []
    for step in range(120):
        x, y = train[step % 4]
        eng.train_step(_cuda(x), _cuda(y), alpha, lr)
        le.append(float(eng.loss_last[0]))
        lp.append(T.train_step(p, opt, torch.from_numpy(x), torch.from_numpy(y), alpha))
    le, lp = np.array(le), np.array(lp)
    assert np.isfinite(le).all() and eng.gate_timeouts() == 0
    for w in range(0, 120, 20):
        a, b = le[w:w + 20].mean(), lp[w:w + 20].mean()
        assert abs(a - b) <= 0.04 * b, (w, a, b)
    assert le[-20:].mean() < 0.66 * le[:4].mean() and lp[-20:].mean() < 0.66 * lp[:4].mean()
    # validation in eval mode
    m.eval()
    xh, lg, _ = eng.forward(_cuda(xv), train=False)
    ve = alpha * float(((xh - _cuda(xv)) ** 2).mean()) + float(torch.nn.functional.cross_entropy(lg, _cuda(yv)))
    with torch.no_grad():
        xr, lr_, _ = T.forward(p, torch.from_numpy(xv), train=False)
        vp = alpha * float(((xr - torch.from_numpy(xv)) ** 2).mean()) + float(torch.nn.functional.cross_entropy(lr_, torch.from_numpy(yv)))
    assert abs(ve - vp) <= 0.05 * vp, (ve, vp)


def test_dy_mode_stores_the_staged_gradient_and_gives_the_same_weight_gradients(monkeypatch):
    """EAE_DY_MASK (round 4, off by default): the backward-data kernels of the four inner layers store the BatchNorm-backward-applied
    gradient dy they stage, and the weight-gradient kernels read that one tensor (SRC_RAWG) behind them instead of transforming
    g and y beside them.  (1) every gradient equals the default mode's bit for bit (the same bf16 operands in the same order);
    (2) the stored dy equals A*g + (B*y + C) recomputed from the stored g, y and the layer's backward coefficients to one bf16 ulp
    at rounding ties; (3) repeated steps are bitwise equal (a store with an SGPR soffset in front of a VALU write of its data
    registers shipped overwritten dwords now and then: tests/test_isa_guard.py)."""
    import ctypes as C
    x, y = gu.make_images(48, 321)
    xd, yd = _cuda(x), _cuda(y)
    grads = {}
    for mask in ("0", "0x3c", "0x3c"):
        monkeypatch.setenv("EAE_DY_MASK", mask)
        m = _model()
        eng = _engine(m, max_batch=48)
        eng.grad_step(xd, yd, 35.0)
        torch.cuda.synchronize()
        g = eng.grads.cpu().numpy().copy()
        if mask in grads:
            assert np.array_equal(grads[mask], g)                      # (3)
        grads[mask] = g
        if mask != "0":
            # (2) deconv2's output map u[1] (idx 1, 16 x 16 x 64) and conv3's output map y[2] (idx 2, 8 x 8 x 128)
            for (kdy, kg, ky, idx, per) in ((5, 3, 2, 1, 16 * 16 * 64), (4, 1, 0, 2, 8 * 8 * 128)):
                bufs = []
                for kind in (kdy, kg, ky):
                    b = np.empty(48 * per, np.uint16)
                    assert eng.lib.eae_debug_read(eng.ctx, kind, idx, b.ctypes.data_as(C.c_void_p), b.nbytes) == b.nbytes
                    bufs.append((b.astype(np.uint32) << 16).view(np.float32))
                dy, gg, yy = bufs
                assert np.isfinite(dy).all() and np.abs(dy).max() > 0
                # the coefficients are not exported: fit dy = A*g + B*y + C per channel by least squares and require a bf16-exact fit
                ch = 64 if idx == 1 else 128
                dy2, g2, y2 = dy.reshape(-1, ch), gg.reshape(-1, ch), yy.reshape(-1, ch)
                for c_ in (0, ch // 2, ch - 1):
                    A = np.stack([g2[:, c_], y2[:, c_], np.ones(len(g2))], 1).astype(np.float64)
                    coef, *_ = np.linalg.lstsq(A, dy2[:, c_].astype(np.float64), rcond=None)
                    fit = A @ coef
                    assert np.abs(fit - dy2[:, c_]).max() <= 2.0 ** -7 * max(1e-30, np.abs(dy2[:, c_]).max()), (idx, c_)
    assert np.array_equal(grads["0"], grads["0x3c"])                   # (1)
