"""Class-weighted cross-entropy with ignored labels in the fused steps (include/eae.h: eae_set_class_weights,
eae_mlp_set_class_weights, eae_op_head_ce_w) against the float64 references of tests/weighted_ce_ref.py, which
tests/test_weighted_ce_reference.py pins to torch.nn.functional.cross_entropy(weight=, ignore_index=).

The head cases use the harness and the tolerances of tests/test_gpu_head_shapes.py (NaN-filled outputs with guard rows; logits
1e-4, loss 1e-4, gradients rtol 1e-3 / atol 1e-6), the MLP cases `_compare_step` and the yardstick-derived bounds of
tests/test_gpu_mlp_shapes.py (yardstick = an fp32 run of the same reference).  Every head case also prints how far an fp32 NumPy
restatement of the formula lies from the float64 one, next to the kernel's own excess over the tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_util as gu
import mlp_ref as M
import weighted_ce_ref as W

pytestmark = pytest.mark.gpu

IGN = -7          # an ignore_index that is neither -1 nor a class: rows with -1, C and 255 are ignored for being out of range


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _no_ignore():
    from eae_amd import _lib
    return _lib.NO_IGNORE


# ---------------------------------------------------------------------------------------------------- 1. eae_op_head_ce_w by shape
def _run_w(lib, z, w1, b1, w2, b2, labels, class_w, ignore_index, plain=False):
    """One eae_op_head_ce_w call (plain: eae_op_head_ce) on NaN-filled outputs with guard rows, as test_gpu_head_shapes._run."""
    import gpu_util as G
    import test_gpu_head_shapes as H
    B, L = z.shape
    Cn = w2.shape[0]
    d = [G.f32(a) for a in (z, w1, b1, w2, b2)]
    lab = torch.from_numpy(np.asarray(labels, np.int64)).to(G.dev())
    cw = None if class_w is None else G.f32(class_w)
    nsc = int(lib.eae_op_head_scratch_floats(B, L, Cn))
    nan = float("nan")
    scratch = torch.full((nsc,), nan, dtype=torch.float32, device=G.dev())
    logits = torch.full((B + H.GUARD, Cn), nan, dtype=torch.float32, device=G.dev())
    dz = torch.full((B + H.GUARD, L), nan, dtype=torch.float32, device=G.dev())
    ng = H._r4(128 * L) + 128 + H._r4(128 * Cn) + H._r4(Cn)
    grads = torch.full((ng + 4 * H.GUARD,), nan, dtype=torch.float32, device=G.dev())
    loss2 = torch.full((2 + H.GUARD,), nan, dtype=torch.float32, device=G.dev())
    args = [G.stream(), *[G.ptr(t) for t in d], G.ptr(lab), B, L, Cn, G.ptr(logits), G.ptr(dz), G.ptr(grads), G.ptr(loss2), G.ptr(scratch), nsc]
    if plain:
        rc = lib.eae_op_head_ce(*args)
    else:
        rc = lib.eae_op_head_ce_w(*args, G.ptr(cw), C.c_longlong(_no_ignore() if ignore_index is None else ignore_index))
    torch.cuda.synchronize()
    return rc, {"logits": logits.cpu().numpy(), "dz": dz.cpu().numpy(), "grads": grads.cpu().numpy(), "loss2": loss2.cpu().numpy(), "ng": ng}


def _head_inputs(B, L, Cn, seed):
    import test_gpu_head_shapes as H
    z, w1, b1, w2, b2, labels = H._case(B, L, Cn, seed=seed)
    rng = np.random.default_rng(seed + 1)
    cw = W.make_weights(rng, Cn)
    labels = W.ignore_some(rng, labels, Cn, IGN)
    if B == 100:                    # one whole block of rows ignored (rows hr .. 2 hr - 1), and the last row
        hr = 16 if L <= 128 else 8
        labels[hr:2 * hr] = np.resize(np.array([IGN, -1, Cn, 255], np.int64), hr)
        labels[-1] = IGN
    return z, w1, b1, w2, b2, labels, cw


def _report_excess(o, ref, ref32, B):
    """Largest excess over rtol 1e-3 / atol 1e-6 of the kernel and of the fp32 NumPy restatement, both against float64 (<= 0: inside)."""
    def exc(a, r):
        return float((np.abs(a - r) - (1e-6 + 1e-3 * np.abs(r))).max())
    print(f"excess over tolerance: dz kernel {exc(o['dz'][:B], ref['dz']):.3e} fp32-numpy {exc(ref32['dz'], ref['dz']):.3e}; "
          f"loss kernel {abs(o['loss2'][0] - ref['loss']):.3e} fp32-numpy {abs(ref32['loss'] - ref['loss']):.3e}")


HEAD_CASES = [(15, 64, 10), (17, 64, 10), (100, 64, 10), (7, 132, 3), (9, 192, 10), (17, 256, 63), (9, 256, 64), (100, 256, 64), (1, 4, 1)]


@pytest.mark.parametrize("B,L,Cn", HEAD_CASES)
def test_head_ce_w_by_shape(lib, B, L, Cn):
    import test_gpu_head_shapes as H
    from eae_amd._lib import check
    z, w1, b1, w2, b2, labels, cw = _head_inputs(B, L, Cn, seed=B * 100003 + L * 101 + Cn)
    if B == 1:
        labels[:] = 0               # the one row counts
    ref = W.head_ref_w(z, w1, b1, w2, b2, labels, cw, IGN)
    ref32 = W.head_ref_w(z, w1, b1, w2, b2, labels, cw, IGN, dtype=np.float32)
    ok = W.counted_rows(labels, Cn, IGN)
    if B > 1:
        assert 0 < ok.sum() < B and ref["W"] > 0
    rc, o = _run_w(lib, z, w1, b1, w2, b2, labels, cw, IGN)
    check(rc)
    _report_excess(o, ref, ref32, B)
    H._check_logits(o, ref, B)
    H._check_loss(o, ref, labels)
    H._check_grads(o, ref, B, L, Cn)
    assert not o["dz"][:B][~ok].any()                     # ignored rows: exact zeros


# ---------------------------------------------------------------------------------------------------- 2. individual modes
@pytest.mark.parametrize("B,L,Cn", [(17, 64, 10), (9, 256, 64)])
def test_head_modes(lib, B, L, Cn):
    import test_gpu_head_shapes as H
    from eae_amd._lib import check
    z, w1, b1, w2, b2, labels, cw = _head_inputs(B, L, Cn, seed=7 + L)
    inr = np.where(W.counted_rows(labels, Cn, None), labels, 1)
    # weights only, every label in range
    ref = W.head_ref_w(z, w1, b1, w2, b2, inr, cw, None)
    rc, o = _run_w(lib, z, w1, b1, w2, b2, inr, cw, None)
    check(rc)
    H._check_logits(o, ref, B); H._check_loss(o, ref, inr); H._check_grads(o, ref, B, L, Cn)
    # ignore only, NULL weights (ignore_index is a class here: its rows do not count either)
    ref = W.head_ref_w(z, w1, b1, w2, b2, labels, None, 2)
    rc, o = _run_w(lib, z, w1, b1, w2, b2, labels, None, 2)
    check(rc)
    H._check_logits(o, ref, B); H._check_loss(o, ref, labels); H._check_grads(o, ref, B, L, Cn)
    assert o["loss2"][1] == ref["correct"] <= W.counted_rows(labels, Cn, 2).sum()
    # all rows ignored: loss 0, every gradient and dz exactly 0, everything finite
    none = np.resize(np.array([IGN, -1, Cn, 255], np.int64), B)
    rc, o = _run_w(lib, z, w1, b1, w2, b2, none, cw, IGN)
    check(rc)
    H._check_logits(o, W.head_ref_w(z, w1, b1, w2, b2, none, cw, IGN), B)
    assert o["loss2"][0] == 0.0 and o["loss2"][1] == 0.0
    assert not o["dz"][:B].any() and not o["grads"][:o["ng"]].any()
    assert np.isnan(o["dz"][B:]).all() and np.isnan(o["grads"][o["ng"]:]).all()
    # NULL weights with EAE_NO_IGNORE: bitwise eae_op_head_ce
    rc, a = _run_w(lib, z, w1, b1, w2, b2, inr, None, None)
    check(rc)
    rc, b = _run_w(lib, z, w1, b1, w2, b2, inr, None, None, plain=True)
    check(rc)
    for k in ("logits", "dz", "grads", "loss2"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    # two calls on the same inputs: bitwise equal
    rc, a = _run_w(lib, z, w1, b1, w2, b2, labels, cw, IGN)
    rc2, b = _run_w(lib, z, w1, b1, w2, b2, labels, cw, IGN)
    check(rc); check(rc2)
    for k in ("logits", "dz", "grads", "loss2"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k


# ---------------------------------------------------------------------------------------------------- 3. fused step vs autograd
CW10 = np.array([0.5, 2.0, 1.0, 3.5, 0.0, 0.25, 4.0, 1.5, 0.75, 2.5], np.float32)


def _ae():
    import test_gpu_ae as A
    return A


def test_fused_step_matches_autograd_with_weighted_criterion(golden):
    """test_gpu_ae.py::test_autograd_drop_in_loop_matches_fused_step with nn.CrossEntropyLoss(weight=w, ignore_index=-1)."""
    import torch.nn as nn
    A = _ae()
    g = golden("ae_fwd_bwd_b8.npz")
    labels = np.array(g["labels"], np.int64)
    labels[[2, 5]] = -1
    x, y = A._cuda(g["x"]), A._cuda(labels)
    alpha = float(g["alpha"])
    w = torch.from_numpy(CW10).cuda()
    m1, m2 = A._model(), A._model()
    e1 = A._engine(m1)
    e1.set_class_weights(CW10, -1)
    e1.reset_loss()
    e1.grad_step(x, y, alpha)
    e1.expose_grads()
    m2.train()
    x_hat, logits, _ = m2(x)
    loss = alpha * nn.MSELoss()(x_hat, x) + nn.CrossEntropyLoss(weight=w, ignore_index=-1)(logits, y)
    loss.backward()
    for (n1, p1), (n2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        a, b = p1.grad.cpu().numpy(), p2.grad.cpu().numpy()
        scale = max(1e-12, np.abs(a).max())
        assert np.abs(a - b).max() <= 2e-2 * scale, (n1, np.abs(a - b).max() / scale)
    assert e1.read_valid() == 6
    # loss_last[2] against torch's CE on the engine's own logits, float64; the correct count over the counted rows
    e1.reset_loss()
    _, lg, _ = e1.forward(x, labels=y, train=True, alpha=alpha, accum=True)
    torch.cuda.synchronize()
    lg64 = lg.double().cpu()
    ce = float(nn.functional.cross_entropy(lg64, torch.from_numpy(labels), weight=torch.from_numpy(CW10).double(), ignore_index=-1))
    assert abs(float(e1.loss_last[2]) - ce) < 1e-4, (float(e1.loss_last[2]), ce)
    acc = e1.loss_accum.tolist()
    assert acc[3] == 8.0 and acc[4] == float(((lg64.argmax(1).numpy() == labels) & (labels >= 0)).sum())
    assert abs(acc[2] - ce * 8) < 8e-4 and e1.read_valid() == 6
    # a forward that does not accumulate its loss does not count either; weights alone (no ignore_index) still ignore, and count, by range
    e1.forward(x, labels=y, train=False, alpha=alpha, accum=False)
    assert e1.read_valid() == 6
    e1.set_class_weights(CW10, None)
    e1.reset_loss()
    e1.forward(x, labels=y, train=False, alpha=alpha, accum=True)
    assert e1.read_valid() == 6 and e1.read_loss()[3] == 8
    e1.set_class_weights(None, None)
    labels[labels < 0] = 0
    e1.reset_loss()
    e1.forward(x, labels=A._cuda(labels), train=False, alpha=alpha, accum=True)
    assert e1.read_valid() == 8 and int(e1.valid.item()) == 0             # feature off: every sample; the device word is not written
    # on, count, off, reset, on again: the count starts with the setting, nothing stale is added
    e1.set_class_weights(CW10, -1)
    e1.forward(x, labels=y, train=False, alpha=alpha, accum=True)
    e1.set_class_weights(None, None)
    e1.reset_loss()
    e1.set_class_weights(CW10, -1)
    e1.forward(x, labels=y, train=False, alpha=alpha, accum=True)
    assert e1.read_valid() == 6


# ---------------------------------------------------------------------------------------------------- 4. grouped step
def test_grouped_members_are_bitwise_what_they_are_alone_and_a_mixed_group_is_rejected(lib):
    from eae_amd import _lib
    from eae_amd.engine import AEEngine
    A = _ae()
    x, y = gu.make_images(8, 100)
    y = np.array(y, np.int64); y[[1, 6]] = -1
    xd, yd = A._cuda(x), A._cuda(y)
    ws = [CW10, CW10[::-1].copy()]
    alphas, lrs = [35.0, 20.0], [5e-3, 1e-3]

    def engines():
        ms = [A._model(), A._model()]
        es = [A._engine(m) for m in ms]
        for e, w in zip(es, ws):
            e.set_class_weights(w, -1)
        return ms, es

    ms, es = engines()
    for _ in range(2):
        AEEngine.group_train_step(es, [xd, xd], [yd, yd], alphas, lrs)
    torch.cuda.synchronize()
    grouped = [(e.params.cpu().numpy().copy(), e.loss_accum.cpu().numpy().copy(), e.read_valid()) for e in es]
    ms2, es2 = engines()
    _lib.check(lib.eae_set_geometry_mult(2))
    try:
        for k, e in enumerate(es2):
            for _ in range(2):
                e.train_step(xd, yd, alphas[k], lrs[k])
    finally:
        _lib.check(lib.eae_set_geometry_mult(1))
    torch.cuda.synchronize()
    for k, e in enumerate(es2):
        assert np.array_equal(grouped[k][0], e.params.cpu().numpy()), k
        assert np.array_equal(grouped[k][1], e.loss_accum.cpu().numpy()), k
        assert grouped[k][2] == e.read_valid() == 12
    assert not np.array_equal(grouped[0][0], grouped[1][0]) and np.isfinite(grouped[0][0]).all()
    # a group mixing on and off is rejected before anything is recorded or launched
    es[1].set_class_weights(None, None)
    before = [e.params.clone() for e in es]
    steps = [int(lib.eae_get_adam_step(e.ctx)) for e in es]
    with pytest.raises(_lib.EaeError, match="-2.*every member or on none"):
        AEEngine.group_train_step(es, [xd, xd], [yd, yd], alphas, lrs)
    torch.cuda.synchronize()
    assert all(torch.equal(b, e.params) for b, e in zip(before, es))
    assert steps == [int(lib.eae_get_adam_step(e.ctx)) for e in es]


# ---------------------------------------------------------------------------------------------------- 5. graph replay
def test_graph_replay_equals_eager_across_a_change_of_the_setting():
    """The pattern of test_gpu_ae.py::test_graph_replay_equals_eager: eae_set_class_weights between steps drops the captured graph, the
    next steps capture again with the new vector."""
    A = _ae()
    x, y = gu.make_images(8, 100)
    y = np.array(y, np.int64); y[[0, 3]] = -1
    xd, yd = A._cuda(x), A._cuda(y)
    res = []
    for no_graph in (False, True):
        if no_graph:
            os.environ.pop("EAE_GRAPH", None)
        else:
            os.environ["EAE_GRAPH"] = "1"
        try:
            m = A._model()
            eng = A._engine(m)
            eng.set_class_weights(CW10, -1)
            for s in range(5):
                eng.train_step(xd, yd, 35.0, 5e-3)
            eng.set_class_weights(CW10[::-1].copy(), -1)
            for s in range(5):
                eng.train_step(xd, yd, 35.0, 5e-3)
            torch.cuda.synchronize()
            res.append((eng.params.cpu().numpy().copy(), eng.bn_running.cpu().numpy().copy(), eng.loss_accum.cpu().numpy().copy()))
        finally:
            os.environ.pop("EAE_GRAPH", None)
    for k in range(3):
        assert np.array_equal(res[0][k], res[1][k]), (k, np.abs(res[0][k] - res[1][k]).max())
    assert np.isfinite(res[0][0]).all()


# ---------------------------------------------------------------------------------------------------- 6. MLP
# (input_dim, classes, batch, data seed): the seeds leave no ReLU tie (asserted on the reference before the launch)
MLP_CASES = [(64, 10, 7, 1), (64, 10, 65, 0), (128, 16, 130, 0)]


def _mlp_case(IN, Cn, B, seed):
    import test_gpu_mlp_shapes as S
    p0, batches = S.case_inputs(IN, Cn, B, 1, seed)
    rng = np.random.default_rng(1000 + 7 * B + seed)
    cw = W.make_weights(rng, Cn)
    x, y, mask = batches[0]
    y = W.ignore_some(rng, y, Cn, IGN)
    return p0, [(x, y, mask)], cw


@pytest.mark.parametrize("IN,Cn,B,seed", MLP_CASES, ids=[f"in{c[0]}-c{c[1]}-b{c[2]}" for c in MLP_CASES])
def test_mlp_train_step_weighted(IN, Cn, B, seed):
    import test_gpu_mlp_shapes as S
    p0, batches, cw = _mlp_case(IN, Cn, B, seed)
    ref = W.mlp_run_w(p0, batches, S.LR, S.WD, cw, IGN)
    yard = W.mlp_run_w(p0, batches, S.LR, S.WD, cw, IGN, dtype=np.float32)
    x, y, mask = batches[0]
    t1, t2 = M.relu_ties(ref[0], yard[0], mask)
    assert int(t1.sum()) + int(t2.sum()) == 0, "ReLU ties: search another data seed"
    ok = W.counted_rows(y, Cn, IGN)
    assert 0 < ok.sum() < B
    top = np.sort(ref[0]["logits"], axis=1)
    assert (top[:, -1] - top[:, -2]).min() > M.TIE_FACTOR * M.deviation(yard[0]["logits"], ref[0]["logits"])
    clf, eng = S._clf(IN, Cn, p0, B)
    eng.set_class_weights(cw, IGN)
    rep = S.Report(f"wce-train-in{IN}-c{Cn}-b{B}")
    before = np.array(eng.stats.tolist()[:3])
    logits = eng.train_step(S._cuda(x), S._cuda(y), lr=S.LR, weight_decay=S.WD, drop_mask=S._cuda(mask), want_logits=True)
    S._compare_step(rep, clf, eng, logits, before, ref[0], yard[0], B, prev=S.start_of(p0), t=1)
    rep.done()
    assert eng.read_valid() == int(ok.sum())


def test_mlp_eval_step_weighted_three_blocks():
    """B = 130: three 64-row blocks with ignored rows in each; every block needs the batch-wide W."""
    import test_gpu_mlp_shapes as S
    IN, Cn, B = 128, 16, 130
    p0 = M.make_state(IN, Cn, 31 + IN + Cn)
    x, y = M.make_batch(B, IN, Cn, 17 + B)
    rng = np.random.default_rng(5)
    cw = W.make_weights(rng, Cn)
    y = W.ignore_some(rng, y, Cn, IGN)
    y[[3, 70, 129]] = [IGN, -1, 255]
    ok = W.counted_rows(y, Cn, IGN)
    assert all(0 < ok[a:b].sum() < b - a for a, b in ((0, 64), (64, 128), (128, 130)))
    c = M.forward(p0, x, False)
    c32 = M.forward(p0, x, False, dtype=np.float32)
    loss, _, correct = W.mlp_dlogits_w(c["logits"], y, cw, IGN)
    loss32, _, _ = W.mlp_dlogits_w(c32["logits"], y, cw, IGN)
    top = np.sort(c["logits"], axis=1)
    assert (top[:, -1] - top[:, -2]).min() > M.TIE_FACTOR * M.deviation(c32["logits"], c["logits"])
    clf, eng = S._clf(IN, Cn, p0, B, train=False)
    eng.set_class_weights(cw, IGN)
    eng.reset_stats()
    rep = S.Report("wce-eval-b130")
    lg = eng.eval_step(S._cuda(x), S._cuda(y), want_logits=True)
    torch.cuda.synchronize()
    rep.check("logits", lg.cpu().numpy(), c["logits"], c32["logits"])
    st = eng.stats.tolist()[:3]
    rep.check("loss sum", st[0], float(loss) * B, float(np.float32(loss32) * np.float32(B)))
    assert st[1] == B and st[2] == correct, (st, correct)
    rep.done()
    assert eng.read_valid() == int(ok.sum())
    a = eng.stats.clone()
    eng.reset_stats()
    eng.eval_step(S._cuda(x), S._cuda(y))
    torch.cuda.synchronize()
    assert a[1] == eng.stats[1] and a[2] == eng.stats[2] and abs(float(a[0] - eng.stats[0])) <= 4 * np.finfo(np.float32).eps * abs(float(a[0]))


# ---------------------------------------------------------------------------------------------------- 7. scene
def _scene_and_raster(seed):
    rng = np.random.default_rng(seed)
    scene = torch.from_numpy(rng.integers(0, 256, (2, 160, 160)).astype(np.uint8)).cuda()
    raster = rng.integers(0, 4, (160, 160)).astype(np.uint8)
    raster[:, 80:] = 255                                   # half the raster is unlabelled
    raster[:80, :80] = np.where(rng.random((80, 80)) < 0.8, 0, raster[:80, :80])      # an imbalanced labelled half
    return scene, torch.from_numpy(raster).cuda()


def test_scene_loader_unlabelled_yields_the_unlabelled_windows():
    import eae_amd
    scene, raster = _scene_and_raster(60)
    label, purity, _ = eae_amd.window_labels(raster, 16, 16, 4)
    assert label.shape == (10, 10) and int((label < 0).sum()) == 50
    loader = eae_amd.SceneLoader(scene, label, divisor=255.0, patch=16, stride=16, batch_size=32, train=False, unlabelled=True)
    assert loader.windows.tolist() == list(range(100)) and torch.equal(loader.labels, label.reshape(-1))
    ys = torch.cat([y for _, y in loader])
    xs = [x for x, _ in loader]
    assert torch.equal(ys, label.reshape(-1)) and int((ys == -1).sum()) == 50
    assert xs[0].shape == (32, 2, 16, 16) and all(torch.isfinite(x).all() for x in xs)
    plain = eae_amd.SceneLoader(scene, label, divisor=255.0, patch=16, stride=16, batch_size=32, train=False)
    assert plain.windows.numel() == 50 and int((plain.labels < 0).sum()) == 0
    w = eae_amd.class_weights(loader.labels, 4)
    assert w.device == label.device and torch.equal(w, eae_amd.class_weights(plain.labels, 4))


def test_fit_autoencoder_on_a_partly_labelled_scene():
    import eae_amd
    scene, raster = _scene_and_raster(61)
    label, _, _ = eae_amd.window_labels(raster, 64, 32, 4)
    assert label.shape == (4, 4) and 0 < int((label < 0).sum()) < 16
    kw = dict(divisor=255.0, patch=64, stride=32, batch_size=8, seed=2, unlabelled=True)
    train, val = eae_amd.SceneLoader(scene, label, train=True, **kw), eae_amd.SceneLoader(scene, label, train=False, **kw)
    torch.manual_seed(0)
    model = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=4, in_channels=2).cuda()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    r = eae_amd.fit_autoencoder(train, val, alpha=30, lr=1e-3, num_classes=4, num_epochs=1, verbose=False, model=model, in_channels=2,
                                ignore_index=-1, class_weight="balanced")
    assert r["epochs"] == 1 and np.isfinite(r["train_curve"]).all() and np.isfinite(r["val_curve"]).all()
    after = model.state_dict()
    for k in ("enc.encoder.0.weight", "dec.decoder.10.weight", "classifier.2.weight"):
        assert torch.isfinite(after[k]).all() and not torch.equal(after[k], before[k]), k
    from eae_amd.engine import engine_for
    eng = engine_for(model)
    assert eng.ignore_index == -1 and torch.equal(eng.class_weights, eae_amd.class_weights(train.labels, 4))
    assert eng.read_valid() == int((label >= 0).sum()) and eng.read_loss()[3] == 16          # the validation pass: every window once


# ---------------------------------------------------------------------------------------------------- 8. rejections touch nothing
def test_rejected_settings_touch_nothing():
    A = _ae()
    x, y = gu.make_images(8, 100)
    xd, yd = A._cuda(x), A._cuda(y)
    m, m0 = A._model(), A._model()
    eng, eng0 = A._engine(m), A._engine(m0)
    for bad in (CW10[:9], np.ones(11, np.float32), -CW10, np.where(CW10 == 0, np.nan, CW10), np.zeros(10, np.float32)):
        with pytest.raises(RuntimeError):
            eng.set_class_weights(bad, -1)
        assert eng.class_weights is None and eng.ignore_index is None
    with pytest.raises(RuntimeError):
        eng.set_class_weights(None, 0.5)
    eng.train_step(xd, yd, 35.0, 5e-3)
    eng0.train_step(xd, yd, 35.0, 5e-3)
    torch.cuda.synchronize()
    assert torch.equal(eng.params, eng0.params) and torch.equal(eng.loss_accum, eng0.loss_accum)      # still the plain criterion
    # the MLP engine: same checks, same state
    import eae_amd
    from eae_amd.mlp_engine import mlp_engine_for
    clf = eae_amd.MLP(input_dim=64, num_classes=10).cuda()
    me = mlp_engine_for(clf)
    for bad in (CW10[:9], -CW10, np.zeros(10, np.float32)):
        with pytest.raises(RuntimeError):
            me.set_class_weights(bad, None)
        assert me.class_weights is None and me.ignore_index is None
