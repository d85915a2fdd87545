"""The references of the class-weighted cross-entropy with ignored labels (tests/weighted_ce_ref.py) pinned to torch on the CPU in
float64 -- value, and gradients by autograd -- and the host-side pieces of the feature that need no GPU: `scene.class_weights`,
`drawable_windows(unlabelled=True)`, the argument checks of `SceneLoader(unlabelled=)` and of `set_class_weights`, and the
`class_weight=` resolution of the fit functions."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mlp_ref as M
import weighted_ce_ref as W

import eae_amd
from eae_amd import scene as S


def _torch_labels(labels, C, ignore_index):
    """torch wants every target in range or equal to ignore_index: rows that do not count get torch's ignore value."""
    ign = -100 if ignore_index is None else ignore_index
    ok = W.counted_rows(labels, C, ignore_index)
    return torch.from_numpy(np.where(ok, labels, ign)), ign


def _head_case(B, L, C, seed, ignore_index):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((B, L)); w1 = rng.standard_normal((128, L)) * 0.2; b1 = rng.standard_normal(128) * 0.1
    w2 = rng.standard_normal((C, 128)) * 0.2; b2 = rng.standard_normal(C) * 0.1
    labels = W.ignore_some(rng, rng.integers(0, C, B), C, ignore_index)
    return z, w1, b1, w2, b2, labels, W.make_weights(rng, C).astype(np.float64)


@pytest.mark.parametrize("B,L,C,ignore_index,weighted", [(17, 64, 10, -1, True), (9, 132, 3, 1, True), (33, 8, 64, 255, True),
                                                          (12, 16, 10, -1, False), (12, 16, 10, None, True), (5, 4, 1, -1, True)])
def test_head_ref_w_is_torch_cross_entropy(B, L, C, ignore_index, weighted):
    z, w1, b1, w2, b2, labels, cw = _head_case(B, L, C, 11 * B + C, -1 if ignore_index is None else ignore_index)
    if ignore_index is None:
        labels = np.where((labels >= 0) & (labels < C), labels, 0)          # weights only: every label in range
    cw = cw if weighted else None
    ref = W.head_ref_w(z, w1, b1, w2, b2, labels, cw, ignore_index)
    t = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (z, w1, b1, w2, b2)]
    lg = torch.relu(t[0] @ t[1].T + t[2]) @ t[3].T + t[4]
    lg.retain_grad()
    tl, ign = _torch_labels(labels, C, ignore_index)
    loss = F.cross_entropy(lg, tl, weight=None if cw is None else torch.tensor(cw), ignore_index=ign, reduction="mean")
    assert ref["W"] > 0 and torch.isfinite(loss)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) < 1e-12
    for name, g in (("dlogits", lg.grad), ("dz", t[0].grad), ("dw1", t[1].grad), ("db1", t[2].grad), ("dw2", t[3].grad), ("db2", t[4].grad)):
        np.testing.assert_allclose(ref[name], g.numpy(), rtol=1e-10, atol=1e-14, err_msg=name)
    ok = W.counted_rows(labels, C, ignore_index)
    assert not ref["dlogits"][~ok].any()                                  # exact zero rows
    assert ref["correct"] == int((lg.detach().numpy().argmax(1) == labels)[ok].sum())


def test_mlp_dlogits_w_is_torch_cross_entropy_and_drives_the_backward():
    rng = np.random.default_rng(3)
    IN, C, B = 16, 10, 21
    p0 = M.make_state(IN, C, 5)
    x, y = M.make_batch(B, IN, C, 9)
    y = W.ignore_some(rng, y, C, -1)
    cw = W.make_weights(rng, C)
    mask = (rng.random((B, M.H1)) >= 0.3).astype(np.float32)
    c = M.forward(p0, x, True, drop_mask=mask)
    loss, dlog, correct = W.mlp_dlogits_w(c["logits"], y, cw, -1)
    lg = torch.tensor(c["logits"], requires_grad=True)
    tl, ign = _torch_labels(y, C, -1)
    tloss = F.cross_entropy(lg, tl, weight=torch.tensor(cw, dtype=torch.float64), ignore_index=ign)
    tloss.backward()
    assert abs(float(loss) - float(tloss.detach())) < 1e-12
    np.testing.assert_allclose(dlog, lg.grad.numpy(), rtol=1e-10, atol=1e-15)
    q = W.mlp_run_w(p0, [(x, y, mask)], 1e-5, 1e-4, cw, -1)[0]
    g = M.backward(p0, c, dlog)
    for k in M.PARAMS:
        assert np.array_equal(q["grad/" + k], g[k]), k
    assert q["correct"] == correct and float(q["loss"]) == float(loss)
    # with every row counted and no weights the weighted criterion is the plain one
    y0 = np.where(W.counted_rows(y, C, -1), y, 0)
    l0, d0, c0 = M.cross_entropy(c["logits"], y0)
    l1, d1, c1 = W.mlp_dlogits_w(c["logits"], y0, None, None)
    assert abs(l0 - l1) < 1e-14 and np.abs(d0 - d1).max() < 1e-16 and c0 == c1


@pytest.mark.parametrize("how", ["all ignored", "only zero-weight classes"])
def test_nothing_counted_is_zero_not_nan(how):
    """The stated deviation from torch (NaN): W = 0 gives loss 0 and zero gradients, all finite."""
    z, w1, b1, w2, b2, labels, cw = _head_case(9, 16, 5, 2, -1)
    if how == "all ignored":
        labels = np.array([-1, 5, 255, -1, -7, 5, 255, -1, -1], np.int64)
    else:
        cw = np.array([0.0, 2.0, 0.0, 1.0, 3.0]); labels = np.array([0, 2, 0, 2, -1, 0, 2, 2, 0], np.int64)
    ref = W.head_ref_w(z, w1, b1, w2, b2, labels, cw, -1)
    assert ref["loss"] == 0.0 and ref["W"] == 0.0
    for k in ("dlogits", "dz", "dw1", "db1", "dw2", "db2"):
        assert not ref[k].any() and np.isfinite(ref[k]).all(), k
    tl, ign = _torch_labels(labels, 5, -1)
    assert torch.isnan(F.cross_entropy(torch.tensor(ref["logits"]), tl, weight=torch.tensor(cw), ignore_index=ign))


# ---------------------------------------------------------------------------------------------------- scene.class_weights
def test_class_weights_formulas_on_hand_made_counts():
    # counts: class 0 x6, class 1 x3, class 2 absent, class 3 x1; -1, 4, 255 do not count
    lab = torch.tensor([[0, 0, 0, 1, -1], [0, 0, 0, 1, 255], [1, 3, 4, -1, -1]], dtype=torch.int64)
    w = S.class_weights(lab, 4)
    assert w.dtype == torch.float32 and w.device == lab.device and w.shape == (4,)
    n, kp = 10.0, 3.0
    np.testing.assert_allclose(w.numpy(), [n / (kp * 6), n / (kp * 3), 0.0, n / (kp * 1)], rtol=1e-6)
    w2 = S.class_weights(lab, 4, scheme="inverse_sqrt")
    raw = np.array([6 ** -0.5, 3 ** -0.5, 0.0, 1.0])
    np.testing.assert_allclose(w2.numpy(), raw * n / (6 ** 0.5 + 3 ** 0.5 + 1.0), rtol=1e-6)
    for ww in (w, w2):                                             # a sample's mean weight is 1 under both schemes
        assert abs(float((ww.double() * torch.tensor([6.0, 3.0, 0.0, 1.0])).sum()) - n) < 1e-5
    # any integer dtype and shape; sklearn's formula on a flat uint8 raster with a 255 nodata value
    r = torch.tensor([1, 1, 2, 255, 255, 2, 2, 2], dtype=torch.uint8)
    np.testing.assert_allclose(S.class_weights(r, 3).numpy(), [0.0, 6 / (2 * 2), 6 / (2 * 4)], rtol=1e-6)
    assert eae_amd.class_weights is S.class_weights and "class_weights" in eae_amd.__all__
    with pytest.raises(RuntimeError, match="nothing to weight"):
        S.class_weights(torch.tensor([-1, 7]), 4)
    with pytest.raises(RuntimeError, match="scheme must be"):
        S.class_weights(lab, 4, scheme="effective")
    with pytest.raises(RuntimeError, match="integer tensor"):
        S.class_weights(lab.float(), 4)


# ---------------------------------------------------------------------------------------------------- unlabelled windows
def test_drawable_windows_unlabelled():
    label = torch.tensor([[0, 1, -1], [2, -1, 1]], dtype=torch.int64)
    purity = torch.tensor([[1.0, 0.5, 0.0], [0.7, 0.0, 0.4]])
    assert S.drawable_windows(label, unlabelled=True).tolist() == [0, 1, 2, 3, 4, 5]
    assert S.drawable_windows(label, unlabelled=False).tolist() == [0, 1, 3, 5]
    # min_purity applies to the labelled windows; an unlabelled window's purity passes
    assert S.drawable_windows(label, purity=purity, min_purity=0.5, unlabelled=True).tolist() == [0, 1, 2, 3, 4]
    w = torch.tensor([5, 4, 3, 3, 0], dtype=torch.int64)             # `windows` still restricts, order and duplicates kept
    assert S.drawable_windows(label, w, unlabelled=True).tolist() == [5, 4, 3, 3, 0]
    assert S.drawable_windows(label, w, purity, 0.6, unlabelled=True).tolist() == [4, 3, 3, 0]


def test_scene_loader_unlabelled_argument_checks():
    sc = torch.zeros((3, 100, 150), dtype=torch.uint8)               # 2 x 3 windows at P 64 / S 32
    none = torch.full((2, 3), -1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no window to draw from"):
        eae_amd.SceneLoader(sc, none, patch=64, stride=32)
    with pytest.raises(RuntimeError) as e:                            # with unlabelled=True they are drawable: only the host scene is refused
        eae_amd.SceneLoader(sc, none, patch=64, stride=32, unlabelled=True)
    assert "no window to draw from" not in str(e.value)
    with pytest.raises(RuntimeError, match="no window to draw from"):
        eae_amd.SceneLoader(sc, none, patch=64, stride=32, unlabelled=True, windows=torch.zeros(0, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------------- engines / fit arguments
def test_class_weight_args_rejections_and_values():
    from eae_amd import _lib
    from eae_amd.engine import class_weight_args
    dev = torch.device("cpu")
    w, ign = class_weight_args(None, None, 10, dev)
    assert w is None and ign == _lib.NO_IGNORE == -2 ** 63
    w, ign = class_weight_args([1, 2, 0.5], -1, 3, dev)
    assert w.dtype == torch.float32 and w.tolist() == [1.0, 2.0, 0.5] and ign == -1
    assert class_weight_args(None, 1, 3, dev) == (None, 1)
    for bad, msg in (([1.0, 2.0], "one entry per class"), ([1.0, -0.5, 1.0], "finite and >= 0"), ([1.0, float("nan"), 1.0], "finite"),
                     ([1.0, float("inf"), 1.0], "finite"), ([0.0, 0.0, 0.0], "all be zero")):
        with pytest.raises(RuntimeError, match=msg):
            class_weight_args(bad, None, 3, dev)
    with pytest.raises(RuntimeError, match="ignore_index"):
        class_weight_args(None, 1.5, 3, dev)


def test_fit_functions_resolve_class_weight():
    import inspect
    from eae_amd import train as T

    class Loader:
        labels = torch.tensor([0, 0, 0, 1, -1, -1])
    np.testing.assert_allclose(T.resolve_class_weight("balanced", Loader(), 3).numpy(), [4 / (2 * 3), 4 / (2 * 1), 0.0], rtol=1e-6)
    v = [1.0, 2.0, 3.0]
    assert T.resolve_class_weight(v, Loader(), 3) is v and T.resolve_class_weight(None, Loader(), 3) is None
    with pytest.raises(RuntimeError, match="exposes its labels"):
        T.resolve_class_weight("balanced", [(torch.zeros(1), torch.zeros(1))], 3)
    for fn in (T.AEStepper.__init__, T.GroupAEStepper.__init__, T.MLPStepper.__init__, T.fit_autoencoder, T.fit_autoencoder_group,
               T.grid_search_autoencoder, T.fit_mlp, T.grid_search_mlp):
        par = inspect.signature(fn).parameters
        assert par["class_weight"].default is None and par["ignore_index"].default is None, fn


def test_grid_drivers_pass_the_criterion_on_only_when_set(tmp_path):
    from eae_amd import train as T
    seen = []

    def fit_fn(tr, va, alpha, lr, **kw):
        seen.append(kw)
        return {"model": None, "train_curve": [1.0], "val_curve": [1.0], "best_val_loss": 1.0, "epochs": 1}

    T.grid_search_autoencoder([], [], alpha_values=(1,), lr_values=(1e-3,), out_dir=str(tmp_path), verbose=False, fit_fn=fit_fn)
    T.grid_search_autoencoder([], [], alpha_values=(1,), lr_values=(1e-3,), out_dir=str(tmp_path), verbose=False, fit_fn=fit_fn,
                              class_weight=[1.0] * 10, ignore_index=-1)
    assert "class_weight" not in seen[0] and "ignore_index" not in seen[0]
    assert seen[1]["class_weight"] == [1.0] * 10 and seen[1]["ignore_index"] == -1
    assert "num_classes" not in seen[0] and "num_classes" not in seen[1]
    # a scheme name is resolved for the grid's own class count, which a custom fit function then receives too

    class Loader(list):
        labels = torch.tensor([0, 0, 3, -1])
    T.grid_search_autoencoder(Loader(), [], alpha_values=(1,), lr_values=(1e-3,), out_dir=str(tmp_path), verbose=False, fit_fn=fit_fn,
                              class_weight="balanced", num_classes=4)
    assert seen[2]["num_classes"] == 4 and seen[2]["class_weight"].tolist() == [0.75, 0.0, 0.0, 1.5]
