"""Accuracy assessment of a class map against a label raster (eae_amd.scene: `scene_confusion`, `evaluate_scene`, `block_split`,
`footprint_mask`; eae_amd.report: `confusion_metrics`): the entry point in the header, the library and the ctypes table; the argument
errors raised on the host; the metrics of a confusion matrix; and the blocked split with its guard band, which is pure host
arithmetic.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd import report as R
from eae_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbol_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    name = "eae_scene_confusion"
    assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
    assert hasattr(raw, name), f"{name} is not exported by the library"
    assert name in _lib.EXPORTS
    for name in ("scene_confusion", "evaluate_scene", "block_split", "footprint_mask", "confusion_metrics",
                 "classification_report_from_confusion"):
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))


def test_c_entry_point_rejects_bad_arguments():
    """The checks of the C call come before any launch, so they run without a device (the pointers are never dereferenced)."""
    lib = _lib.load()
    buf = (C.c_longlong * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(truth=p, eb=1, h=4, w=4, pred=p, ch=1, cw=1, cell=4, oy=0, ox=0, k=3, acc=0, counts=p)
    bad = [dict(truth=None), dict(pred=None), dict(counts=None), dict(eb=2), dict(k=0), dict(k=65), dict(cell=0), dict(oy=-1),
           dict(ox=-1), dict(h=0), dict(w=0), dict(ch=0), dict(cw=0), dict(acc=2)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.eae_scene_confusion(None, a["truth"], a["eb"], a["h"], a["w"], a["pred"], a["ch"], a["cw"], a["cell"], a["oy"], a["ox"],
                                     None, a["k"], a["acc"], a["counts"])
        assert rc == -2 and b"scene_confusion" in lib.eae_last_error(), change


# ---------------------------------------------------------------------------------------------------- argument errors (host tensors)
def test_scene_confusion_host_errors():
    truth = torch.zeros((40, 50), dtype=torch.uint8)
    pred = torch.zeros((5, 7), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.scene_confusion(pred, truth.to(torch.float32), 3, cell=8)
    for k in (0, 65):
        with pytest.raises(RuntimeError, match=r"num_classes must be in 1\.\.64"):
            eae_amd.scene_confusion(pred, truth, k, cell=8)
    with pytest.raises(RuntimeError, match="cell must be positive"):
        eae_amd.scene_confusion(pred, truth, 3, cell=0)
    for origin in ((-1, 0), (0, -3)):
        with pytest.raises(RuntimeError, match="origin must not be negative"):
            eae_amd.scene_confusion(pred, truth, 3, cell=8, origin=origin)
    with pytest.raises(RuntimeError, match="origin must be a pair"):
        eae_amd.scene_confusion(pred, truth, 3, cell=8, origin=4)
    with pytest.raises(RuntimeError, match=r"mask must be a \[H, W\]"):
        eae_amd.scene_confusion(pred, truth, 3, cell=8, mask=torch.zeros((40, 49), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="mask dtype"):
        eae_amd.scene_confusion(pred, truth, 3, cell=8, mask=torch.zeros((40, 50), dtype=torch.int32))
    for bad in (pred.to(torch.int32), pred[0], pred.to(torch.float32)):
        with pytest.raises(RuntimeError, match="2-D int64"):
            eae_amd.scene_confusion(bad, truth, 3, cell=8)
    with pytest.raises(RuntimeError, match=r"\[H, W\]"):
        eae_amd.scene_confusion(pred, truth[0], 3, cell=8)
    with pytest.raises(RuntimeError, match="empty"):
        eae_amd.scene_confusion(pred[:0], truth, 3, cell=8)
    with pytest.raises(RuntimeError, match="ignore must be"):
        eae_amd.scene_confusion(pred, truth, 3, cell=8, ignore=[1.5])
    with pytest.raises(RuntimeError, match="out must be"):
        eae_amd.scene_confusion(pred, truth, 3, cell=8, out=torch.zeros((3, 3), dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HIP device"):           # everything is in order but the tensors are on the host
        eae_amd.scene_confusion(pred, truth, 3, cell=8)


def test_evaluate_scene_host_errors():
    torch.manual_seed(0)
    ae = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3).eval()
    mlp = eae_amd.MLP(64, 10).eval()
    scene = torch.zeros((3, 150, 200), dtype=torch.uint8)
    truth = torch.zeros((150, 200), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="blend=False needs stride == patch"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth, 255.0, stride=32)
    with pytest.raises(RuntimeError, match="label raster of the scene's size"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth[:, :199], 255.0)
    with pytest.raises(RuntimeError, match="label raster of the scene's size"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth.T.contiguous(), 255.0, stride=32, blend=True)
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth.to(torch.float32), 255.0)
    with pytest.raises(RuntimeError, match="region must be"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth, 255.0, region=torch.ones((150, 199), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="stride that divides"):
        eae_amd.evaluate_scene(scene, ae, mlp, truth, 255.0, stride=48, blend=True)
    with pytest.raises(RuntimeError, match="mlp must be an MLP"):
        eae_amd.evaluate_scene(scene, ae, ae, truth, 255.0)
    with pytest.raises(RuntimeError):                               # everything is in order but the scene is a host tensor
        eae_amd.evaluate_scene(scene, ae, mlp, truth, 255.0)


# ---------------------------------------------------------------------------------------------------- confusion_metrics
def _expand(m):
    """(labels, preds) lists with m[i, j] samples of true class i predicted as j."""
    ii, jj = np.nonzero(m)
    reps = m[ii, jj]
    return np.repeat(ii, reps), np.repeat(jj, reps)


@pytest.mark.parametrize("k,seed", [(2, 0), (5, 1), (10, 2)])
def test_confusion_metrics_equals_class_metrics(k, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 30, (k, k))
    m += np.eye(k, dtype=m.dtype)                     # no class is absent from the lists, so class_metrics sees all K
    labels, preds = _expand(m)
    ref = R.class_metrics(labels, preds)
    got = R.confusion_metrics(m, num_classes=k)
    padded = np.zeros((k + 1, k + 1), dtype=np.int64)            # the same matrix with an empty unlabelled row / unclassified column
    padded[:k, :k] = m
    for g in (got, R.confusion_metrics(padded), R.confusion_metrics(torch.from_numpy(padded))):
        assert g["classes"].tolist() == ref["classes"].tolist()
        for key in ("precision", "recall", "f1"):
            assert np.abs(g[key] - ref[key]).max() <= 1e-12, key
        assert g["support"].tolist() == ref["support"].tolist() and g["total"] == ref["total"]
        assert abs(g["accuracy"] - ref["accuracy"]) <= 1e-12
        for key in ("macro", "weighted"):
            assert np.abs(np.array(g[key]) - np.array(ref[key])).max() <= 1e-12, key
        assert g["unclassified"].tolist() == [0] * k and g["area"].tolist() == m.sum(0).tolist()
    assert R.classification_report_from_confusion(m, num_classes=k) == R.classification_report(labels, preds)
    try:
        from sklearn.metrics import cohen_kappa_score
    except ImportError:
        return
    assert abs(got["kappa"] - cohen_kappa_score(labels, preds)) <= 1e-12


def test_confusion_metrics_hand_worked():
    """K = 2; row 2 = unlabelled truth, column 2 = not classified.
         M = [[5, 1], [2, 6]], u = [2, 0], a = [3, 1]:  support = [8, 8], mapped (labelled rows) = [7, 7]
         recall = [5/8, 6/8], precision = [5/7, 6/7], iou = [5/(8+7-5), 6/(8+7-6)], accuracy = 11/16
         kappa: po = 11/16, pe = (8*7 + 8*7) / 16^2 = 7/16 -> (4/16) / (9/16) = 4/9;  area = [5+2+3, 1+6+1]"""
    cm = np.array([[5, 1, 2], [2, 6, 0], [3, 1, 4]])
    g = R.confusion_metrics(cm)
    assert g["support"].tolist() == [8, 8] and g["total"] == 16
    assert np.allclose(g["recall"], [5 / 8, 6 / 8], rtol=0, atol=1e-15)
    assert np.allclose(g["precision"], [5 / 7, 6 / 7], rtol=0, atol=1e-15)
    assert np.allclose(g["iou"], [0.5, 6 / 9], rtol=0, atol=1e-15)
    assert abs(g["accuracy"] - 11 / 16) < 1e-15 and abs(g["kappa"] - 4 / 9) < 1e-15
    assert g["unclassified"].tolist() == [2, 0] and g["area"].tolist() == [10, 8]
    assert abs(g["mean_iou"] - (0.5 + 6 / 9) / 2) < 1e-15
    # zero division gives 0: a class that never occurs and is never predicted
    z = R.confusion_metrics(np.array([[4, 0, 0], [0, 0, 0], [0, 0, 0]]))
    assert z["recall"].tolist() == [1.0, 0.0] and z["precision"].tolist() == [1.0, 0.0] and z["iou"].tolist() == [1.0, 0.0]
    assert z["kappa"] == 0.0 and z["accuracy"] == 1.0
    empty = R.confusion_metrics(np.zeros((3, 3), dtype=np.int64))
    assert empty["accuracy"] == 0.0 and empty["kappa"] == 0.0 and empty["total"] == 0
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((1, 1))):
        with pytest.raises(ValueError):
            R.confusion_metrics(bad)
    with pytest.raises(ValueError):
        R.confusion_metrics(np.zeros((4, 4)), num_classes=2)
    try:
        from sklearn.metrics import cohen_kappa_score
    except ImportError:
        return
    labels, preds = _expand(cm[:2])                   # the labelled rows; prediction 2 = not classified
    assert abs(g["kappa"] - cohen_kappa_score(labels, preds)) <= 1e-12


# ---------------------------------------------------------------------------------------------------- footprint_mask, block_split
def _footprint_loop(ids, n_w, p, s, h, w):
    out = np.zeros((h, w), dtype=bool)
    for n in ids:
        y, x = (n // n_w) * s, (n % n_w) * s
        out[y:y + p, x:x + p] = True
    return out


@pytest.mark.parametrize("h,w,p,s", [(37, 41, 16, 5), (40, 40, 8, 8), (30, 50, 12, 1), (48, 20, 20, 7)])
def test_footprint_mask_matches_a_loop(h, w, p, s):
    n_h, n_w = S.window_grid(h, w, p, s, any_patch=True)
    g = torch.Generator().manual_seed(h + s)
    for count in (0, 1, 3, n_h * n_w):
        ids = torch.randperm(n_h * n_w, generator=g)[:count]
        got = eae_amd.footprint_mask(ids, n_w, p, s, h, w)
        assert got.dtype == torch.bool and tuple(got.shape) == (h, w) and got.device.type == "cpu"
        assert np.array_equal(got.numpy(), _footprint_loop(ids.tolist(), n_w, p, s, h, w)), count
    dup = torch.tensor([0, 0, n_w + 1], dtype=torch.int64)                  # duplicates are one footprint
    assert np.array_equal(eae_amd.footprint_mask(dup, n_w, p, s, h, w).numpy(), _footprint_loop(dup.tolist(), n_w, p, s, h, w))
    # a raster smaller than the grid's extent clips the footprints
    clip = eae_amd.footprint_mask(torch.arange(n_h * n_w), n_w, p, s, h - 3, w - 2)
    assert np.array_equal(clip.numpy(), _footprint_loop(range(n_h * n_w), n_w, p, s, h, w)[:h - 3, :w - 2])
    with pytest.raises(RuntimeError, match="1-D int64"):
        eae_amd.footprint_mask(torch.arange(3, dtype=torch.int32), n_w, p, s, h, w)
    with pytest.raises(RuntimeError, match="negative"):
        eae_amd.footprint_mask(torch.tensor([-1]), n_w, p, s, h, w)


@pytest.mark.parametrize("p,s", [(64, 64), (64, 32), (64, 16), (48, 20)])
@pytest.mark.parametrize("block", [1, 3])
def test_block_split_partitions_and_keeps_the_sides_apart(p, s, block):
    n_h, n_w = 9, 13
    h, w = (n_h - 1) * s + p, (n_w - 1) * s + p
    train, val, dropped = eae_amd.block_split(n_h, n_w, p, s, block, val_fraction=0.25, seed=4)
    for t in (train, val, dropped):
        assert t.dtype == torch.int64 and t.device.type == "cpu" and t.dim() == 1
        assert t.tolist() == sorted(set(t.tolist()))
    assert sorted(train.tolist() + val.tolist() + dropped.tolist()) == list(range(n_h * n_w))
    assert val.numel() > 0
    n_blocks = -(-n_h // block) * -(-n_w // block)
    order = torch.randperm(n_blocks, generator=torch.Generator().manual_seed(4))[:max(1, round(0.25 * n_blocks))]
    b_w = -(-n_w // block)
    want = [n for n in range(n_h * n_w) if (n // n_w // block) * b_w + (n % n_w) // block in set(order.tolist())]
    assert val.tolist() == want
    # the guard band: no training pixel is a validation pixel, and nothing is dropped that does not touch validation
    f_train = eae_amd.footprint_mask(train, n_w, p, s, h, w)
    f_val = eae_amd.footprint_mask(val, n_w, p, s, h, w)
    assert not bool((f_train & f_val).any())
    for n in dropped.tolist():
        assert bool((eae_amd.footprint_mask(torch.tensor([n]), n_w, p, s, h, w) & f_val).any()), n
    if s == p:
        assert dropped.numel() == 0
    again = eae_amd.block_split(n_h, n_w, p, s, block, val_fraction=0.25, seed=4)
    assert all(torch.equal(a, b) for a, b in zip(again, (train, val, dropped)))
    other = eae_amd.block_split(n_h, n_w, p, s, block, val_fraction=0.25, seed=5)
    assert not torch.equal(other[1], val)


def test_block_split_arguments():
    assert eae_amd.block_split(1, 1, 64, 64, 4)[1].tolist() == [0]              # one block: it is the validation block
    t, v, d = eae_amd.block_split(4, 4, 64, 64, 2, val_fraction=0.01)           # at least one block
    assert v.numel() == 4 and t.numel() == 12 and d.numel() == 0
    for args in [(0, 3, 64, 32, 2), (3, 0, 64, 32, 2), (3, 3, 64, 0, 2), (3, 3, 64, 65, 2), (3, 3, 64, 32, 0)]:
        with pytest.raises(RuntimeError):
            eae_amd.block_split(*args)
    for f in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(RuntimeError, match="val_fraction"):
            eae_amd.block_split(3, 3, 64, 32, 2, val_fraction=f)
