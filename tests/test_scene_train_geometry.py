"""Training from a scene (eae_amd.scene: `stage_scene_windows`, `window_labels`, `SceneLoader`): the two entry points in the header,
the library and the ctypes table; the argument errors raised on the host; and the id schedule of a `SceneLoader`, which is pure
host arithmetic (`window_schedule`, `drawable_windows`).  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd import scene as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eae_scene_stage_windows", "eae_scene_window_labels")


def test_new_symbols_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.EXPORTS
    for name in ("EAE_CROP_WINDOW 0", "EAE_CROP_SCENE 1"):
        assert re.search(r"#define\s+" + name.replace(" ", r"\s+") + r"\b", src)
    for name in ("stage_scene_windows", "window_labels", "SceneLoader", "window_schedule", "drawable_windows"):
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))


def test_any_patch_grid_is_opt_in():
    """The model-free calls take any positive patch size; `window_grid` itself keeps the model's rule."""
    assert S.window_grid(37, 41, 16, 5, any_patch=True) == (5, 6)
    assert S.window_grid(70, 64, 64, 3, any_patch=True) == S.window_grid(70, 64, 64, 3) == (3, 1)
    with pytest.raises(RuntimeError, match="multiple of 64"):
        S.window_grid(37, 41, 16, 5)
    for h, w, p, s in [(37, 41, 0, 1), (37, 41, 16, 0), (37, 41, 16, 17), (15, 41, 16, 5), (37, 15, 16, 5)]:
        with pytest.raises(RuntimeError):
            S.window_grid(h, w, p, s, any_patch=True)


# ---------------------------------------------------------------------------------------------------- argument errors (host tensors)
def _scene(c=3, h=100, w=150):
    return torch.zeros((c, h, w), dtype=torch.uint8)


def test_stage_scene_windows_host_errors():
    sc, ids = _scene(), torch.tensor([0, 3, 1], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="crop must be"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids, crop="jitter")
    with pytest.raises(RuntimeError, match="crop must be"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids, crop=1)
    with pytest.raises(RuntimeError, match=r"params must be int32 \[B,3\]"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids, params=torch.zeros((2, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"params must be int32 \[B,3\]"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids, params=torch.zeros((3, 2), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="noise must be"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids, noise=torch.zeros((3, 3, 64, 32)))
    with pytest.raises(RuntimeError, match="1-D int64"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids.to(torch.int32))
    with pytest.raises(RuntimeError, match="windows is empty"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids[:0])
    with pytest.raises(RuntimeError, match="stride must be"):
        eae_amd.stage_scene_windows(sc, 255.0, 64, 65, ids)
    with pytest.raises(RuntimeError, match="smaller than one"):
        eae_amd.stage_scene_windows(sc, 255.0, 128, 64, ids)
    with pytest.raises(RuntimeError, match="planar tensor"):
        eae_amd.stage_scene_windows(sc[0], 255.0, 64, 32, ids)
    with pytest.raises(RuntimeError):                               # everything is in order but the scene is a host tensor
        eae_amd.stage_scene_windows(sc, 255.0, 64, 32, ids)


def test_window_labels_host_errors():
    r = torch.zeros((100, 150), dtype=torch.uint8)
    for k in (0, 65, -1):
        with pytest.raises(RuntimeError, match=r"num_classes must be in 1\.\.64"):
            eae_amd.window_labels(r, 64, 32, k)
    with pytest.raises(RuntimeError, match=r"\[H, W\]"):
        eae_amd.window_labels(r[None], 64, 32, 10)
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.window_labels(r.float(), 64, 32, 10)
    with pytest.raises(RuntimeError, match="smaller than one"):
        eae_amd.window_labels(r, 128, 32, 10)
    with pytest.raises(RuntimeError, match="stride must be"):
        eae_amd.window_labels(r, 64, 0, 10)
    with pytest.raises(RuntimeError, match="at most 4080"):
        eae_amd.window_labels(torch.zeros((5000, 5000), dtype=torch.uint8), 4096, 64, 10)
    with pytest.raises(RuntimeError, match="ignore must be"):
        eae_amd.window_labels(r, 64, 32, 10, ignore=[1.5])
    with pytest.raises(RuntimeError):                               # everything is in order but the raster is a host tensor
        eae_amd.window_labels(r, 64, 32, 10, ignore=3)


def test_scene_loader_host_errors():
    sc = _scene()                                                   # 100 x 150 at P 64 / S 32: a 2 x 3 grid
    label = torch.tensor([[0, 1, -1], [2, -1, 1]], dtype=torch.int64)
    purity = torch.tensor([[1.0, 0.5, 0.0], [0.7, 0.0, 0.4]])
    with pytest.raises(RuntimeError, match="crop must be"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, crop="both")
    for bs in (0, -4):
        with pytest.raises(RuntimeError, match="batch_size must be positive"):
            eae_amd.SceneLoader(sc, label, patch=64, stride=32, batch_size=bs)
    # the label map of a raster whose H x W differs from the scene's has another grid (here 100 x 182: 2 x 4)
    other = torch.zeros(S.window_grid(100, 182, 64, 32), dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"label must be the int64 \[nH, nW\] = \[2, 3\]"):
        eae_amd.SceneLoader(sc, other, patch=64, stride=32)
    with pytest.raises(RuntimeError, match=r"label must be the int64 \[nH, nW\]"):
        eae_amd.SceneLoader(sc, torch.zeros((100, 150), dtype=torch.int64), patch=64, stride=32)      # the raster itself
    with pytest.raises(RuntimeError, match=r"label must be the int64 \[nH, nW\]"):
        eae_amd.SceneLoader(sc, label.to(torch.int32), patch=64, stride=32)
    # an empty drawable set: no labelled window at all, none among the given ones, none pure enough
    with pytest.raises(RuntimeError, match="no window to draw from"):
        eae_amd.SceneLoader(sc, torch.full((2, 3), -1, dtype=torch.int64), patch=64, stride=32)
    with pytest.raises(RuntimeError, match="no window to draw from"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, windows=torch.tensor([2, 4], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no window to draw from"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, purity=purity, min_purity=1.5)
    with pytest.raises(RuntimeError, match="min_purity needs the purity map"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, min_purity=0.5)
    with pytest.raises(RuntimeError, match="outside the grid"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, windows=torch.tensor([0, 6], dtype=torch.int64))
    with pytest.raises(RuntimeError):                               # everything is in order but the scene is a host tensor
        eae_amd.SceneLoader(sc, label, patch=64, stride=32)


# ---------------------------------------------------------------------------------------------------- the id schedule
def test_drawable_windows():
    label = torch.tensor([[0, 1, -1], [2, -1, 1]], dtype=torch.int64)
    purity = torch.tensor([[1.0, 0.5, 0.0], [0.7, 0.0, 0.4]])
    assert S.drawable_windows(label).tolist() == [0, 1, 3, 5]
    assert S.drawable_windows(label, purity=purity, min_purity=0.5).tolist() == [0, 1, 3]
    assert S.drawable_windows(label, purity=purity, min_purity=0.0).tolist() == [0, 1, 3, 5]
    # the given order (and duplicates) are kept
    w = torch.tensor([5, 4, 3, 3, 0], dtype=torch.int64)
    assert S.drawable_windows(label, w).tolist() == [5, 3, 3, 0]
    assert S.drawable_windows(label, w, purity, 0.6).tolist() == [3, 3, 0]
    assert S.drawable_windows(label, w[:0]).numel() == 0


@pytest.mark.parametrize("n,bs", [(6, 4), (8, 4), (3, 4), (1, 1), (13, 5)])
def test_schedule_len_and_cover(n, bs):
    full = S.window_schedule(n, bs, 0, seed=7)
    assert len(full) == S.schedule_len(n, bs) == -(-n // bs)
    assert sorted(torch.cat(full).tolist()) == list(range(n))
    assert all(b.numel() == bs for b in full[:-1]) and full[-1].numel() == n - bs * (len(full) - 1)
    cut = S.window_schedule(n, bs, 0, seed=7, drop_last=True) if n >= bs else []
    assert len(cut) == S.schedule_len(n, bs, drop_last=True) == n // bs
    assert all(b.numel() == bs for b in cut)
    # drop_last drops the tail of the same order
    assert [b.tolist() for b in cut] == [b.tolist() for b in full[:len(cut)]]


def test_schedule_order():
    n, bs, seed = 23, 4, 11
    a = [[b.tolist() for b in S.window_schedule(n, bs, e, seed=seed)] for e in (0, 1)]
    b = [[b.tolist() for b in S.window_schedule(n, bs, e, seed=seed)] for e in (0, 1)]
    assert a == b                                                   # one seed: the same sequence over two epochs
    assert a[0] != a[1]                                             # epoch 0 and epoch 1 differ
    for e in (0, 1):                                                # the documented permutation
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed + e)).tolist()
        assert sum(a[e], []) == perm
    assert sum(a[0], []) != torch.cat(S.window_schedule(n, bs, 0, seed=seed + 5)).tolist()          # another seed, another order
    for e in (0, 3):                                                # shuffle=False: ascending, every epoch
        asc = S.window_schedule(n, bs, e, seed=seed, shuffle=False)
        assert torch.cat(asc).tolist() == list(range(n))
    with pytest.raises(RuntimeError, match="batch_size must be positive"):
        S.window_schedule(n, 0, 0)
    with pytest.raises(RuntimeError, match="no window"):
        S.window_schedule(0, 4, 0)


def test_loader_ids_follow_the_schedule():
    """The ids a loader stages are ``windows[schedule]``: two loaders' worth of bookkeeping over disjoint window sets."""
    label = torch.tensor([[0, 1, -1, 2], [2, -1, 1, 0], [1, 1, 0, -1]], dtype=torch.int64)
    ids = S.drawable_windows(label)
    perm = torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(0))
    train, val = ids[perm[:6]], ids[perm[6:]]
    assert not set(train.tolist()) & set(val.tolist())
    for w in (train, val):
        draw = S.drawable_windows(label, w)
        assert draw.tolist() == w.tolist()
        for e in (0, 1):
            got = [draw[b].tolist() for b in S.window_schedule(draw.numel(), 4, e, seed=3)]
            assert sorted(sum(got, [])) == sorted(w.tolist())
            assert all((label.reshape(-1)[torch.tensor(g)] >= 0).all() for g in got)
