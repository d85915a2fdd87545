"""Classify whole scenes: sliding-window latents and class maps from a planar raster [C,H,W] held on the device.

A model of size P x P (the encoder's ``image_size``) runs over windows placed at stride S on both axes; only whole windows are used
(`window_grid`).  The input value is ``(float)v / divisor[c]``, the eval-mode expression of `stage_bands`.  conv1 reads the scene
directly (no staged fp32 [B,C,P,P] batch), the MLP reads the engine's latent rows in place, and one C call covers the scene
(include/eae.h, "scene classification").  Everything runs in eval mode: BatchNorm with running statistics, no dropout.

- `scene_windows` gathers windows as the fp32 NCHW batch the encoder reads (bitwise `stage_bands(train=False)` on host-cut windows);
- `encode_scene` returns the latents z [nH*nW, L] (clustering, retrieval);
- `classify_scene` returns probabilities [K,nH,nW] and labels [nH,nW], or with ``blend=True`` (S divides P) the map of S x S cells,
  each the mean probability of the windows that cover it, [K,nH+k-1,nW+k-1] with k = P/S.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import check
from .engine import _ptr, _stream, _require_gpu, engine_for

_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}


# ---------------------------------------------------------------------------------------------------- grid arithmetic (pure Python)
def window_grid(height, width, patch, stride):
    """(nH, nW): whole P x P windows at stride S in an H x W scene.  Window n = i*nW + j starts at pixel (i*S, j*S)."""
    height, width, patch, stride = int(height), int(width), int(patch), int(stride)
    if patch <= 0 or patch % 64:
        raise RuntimeError(f"the patch size must be a positive multiple of 64, got {patch}")
    if not 1 <= stride <= patch:
        raise RuntimeError(f"stride must be in 1..{patch} (the patch size), got {stride}")
    if height < patch or width < patch:
        raise RuntimeError(f"scene {height} x {width} is smaller than one {patch} x {patch} window")
    return (height - patch) // stride + 1, (width - patch) // stride + 1


def window_origin(n, n_w, stride):
    """Top-left pixel (y, x) of window n of a grid with n_w windows per row."""
    i, j = divmod(int(n), int(n_w))
    return i * int(stride), j * int(stride)


def cell_grid(n_h, n_w, patch, stride):
    """(cH, cW, k) of the blended cell map: S x S cells, k = P/S windows per axis cover a cell (S must divide P)."""
    patch, stride = int(patch), int(stride)
    if stride < 1 or patch % stride:
        raise RuntimeError(f"blend=True needs a stride that divides the patch size ({patch}), got {stride}")
    k = patch // stride
    return int(n_h) + k - 1, int(n_w) + k - 1, k


def cell_windows(ci, cj, n_h, n_w, k):
    """Window rows i0..i1 and columns j0..j1 (inclusive) that cover cell (ci, cj)."""
    return max(0, ci - k + 1), min(n_h - 1, ci), max(0, cj - k + 1), min(n_w - 1, cj)


def cell_coverage(n_h, n_w, k):
    """Number of windows covering each cell, as a [n_h+k-1, n_w+k-1] int64 CPU tensor."""
    rows = torch.tensor([min(n_h - 1, c) - max(0, c - k + 1) + 1 for c in range(n_h + k - 1)], dtype=torch.int64)
    cols = torch.tensor([min(n_w - 1, c) - max(0, c - k + 1) + 1 for c in range(n_w + k - 1)], dtype=torch.int64)
    return rows[:, None] * cols[None, :]


# ---------------------------------------------------------------------------------------------------- argument checks
def _encoder_of(encoder):
    from .modules import Encoder, SupervisedAutoencoder
    if isinstance(encoder, SupervisedAutoencoder):
        return encoder.enc
    if isinstance(encoder, Encoder):
        return encoder
    raise RuntimeError(f"encoder must be an Encoder or a SupervisedAutoencoder, got {type(encoder).__name__}")


def _scene_desc(scene, divisor, patch, stride):
    """Validate the scene (before any device work) and return (EaeScene, keep-alive tensors, nH, nW)."""
    if not isinstance(scene, torch.Tensor) or scene.dim() != 3:
        raise RuntimeError("scene must be a planar tensor [C,H,W]")
    if scene.dtype not in _DTYPES:
        raise RuntimeError(f"scene dtype must be uint8, uint16 or float32, got {scene.dtype}")
    _require_gpu(scene.device)
    c, h, w = (int(v) for v in scene.shape)
    if not 1 <= c <= 16:
        raise RuntimeError(f"scene: in_channels must be in 1..16, got {c}")
    n_h, n_w = window_grid(h, w, patch, stride)
    div = torch.as_tensor(divisor, dtype=torch.float32).reshape(-1)
    if div.numel() == 1:
        div = div.expand(c)
    if div.numel() != c:
        raise RuntimeError(f"divisor must have one value per band ({c}), got {div.numel()}")
    div = div.to(scene.device).contiguous()
    scene = scene.contiguous()
    desc = _lib.EaeScene(C.c_void_p(scene.data_ptr()), C.c_void_p(div.data_ptr()), _DTYPES[scene.dtype], c, h, w, int(patch),
                         int(stride))
    return desc, (scene, div), n_h, n_w


def _range(first, count, total):
    first = int(first)
    count = total - first if count is None else int(count)
    if first < 0 or count <= 0 or first + count > total:
        raise RuntimeError(f"windows {first}..{first + count - 1} are outside the grid of {total}")
    return first, count


# ---------------------------------------------------------------------------------------------------- public functions
def scene_windows(scene, divisor, patch, stride, first=0, count=None):
    """fp32 NCHW [count,C,P,P] of windows first .. first+count-1 (count=None: to the end of the grid)."""
    desc, keep, n_h, n_w = _scene_desc(scene, divisor, patch, stride)
    first, count = _range(first, count, n_h * n_w)
    lib = _lib.load()
    out = torch.empty((count, keep[0].shape[0], int(patch), int(patch)), dtype=torch.float32, device=keep[0].device)
    with torch.cuda.device(keep[0].device):
        check(lib.eae_scene_windows(_stream(), C.byref(desc), first, count, _ptr(out)))
    return out


def _prepare(scene, encoder, divisor, stride, batch):
    enc = _encoder_of(encoder)
    patch = int(enc.image_size)
    stride = patch if stride is None else int(stride)
    desc, keep, n_h, n_w = _scene_desc(scene, divisor, patch, stride)
    if desc.C != int(enc.in_channels):
        raise RuntimeError(f"scene has {desc.C} bands, the encoder takes in_channels={enc.in_channels}")
    if int(batch) < 1:
        raise RuntimeError(f"batch must be positive, got {batch}")
    if next(enc.parameters()).device != keep[0].device:
        raise RuntimeError("the scene and the model must be on the same device")
    eng = engine_for(enc, max_batch=int(batch))
    if eng.quant != 0:
        raise RuntimeError("scene classification supports bf16 engines only (quant=1 / fp8 is not supported)")
    eng.params_changed()
    return eng, desc, keep, n_h, n_w, patch, stride


def encode_scene(scene, encoder, divisor=1.0, stride=None, batch=512):
    """Latents z [nH*nW, L] of every window (row n = window i*nW + j), eval-mode encoder, `batch` windows per encoder pass (the
    engine's max_batch, at least this).  stride=None: the patch size (non-overlapping windows)."""
    eng, desc, keep, n_h, n_w, _, _ = _prepare(scene, encoder, divisor, stride, batch)
    n = n_h * n_w
    z = torch.empty((n, eng.latent), dtype=torch.float32, device=eng.device)
    with torch.cuda.device(eng.device):
        check(eng.lib.eae_scene_encode(eng.ctx, _stream(), C.byref(desc), 0, n, _ptr(z)))
    return z


def classify_scene(scene, encoder, mlp, divisor=1.0, stride=None, batch=512, blend=False):
    """(probs [K,nH,nW] float32 softmax, labels [nH,nW] int64 argmax) of every window: encoder -> MLP in eval mode, one C call.
    blend=True (stride divides the patch size, k = P/S): the map of S x S cells instead, probs [K,nH+k-1,nW+k-1] = mean over the
    windows covering each cell, labels = argmax of that map."""
    from .mlp_engine import mlp_engine_for
    from .modules import MLP
    if not isinstance(mlp, MLP):
        raise RuntimeError(f"mlp must be an MLP, got {type(mlp).__name__}")
    enc = _encoder_of(encoder)
    if int(mlp.input_dim) != int(enc.latent_dim):
        raise RuntimeError(f"the MLP takes input_dim={mlp.input_dim}, the encoder's latent_dim is {enc.latent_dim}")
    if blend:
        patch = int(enc.image_size)
        cell_grid(1, 1, patch, patch if stride is None else int(stride))      # the stride must divide the patch size
    eng, desc, keep, n_h, n_w, patch, stride = _prepare(scene, encoder, divisor, stride, batch)
    if next(mlp.parameters()).device != eng.device:
        raise RuntimeError("the MLP and the encoder must be on the same device")
    meng = mlp_engine_for(mlp)
    k_cls = int(mlp.num_classes)
    probs = torch.empty((k_cls, n_h, n_w), dtype=torch.float32, device=eng.device)
    labels = torch.empty((n_h, n_w), dtype=torch.int64, device=eng.device)
    with torch.cuda.device(eng.device):
        check(eng.lib.eae_scene_classify(eng.ctx, meng.ctx, _stream(), C.byref(desc), 0, n_h * n_w, _ptr(probs), _ptr(labels)))
        if not blend:
            return probs, labels
        c_h, c_w, k = cell_grid(n_h, n_w, patch, stride)
        cprobs = torch.empty((k_cls, c_h, c_w), dtype=torch.float32, device=eng.device)
        clabels = torch.empty((c_h, c_w), dtype=torch.int64, device=eng.device)
        check(eng.lib.eae_scene_blend(_stream(), _ptr(probs), k_cls, n_h, n_w, k, _ptr(cprobs), _ptr(clabels)))
    return cprobs, clabels
