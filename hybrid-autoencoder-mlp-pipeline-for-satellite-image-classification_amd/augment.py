"""On-device input staging: the reference's loader-side transforms (R.md:211-234) as one HIP kernel.

`augment_batch(u8, train=True)` takes a uint8 HWC batch already on the device ([B,H,W,3], 12 KB/img over PCIe instead of
48 KB of fp32) and returns the fp32 NCHW tensor the encoder reads: RandomHorizontalFlip -> RandomCrop(H, padding=4) ->
ToTensor -> AddGaussianNoise(0, 0.03) in training mode, ToTensor in eval mode.

`stage_bands(data, divisor, index)` does the same for multispectral data (in_channels 1..16): a uint8 / uint16 planar dataset
[N,C,H,W] kept on the device, gathered by index, each band divided by its own divisor (e.g. 10000 for Sentinel-2 reflectance).
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check
from .engine import _ptr, _stream, _require_gpu


def augment_batch(u8, train=True, noise_std=0.03, seed=0, step=0, params=None, noise=None):
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise RuntimeError(f"expected uint8 HWC batch [B,H,W,3], got {tuple(u8.shape)} {u8.dtype}")
    _require_gpu(u8.device)
    lib = _lib.load()
    u8 = u8.contiguous()
    b, h, w, _ = u8.shape
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=u8.device)
    if params is not None:
        params = params.to(device=u8.device, dtype=torch.int32).contiguous()
        if params.shape != (b, 3):
            raise RuntimeError("params must be int32 [B,3] = (flip, top, left)")
    if noise is not None:
        noise = noise.to(device=u8.device, dtype=torch.float32).contiguous()
        if noise.shape != out.shape:
            raise RuntimeError("noise must be [B,3,H,W]")
    check(lib.eae_augment(_stream(), _ptr(u8), _ptr(out), b, h, w, int(train), float(noise_std), int(seed) & (2**64 - 1),
                          int(step) & (2**64 - 1), _ptr(params), _ptr(noise)))
    return out


def stage_bands(data, divisor, index=None, train=True, noise_std=0.03, seed=0, step=0, params=None, noise=None):
    """fp32 NCHW [B,C,H,W] batch from a uint8 / uint16 dataset `data` [N,C,H,W] on the device: images `index` (int64 [B]; None =
    all N), flip -> pad-4 crop -> / divisor[c] -> + noise_std * N(0,1) (train=False: the division only).  Randomness: Philox
    keyed by (seed, step), or explicit `params` int32 [B,3] = (flip, top, left) and `noise` [B,C,H,W] (include/eae.h eae_stage_bands)."""
    if data.dtype not in (torch.uint8, torch.uint16) or data.dim() != 4:
        raise RuntimeError(f"expected a uint8 or uint16 dataset [N,C,H,W], got {tuple(data.shape)} {data.dtype}")
    _require_gpu(data.device)
    n, c, h, w = data.shape
    if not 1 <= c <= 16:
        raise RuntimeError(f"stage_bands: in_channels must be in 1..16, got {c}")
    lib = _lib.load()
    data = data.contiguous()
    div = torch.as_tensor(divisor, dtype=torch.float32).to(data.device).reshape(-1)
    if div.numel() == 1:
        div = div.expand(c)
    if div.numel() != c:
        raise RuntimeError(f"divisor must have one value per band ({c}), got {div.numel()}")
    div = div.contiguous()
    if index is not None:
        index = torch.as_tensor(index).to(device=data.device, dtype=torch.int64).reshape(-1).contiguous()
        b = index.numel()
    else:
        b = n
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=data.device)
    if params is not None:
        params = params.to(device=data.device, dtype=torch.int32).contiguous()
        if params.shape != (b, 3):
            raise RuntimeError("params must be int32 [B,3] = (flip, top, left)")
    if noise is not None:
        noise = noise.to(device=data.device, dtype=torch.float32).contiguous()
        if noise.shape != out.shape:
            raise RuntimeError(f"noise must be [B,C,H,W] = {tuple(out.shape)}")
    check(lib.eae_stage_bands(_stream(), _ptr(data), data.element_size(), n, c, h, w, _ptr(index), b, _ptr(div), _ptr(out), int(train),
                              float(noise_std), int(seed) & (2**64 - 1), int(step) & (2**64 - 1), _ptr(params), _ptr(noise)))
    return out
