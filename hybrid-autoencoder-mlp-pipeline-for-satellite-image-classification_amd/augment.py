"""On-device input staging: the reference's loader-side transforms (R.md:211-234) as one HIP kernel.

`augment_batch(u8, train=True)` takes a uint8 HWC batch already on the device ([B,H,W,3], 12 KB/img over PCIe instead of
48 KB of fp32) and returns the fp32 NCHW tensor the encoder reads: RandomHorizontalFlip -> RandomCrop(H, padding=4) ->
ToTensor -> AddGaussianNoise(0, 0.03) in training mode, ToTensor in eval mode.

`stage_bands(data, divisor, index)` does the same for multispectral data (in_channels 1..16): a uint8 / uint16 planar dataset
[N,C,H,W] kept on the device, gathered by index, each band divided by its own divisor (e.g. 10000 for Sentinel-2 reflectance).

`Augment` is the stronger policy both take as ``augment=`` (and `stage_scene_windows` and `SceneLoader`, scene.py): the eight
rotations and flips of the square, a small rotation and scale, and a per-band gain and offset (include/eae.h, "augmentation policy").
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._lib import check
from .engine import _ptr, _stream, _require_gpu


class Augment:
    """The augmentation policy of the staging calls; off by default, every part on its own.

    dihedral   a random quarter turn per image (counter-clockwise, as ``np.rot90``); with the flip that is all of D4.  Square images.
    rotate     theta_max in degrees (0..180): a rotation about the centre by theta uniform in [-theta_max, theta_max).
    scale      s in [0, 1): a scale about the centre by sigma uniform in [1 - s, 1 + s); bilinear sampling, zeros outside.
    gain       in [0, 1): one gain per image, uniform in [1 - gain, 1 + gain).
    band_gain  in [0, 1): one gain per image and band, uniform in [1 - band_gain, 1 + band_gain).
    offset     >= 0: one offset per image and band, uniform in [-offset, offset), in output units (after the divisor).

    The order, in the image's direction: flip -> pad-4 crop -> quarter turns -> rotation and scale -> / divisor -> gain and offset ->
    noise.  (flip, top, left) of a batch position are what they are without a policy; ``train=False`` ignores the policy."""

    _FIELDS = ("rotate", "scale", "gain", "band_gain", "offset")

    def __init__(self, dihedral=False, rotate=0.0, scale=0.0, gain=0.0, band_gain=0.0, offset=0.0, _draw_mode=0):
        if not isinstance(dihedral, (bool, numbers.Integral)):
            raise RuntimeError(f"Augment: dihedral must be a bool, got {dihedral!r}")
        self.dihedral = bool(dihedral)
        for name, v in zip(self._FIELDS, (rotate, scale, gain, band_gain, offset)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise RuntimeError(f"Augment: {name} must be a finite number, got {v!r}")
            if v < 0:
                raise RuntimeError(f"Augment: {name} must not be negative, got {v!r}")
            setattr(self, name, float(v))
        if self.rotate > 180.0:
            raise RuntimeError(f"Augment: rotate must be at most 180 degrees, got {rotate!r}")
        for name in ("scale", "gain", "band_gain"):
            if getattr(self, name) >= 1.0:
                raise RuntimeError(f"Augment: {name} must be below 1, got {getattr(self, name)!r}")
        if _draw_mode not in (0, 1, 2):
            raise RuntimeError(f"Augment: _draw_mode must be 0, 1 or 2, got {_draw_mode!r}")
        self._draw_mode = int(_draw_mode)

    def __repr__(self):
        return "Augment(dihedral=%r, %s)" % (self.dihedral, ", ".join(f"{n}={getattr(self, n)!r}" for n in self._FIELDS))

    def _struct(self):
        return _lib.EaeAug(int(self.dihedral), self.rotate, self.scale, self.gain, self.band_gain, self.offset, self._draw_mode)


def _aug_args(augment, params, geom, affine, radio, b, c, h, w, dev):
    """The policy and the explicit draws of a staging call, validated for a [b,c,h,w] batch: None when the call is the plain one, else
    (policy struct or None, geom, affine, radio) with the tensors on ``dev`` as the C call reads them."""
    if augment is not None and not isinstance(augment, Augment):
        raise RuntimeError(f"augment must be an eae_amd.Augment or None, got {type(augment).__name__}")
    if augment is None and geom is None and affine is None and radio is None:
        return None
    if params is not None:
        raise RuntimeError("with augment= or explicit geom / affine / radio the geometric draws are geom int32 [B,4] = "
                           "(flip, top, left, rot), not params [B,3]")
    if ((augment is not None and augment.dihedral) or geom is not None) and h != w:
        raise RuntimeError(f"quarter turns (Augment(dihedral=True), geom) need square images, got {h} x {w}")

    def draw(t, name, shape, dtype, what):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            raise RuntimeError(f"{name} must be {what} with B = {b}" + (f", C = {c}" if name == "radio" else ""))
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must be {what}, got dtype {t.dtype}")
        return t.to(device=dev).contiguous()

    geom = draw(geom, "geom", (b, 4), torch.int32, "int32 [B,4] = (flip, top, left, rot)")
    affine = draw(affine, "affine", (b, 2), torch.float32, "float32 [B,2] = (a, b)")
    radio = draw(radio, "radio", (b, c, 2), torch.float32, "float32 [B,C,2] = (gain, offset)")
    return (augment._struct() if augment is not None else None), geom, affine, radio


def _plain_draws(params, noise, shape, dev):
    """The explicit draws of a plain staging call for an output of ``shape`` = (b, c, h, w), on ``dev`` as the C call reads them:
    ``params`` int32 [B,3] = (flip, top, left) and ``noise`` float32 [B,C,H,W], each or None."""
    if params is not None:
        if not isinstance(params, torch.Tensor) or tuple(params.shape) != (shape[0], 3):
            raise RuntimeError(f"params must be int32 [B,3] = (flip, top, left) with B = {shape[0]}")
        params = params.to(device=dev, dtype=torch.int32).contiguous()
    if noise is not None:
        if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != tuple(shape):
            raise RuntimeError(f"noise must be [B,C,H,W] = {tuple(shape)}")
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
    return params, noise


def augment_batch(u8, train=True, noise_std=0.03, seed=0, step=0, params=None, noise=None, augment=None, geom=None, affine=None,
                  radio=None):
    """fp32 NCHW [B,3,H,W] of a uint8 HWC batch on the device (module docstring).  ``augment``: an `Augment` policy; ``geom`` int32
    [B,4] = (flip, top, left, rot), ``affine`` float32 [B,2] = (a, b), ``radio`` float32 [B,3,2] = (gain, offset): explicit draws in
    place of the policy's (parity tests).  Without any of them the call is the plain one."""
    if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise RuntimeError(f"expected uint8 HWC batch [B,H,W,3], got {tuple(u8.shape)} {u8.dtype}")
    b, h, w, _ = u8.shape
    aug = _aug_args(augment, params, geom, affine, radio, b, 3, h, w, u8.device)
    _require_gpu(u8.device)
    lib = _lib.load()
    u8 = u8.contiguous()
    out = torch.empty((b, 3, h, w), dtype=torch.float32, device=u8.device)
    params, noise = _plain_draws(params, noise, out.shape, u8.device)
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    if aug is None:
        check(lib.eae_augment(_stream(), _ptr(u8), _ptr(out), b, h, w, int(train), float(noise_std), seed, step, _ptr(params),
                              _ptr(noise)))
    else:
        pol, geom, affine, radio = aug
        check(lib.eae_augment_aug(_stream(), _ptr(u8), _ptr(out), b, h, w, int(train), float(noise_std), seed, step, pol, _ptr(geom),
                                  _ptr(affine), _ptr(radio), _ptr(noise)))
    return out


def stage_bands(data, divisor, index=None, train=True, noise_std=0.03, seed=0, step=0, params=None, noise=None, augment=None,
                geom=None, affine=None, radio=None):
    """fp32 NCHW [B,C,H,W] batch from a uint8 / uint16 dataset `data` [N,C,H,W] on the device: images `index` (int64 [B]; None =
    all N), flip -> pad-4 crop -> / divisor[c] -> + noise_std * N(0,1) (train=False: the division only).  Randomness: Philox
    keyed by (seed, step), or explicit `params` int32 [B,3] = (flip, top, left) and `noise` [B,C,H,W] (include/eae.h eae_stage_bands).
    ``augment``: an `Augment` policy; ``geom`` int32 [B,4] = (flip, top, left, rot), ``affine`` float32 [B,2] = (a, b), ``radio``
    float32 [B,C,2] = (gain, offset): explicit draws in place of the policy's (include/eae.h, "augmentation policy")."""
    if data.dtype not in (torch.uint8, torch.uint16) or data.dim() != 4:
        raise RuntimeError(f"expected a uint8 or uint16 dataset [N,C,H,W], got {tuple(data.shape)} {data.dtype}")
    n, c, h, w = data.shape
    b = n if index is None else torch.as_tensor(index).numel()
    aug = _aug_args(augment, params, geom, affine, radio, b, c, h, w, data.device)
    _require_gpu(data.device)
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
    out = torch.empty((b, c, h, w), dtype=torch.float32, device=data.device)
    params, noise = _plain_draws(params, noise, out.shape, data.device)
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    if aug is None:
        check(lib.eae_stage_bands(_stream(), _ptr(data), data.element_size(), n, c, h, w, _ptr(index), b, _ptr(div), _ptr(out), int(train),
                                  float(noise_std), seed, step, _ptr(params), _ptr(noise)))
    else:
        pol, geom, affine, radio = aug
        check(lib.eae_stage_bands_aug(_stream(), _ptr(data), data.element_size(), n, c, h, w, _ptr(index), b, _ptr(div), _ptr(out),
                                      int(train), float(noise_std), seed, step, pol, _ptr(geom), _ptr(affine), _ptr(radio),
                                      _ptr(noise)))
    return out
