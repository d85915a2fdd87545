"""Classify whole scenes: sliding-window latents and class maps from a planar raster [C,H,W] held on the device.

A model of size P x P (the encoder's ``image_size``) runs over windows placed at stride S on both axes; only whole windows are used
(`window_grid`).  The input value is ``(float)v / divisor[c]``, the eval-mode expression of `stage_bands`.  conv1 reads the scene
directly (no staged fp32 [B,C,P,P] batch), the MLP reads the engine's latent rows in place, and one C call covers the scene
(include/eae.h, "scene classification").  Everything runs in eval mode: BatchNorm with running statistics, no dropout.

- `scene_windows` gathers windows as the fp32 NCHW batch the encoder reads (bitwise `stage_bands(train=False)` on host-cut windows);
- `encode_scene` returns the latents z [nH*nW, L] (clustering, retrieval);
- `classify_scene` returns probabilities [K,nH,nW] and labels [nH,nW], or with ``blend=True`` (S divides P) the map of S x S cells,
  each the mean probability of the windows that cover it, [K,nH+k-1,nW+k-1] with k = P/S.

Nodata and masked windows.  Pixel (y, x) is invalid when it matches ``nodata`` (``rule="all"``, the default and rasterio's
dataset-mask convention: every band equals it; ``rule="any"``: at least one band does) or when ``mask[y, x] != 0`` (``mask``: a
[H, W] bool / uint8 tensor on the scene's device).  For uint8 / uint16 scenes ``nodata`` must be an integer in the dtype's range
(an integral float such as rasterio's 0.0 is accepted); for fp32 scenes ``float("nan")`` matches NaN and any other value matches by
``==`` after rounding to float32.  Window n is invalid when it holds more than t = floor(max_invalid * P * P) invalid pixels
(`invalid_threshold`; ``max_invalid`` in [0, 1), default 0: one invalid pixel excludes the window).  A valid window that holds some
invalid pixels (t > 0) is encoded with those pixels as stored: nothing is filled in.
- `window_invalid_counts` returns the invalid pixels of every window, `valid_windows` the ascending ids of the valid ones;
- `classify_scene(nodata=, mask=)` encodes only the valid windows: the others get label -1 and probability 0 for every class, and the
  blend averages each cell over its valid covering windows only (a cell with none: label -1, probabilities 0);
- ``windows=`` (`encode_scene`, `classify_scene`) runs the model over a device list of window ids instead of the whole grid.

Reconstruction (the decoder half: what the model cannot explain -- anomaly and change screening, quality control of a trained
encoder, choosing windows worth labelling).  The autoencoder runs encoder -> decoder over the windows and deconv4's epilogue reads its
MSE target from the scene itself, by the expression conv1 read it with: no [B,C,P,P] batch of windows or of x_hat is written.
- `scene_reconstruction_error` returns err [nH,nW], the mean of (x_hat - x)^2 over each window's C*P*P elements (``per_band=True``:
  also band_err [C,nH,nW]); windows that are not run (invalid under nodata / mask, or absent from ``windows=``) hold NaN;
- `reconstruct_scene` returns the stitched x_hat [C,Hg,Wg] over the grid's extent (`owned_span`: every pixel is written by the one
  window that owns it, the centre S x S of each window extended to the extent's edges, so nothing is accumulated and the windows'
  border artefacts are dropped), in the units of ``scene / divisor``; ``residual=True`` adds the per-pixel band mean of
  (x_hat - x)^2 [Hg,Wg].  Pixels owned by a window that is not run hold NaN.

Borders (``border="constant" | "edge" | "reflect"``, every function above): the grid is laid over a VIRTUAL padded scene that covers
the whole raster (`border_grid`: as many windows as it takes, the excess split around the scene with ``anchor="center"`` or put
behind it with ``anchor="origin"``), and a virtual pixel outside the scene is resolved when a kernel loads it (`border_source`): no
padded copy is made.  Every function returns bitwise what it returns with ``border=None`` on
``np.pad(scene, ((0,0),(pt,pb),(pl,pr)), mode)`` (``"constant"``: ``constant_values=fill``; ``"reflect"`` does not repeat the edge
pixel) with the mask padded alike (0 in constant mode): mirrored and replicated pixels are as valid as their source, constant ones
are invalid when ``fill`` matches ``nodata``; the error maps average over the window as the model saw it.  Window (i, j) starts at
scene pixel (i*S - pt, j*S - pl), so with ``anchor="origin"`` cell (ci, cj) of a blended map starts at pixel (ci*S, cj*S).  Window
and cell maps have the shapes of the virtual grid; `reconstruct_scene` returns the real scene, [C,H,W] and [H,W].  The scene may be
smaller than one patch.

Training from a scene (the loader side: the model is trained by `fit_autoencoder`, `fit_mlp` and their kin, which take any iterable of
(imgs, labels) with a ``batch_size``).  No patch dataset is cut -- with overlapping windows it would be (P/S)^2 times the scene -- and no
per-patch label is made on the host; no model runs, so P is any positive size; the grid is that of whole windows (no border).
- `window_labels` turns a label raster [H,W] (a land-cover map, rasterised polygons; values in [0,K) are classes, everything else is
  unlabelled) into the majority class of every window, with its purity and the window's labelled share;
- `stage_scene_windows` returns the augmented fp32 batch [B,C,P,P] of a list of window ids: `stage_bands`' transform and random
  stream, the windows gathered from the scene.  ``crop="window"`` is bitwise `stage_bands` on the materialised windows (the pad-4
  crop reads 0 outside the window); ``crop="scene"`` lets the crop slide the window over its real neighbourhood (0 only outside the
  scene), so no black frame appears;
- `SceneLoader` is the iterable over (x, y) batches of the labelled windows: epoch e orders the ids by
  ``torch.randperm(n, generator=torch.Generator().manual_seed(seed + e))`` (`window_schedule`) and batch i is
  ``stage_scene_windows(ids, seed=seed, step=e * len(loader) + i)``; nothing inside an epoch synchronises the host.

Accuracy assessment (how good is the map `classify_scene` returned?).  The class map is compared with the label raster pixel by pixel
on the device: the raster and an optional mask are read once, the map is looked up per cell, and no upsampled copy of the map is made.
- `scene_confusion` returns the int64 [K+1,K+1] confusion counts of a cell map against a label raster (row K: unlabelled truth,
  column K: not classified), exact and identical from run to run; `report.confusion_metrics` turns them into user's / producer's
  accuracy, IoU, kappa and the mapped area per class;
- `evaluate_scene` is `classify_scene` followed by `scene_confusion` with the map's cell size and origin;
- `block_split` cuts the window grid into blocks, gives some to validation and drops the training windows that share pixels with a
  validation window (overlapping windows make a random split of window ids leak); `footprint_mask` is the pixel footprint of a list
  of windows, the ``region=`` an honest validation figure is assessed over.

Clustering (no labels yet: the unsupervised map).  `cluster.cluster_scene` takes the window set as `classify_scene` does, encodes it
with `encode_scene` and runs k-means over the latents on the device (`cluster.kmeans_fit`), or applies given centroids to another
scene; windows that are not run hold -1 in the cluster map.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import NamedTuple

import torch

from . import _lib
from ._lib import check
from .engine import _ptr, _stream, _require_gpu, engine_for
from .augment import Augment, _aug_args, _plain_draws

_DTYPES = {torch.uint8: 0, torch.uint16: 1, torch.float32: 2}


# ---------------------------------------------------------------------------------------------------- grid arithmetic (pure Python)
def window_grid(height, width, patch, stride, any_patch=False):
    """(nH, nW): whole P x P windows at stride S in an H x W scene.  Window n = i*nW + j starts at pixel (i*S, j*S).  P is a
    multiple of 64, a model's image size; any_patch=True takes every positive P (the calls that run no model: `scene_windows`
    without a border, `stage_scene_windows`, `window_labels`, `SceneLoader`)."""
    height, width, patch, stride = int(height), int(width), int(patch), int(stride)
    if any_patch and patch <= 0:
        raise RuntimeError(f"the patch size must be positive, got {patch}")
    if not any_patch and (patch <= 0 or patch % 64):
        raise RuntimeError(f"the patch size must be a positive multiple of 64, got {patch}")
    if not 1 <= stride <= patch:
        raise RuntimeError(f"stride must be in 1..{patch} (the patch size), got {stride}")
    if height < patch or width < patch:
        raise RuntimeError(f"scene {height} x {width} is smaller than one {patch} x {patch} window")
    return (height - patch) // stride + 1, (width - patch) // stride + 1


_BORDERS = {None: 0, "constant": 1, "edge": 2, "reflect": 3}


def border_grid(height, width, patch, stride, anchor="center"):
    """(nH, nW, (pt, pb, pl, pr)): the grid that covers an H x W scene and the pads of its virtual scene.  Per axis
    n = max(0, ceil((len - P) / S)) + 1 windows span (n-1)*S + P pixels; the excess over len (< P) is split excess//2 in front and
    the rest behind (``anchor="center"``) or put behind (``anchor="origin"``: window (i, j) starts at pixel (i*S, j*S))."""
    height, width, patch, stride = int(height), int(width), int(patch), int(stride)
    if patch <= 0 or patch % 64:
        raise RuntimeError(f"the patch size must be a positive multiple of 64, got {patch}")
    if not 1 <= stride <= patch:
        raise RuntimeError(f"stride must be in 1..{patch} (the patch size), got {stride}")
    if height < 1 or width < 1:
        raise RuntimeError(f"scene {height} x {width} is empty")
    if anchor not in ("center", "origin"):
        raise RuntimeError(f"anchor must be 'center' or 'origin', got {anchor!r}")

    def axis(n_px):
        n = max(0, -((patch - n_px) // stride)) + 1          # -(-a // b) = ceil(a / b)
        excess = (n - 1) * stride + patch - n_px
        lead = excess // 2 if anchor == "center" else 0
        return n, lead, excess - lead

    n_h, pt, pb = axis(height)
    n_w, pl, pr = axis(width)
    return n_h, n_w, (pt, pb, pl, pr)


def border_source(v, pad, n, mode):
    """Source index on an axis of length n of virtual coordinate v behind a leading pad, as ``np.pad`` places it; None for a pixel
    of the constant fill.  s = v - pad inside [0, n) is the pixel itself; "edge" clamps s to [0, n-1]; "reflect" is -s for s < 0 and
    2(n-1) - s for s >= n (one reflection: the pads are at most n - 1)."""
    if mode not in ("constant", "edge", "reflect"):
        raise RuntimeError(f"border must be 'constant', 'edge' or 'reflect', got {mode!r}")
    v, pad, n = int(v), int(pad), int(n)
    s = v - pad
    if 0 <= s < n:
        return s
    if mode == "constant":
        return None
    if mode == "edge":
        return 0 if s < 0 else n - 1
    s = -s if s < 0 else 2 * (n - 1) - s
    if not 0 <= s < n:
        raise RuntimeError(f"coordinate {v} needs more than one reflection of an axis of length {n} behind a pad of {pad}")
    return s


def window_origin(n, n_w, stride):
    """Top-left pixel (y, x) of window n of a grid with n_w windows per row."""
    i, j = divmod(int(n), int(n_w))
    return i * int(stride), j * int(stride)


def owned_span(i, n, patch, stride):
    """(lo, hi): the pixels [lo, hi) of one axis of the grid's extent [0, (n-1)*S + P) that window i of n OWNS in a stitched raster.
    With m = (P - S) / 2 window i owns [i*S + m, i*S + m + S), extended to 0 for i = 0 and to the extent's end for i = n - 1: the
    spans of the n windows partition the extent.  P - S must be even."""
    i, n, patch, stride = int(i), int(n), int(patch), int(stride)
    if patch <= 0 or not 1 <= stride <= patch:
        raise RuntimeError(f"stride must be in 1..{patch} (the patch size), got {stride}")
    if (patch - stride) % 2:
        raise RuntimeError(f"a stitched raster needs an even patch - stride (centred owned spans), got {patch} - {stride}")
    if n < 1 or not 0 <= i < n:
        raise RuntimeError(f"window {i} is outside 0..{n - 1}")
    m = (patch - stride) // 2
    lo = 0 if i == 0 else i * stride + m
    hi = (n - 1) * stride + patch if i == n - 1 else i * stride + m + stride
    return lo, hi


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


def invalid_threshold(patch, max_invalid):
    """t = floor(max_invalid * P * P): a window with more than t invalid pixels is excluded (max_invalid in [0, 1))."""
    patch = int(patch)
    if patch <= 0:
        raise RuntimeError(f"the patch size must be positive, got {patch}")
    if isinstance(max_invalid, bool) or not isinstance(max_invalid, numbers.Real):
        raise RuntimeError(f"max_invalid must be a number in [0, 1), got {max_invalid!r}")
    m = float(max_invalid)
    if not 0.0 <= m < 1.0:                              # also rejects NaN
        raise RuntimeError(f"max_invalid must be in [0, 1), got {max_invalid}")
    return math.floor(m * patch * patch)


def valid_coverage(valid, k):
    """Number of valid windows covering each S x S cell: ``valid`` is a boolean [nH, nW] window-validity map, k = P/S; the result is
    a [nH+k-1, nW+k-1] int64 CPU tensor (`cell_coverage` when every window is valid).  The blend divides by this count."""
    if not isinstance(valid, torch.Tensor) or valid.dim() != 2 or valid.dtype != torch.bool:
        raise RuntimeError("valid must be a boolean [nH, nW] tensor")
    k = int(k)
    if k < 1:
        raise RuntimeError(f"k must be positive, got {k}")
    v = valid.cpu().to(torch.int64)
    n_h, n_w = v.shape
    if n_h < 1 or n_w < 1:
        raise RuntimeError("valid must hold at least one window")
    # box sums of k x k windows of the zero-padded map: cell (ci, cj) is covered by windows [ci-k+1, ci] x [cj-k+1, cj]
    pad = torch.zeros((n_h + 2 * (k - 1), n_w + 2 * (k - 1)), dtype=torch.int64)
    pad[k - 1:k - 1 + n_h, k - 1:k - 1 + n_w] = v
    ii = pad.cumsum(0).cumsum(1)
    ii = torch.nn.functional.pad(ii, (1, 0, 1, 0))
    c_h, c_w = n_h + k - 1, n_w + k - 1
    return ii[k:k + c_h, k:k + c_w] - ii[0:c_h, k:k + c_w] - ii[k:k + c_h, 0:c_w] + ii[0:c_h, 0:c_w]


_RULES = {"all": 0, "any": 1}
_NODATA_NONE, _NODATA_VALUE, _NODATA_NAN = 0, 1, 2
_INT_RANGE = {torch.uint8: 255, torch.uint16: 65535}


# ---------------------------------------------------------------------------------------------------- argument checks
def _nodata_arg(dtype, nodata):
    """(mode, value) of the C call for a nodata value of a scene of this dtype."""
    if nodata is None:
        return _NODATA_NONE, 0.0
    if isinstance(nodata, bool) or not isinstance(nodata, numbers.Real):
        raise RuntimeError(f"nodata must be a number, got {nodata!r}")
    if dtype in _INT_RANGE:
        v = float(nodata)
        if math.isnan(v) or not v.is_integer() or not 0 <= v <= _INT_RANGE[dtype]:
            raise RuntimeError(f"nodata of a {str(dtype).replace('torch.', '')} scene must be an integer in 0..{_INT_RANGE[dtype]}, "
                               f"got {nodata!r}")
        return _NODATA_VALUE, v
    v = float(nodata)
    return (_NODATA_NAN, 0.0) if math.isnan(v) else (_NODATA_VALUE, v)


def _mask_arg(scene, mask):
    """The mask as a contiguous uint8 [H, W] tensor on the scene's device (bool is viewed, not copied), or None."""
    if mask is None:
        return None
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2 or tuple(mask.shape) != tuple(scene.shape[1:]):
        raise RuntimeError(f"mask must be a [H, W] = {list(scene.shape[1:])} tensor")
    if mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"mask dtype must be bool or uint8, got {mask.dtype}")
    if mask.device != scene.device:
        raise RuntimeError(f"mask is on {mask.device}, the scene on {scene.device}")
    mask = mask.contiguous()
    return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def _rule_arg(rule):
    if rule not in _RULES:
        raise RuntimeError(f"rule must be 'all' or 'any', got {rule!r}")
    return _RULES[rule]


def _border_arg(scene, patch, stride, border, fill, anchor, any_patch=False):
    """(mode id, fill, nH, nW, pads) for a scene that has passed `_check_scene`: the grid of whole windows for border=None (any_patch:
    `window_grid`), else `border_grid` and the checks of the mode."""
    h, w = int(scene.shape[1]), int(scene.shape[2])
    if border not in _BORDERS:
        raise RuntimeError(f"border must be None, 'constant', 'edge' or 'reflect', got {border!r}")
    if anchor not in ("center", "origin"):
        raise RuntimeError(f"anchor must be 'center' or 'origin', got {anchor!r}")
    if isinstance(fill, bool) or not isinstance(fill, numbers.Real):
        raise RuntimeError(f"fill must be a number, got {fill!r}")
    fill = float(fill)
    if border != "constant":
        if fill != 0.0:
            raise RuntimeError(f"fill is the value of border='constant' pixels; got fill={fill!r} with border={border!r}")
        if border is None:
            return (0, 0.0) + window_grid(h, w, patch, stride, any_patch) + ((0, 0, 0, 0),)
    elif scene.dtype in _INT_RANGE and (math.isnan(fill) or not fill.is_integer() or not 0 <= fill <= _INT_RANGE[scene.dtype]):
        raise RuntimeError(f"fill of a {str(scene.dtype).replace('torch.', '')} scene must be an integer in "
                           f"0..{_INT_RANGE[scene.dtype]}, got {fill!r}")
    n_h, n_w, pads = border_grid(h, w, patch, stride, anchor)
    if border == "reflect" and (max(pads[:2]) > h - 1 or max(pads[2:]) > w - 1):
        raise RuntimeError(f"border='reflect' mirrors once: the pads {pads} (top, bottom, left, right) must stay below the scene's "
                           f"{h} x {w}")
    return _BORDERS[border], fill, n_h, n_w, pads


def _check_scene(scene):
    """The one check of the scene tensor's rank and dtype."""
    if not isinstance(scene, torch.Tensor) or scene.dim() != 3:
        raise RuntimeError("scene must be a planar tensor [C,H,W]")
    if scene.dtype not in _DTYPES:
        raise RuntimeError(f"scene dtype must be uint8, uint16 or float32, got {scene.dtype}")


def _invalid_args(scene, nodata, mask, rule):
    """Validate nodata / mask / rule against the scene: (mode, value, rule id, uint8 mask or None)."""
    rid = _rule_arg(rule)
    _check_scene(scene)
    mode, value = _nodata_arg(scene.dtype, nodata)
    return mode, value, rid, _mask_arg(scene, mask)


def _windows_arg(windows, device, n_windows, allow_empty, check_range=True):
    """Validate a window-id list: 1-D int64 on the scene's device, ids in [0, nH*nW) (one aminmax readback; check_range=False
    leaves the ids unread)."""
    if not isinstance(windows, torch.Tensor) or windows.dim() != 1 or windows.dtype != torch.int64:
        raise RuntimeError("windows must be a 1-D int64 tensor of window ids")
    if windows.device != device:
        raise RuntimeError(f"windows is on {windows.device}, the scene on {device}")
    if windows.numel() == 0:
        if not allow_empty:
            raise RuntimeError("windows is empty")
        return windows
    if not check_range:
        return windows.contiguous()
    lo, hi = (int(v) for v in torch.aminmax(windows))
    if lo < 0 or hi >= n_windows:
        raise RuntimeError(f"window ids {lo}..{hi} are outside the grid of {n_windows}")
    return windows.contiguous()


def _encoder_of(encoder):
    from .modules import Encoder, SupervisedAutoencoder
    if isinstance(encoder, SupervisedAutoencoder):
        return encoder.enc
    if isinstance(encoder, Encoder):
        return encoder
    raise RuntimeError(f"encoder must be an Encoder or a SupervisedAutoencoder, got {type(encoder).__name__}")


class _Host(NamedTuple):
    """A scene call as the host checks leave it, before anything touches a device.  `_geometry` fills the first nine fields (what
    `_desc` makes a descriptor from); `_host_plan` adds the rest for the functions that run a model."""
    scene: torch.Tensor
    div: torch.Tensor            # fp32 [C], wherever the caller's divisor was
    patch: int
    stride: int
    n_h: int
    n_w: int
    border: int                  # mode id
    fill: float
    pads: tuple
    enc: object = None
    batch: int = 0
    nodata: tuple = (0, 0.0)     # (mode, value) of the C call
    rule: int = 0
    mask: object = None          # uint8 [H, W] or None
    t: int = 0                   # `invalid_threshold`
    windows: object = None       # the caller's ids (type, dtype, device and emptiness checked; their range is not: it needs a readback)

    @property
    def masked(self):
        return self.nodata[0] != _NODATA_NONE or self.mask is not None

    @property
    def n_max(self):
        """Upper bound on the number of windows to run: exact unless `masked`, where the valid windows are counted on the device."""
        return self.n_h * self.n_w if self.windows is None else int(self.windows.numel())

    def scatter(self, ids, rows, fill, channels_first=False, flat=False):
        """Per-window rows [n_run] or [n_run, F] of the run windows (ids; None: the whole grid, in order) as a map over the grid:
        [nH, nW] or [nH, nW, F], `fill` where no window ran.  channels_first: [F, nH, nW]; flat: the grid as one axis of nH * nW."""
        if ids is None:
            out = rows.clone()
        else:
            out = torch.full((self.n_h * self.n_w,) + rows.shape[1:], fill, dtype=rows.dtype, device=rows.device)
            out[ids] = rows
        if not flat:
            out = out.reshape((self.n_h, self.n_w) + rows.shape[1:])
        return out.movedim(-1, 0).contiguous() if channels_first else out


def _geometry(scene, divisor, patch, stride, border=None, fill=0, anchor="center", any_patch=False):
    """Every host-side check of a scene that has passed `_check_scene`: the grid (of the virtual scene under a border), the border
    arguments, the band count and the divisor.  No device is touched."""
    c = int(scene.shape[0])
    mode, fill, n_h, n_w, pads = _border_arg(scene, patch, stride, border, fill, anchor, any_patch)
    if not 1 <= c <= 16:
        raise RuntimeError(f"scene: in_channels must be in 1..16, got {c}")
    div = torch.as_tensor(divisor, dtype=torch.float32).reshape(-1)
    if div.numel() == 1:
        div = div.expand(c)
    if div.numel() != c:
        raise RuntimeError(f"divisor must have one value per band ({c}), got {div.numel()}")
    return _Host(scene, div, int(patch), int(stride), n_h, n_w, mode, fill, pads)


def _desc(g):
    """(EaeScene, keep-alive tensors) of a `_Host`: the first step that needs the device."""
    _require_gpu(g.scene.device)
    div = g.div.to(g.scene.device).contiguous()
    scene = g.scene.contiguous()
    c, h, w = (int(v) for v in scene.shape)
    desc = _lib.EaeScene(C.c_void_p(scene.data_ptr()), C.c_void_p(div.data_ptr()), _DTYPES[scene.dtype], c, h, w, g.patch, g.stride,
                         g.border, *g.pads, g.fill)
    return desc, (scene, div)


def _scene_desc(scene, divisor, patch, stride, border=None, fill=0, anchor="center", any_patch=False):
    """(EaeScene, keep-alive tensors, nH, nW) for the functions that run no model: `_geometry`, then `_desc`."""
    g = _geometry(scene, divisor, patch, stride, border, fill, anchor, any_patch)
    return _desc(g) + (g.n_h, g.n_w)


def _invalid_counts(desc, keep, n_h, n_w, mode, value, rule, mask):
    lib = _lib.load()
    dev = keep[0].device
    rows = torch.empty(((n_h - 1) * desc.stride + desc.patch, n_w), dtype=torch.int32, device=dev)
    counts = torch.empty((n_h, n_w), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(lib.eae_scene_invalid_counts(_stream(), C.byref(desc), mode, value, rule, _ptr(mask), _ptr(rows), _ptr(counts)))
    return counts


def _select(counts, t):
    lib = _lib.load()
    n = counts.numel()
    ids = torch.empty(n, dtype=torch.int64, device=counts.device)
    cnt = torch.empty(1, dtype=torch.int64, device=counts.device)
    with torch.cuda.device(counts.device):
        check(lib.eae_scene_select(_stream(), _ptr(counts), n, int(t), _ptr(ids), _ptr(cnt)))
    return ids[:int(cnt.item())]


def _range(first, count, total):
    first = int(first)
    count = total - first if count is None else int(count)
    if first < 0 or count <= 0 or first + count > total:
        raise RuntimeError(f"windows {first}..{first + count - 1} are outside the grid of {total}")
    return first, count


# ---------------------------------------------------------------------------------------------------- public functions
def scene_windows(scene, divisor, patch, stride, first=0, count=None, border=None, fill=0, anchor="center"):
    """fp32 NCHW [count,C,P,P] of windows first .. first+count-1 (count=None: to the end of the grid).  border / fill / anchor:
    module docstring, "Borders".  No model runs: without a border P is any positive size."""
    _check_scene(scene)
    g = _geometry(scene, divisor, patch, stride, border, fill, anchor, any_patch=True)
    first, count = _range(first, count, g.n_h * g.n_w)
    desc, keep = _desc(g)
    lib = _lib.load()
    out = torch.empty((count, keep[0].shape[0], int(patch), int(patch)), dtype=torch.float32, device=keep[0].device)
    with torch.cuda.device(keep[0].device):
        check(lib.eae_scene_windows(_stream(), C.byref(desc), first, count, _ptr(out)))
    return out


def window_invalid_counts(scene, patch, stride, nodata=None, mask=None, rule="all", border=None, fill=0, anchor="center"):
    """Invalid pixels of every P x P window at stride S: int32 [nH, nW] on the scene's device (see the module docstring for what
    makes a pixel invalid).  Every scene element and mask byte inside the grid's extent is read once (under a border: once per
    virtual pixel that resolves to it)."""
    mode, value, rid, m = _invalid_args(scene, nodata, mask, rule)
    desc, keep, n_h, n_w = _scene_desc(scene, 1.0, patch, stride, border, fill, anchor)
    return _invalid_counts(desc, keep + (m,), n_h, n_w, mode, value, rid, m)


def valid_windows(scene, patch, stride, nodata=None, mask=None, max_invalid=0.0, rule="all", border=None, fill=0, anchor="center"):
    """Ascending int64 ids (on the scene's device) of the windows with at most floor(max_invalid * P * P) invalid pixels.
    The number of valid windows is read back once (``.item()``) to size the result: this is the one host synchronisation of the
    nodata / mask path."""
    t = invalid_threshold(patch, max_invalid)
    counts = window_invalid_counts(scene, patch, stride, nodata=nodata, mask=mask, rule=rule, border=border, fill=fill, anchor=anchor)
    return _select(counts, t)


def _prepare(enc, batch):
    """The engine of the encoder: bf16 only, parameters re-read."""
    eng = engine_for(enc, max_batch=batch)
    if eng.quant != 0:
        raise RuntimeError("scene classification supports bf16 engines only (quant=1 / fp8 is not supported)")
    eng.params_changed()
    return eng


class _Plan(NamedTuple):
    """What a model-running scene function works from on the device (`_device_plan`).  windows: None = every window of the grid (the
    range entry points of the C library, no id list), else the int64 ids of the windows to run (the index-driven ones; may be empty)."""
    eng: object
    desc: object
    keep: tuple
    n_h: int
    n_w: int
    patch: int
    stride: int
    windows: object

    def out(self, shape, fill, dtype=torch.float32):
        """An output over the grid: every element is written when the whole grid runs, a subset leaves `fill` elsewhere."""
        if self.windows is None:
            return torch.empty(shape, dtype=dtype, device=self.eng.device)
        return torch.full(shape, fill, dtype=dtype, device=self.eng.device)

    def run(self, range_fn, index_fn, *outs, head=()):
        """The one C call over the window set, writing `outs`: the range entry point for the whole grid, the index-driven one for a
        list of ids, none for an empty list (the forward generation stays put).  head: arguments between the context and the stream."""
        eng, w = self.eng, self.windows
        with torch.cuda.device(eng.device):
            if w is None:
                check(range_fn(eng.ctx, *head, _stream(), C.byref(self.desc), 0, self.n_h * self.n_w, *map(_ptr, outs)))
            elif w.numel():
                check(index_fn(eng.ctx, *head, _stream(), C.byref(self.desc), _ptr(w), w.numel(), *map(_ptr, outs)))


def _host_plan(scene, encoder, divisor, stride, batch, nodata=None, mask=None, max_invalid=0.0, rule="all", windows=None,
               allow_empty=True, blend=False, stitched=False, border=None, fill=0, anchor="center", mlp=...):
    """Every model-running scene function starts here: all the validation that needs no device, as a `_Host`.  Neither the library nor
    an engine is loaded, so a bad argument is reported by its own message on any machine.  mlp: the classifier that reads the
    latents, where there is one."""
    if mlp is not ...:
        from .modules import MLP
        if not isinstance(mlp, MLP):
            raise RuntimeError(f"mlp must be an MLP, got {type(mlp).__name__}")
        if int(mlp.input_dim) != int(_encoder_of(encoder).latent_dim):
            raise RuntimeError(f"the MLP takes input_dim={mlp.input_dim}, the encoder's latent_dim is {_encoder_of(encoder).latent_dim}")
    rid = _rule_arg(rule)
    enc = _encoder_of(encoder)
    patch = int(enc.image_size)
    t = invalid_threshold(patch, max_invalid)
    if windows is not None and (nodata is not None or mask is not None):
        raise RuntimeError("windows= cannot be combined with nodata= or mask=")
    _check_scene(scene)
    g = _geometry(scene, divisor, patch, patch if stride is None else int(stride), border, fill, anchor)
    if blend:
        cell_grid(g.n_h, g.n_w, patch, g.stride)         # the stride must divide the patch size
    if stitched:
        owned_span(0, g.n_h, patch, g.stride)            # patch - stride must be even
    nd = _nodata_arg(scene.dtype, nodata)
    m = _mask_arg(scene, mask)
    if windows is not None:
        windows = _windows_arg(windows, scene.device, g.n_h * g.n_w, allow_empty, check_range=False)
    if scene.shape[0] != int(enc.in_channels):
        raise RuntimeError(f"scene has {scene.shape[0]} bands, the encoder takes in_channels={enc.in_channels}")
    if int(batch) < 1:
        raise RuntimeError(f"batch must be positive, got {batch}")
    if next(enc.parameters()).device != scene.device:
        raise RuntimeError("the scene and the model must be on the same device")
    return g._replace(enc=enc, batch=int(batch), nodata=nd, rule=rid, mask=m, t=t, windows=windows)


def _device_plan(h):
    """The device half of a model-running function, from its `_Host`: `_require_gpu` and the descriptor (`_desc`), the range of the
    caller's window ids (one aminmax readback), the engine (`_prepare`), and under nodata / mask the valid ids (`_select`: the one
    ``.item()``; ids it produced are not read back again)."""
    desc, keep = _desc(h)
    windows = h.windows
    if windows is not None:
        windows = _windows_arg(windows, h.scene.device, h.n_h * h.n_w, allow_empty=True, check_range=True)
    eng = _prepare(h.enc, h.batch)
    if h.masked:
        windows = _select(_invalid_counts(desc, keep + (h.mask,), h.n_h, h.n_w, *h.nodata, h.rule, h.mask), h.t)
    return _Plan(eng, desc, keep, h.n_h, h.n_w, h.patch, h.stride, windows)


def _scene_latents(h, admit=None):
    """(ids, z): the window set of a `_Host` -- None for the whole grid, else the int64 ids run, the caller's or under nodata / mask
    the valid ones -- and its latents z [n_run, L], row by row in that order.  One descriptor, one select, one index-driven encode.
    admit(n_run) is called once the number is known and before the encoder runs (default: at least one window)."""
    p = _device_plan(h)
    n = p.n_h * p.n_w if p.windows is None else p.windows.numel()
    if admit is not None:
        admit(n)
    elif n == 0:
        raise RuntimeError("no valid window")
    z = torch.empty((n, p.eng.latent), dtype=torch.float32, device=p.eng.device)
    p.run(p.eng.lib.eae_scene_encode, p.eng.lib.eae_scene_encode_windows, z)
    return p.windows, z


def encode_scene(scene, encoder, divisor=1.0, stride=None, batch=512, windows=None, border=None, fill=0, anchor="center"):
    """Latents z [nH*nW, L] of every window (row n = window i*nW + j), eval-mode encoder, `batch` windows per encoder pass (the
    engine's max_batch, at least this).  stride=None: the patch size (non-overlapping windows).
    windows: a non-empty 1-D int64 device tensor of window ids (any order, duplicates allowed): z [len(windows), L] in that order.
    border / fill / anchor: module docstring, "Borders" (the grid is then `border_grid`'s)."""
    return _scene_latents(_host_plan(scene, encoder, divisor, stride, batch, windows=windows, allow_empty=False, border=border,
                                     fill=fill, anchor=anchor))[1]


def classify_scene(scene, encoder, mlp, divisor=1.0, stride=None, batch=512, blend=False, nodata=None, mask=None, max_invalid=0.0,
                   rule="all", windows=None, border=None, fill=0, anchor="center"):
    """(probs [K,nH,nW] float32 softmax, labels [nH,nW] int64 argmax) of every window: encoder -> MLP in eval mode, one C call.
    blend=True (stride divides the patch size, k = P/S): the map of S x S cells instead, probs [K,nH+k-1,nW+k-1] = mean over the
    windows covering each cell, labels = argmax of that map.

    nodata / mask / max_invalid / rule (module docstring): only the valid windows are encoded (`valid_windows`, one host readback);
    windows: a 1-D int64 device tensor of window ids, the only windows classified (not combined with nodata / mask).  Either way the
    other windows get label -1 and probability 0, and blend=True averages each cell over its classified windows only (no such
    window: label -1, probabilities 0).  Without a valid window nothing is launched.  With all of them None the plain path runs.

    border / fill / anchor (module docstring, "Borders"): the grid covers the whole scene (`border_grid`), so every pixel lies in a
    window and, with blend=True, in a cell of the virtual grid's cell map."""
    return _classify(_host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, blend=blend,
                                border=border, fill=fill, anchor=anchor, mlp=mlp), mlp, blend)


def _classify(h, mlp, blend):
    """`classify_scene` from its `_Host`."""
    from .mlp_engine import mlp_engine_for
    p = _device_plan(h)
    eng, n_h, n_w = p.eng, p.n_h, p.n_w
    if next(mlp.parameters()).device != eng.device:
        raise RuntimeError("the MLP and the encoder must be on the same device")
    meng = mlp_engine_for(mlp)
    k_cls = int(mlp.num_classes)
    probs = p.out((k_cls, n_h, n_w), 0.0)
    labels = p.out((n_h, n_w), -1, torch.int64)
    p.run(eng.lib.eae_scene_classify, eng.lib.eae_scene_classify_windows, probs, labels, head=(meng.ctx,))
    if not blend:
        return probs, labels
    c_h, c_w, k = cell_grid(n_h, n_w, p.patch, p.stride)
    cprobs = torch.empty((k_cls, c_h, c_w), dtype=torch.float32, device=eng.device)
    clabels = torch.empty((c_h, c_w), dtype=torch.int64, device=eng.device)
    with torch.cuda.device(eng.device):
        if p.windows is None:
            check(eng.lib.eae_scene_blend(_stream(), _ptr(probs), k_cls, n_h, n_w, k, _ptr(cprobs), _ptr(clabels)))
        else:
            check(eng.lib.eae_scene_blend_valid(_stream(), _ptr(probs), _ptr(labels), k_cls, n_h, n_w, k, _ptr(cprobs), _ptr(clabels)))
    return cprobs, clabels


# ---------------------------------------------------------------------------------------------------- reconstruction
def _autoencoder_arg(autoencoder):
    from .modules import SupervisedAutoencoder
    if not isinstance(autoencoder, SupervisedAutoencoder):
        raise RuntimeError(f"autoencoder must be a SupervisedAutoencoder (the decoder is needed), got {type(autoencoder).__name__}")


def scene_reconstruction_error(scene, autoencoder, divisor=1.0, stride=None, batch=512, per_band=False, nodata=None, mask=None,
                               max_invalid=0.0, rule="all", windows=None, border=None, fill=0, anchor="center"):
    """err [nH,nW] float32: the mean of (x_hat - x)^2 over the C*P*P elements of every window, x = scene / divisor as the encoder
    read it, x_hat = the eval-mode autoencoder's reconstruction of the window; one C call, no staged batch (module docstring).
    per_band=True: (err, band_err [C,nH,nW]), the mean over each band.  The sums are deterministic and do not depend on ``batch``.

    nodata / mask / max_invalid / rule: only the valid windows are run (`valid_windows`, one host readback); windows: a 1-D int64
    device tensor of window ids, the only windows run (not combined with nodata / mask).  Either way the other windows hold NaN;
    without a window to run nothing is launched.  A valid window that holds some invalid pixels is scored with them as stored.
    border / fill / anchor (module docstring, "Borders"): the mean runs over the window as the model saw it, padded pixels included."""
    _autoencoder_arg(autoencoder)
    p = _device_plan(_host_plan(scene, autoencoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, border=border,
                                fill=fill, anchor=anchor))
    err = p.out((p.n_h, p.n_w), float("nan"))
    band = p.out((p.desc.C, p.n_h, p.n_w), float("nan")) if per_band else None
    p.run(p.eng.lib.eae_scene_recon_error, p.eng.lib.eae_scene_recon_error_windows, err, band)
    return (err, band) if per_band else err


def reconstruct_scene(scene, autoencoder, divisor=1.0, stride=None, batch=512, residual=False, nodata=None, mask=None,
                      max_invalid=0.0, rule="all", windows=None, border=None, fill=0, anchor="center"):
    """recon [C,Hg,Wg] float32 over the grid's extent (Hg = (nH-1)*S + P): the eval-mode autoencoder's x_hat of every window, each
    pixel taken from the one window that owns it (`owned_span`; patch - stride must be even), in the units of ``scene / divisor``.
    residual=True: (recon, residual [Hg,Wg]), the mean over the bands of (x_hat - x)^2 of each pixel.

    nodata / mask / max_invalid / rule / windows as for `scene_reconstruction_error`: pixels owned by a window that is not run hold
    NaN (in both outputs).

    border / fill / anchor (module docstring, "Borders"): recon [C,H,W] and residual [H,W] of the REAL scene.  The owned spans are
    those of the virtual grid, which covers the scene, so every pixel has an owner; a window stores the real pixels of its span."""
    _autoencoder_arg(autoencoder)
    p = _device_plan(_host_plan(scene, autoencoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, stitched=True,
                                border=border, fill=fill, anchor=anchor))
    h_g, w_g = (p.n_h - 1) * p.stride + p.patch, (p.n_w - 1) * p.stride + p.patch
    if border is not None:
        h_g, w_g = p.desc.H, p.desc.W
    recon = p.out((p.desc.C, h_g, w_g), float("nan"))
    res = p.out((h_g, w_g), float("nan")) if residual else None
    fn = p.eng.lib.eae_scene_reconstruct                 # one entry point: windows = NULL is the whole grid
    p.run(lambda ctx, st, desc, first, n, *outs: fn(ctx, st, desc, None, n, *outs), fn, recon, res)
    return (recon, res) if residual else recon


# ---------------------------------------------------------------------------------------------------- training from a scene
_CROPS = {"window": 0, "scene": 1}
_MAX_LABEL_PATCH = 4080


def _crop_arg(crop):
    if crop not in _CROPS:
        raise RuntimeError(f"crop must be 'window' or 'scene', got {crop!r}")
    return _CROPS[crop]


def stage_scene_windows(scene, divisor, patch, stride, windows, train=True, noise_std=0.03, seed=0, step=0, params=None, noise=None,
                        crop="window", augment=None, geom=None, affine=None, radio=None):
    """fp32 NCHW [B,C,P,P]: `stage_bands`' transform of the windows ``windows`` (1-D int64 ids on the scene's device, any order,
    duplicates allowed) of the grid of whole P x P windows at stride S: flip -> pad-4 crop -> / divisor[c] -> + noise_std * N(0,1)
    (train=False: the division only, bitwise `scene_windows`).  Randomness as `stage_bands`: Philox keyed by (seed, step), the same
    stream, or explicit ``params`` int32 [B,3] = (flip, top, left) and ``noise`` [B,C,P,P].
    crop="window": outside the window the crop reads 0 -- bitwise `stage_bands` on the materialised windows; crop="scene": it reads
    the scene's own pixels around the window (0 outside the scene).  The ids are not read on the host (no synchronisation): an id
    outside the grid gives a NaN image, as an index outside the dataset does in `stage_bands`.
    ``augment``: an `Augment` policy (quarter turns, a small rotation and scale, per-band gain and offset); with crop="scene" a turned
    window reads its real neighbours.  ``geom`` int32 [B,4] = (flip, top, left, rot), ``affine`` float32 [B,2] = (a, b), ``radio``
    float32 [B,C,2] = (gain, offset): explicit draws in place of the policy's (include/eae.h, "augmentation policy")."""
    cid = _crop_arg(crop)
    _check_scene(scene)
    windows = _windows_arg(windows, scene.device, 0, allow_empty=False, check_range=False)
    b, c, p = windows.numel(), int(scene.shape[0]), int(patch)
    aug = _aug_args(augment, params, geom, affine, radio, b, c, p, p, scene.device)
    params, noise = _plain_draws(params, noise, (b, c, p, p), scene.device)
    desc, keep, _, _ = _scene_desc(scene, divisor, patch, stride, any_patch=True)        # grid, device, bands, divisor
    return _stage_windows(desc, keep, windows, train, noise_std, seed, step, params, noise, cid, aug)


def _stage_windows(desc, keep, windows, train, noise_std, seed, step, params, noise, cid, aug=None):
    """The C call of `stage_scene_windows` on a validated scene descriptor (`_scene_desc`) and id list: what a `SceneLoader` runs
    per batch.  aug: None (the plain call) or `_aug_args`' (policy, geom, affine, radio)."""
    dev, b = keep[0].device, windows.numel()
    lib = _lib.load()
    out = torch.empty((b, desc.C, desc.patch, desc.patch), dtype=torch.float32, device=dev)
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    with torch.cuda.device(dev):
        if aug is None:
            check(lib.eae_scene_stage_windows(_stream(), C.byref(desc), _ptr(windows), b, _ptr(out), int(bool(train)), float(noise_std),
                                              seed, step, _ptr(params), _ptr(noise), cid))
        else:
            pol, geom, affine, radio = aug
            check(lib.eae_scene_stage_windows_aug(_stream(), C.byref(desc), _ptr(windows), b, _ptr(out), int(bool(train)),
                                                  float(noise_std), seed, step, pol, _ptr(geom), _ptr(affine), _ptr(radio),
                                                  _ptr(noise), cid))
    return out


def _ignore_arg(ignore, k):
    """The classes of [0, k) that ``ignore`` (None, one integer or a list of them) declares unlabelled, ascending; any other value
    is unlabelled already."""
    if ignore is None:
        ignore = []
    elif isinstance(ignore, numbers.Integral) and not isinstance(ignore, bool):
        ignore = [int(ignore)]
    else:
        ignore = list(ignore)
        if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in ignore):
            raise RuntimeError(f"ignore must be an integer or a list of integers, got {ignore!r}")
    return sorted({int(v) for v in ignore if 0 <= int(v) < k})


def _label_raster(raster, k, ignore):
    """An integer label raster as the kernels read it: contiguous uint8 or int32 (other dtypes converted to int32, values outside
    [0, k) becoming -1), the `_ignore_arg` classes replaced by an unlabelled value."""
    if raster.dtype not in (torch.uint8, torch.int32):
        wide = raster.to(torch.int64)
        raster = torch.where((wide >= 0) & (wide < k), wide, -1).to(torch.int32)
    if ignore:
        hit = raster == ignore[0]
        for v in ignore[1:]:
            hit = hit | (raster == v)
        raster = raster.masked_fill(hit, 255 if raster.dtype == torch.uint8 else -1)          # K <= 64: 255 is never a class
    return raster.contiguous()


def window_labels(raster, patch, stride, num_classes, ignore=None):
    """(label int64 [nH,nW], purity float32 [nH,nW], labelled float32 [nH,nW]) of every whole P x P window at stride S over a label
    raster [H,W] on the device (any integer dtype; uint8 and int32 are read as they are, the others converted to int32).  A pixel is
    labelled when its value is in [0, num_classes), num_classes in 1..64; every other value (255, negatives, >= K) is unlabelled, and
    so are the values of ``ignore`` (one value or a list).  label = the class with the most labelled pixels (the lowest on a tie), -1
    for a window without a labelled pixel; purity = that class's pixels / P^2; labelled = labelled pixels / P^2.  Exact integer
    counts underneath: identical from run to run."""
    k = int(num_classes)
    if not 1 <= k <= 64:
        raise RuntimeError(f"num_classes must be in 1..64, got {num_classes}")
    if not isinstance(raster, torch.Tensor) or raster.dim() != 2:
        raise RuntimeError("raster must be a [H, W] tensor of class ids")
    if raster.dtype.is_floating_point or raster.dtype.is_complex or raster.dtype == torch.bool:
        raise RuntimeError(f"raster must have an integer dtype, got {raster.dtype}")
    patch, stride = int(patch), int(stride)
    if patch > _MAX_LABEL_PATCH:
        raise RuntimeError(f"the patch size must be at most {_MAX_LABEL_PATCH}, got {patch}")
    h, w = (int(v) for v in raster.shape)
    n_h, n_w = window_grid(h, w, patch, stride, any_patch=True)
    ignore = _ignore_arg(ignore, k)
    _require_gpu(raster.device)
    raster = _label_raster(raster, k, ignore)
    dev = raster.device
    label = torch.empty((n_h, n_w), dtype=torch.int64, device=dev)
    count = torch.empty((n_h, n_w), dtype=torch.int32, device=dev)
    labelled = torch.empty((n_h, n_w), dtype=torch.int32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        check(lib.eae_scene_window_labels(_stream(), _ptr(raster), raster.element_size(), h, w, patch, stride, k, _ptr(label),
                                          _ptr(count), _ptr(labelled)))
    pp = float(patch * patch)
    return label, count.to(torch.float32) / pp, labelled.to(torch.float32) / pp


def window_schedule(n, batch_size, epoch, seed=0, shuffle=True, drop_last=False):
    """The batches of one epoch over n drawable windows, as a list of 1-D int64 CPU tensors of POSITIONS in 0..n-1 (pure host
    arithmetic).  shuffle: the order is ``torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch))``, else ascending;
    consecutive runs of batch_size, the short last one dropped with drop_last."""
    n, batch_size, epoch = int(n), int(batch_size), int(epoch)
    if n < 1:
        raise RuntimeError(f"no window to draw from (n = {n})")
    if batch_size < 1:
        raise RuntimeError(f"batch_size must be positive, got {batch_size}")
    if epoch < 0:
        raise RuntimeError(f"epoch must not be negative, got {epoch}")
    order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed) + epoch)) if shuffle else torch.arange(n)
    stop = n - n % batch_size if drop_last else n
    return [order[i:min(i + batch_size, stop)] for i in range(0, stop, batch_size)]


def schedule_len(n, batch_size, drop_last=False):
    """Number of batches `window_schedule` yields."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise RuntimeError(f"batch_size must be positive, got {batch_size}")
    return n // batch_size if drop_last else -(-n // batch_size)


def class_weights(labels, num_classes, scheme="balanced"):
    """Class weights [num_classes] float32 (on the tensor's device; CPU tensors work) from the class counts of an integer tensor of
    any shape -- a `window_labels` map, a loader's ``.labels``, a label raster.  Values outside [0, K) do not count (-1, 255).
    "balanced": n / (K_present * count_c), scikit-learn's class_weight="balanced" over the classes present; "inverse_sqrt":
    proportional to 1 / sqrt(count_c), scaled like "balanced" so that sum_c count_c * w_c = n (a sample's mean weight is 1).  A class
    without a sample gets weight 0.  For `set_class_weights` of the engines and ``class_weight=`` of the fit functions."""
    k = int(num_classes)
    if k < 1:
        raise RuntimeError(f"num_classes must be positive, got {num_classes}")
    if not isinstance(labels, torch.Tensor) or labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise RuntimeError("labels must be an integer tensor of class ids")
    if scheme not in ("balanced", "inverse_sqrt"):
        raise RuntimeError(f"scheme must be 'balanced' or 'inverse_sqrt', got {scheme!r}")
    flat = labels.reshape(-1).to(torch.int64)
    ok = (flat >= 0) & (flat < k)
    count = torch.bincount(torch.where(ok, flat, k), minlength=k + 1)[:k].to(torch.float64)       # bin K takes what does not count
    n = count.sum()
    if float(n) == 0.0:
        raise RuntimeError("no label in [0, num_classes): nothing to weight")
    present = count > 0
    safe = torch.where(present, count, torch.ones_like(count))
    if scheme == "balanced":
        w = n / (present.sum() * safe)
    else:
        w = safe.rsqrt() * (n / torch.where(present, count.sqrt(), torch.zeros_like(count)).sum())
    return torch.where(present, w, torch.zeros_like(w)).to(torch.float32)


def drawable_windows(label, windows=None, purity=None, min_purity=0.0, unlabelled=False):
    """The ids a `SceneLoader` draws from, in the order given: ``windows`` (1-D int64; None = every window of the
    label map, ascending) restricted to ``label >= 0`` and, when ``purity`` is given, to ``purity >= min_purity``.  unlabelled=True
    keeps the windows with label -1 too (their purity passes): with ``ignore_index=-1`` in the fit they train the reconstruction
    only.  Works on the tensors' own device (one readback of the number kept)."""
    if not isinstance(label, torch.Tensor) or label.dim() != 2 or label.dtype != torch.int64:
        raise RuntimeError("label must be an int64 [nH, nW] map of window labels (`window_labels`)")
    flat = label.reshape(-1)
    if windows is None:
        windows = torch.arange(flat.numel(), dtype=torch.int64, device=label.device)
    else:
        windows = _windows_arg(windows, label.device, flat.numel(), allow_empty=True)
    lab = flat[windows]
    keep = torch.ones_like(lab, dtype=torch.bool) if unlabelled else lab >= 0
    if purity is not None:
        if not isinstance(purity, torch.Tensor) or tuple(purity.shape) != tuple(label.shape):
            raise RuntimeError(f"purity must be a [nH, nW] = {list(label.shape)} tensor")
        if purity.device != label.device:
            raise RuntimeError(f"purity is on {purity.device}, label on {label.device}")
        pure = purity.reshape(-1)[windows] >= float(min_purity)
        keep = keep & ((pure | (lab < 0)) if unlabelled else pure)
    elif float(min_purity) > 0.0:
        raise RuntimeError("min_purity needs the purity map (`window_labels`)")
    return windows[keep]


class SceneLoader:
    """Iterable of (x [b,C,P,P] float32, y [b] int64) batches of the labelled windows of a scene, both on the scene's device: what
    `fit_autoencoder`, `fit_autoencoder_group`, `grid_search_autoencoder`, `extract_features`, `fit_mlp` and `evaluate` take as a
    loader.  ``label`` (and ``purity``) are `window_labels`' maps [nH,nW] of the scene's grid at (patch, stride; None: the patch size).

    The drawable ids (``.windows``) are ``windows`` (default: all) restricted to label >= 0 and, with ``purity``, to
    purity >= min_purity (`drawable_windows`); two loaders over disjoint ``windows`` make a train / validation split.  Epoch e
    (counted per ``__iter__``, or set with `set_epoch`) takes the ids in `window_schedule`'s order -- shuffled when ``shuffle``
    (default: ``train``) -- and batch i is ``stage_scene_windows(ids, train=train, seed=seed, step=e * len(self) + i, noise_std=,
    crop=, augment=)`` with ``y = label.reshape(-1)[ids]`` (``augment``: an `Augment` policy, None by default).  The epoch's order
    is uploaded once when the iterator starts; nothing inside an epoch synchronises the host.

    unlabelled=True keeps the windows without a label as well (``y = -1``; ``windows`` and ``min_purity`` still apply to the labelled
    ones): fit with ``ignore_index=-1`` and the whole scene trains the reconstruction while only the labelled windows train the
    classifier ("imbalanced / partly labelled scene").  ``.labels`` then holds the -1 entries, which
    `class_weights` and ``class_weight="balanced"`` do not count."""

    def __init__(self, scene, label, divisor=1.0, patch=64, stride=None, batch_size=64, windows=None, min_purity=0.0, purity=None,
                 train=True, shuffle=None, drop_last=False, noise_std=0.03, crop="window", seed=0, unlabelled=False, augment=None):
        _crop_arg(crop)
        if augment is not None and not isinstance(augment, Augment):
            raise RuntimeError(f"augment must be an eae_amd.Augment or None, got {type(augment).__name__}")
        self.augment = augment
        _check_scene(scene)
        self.patch = int(patch)
        self.stride = self.patch if stride is None else int(stride)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise RuntimeError(f"batch_size must be positive, got {batch_size}")
        n_h, n_w = window_grid(scene.shape[1], scene.shape[2], self.patch, self.stride, any_patch=True)
        if not isinstance(label, torch.Tensor) or label.dtype != torch.int64 or tuple(label.shape) != (n_h, n_w):
            got = tuple(label.shape) if isinstance(label, torch.Tensor) else type(label).__name__
            raise RuntimeError(f"label must be the int64 [nH, nW] = {[n_h, n_w]} map `window_labels` returns for a raster of the "
                               f"scene's {scene.shape[1]} x {scene.shape[2]} pixels at this patch and stride, got {got}")
        if label.device != scene.device:
            raise RuntimeError(f"label is on {label.device}, the scene on {scene.device}")
        self.unlabelled = bool(unlabelled)
        self.windows = drawable_windows(label, windows, purity, min_purity, unlabelled=self.unlabelled)
        if self.windows.numel() == 0:
            raise RuntimeError("no window to draw from: none of the given windows is labelled (and pure enough)")
        # device, band count and divisor are checked here, before the first epoch; the divisor stays on the device as fp32 [C]
        self._desc, self._keep, _, _ = _scene_desc(scene, divisor, self.patch, self.stride, any_patch=True)
        self.scene, self.divisor = self._keep
        self.labels = label.reshape(-1)[self.windows]
        self.train = bool(train)
        self.shuffle = self.train if shuffle is None else bool(shuffle)
        self.drop_last = bool(drop_last)
        self.noise_std, self.crop, self.seed = float(noise_std), crop, int(seed)
        if len(self) == 0:
            raise RuntimeError(f"drop_last leaves no batch: {self.windows.numel()} windows, batch_size {self.batch_size}")
        self.epoch = 0

    def __len__(self):
        return schedule_len(self.windows.numel(), self.batch_size, self.drop_last)

    def set_epoch(self, epoch):
        """The epoch the next ``__iter__`` runs (it then goes on counting from there)."""
        if int(epoch) < 0:
            raise RuntimeError(f"epoch must not be negative, got {epoch}")
        self.epoch = int(epoch)

    def schedule(self, epoch):
        """`window_schedule` of this loader for an epoch: positions in ``.windows``, on the host."""
        return window_schedule(self.windows.numel(), self.batch_size, epoch, self.seed, self.shuffle, self.drop_last)

    def __iter__(self):
        e = self.epoch                                       # taken here, not at the first next(): one epoch per __iter__
        self.epoch = e + 1
        return self._batches(e)

    def _batches(self, e):
        batches = self.schedule(e)
        dev = self.windows.device
        order = torch.cat(batches).pin_memory().to(dev, non_blocking=True)             # one upload per epoch
        ids, ys = self.windows[order], self.labels[order]
        base, at, cid = e * len(self), 0, _CROPS[self.crop]
        aug = None if self.augment is None else (self.augment._struct(), None, None, None)
        for i, b in enumerate(batches):
            w = ids[at:at + b.numel()]
            x = _stage_windows(self._desc, self._keep, w, self.train, self.noise_std, self.seed, base + i, None, None, cid, aug)
            yield x, ys[at:at + b.numel()]
            at += b.numel()


# ---------------------------------------------------------------------------------------------------- accuracy assessment
_INT_MAX = 2 ** 31 - 1


def scene_confusion(pred, truth, num_classes, cell=1, origin=(0, 0), mask=None, ignore=None, out=None):
    """Confusion counts int64 [K+1,K+1] (on the device) of a class map against a label raster, pixel by pixel.  ``truth`` [H,W] is a
    label raster of any integer dtype (read as `window_labels` reads it; the values of ``ignore`` count as unlabelled), ``pred`` an
    int64 [cH,cW] map of ``cell`` x ``cell`` cells: pixel (y, x) lies in cell ((y + oy) // cell, (x + ox) // cell), (oy, ox) =
    ``origin``.  Every pixel with ``mask[y, x] == 0`` (``mask``: bool / uint8 [H,W], or None) adds 1 to counts[r, c]: r = the truth
    value in [0, K), else K (unlabelled); c = the cell's value in [0, K), else K (not classified: -1, any other value, a pixel the
    map does not cover).  ``out=``: an earlier result to add to (assessment over several scenes); otherwise the counts start at 0.
    cell=1 compares two maps of one shape, for example `classify_scene`'s window labels with `window_labels`' majority map.
    Exact integer counts: identical from run to run.  `report.confusion_metrics` turns the matrix into accuracy figures."""
    k = int(num_classes)
    if not 1 <= k <= 64:
        raise RuntimeError(f"num_classes must be in 1..64, got {num_classes}")
    if not isinstance(truth, torch.Tensor) or truth.dim() != 2:
        raise RuntimeError("truth must be a [H, W] tensor of class ids")
    if truth.dtype.is_floating_point or truth.dtype.is_complex or truth.dtype == torch.bool:
        raise RuntimeError(f"truth must have an integer dtype, got {truth.dtype}")
    if not isinstance(pred, torch.Tensor) or pred.dim() != 2 or pred.dtype != torch.int64:
        raise RuntimeError("pred must be a 2-D int64 map of class ids")
    cell = int(cell)
    if not 1 <= cell <= _INT_MAX:
        raise RuntimeError(f"cell must be positive, got {cell}")
    try:
        oy, ox = (int(v) for v in origin)
    except (TypeError, ValueError):
        raise RuntimeError(f"origin must be a pair (oy, ox) of integers, got {origin!r}") from None
    if not (0 <= oy <= _INT_MAX and 0 <= ox <= _INT_MAX):
        raise RuntimeError(f"origin must not be negative, got {origin!r}")
    h, w = (int(v) for v in truth.shape)
    c_h, c_w = (int(v) for v in pred.shape)
    if min(h, w, c_h, c_w) < 1:
        raise RuntimeError(f"empty truth {[h, w]} or pred {[c_h, c_w]}")
    if max(h, w, c_h, c_w) > _INT_MAX:
        raise RuntimeError("truth or pred is too large")
    if pred.device != truth.device:
        raise RuntimeError(f"pred is on {pred.device}, truth on {truth.device}")
    m = _mask_arg(truth.unsqueeze(0), mask)
    ignore = _ignore_arg(ignore, k)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or tuple(out.shape) != (k + 1, k + 1) or not out.is_contiguous():
            raise RuntimeError(f"out must be a contiguous int64 [{k + 1}, {k + 1}] tensor (an earlier result)")
        if out.device != truth.device:
            raise RuntimeError(f"out is on {out.device}, truth on {truth.device}")
    _require_gpu(truth.device)
    truth = _label_raster(truth, k, ignore)
    pred = pred.contiguous()
    counts = torch.empty((k + 1, k + 1), dtype=torch.int64, device=truth.device) if out is None else out
    lib = _lib.load()
    with torch.cuda.device(truth.device):
        check(lib.eae_scene_confusion(_stream(), _ptr(truth), truth.element_size(), h, w, _ptr(pred), c_h, c_w, cell, oy, ox, _ptr(m),
                                      k, int(out is not None), _ptr(counts)))
    return counts


def evaluate_scene(scene, encoder, mlp, truth, divisor=1.0, stride=None, batch=512, blend=False, nodata=None, mask=None,
                   max_invalid=0.0, rule="all", windows=None, border=None, fill=0, anchor="center", ignore=None, region=None):
    """Classify a scene and assess the map against a label raster ``truth`` [H,W] of the scene's size: `classify_scene` with the
    same arguments, then `scene_confusion` with the map's geometry -- blend=True: the cells of S x S pixels; blend=False: the
    windows themselves, which must not overlap (stride == patch: overlapping windows without blending give a pixel no single class);
    origin = the leading pads of the border grid (cell (ci, cj) starts at pixel (ci*S - pt, cj*S - pl)).  ``ignore``: truth values
    to count as unlabelled.  ``region``: a [H,W] tensor, non-zero where a pixel is to be assessed (`footprint_mask` of the
    validation windows of a `block_split`); None assesses every pixel.  ``mask`` / ``nodata`` decide which windows are classified,
    as in `classify_scene`; their pixels stay in the counts, under "not classified" where the window was left out.

    Returns {"confusion": int64 [K+1,K+1] on the device, "metrics": `report.confusion_metrics` of it, "probs", "labels": what
    `classify_scene` returned}."""
    from .report import confusion_metrics
    plan = _host_plan(scene, encoder, divisor, stride, batch, nodata, mask, max_invalid, rule, windows, blend=blend, border=border,
                      fill=fill, anchor=anchor, mlp=mlp)
    if not blend and plan.stride != plan.patch:
        raise RuntimeError(f"blend=False needs stride == patch ({plan.patch}): overlapping windows give a pixel no single class without "
                           f"blending, got stride {plan.stride}")
    h, w = int(scene.shape[1]), int(scene.shape[2])
    if not isinstance(truth, torch.Tensor) or tuple(truth.shape) != (h, w):
        got = tuple(truth.shape) if isinstance(truth, torch.Tensor) else type(truth).__name__
        raise RuntimeError(f"truth must be a [H, W] = {[h, w]} label raster of the scene's size, got {got}")
    if truth.device != scene.device:
        raise RuntimeError(f"truth is on {truth.device}, the scene on {scene.device}")
    exclude = None
    if region is not None:
        if not isinstance(region, torch.Tensor) or tuple(region.shape) != (h, w) or region.dtype.is_floating_point:
            raise RuntimeError(f"region must be a bool or integer [H, W] = {[h, w]} tensor")
        if region.device != scene.device:
            raise RuntimeError(f"region is on {region.device}, the scene on {scene.device}")
        exclude = region == 0
    k = int(mlp.num_classes)
    # the remaining host checks of scene_confusion, before a kernel runs (truth's dtype, K, ignore)
    if truth.dtype.is_floating_point or truth.dtype.is_complex or truth.dtype == torch.bool:
        raise RuntimeError(f"truth must have an integer dtype, got {truth.dtype}")
    if not 1 <= k <= 64:
        raise RuntimeError(f"the MLP's num_classes must be in 1..64, got {k}")
    _ignore_arg(ignore, k)
    probs, labels = _classify(plan, mlp, blend)
    cm = scene_confusion(labels, truth, k, cell=plan.stride, origin=(plan.pads[0], plan.pads[2]), mask=exclude, ignore=ignore)
    return {"confusion": cm, "metrics": confusion_metrics(cm), "probs": probs, "labels": labels}


def block_split(n_h, n_w, patch, stride, block, val_fraction=0.2, seed=0):
    """A spatially blocked train / validation split of an n_h x n_w window grid (pure host arithmetic): `SceneLoader` windows
    overlap when S < P, so a random split of window ids shares pixels between the two sides and inflates validation accuracy.  The
    grid is cut into blocks of ``block`` x ``block`` windows (row-major block ids, the last row / column of blocks may be smaller);
    the blocks are ordered by ``torch.randperm(n_blocks, generator=torch.Generator().manual_seed(seed))`` and the first
    max(1, round(val_fraction * n_blocks)) of them are validation.  A training-side window whose pixel footprint intersects a
    validation window's is dropped: the guard band, ceil(P/S) - 1 windows wide.  Returns (train_ids, val_ids, dropped_ids), ascending
    int64 CPU tensors that partition the grid; they feed ``SceneLoader(windows=...)`` and `footprint_mask`."""
    n_h, n_w, patch, stride, block = int(n_h), int(n_w), int(patch), int(stride), int(block)
    if n_h < 1 or n_w < 1:
        raise RuntimeError(f"the grid {n_h} x {n_w} is empty")
    if patch < 1 or not 1 <= stride <= patch:
        raise RuntimeError(f"stride must be in 1..{patch} (the patch size), got {stride}")
    if block < 1:
        raise RuntimeError(f"block must be positive, got {block}")
    f = float(val_fraction)
    if not 0.0 < f < 1.0:
        raise RuntimeError(f"val_fraction must be in (0, 1), got {val_fraction}")
    b_h, b_w = -(-n_h // block), -(-n_w // block)
    n_blocks = b_h * b_w
    order = torch.randperm(n_blocks, generator=torch.Generator().manual_seed(int(seed)))
    is_val_block = torch.zeros(n_blocks, dtype=torch.bool)
    is_val_block[order[:max(1, round(f * n_blocks))]] = True
    bi = torch.arange(n_h) // block
    bj = torch.arange(n_w) // block
    val = is_val_block[bi[:, None] * b_w + bj[None, :]]                       # [n_h, n_w]
    g = -(-patch // stride) - 1                 # windows i and i' share pixels on an axis exactly when |i - i'| * S < P: |i - i'| <= g
    near = torch.nn.functional.max_pool2d(val[None, None].to(torch.float32), 2 * g + 1, stride=1, padding=g)[0, 0] > 0
    dropped = near & ~val
    flat = lambda m: torch.nonzero(m.reshape(-1)).reshape(-1)           # noqa: E731  ascending int64 ids
    return flat(~near), flat(val), flat(dropped)


def footprint_mask(ids, n_w, patch, stride, height, width, device=None):
    """bool [height, width]: true where one of the windows ``ids`` (1-D int64 ids of a grid of whole windows with n_w per row, window
    n at pixel (n // n_w * S, n % n_w * S)) covers the pixel, clipped to the raster.  Torch only (a 2-D difference array and two
    cumulative sums, any S), on ``device`` (default: where ``ids`` is), CPU included.  What `evaluate_scene` takes as ``region=``."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 1 or ids.dtype != torch.int64:
        raise RuntimeError("ids must be a 1-D int64 tensor of window ids")
    n_w, patch, stride, height, width = int(n_w), int(patch), int(stride), int(height), int(width)
    if n_w < 1 or patch < 1 or stride < 1 or height < 1 or width < 1:
        raise RuntimeError("n_w, patch, stride, height and width must be positive")
    dev = ids.device if device is None else torch.device(device)
    ids = ids.to(dev)
    if ids.numel() and int(ids.min()) < 0:
        raise RuntimeError("window ids must not be negative")
    y0 = torch.clamp(torch.div(ids, n_w, rounding_mode="floor") * stride, max=height)
    x0 = torch.clamp(ids % n_w * stride, max=width)
    y1, x1 = torch.clamp(y0 + patch, max=height), torch.clamp(x0 + patch, max=width)
    diff = torch.zeros((height + 1) * (width + 1), dtype=torch.int32, device=dev)
    one = torch.ones(ids.numel(), dtype=torch.int32, device=dev)
    for yy, xx, s in ((y0, x0, one), (y0, x1, -one), (y1, x0, -one), (y1, x1, one)):
        diff.index_add_(0, yy * (width + 1) + xx, s)
    cover = diff.reshape(height + 1, width + 1).cumsum(0, dtype=torch.int32).cumsum(1, dtype=torch.int32)
    return cover[:height, :width] > 0
