"""Plain NumPy restatement of the staging kernel's random stream and transform without a policy (csrc/eae_stage.h: philox4,
stage_draw_geom, stage_draw_noise4; csrc/eae_stage.hip: stage_kernel over AugSrcHwc, AugSrcBands, AugSrcScene).

The stream is counter-based Philox4x32-10 (`mlp_ref.philox4x32_10`, itself pinned by the Random123 known-answer vectors), keyed by
(seed, step):

  geometric draws of batch position b    counter (b, 0x5eed, step lo, step hi), key (seed lo, seed hi)
                                          flip = w0 >> 31, top = (w1 * 9) >> 32, left = (w2 * 9) >> 32
  noise of pixel p (flat over [B][H][W])  counter (p lo, ((p hi ^ 0xA5A5) + (c0 << 16)) mod 2^32, step lo, step hi),
  and band group c0 in {0, 4, 8, 12}      key (seed lo, ~seed hi)
                                          u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24, u3, u4 likewise from w2, w3
                                          bands c0 .. c0 + 3: r1 cos(t u2), r1 sin(t u2), r2 cos(t u4), r2 sin(t u4),
                                          r = sqrt(-2 ln u), t = float32(6.28318530718)

The noise is computed in float64: the high-precision reference of the device's fast __logf, __cosf and __sinf."""
import numpy as np

from mlp_ref import philox4x32_10

_M64 = 0xFFFFFFFFFFFFFFFF
_M32 = 0xFFFFFFFF
TAU = float(np.float32(6.28318530718))          # the kernel's constant, not 2 pi
PARAMS_TAG = 0x5eed
NOISE_TAG = 0xA5A5


def _split(v):
    v = int(v) & _M64
    return v & _M32, v >> 32


def stage_params(seed, step, B):
    """(flip, top, left), int32 [B] each: the geometric draws of batch positions 0 .. B-1."""
    (seed_lo, seed_hi), (step_lo, step_hi) = _split(seed), _split(step)
    b = np.arange(B, dtype=np.uint64)
    w = philox4x32_10((b, PARAMS_TAG, step_lo, step_hi), (seed_lo, seed_hi))
    flip = (w[0] >> np.uint32(31)).astype(np.int32)
    top = ((w[1].astype(np.uint64) * np.uint64(9)) >> np.uint64(32)).astype(np.int32)
    left = ((w[2].astype(np.uint64) * np.uint64(9)) >> np.uint64(32)).astype(np.int32)
    return flip, top, left


def params_array(seed, step, B):
    """`stage_params` as the int32 [B,3] array the kernels take for explicit draws."""
    return np.stack(stage_params(seed, step, B), 1).astype(np.int32)


def noise4(words):
    """The four standard normals (float64) of one Philox call's output words: two Box-Muller pairs."""
    u1 = ((words[0] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (words[1] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    u3 = ((words[2] >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u4 = (words[3] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r1, r2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    return [r1 * np.cos(TAU * u2), r1 * np.sin(TAU * u2), r2 * np.cos(TAU * u4), r2 * np.sin(TAU * u4)]


def stage_noise(seed, step, B, C, H, W):
    """float64 [B,C,H,W]: the standard normals the kernels draw for a batch of that shape."""
    (seed_lo, seed_hi), (step_lo, step_hi) = _split(seed), _split(step)
    p = np.arange(B * H * W, dtype=np.uint64)
    p_lo, p_hi = p & np.uint64(_M32), p >> np.uint64(32)
    out = np.empty((B, C, H, W), np.float64)
    for c0 in range(0, C, 4):
        c1 = ((p_hi ^ np.uint64(NOISE_TAG)) + np.uint64(c0 << 16)) & np.uint64(_M32)
        z = noise4(philox4x32_10((p_lo, c1, step_lo, step_hi), (seed_lo, ~seed_hi & _M32)))
        for j in range(min(4, C - c0)):
            out[:, c0 + j] = z[j].reshape(B, H, W)
    return out


def _crop(img, flip, top, left):
    """flip -> zero pad of 4 -> crop at (top, left), for one image whose last two axes are (H, W)."""
    h, w = img.shape[-2:]
    if flip:
        img = img[..., ::-1]
    pad = np.zeros(img.shape[:-2] + (h + 8, w + 8), img.dtype)
    pad[..., 4:4 + h, 4:4 + w] = img
    return pad[..., top:top + h, left:left + w]


def stage_transform(imgs, params, div):
    """fp32 [B,C,H,W] of planar images [B,C,H,W] (any H, W): flip -> pad-4 crop (zeros) -> / div[c] (fp32 true division).
    params: [B] rows of (flip, top, left), or the tuple of three arrays `stage_params` returns."""
    if isinstance(params, tuple):
        params = np.stack(params, 1)
    b, c, h, w = imgs.shape
    div = np.broadcast_to(np.asarray(div, np.float32).reshape(-1), (c,))
    out = np.zeros((b, c, h, w), np.float32)
    for n in range(b):
        flip, top, left = (int(v) for v in params[n])
        out[n] = _crop(imgs[n], flip, top, left).astype(np.float32) / div[:, None, None]
    return out


def scene_transform(scene, origins, p, params, div, crop):
    """fp32 [B,C,P,P] of the P x P windows of a planar scene [C,H,W] at `origins` [B] = (oy, ox) (stage_scene_windows).
    crop="window": `stage_transform` of the windows; crop="scene": the same flip and crop of the window's neighbourhood in the
    zero-padded scene, so the crop reads the real pixels around the window."""
    if isinstance(params, tuple):
        params = np.stack(params, 1)
    if crop == "window":
        return stage_transform(np.stack([scene[:, oy:oy + p, ox:ox + p] for oy, ox in origins]), params, div)
    assert crop == "scene"
    div = np.broadcast_to(np.asarray(div, np.float32).reshape(-1), (scene.shape[0],))
    padded = np.pad(scene, ((0, 0), (4, 4), (4, 4)))
    out = np.empty((len(origins), scene.shape[0], p, p), np.float32)
    for b, (oy, ox) in enumerate(origins):
        flip, top, left = (int(v) for v in params[b])
        ext = padded[:, oy:oy + p + 8, ox:ox + p + 8]
        if flip:
            ext = ext[..., ::-1]
        out[b] = ext[:, top:top + p, left:left + p].astype(np.float32) / div[:, None, None]
    return out


def stage_transform_hwc(u8, params):
    """fp32 [B,3,H,W] of uint8 HWC images [B,H,W,3]: `stage_transform` with ToTensor's / 255 (augment_batch)."""
    assert u8.dtype == np.uint8 and u8.shape[3] == 3
    return stage_transform(np.ascontiguousarray(u8.transpose(0, 3, 1, 2)), params, np.float32(255))


def add_noise(v, noise, std):
    """v + std * noise with one fp32 rounding (the kernels' fmaf): fp32 std, the product exact in float64."""
    return (v.astype(np.float64) + np.float64(np.float32(std)) * noise.astype(np.float64)).astype(np.float32)


def stage_ref(data, idx, div, params, noise, std):
    """NumPy restatement: flip -> pad-4 crop (zeros) -> / divisor[c] (fp32 true division) -> + std * noise (one fp32 rounding)."""
    out = stage_transform(data[idx], params, div)
    if noise is not None:
        out = add_noise(out, noise, std)
    return out
