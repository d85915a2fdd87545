"""Plain NumPy restatement of the augmentation policy of the staging calls (include/eae.h, "augmentation policy"; csrc/eae_stage.hip),
on `mlp_ref.philox4x32_10` and `stage_ref`.

Random draws.  (flip, top, left) are `stage_ref.stage_params`, whatever the policy.  With (seed lo, seed hi) and (step lo, step hi)
the 32-bit halves of seed and step, and b the batch position:

  quarter turn of image b                 the geometric call itself: counter (b, 0x5eed, step lo, step hi), key (seed lo, seed hi);
                                          rot = w3 >> 30 (words 0..2 are flip, top, left)
  theta, sigma, image gain g of image b   counter (b, 0xA061, step lo, step hi), key (~seed lo, seed hi)
                                          theta [degrees] = U(w0; -rotate, 2 rotate), sigma = U(w1; 1 - scale, 2 scale),
                                          g = U(w2; 1 - gain, 2 gain)
  band gains of image b, group c0         counter (b, 0xA062 + (c0 << 16), step lo, step hi), key (~seed lo, seed hi)
                                          g_c of band c0 + j = U(w_j; 1 - band_gain, 2 band_gain)
  band offsets of image b, group c0       counter (b, 0xA063 + (c0 << 16), step lo, step hi), key (~seed lo, seed hi)
                                          o_c of band c0 + j = U(w_j; -offset, 2 offset)

c0 in {0, 4, 8, 12}; U(w; lo, width) = fl32((w >> 8) 2^-24 * width + lo), one rounding (an fma); 1 - x is an fp32 subtraction.  The key
differs from the geometric call's (seed lo, seed hi) in its first word and from the noise calls' (seed lo, ~seed hi) in both, so the
three families never share a Philox input.  theta in radians is fl32(theta * fl32(pi / 180)); (a, b) = (cos theta / sigma,
sin theta / sigma) are computed here in float64 and rounded once: the reference of the device's sincosf and division.

Transform.  The quarter turn is stated on images: `integer_image` flips a neighbourhood of the window, slices the crop out of it and
turns it with np.rot90.  The bilinear path samples that image (extended by a margin, so that taps outside the output frame are what
the integer path reads there) at X = fl32(fl32(a u - fl32(b v)) + c), Y = fl32(fl32(b u + fl32(a v)) + c), u = x - c, v = y - c.

fp32 roundings are restated in float64: a product of two fp32 numbers is exact there, and the sums met here (coordinates of a few
units, coefficients of magnitude >= 2^-24 or exactly 0) are too, so rounding the float64 result to fp32 is the single rounding of
the device's fma."""
import numpy as np

from mlp_ref import philox4x32_10
import stage_ref as S

_M32 = 0xFFFFFFFF
TAG_IMAGE, TAG_GAIN, TAG_OFFSET = 0xA061, 0xA062, 0xA063
DEG = np.float32(0.017453292519943295)
F32 = np.float32


class Policy:
    """The fields of eae_amd.Augment."""
    def __init__(self, dihedral=False, rotate=0.0, scale=0.0, gain=0.0, band_gain=0.0, offset=0.0):
        self.dihedral, self.rotate, self.scale = bool(dihedral), F32(rotate), F32(scale)
        self.gain, self.band_gain, self.offset = F32(gain), F32(band_gain), F32(offset)

    def kwargs(self):
        return dict(dihedral=self.dihedral, rotate=float(self.rotate), scale=float(self.scale), gain=float(self.gain),
                    band_gain=float(self.band_gain), offset=float(self.offset))


def fma32(a, b, c):
    """fl32(a * b + c) of fp32 arrays, through float64 (module docstring)."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def uniform(w, lo, width):
    u = ((w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24).astype(F32)          # exact
    return fma32(u, F32(width), F32(lo))


def geom_words(seed, step, B):
    (seed_lo, seed_hi), (step_lo, step_hi) = S._split(seed), S._split(step)
    return philox4x32_10((np.arange(B, dtype=np.uint64), S.PARAMS_TAG, step_lo, step_hi), (seed_lo, seed_hi))


def geom_array(seed, step, B, dihedral=True):
    """int32 [B,4] = (flip, top, left, rot): `stage_ref.params_array` and the quarter turn, word 3 of the same call."""
    rot = (geom_words(seed, step, B)[3] >> np.uint32(30)).astype(np.int32)
    if not dihedral:
        rot = np.zeros_like(rot)
    return np.concatenate([S.params_array(seed, step, B), rot[:, None]], 1).astype(np.int32)


def _aug_words(seed, step, B, tag, c0):
    (seed_lo, seed_hi), (step_lo, step_hi) = S._split(seed), S._split(step)
    return philox4x32_10((np.arange(B, dtype=np.uint64), tag + (c0 << 16), step_lo, step_hi), (~seed_lo & _M32, seed_hi))


def image_draws(seed, step, B, pol):
    """(theta [degrees], sigma, g), fp32 [B] each."""
    w = _aug_words(seed, step, B, TAG_IMAGE, 0)
    theta = uniform(w[0], -pol.rotate, F32(2) * pol.rotate)
    sigma = uniform(w[1], F32(1) - pol.scale, F32(2) * pol.scale)
    g = uniform(w[2], F32(1) - pol.gain, F32(2) * pol.gain)
    return theta, sigma, g


def affine_array(seed, step, B, pol):
    """float32 [B,2] = (a, b) = (cos theta / sigma, sin theta / sigma), float64 arithmetic rounded once."""
    theta, sigma, _ = image_draws(seed, step, B, pol)
    rad = (theta.astype(np.float64) * np.float64(DEG)).astype(F32).astype(np.float64)
    return np.stack([np.cos(rad) / sigma.astype(np.float64), np.sin(rad) / sigma.astype(np.float64)], 1).astype(F32)


def band_draws(seed, step, B, C, pol):
    """(g_c, o_c), fp32 [B,C] each."""
    gains, offs = np.empty((B, C), F32), np.empty((B, C), F32)
    for c0 in range(0, C, 4):
        wg, wo = _aug_words(seed, step, B, TAG_GAIN, c0), _aug_words(seed, step, B, TAG_OFFSET, c0)
        for j in range(min(4, C - c0)):
            gains[:, c0 + j] = uniform(wg[j], F32(1) - pol.band_gain, F32(2) * pol.band_gain)
            offs[:, c0 + j] = uniform(wo[j], -pol.offset, F32(2) * pol.offset)
    return gains, offs


def radio_array(seed, step, B, C, pol):
    """float32 [B,C,2] = (fl32(g g_c), o_c): the policy's radiometric draws as the explicit `radio` argument."""
    _, _, g = image_draws(seed, step, B, pol)
    gains, offs = band_draws(seed, step, B, C, pol)
    total = (g.astype(np.float64)[:, None] * gains.astype(np.float64)).astype(F32)
    return np.stack([total, offs], 2).astype(F32)


def apply_radio(v, radio):
    """fl32(v * gain + offset) of v [B,C,H,W] with radio [B,C,2]."""
    return fma32(v, radio[:, :, 0, None, None], radio[:, :, 1, None, None])


# ---------------------------------------------------------------------------------------------------- the transform
def window_neighbourhood(win, e):
    """[C,P+2e,P+2e]: the window [C,P,P] with zeros around it (crop="window", stage_bands, augment_batch)."""
    return np.pad(win, ((0, 0), (e, e), (e, e)))


def scene_neighbourhood(scene, oy, ox, p, e):
    """[C,P+2e,P+2e]: the scene [C,H,W] around the window at (oy, ox), zeros outside the scene (crop="scene")."""
    pad = np.pad(scene, ((0, 0), (e, e), (e, e)))
    return pad[:, oy:oy + p + 2 * e, ox:ox + p + 2 * e]


def integer_image(neigh, p, geom, m=0):
    """Raw [C,P+2m,P+2m]: flip -> pad-4 crop -> rot quarter turns (np.rot90) of the window in the middle of `neigh`, on the output
    frame extended by m pixels on every side (m = 0: the output itself).  The margin e of `neigh` must be at least m + 4."""
    flip, top, left, rot = (int(v) for v in geom)
    e = (neigh.shape[-1] - p) // 2
    assert neigh.shape[-1] == neigh.shape[-2] == p + 2 * e and e >= m + 4
    if flip:
        neigh = neigh[..., ::-1]                                   # about the window's own axis: the margins are equal
    y0, x0 = e + top - 4 - m, e + left - 4 - m
    ext = neigh[..., y0:y0 + p + 2 * m, x0:x0 + p + 2 * m]
    return np.rot90(ext, rot, axes=(-2, -1))


def sample_positions(p, a, b):
    """(X, Y) fp32 [P,P]: where output pixel (x, y) samples the integer image, with the device's roundings."""
    c = F32((p - 1) / 2)
    x = np.arange(p, dtype=F32)[None, :] - c
    y = np.arange(p, dtype=F32)[:, None] - c
    x, y = np.broadcast_arrays(x, y)
    a, b = F32(a), F32(b)
    bv = fma32(b, y, F32(0))
    av = fma32(a, y, F32(0))
    big_x = (fma32(a, x, -bv).astype(np.float64) + np.float64(c)).astype(F32)
    big_y = (fma32(b, x, av).astype(np.float64) + np.float64(c)).astype(F32)
    return big_x, big_y


def bilinear64(ext, m, big_x, big_y):
    """float64 [C,P,P]: bilinear interpolation of the raw extended image `ext` (margin m) at the fp32 positions, with their fp32
    fractions; also the mask of pixels whose four taps lie inside the output frame [0, P)."""
    p = ext.shape[-1] - 2 * m
    xf, yf = np.floor(big_x), np.floor(big_y)
    fx, fy = (big_x - xf).astype(np.float64), (big_y - yf).astype(np.float64)
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    assert xi.min() >= -m and xi.max() + 1 < p + m and yi.min() >= -m and yi.max() + 1 < p + m, "margin too small"
    e64 = ext.astype(np.float64)
    t00, t01 = e64[:, yi + m, xi + m], e64[:, yi + m, xi + m + 1]
    t10, t11 = e64[:, yi + m + 1, xi + m], e64[:, yi + m + 1, xi + m + 1]
    val = (t00 * (1 - fx) + t01 * fx) * (1 - fy) + (t10 * (1 - fx) + t11 * fx) * fy
    inner = (xi >= 0) & (xi + 1 < p) & (yi >= 0) & (yi + 1 < p)
    return val, inner


def transform(neighs, p, geom, div, affine=None, m=None):
    """float64 [B,C,P,P]: the policy's geometric part and the division for neighbourhoods [B][C,P+2e,P+2e].  Without `affine` the
    values are exactly the device's fp32 ones (one true division); with it they are the float64 bilinear values."""
    c = neighs[0].shape[0]
    div = np.broadcast_to(np.asarray(div, F32).reshape(-1), (c,))
    out = np.empty((len(neighs), c, p, p), np.float64)
    for n, neigh in enumerate(neighs):
        if affine is None:
            raw = integer_image(neigh, p, geom[n])
            out[n] = (raw.astype(F32) / div[:, None, None]).astype(np.float64)
        else:
            ext = integer_image(neigh, p, geom[n], m)
            val, _ = bilinear64(ext, m, *sample_positions(p, affine[n][0], affine[n][1]))
            out[n] = val / div.astype(np.float64)[:, None, None]
    return out


def hwc_windows(u8):
    """uint8 HWC [B,H,W,3] as planar images [B,3,H,W]."""
    return np.ascontiguousarray(u8.transpose(0, 3, 1, 2))
