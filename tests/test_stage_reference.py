"""The staging stream's NumPy restatement (stage_ref.py) by itself: its layout, written out by hand once per function, and the
statistical conditions the GPU tests of test_gpu_stage_rng.py rely on, at that file's (seed, step) pairs and shapes.  Every bound
is a multiple of the statistic's own standard error or a chi-square quantile; none is taken from what the stream gives."""
import math

import numpy as np
import pytest

import stage_ref as S
from mlp_ref import philox4x32_10
from test_gpu_stage_rng import (GEOM_B, GEOM_N, H, NOISE_B, NOISE_BOUND, NOISE_BOUND_CAP, NOISE_CASES, NOISE_DEV_MEASURED, SCENE_B,
                                SEED_STEPS, W, coded_bands, coded_hwc)

NOISE_SHAPE = (32, 16, H, W)


def chi2_quantile_999(k):
    """The 99.9 % quantile of chi-square with k degrees of freedom (Wilson-Hilferty without scipy: 1 % high at k = 8)."""
    try:
        from scipy.stats import chi2
        return float(chi2.ppf(0.999, k))
    except ImportError:
        z = 3.090232306167813
        return k * (1.0 - 2.0 / (9.0 * k) + z * math.sqrt(2.0 / (9.0 * k))) ** 3


def _chi2(counts):
    e = counts.sum() / counts.size
    return float(((counts - e) ** 2 / e).sum())


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.fixture(scope="module", params=SEED_STEPS, ids=lambda p: f"{p[0]}-{p[1]}")
def noise(request):
    seed, step = request.param
    z = S.stage_noise(seed, step, *NOISE_SHAPE)
    z.setflags(write=False)
    return seed, step, z


# ---------------------------------------------------------------------------------------------------- the cases
def test_cases_are_the_ones_of_the_gpu_file():
    assert SEED_STEPS == [(3, 5), (0, 0), (2 ** 40 + 7, 2 ** 33 + 1)]
    assert (H, W, GEOM_B, GEOM_N, NOISE_B, SCENE_B) == (12, 20, 4095, 3, 5, 7)
    assert H != W and min(H, W) >= 9
    assert (GEOM_B * H * W) % 256 and (NOISE_B * H * W) % 256               # a partial last workgroup
    assert GEOM_B * H * W > 256 and NOISE_B * H * W > 256                   # more than one workgroup
    widths = {c for k, c, _, _ in NOISE_CASES if k == "bands"}
    assert widths == {1, 3, 4, 5, 13, 16}
    assert {p for k, c, _, p in NOISE_CASES if k == "bands" and c == 13} == {0, 1, 2}
    assert {d for k, _, d, _ in NOISE_CASES if k == "bands"} == {"uint8", "uint16"}
    assert any(k == "augment" for k, _, _, _ in NOISE_CASES)
    assert NOISE_BOUND == 8 * NOISE_DEV_MEASURED and NOISE_BOUND <= NOISE_BOUND_CAP == 1e-3


def test_coded_images_tell_every_draw_apart():
    data = coded_bands()
    assert data.shape == (GEOM_N, 1, H, W) and data[2, 0, 11, 19] == 1 + 240 * 2 + 20 * 11 + 19 and data.min() == 1
    cells = [(f, t, le) for f in (0, 1) for t in range(9) for le in range(9)]
    outs = {S.stage_transform(data[n:n + 1], [cell], 1.0).tobytes() for n in range(GEOM_N) for cell in cells}
    assert len(outs) == GEOM_N * 162
    u8 = coded_hwc(253)
    assert tuple(u8[252, 11, 19]) == (11, 19, 1) and tuple(u8[250, 0, 0]) == (0, 0, 250)
    outs = {S.stage_transform_hwc(u8[b:b + 1], [cell]).tobytes() for b in (0, 1) for cell in cells}
    assert len(outs) == 2 * 162


# ---------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_stage_params_layout(seed, step):
    w = [int(v) for v in philox4x32_10((2, 0x5eed, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))]
    flip, top, left = S.stage_params(seed, step, 4)
    assert all(a.dtype == np.int32 and a.shape == (4,) for a in (flip, top, left))
    assert (int(flip[2]), int(top[2]), int(left[2])) == (w[0] >> 31, (w[1] * 9) >> 32, (w[2] * 9) >> 32)
    assert np.array_equal(S.params_array(seed, step, 4), np.stack([flip, top, left], 1))


@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_stage_noise_layout(seed, step):
    B, C, b, y, x = 2, 13, 1, 7, 3
    p = (b * H + y) * W + x
    key = (seed & 0xFFFFFFFF, ~(seed >> 32) & 0xFFFFFFFF)
    w = [int(v) for v in philox4x32_10((p, (0 ^ 0xA5A5) + (8 << 16), step & 0xFFFFFFFF, step >> 32), key)]
    u = [((w[0] >> 8) + 1) / 2 ** 24, (w[1] >> 8) / 2 ** 24, ((w[2] >> 8) + 1) / 2 ** 24, (w[3] >> 8) / 2 ** 24]
    tau = float(np.float32(6.28318530718))
    assert tau == S.TAU and tau != 2 * math.pi
    r1, r2 = math.sqrt(-2 * math.log(u[0])), math.sqrt(-2 * math.log(u[2]))
    want = [r1 * math.cos(tau * u[1]), r1 * math.sin(tau * u[1]), r2 * math.cos(tau * u[3]), r2 * math.sin(tau * u[3])]
    z = S.stage_noise(seed, step, B, C, H, W)
    assert z.dtype == np.float64 and z.shape == (B, C, H, W)
    np.testing.assert_allclose(z[b, 8:12, y, x], want, rtol=0, atol=1e-14)
    # group 0 of the same pixel has the plain 0xA5A5 word, and a narrower batch draws the same values for the bands it has
    w0 = philox4x32_10((p, 0xA5A5, step & 0xFFFFFFFF, step >> 32), key)
    np.testing.assert_allclose(z[b, 0:4, y, x], [float(v) for v in S.noise4(w0)], rtol=0, atol=1e-14)
    assert np.array_equal(S.stage_noise(seed, step, B, 5, H, W), z[:, :5])
    assert len({z[b, c, y, x] for c in range(C)}) == C


def test_stage_transform_layout():
    img = np.arange(1, 1 + 2 * H * W).reshape(1, 2, H, W).astype(np.uint16)
    div = np.array([1.0, 3.0], np.float32)
    out = S.stage_transform(img, [(0, 4, 4)], div)
    assert out.dtype == np.float32 and np.array_equal(out[0, 0], img[0, 0]) and np.array_equal(out[0, 1], img[0, 1].astype(np.float32) / np.float32(3))
    out = S.stage_transform(img, [(0, 0, 8)], div)               # top 0: down by 4 rows; left 8: left by 4 columns
    assert out[0, 0, 4, 0] == img[0, 0, 0, 4] and (out[0, 0, :4] == 0).all() and (out[0, 0, :, W - 4:] == 0).all()
    out = S.stage_transform(img, [(1, 8, 0)], div)               # flipped first, then cropped
    assert out[0, 0, 0, 4] == img[0, 0, 4, W - 1] and (out[0, 0, H - 4:] == 0).all() and (out[0, 0, :, :4] == 0).all()
    hwc = np.ascontiguousarray(img.astype(np.uint8)[:, [0, 1, 0]].transpose(0, 2, 3, 1))
    assert np.array_equal(S.stage_transform_hwc(hwc, [(1, 2, 7)]),
                          S.stage_transform(img.astype(np.uint8)[:, [0, 1, 0]], [(1, 2, 7)], np.float32(255)))
    assert np.array_equal(S.stage_transform(img, S.stage_params(3, 5, 1), div), S.stage_transform(img, S.params_array(3, 5, 1), div))


@pytest.mark.parametrize("crop", ["window", "scene"])
def test_scene_transform_is_the_per_pixel_statement(crop):
    """`scene_transform` against the transform written out pixel by pixel (include/eae.h, eae_scene_stage_windows): output (y, x)
    reads window-local (sy, sx) = (y + top - 4, x + left - 4), mirrored to P - 1 - sx when flipped; crop="window" reads 0 when the
    unflipped position leaves the window, crop="scene" when the scene pixel leaves the scene."""
    c, hs, ws, p = 2, 21, 26, 8
    scene = np.arange(1, 1 + c * hs * ws).reshape(c, hs, ws).astype(np.uint16)
    div = np.array([1.0, 3.0], np.float32)
    origins = [(0, 0), (hs - p, ws - p), (0, ws - p), (hs - p, 0), (5, 7), (6, 9)]
    params = [(0, 0, 0), (1, 8, 8), (1, 0, 8), (0, 8, 0), (1, 4, 2), (0, 2, 5)]
    ref = np.zeros((len(origins), c, p, p), np.float32)
    for b, ((oy, ox), (flip, top, left)) in enumerate(zip(origins, params)):
        for y in range(p):
            for x in range(p):
                sy, sx = y + top - 4, x + left - 4
                in_window = 0 <= sy < p and 0 <= sx < p
                if flip:
                    sx = p - 1 - sx
                gy, gx = oy + sy, ox + sx
                if in_window if crop == "window" else (0 <= gy < hs and 0 <= gx < ws):
                    ref[b, :, y, x] = scene[:, gy, gx].astype(np.float32) / div
    got = S.scene_transform(scene, origins, p, params, div, crop)
    assert got.dtype == np.float32 and np.array_equal(got, ref)
    other = S.scene_transform(scene, origins, p, params, div, "scene" if crop == "window" else "window")
    assert not np.array_equal(got, other)                          # the corner windows tell the two crops apart


# ---------------------------------------------------------------------------------------------------- geometric draws
@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_geometric_draws_are_uniform(seed, step):
    B = GEOM_B
    flip, top, left = S.stage_params(seed, step, B)
    assert set(np.unique(flip)) == {0, 1}
    for a in (top, left):
        assert a.min() == 0 and a.max() == 8
    mean_flip = float(flip.mean())
    chi_top, chi_left = _chi2(np.bincount(top, minlength=9)), _chi2(np.bincount(left, minlength=9))
    cells = np.bincount((flip * 9 + top) * 9 + left, minlength=162)
    chi_joint = _chi2(cells)
    print(f"seed={seed} step={step}: mean flip {mean_flip:.4f}, chi2 top {chi_top:.1f} left {chi_left:.1f} joint {chi_joint:.1f}, "
          f"smallest cell {cells.min()}")
    assert abs(mean_flip - 0.5) <= 4 * 0.5 / math.sqrt(B)
    q8, q161 = chi2_quantile_999(8), chi2_quantile_999(161)
    assert 26.0 < q8 < 26.5 and 220.0 < q161 < 223.0
    assert chi_top < q8 and chi_left < q8
    assert chi_joint < q161
    assert cells.shape == (162,) and cells.min() >= 1          # every crop offset in both flip states, for the GPU test


def test_high_bits_matter_for_the_geometric_draws():
    base = S.params_array(3, 5, 64)
    assert not np.array_equal(base, S.params_array(3 | 1 << 32, 5, 64))
    assert not np.array_equal(base, S.params_array(3, 5 | 1 << 32, 64))
    assert not np.array_equal(base, S.params_array(3, 6, 64)) and not np.array_equal(base, S.params_array(4, 5, 64))
    assert np.array_equal(base, S.params_array(3 + 2 ** 64, 5 - 2 ** 64, 64))            # masked to 64 bits
    assert np.array_equal(base[:7], S.params_array(3, 5, 7))                               # keyed on b alone


# ---------------------------------------------------------------------------------------------------- noise
def test_noise_moments(noise):
    seed, step, z = noise
    n = z.size
    assert n == 122880 and np.isfinite(z).all()
    mean, std = float(z.mean()), float(z.std())
    m4 = float((((z - mean) / std) ** 4).mean())
    print(f"seed={seed} step={step}: mean {mean:.4f}, std - 1 {std - 1:.4f}, m4 - 3 {m4 - 3:.4f}")
    assert abs(mean) <= 4 / math.sqrt(n)
    assert abs(std - 1) <= 4 / math.sqrt(2 * n)
    assert abs(m4 - 3) <= 4 * math.sqrt(24 / n)


def test_noise_bands_are_uncorrelated(noise):
    seed, step, z = noise
    B, C = NOISE_SHAPE[:2]
    r = np.corrcoef(z.transpose(1, 0, 2, 3).reshape(C, -1))
    worst = float(np.abs(r - np.eye(C)).max())
    print(f"seed={seed} step={step}: largest band correlation {worst:.4f}")
    assert worst <= 4.5 / math.sqrt(B * H * W)


def test_noise_is_uncorrelated_with_other_keys_and_along_pixels(noise):
    seed, step, z = noise
    bound = 4 / math.sqrt(z.size)
    for s2, t2 in ((seed, step + 1), (seed ^ 1 << 32, step), (seed, step ^ 1 << 32)):
        r = _corr(z, S.stage_noise(s2, t2, *NOISE_SHAPE))
        print(f"seed={seed} step={step} against seed={s2} step={t2}: {r:.4f}")
        assert abs(r) <= bound
    flat = z.transpose(1, 0, 2, 3).reshape(NOISE_SHAPE[1], -1)             # [C][p]: neighbours along the flat pixel index
    r = _corr(flat[:, :-1], flat[:, 1:])
    print(f"seed={seed} step={step}: lag-1 pixel correlation {r:.4f}")
    assert abs(r) <= bound
