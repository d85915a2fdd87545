"""The NumPy restatement of the augmentation policy (augment_ref.py) on its own, without a GPU: that it is the transform the header
describes -- orientation, centre and sign of the rotation, the draws' ranges -- and the statistical conditions the GPU tests of
test_gpu_augment.py rely on, for the very cases they run."""
import numpy as np
import pytest

import augment_ref as R
import stage_ref as S
from test_gpu_augment import SEED_STEPS, GEOM_B, HW, FULL, MARGIN, AFFINE_CASES, d4_geom, coded_bands

P = 16


def _asym(p=HW):
    """An image without any symmetry: position-coded."""
    return (1 + np.arange(p * p)).reshape(1, p, p).astype(np.uint16)


def test_the_eight_elements_are_distinct_and_four_turns_are_the_identity():
    img = _asym()
    neigh = R.window_neighbourhood(img, 4)
    seen = {R.integer_image(neigh, HW, (f, 4, 4, r)).tobytes() for f in (0, 1) for r in range(4)}
    assert len(seen) == 8
    assert np.array_equal(R.integer_image(neigh, HW, (0, 4, 4, 0)), img)
    once = R.integer_image(neigh, HW, (0, 4, 4, 1))
    assert np.array_equal(once, np.rot90(img, 1, axes=(-2, -1))) and once[0, HW - 1, 0] == img[0, 0, 0]      # counter-clockwise
    turned = img
    for _ in range(4):
        turned = R.integer_image(R.window_neighbourhood(turned, 4), HW, (0, 4, 4, 1))
    assert np.array_equal(turned, img)
    # rot = 0 is stage_ref's transform, for every flip and crop
    for geom in d4_geom():
        if geom[3] == 0:
            assert np.array_equal(R.integer_image(neigh, HW, geom), S._crop(img, *geom[:3]))


@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_the_policy_leaves_flip_top_left_alone_and_rot_is_word_3(seed, step):
    geom = R.geom_array(seed, step, GEOM_B)
    assert np.array_equal(geom[:, :3], S.params_array(seed, step, GEOM_B))
    assert np.array_equal(geom[:, 3], (R.geom_words(seed, step, GEOM_B)[3] >> np.uint32(30)).astype(np.int32))
    assert set(geom[:, 3].tolist()) == {0, 1, 2, 3}
    assert not R.geom_array(seed, step, GEOM_B, dihedral=False)[:, 3].any()


@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_coverage_at_b_4095(seed, step):
    """Every (flip, rot) occurs with every top, and with every left: two 8 x 9 tables (the 648 joint cells cannot all be hit)."""
    flip, top, left, rot = R.geom_array(seed, step, GEOM_B).T
    for off in (top, left):
        table = np.zeros((8, 9), np.int64)
        np.add.at(table, (flip * 4 + rot, off), 1)
        assert (table > 0).all(), table
    # and the coded images tell every (n, flip, top, left, rot) apart at the centred crop
    neigh = [R.window_neighbourhood(im, 4) for im in coded_bands()]
    assert len({R.integer_image(nb, HW, (f, 4, 4, r)).tobytes() for nb in neigh for f in (0, 1) for r in range(4)}) == 24


def test_bilinear_warp_of_a_ramp():
    """I = 3 x + 5 y is reproduced exactly by bilinear interpolation, so the sampled value tells where the sample was taken: the
    centre is (P - 1) / 2, and positive theta turns the content counter-clockwise."""
    m = MARGIN
    yy, xx = np.mgrid[-m:P + m, -m:P + m]
    ext = (3.0 * xx + 5.0 * yy)[None]
    theta, sigma = np.deg2rad(10.0), 1.05
    a, b = np.float32(np.cos(theta) / sigma), np.float32(np.sin(theta) / sigma)
    big_x, big_y = R.sample_positions(P, a, b)
    val, inner = R.bilinear64(ext, m, big_x, big_y)
    assert np.allclose(val[0], 3.0 * big_x.astype(np.float64) + 5.0 * big_y.astype(np.float64), rtol=0, atol=1e-9)
    c = (P - 1) / 2
    y, x = np.mgrid[0:P, 0:P]
    want_x = float(a) * (x - c) - float(b) * (y - c) + c
    want_y = float(b) * (x - c) + float(a) * (y - c) + c
    assert np.abs(big_x - want_x).max() < 1e-5 and np.abs(big_y - want_y).max() < 1e-5
    assert inner.any() and not inner.all()
    # direction: a bright pixel right of the centre ends up above it (smaller y) after a counter-clockwise turn
    img = np.zeros((1, P, P))
    img[0, 8, 13] = 1.0
    ext = np.pad(img, ((0, 0), (m, m), (m, m)))
    val, _ = R.bilinear64(ext, m, *R.sample_positions(P, np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))))
    yb, xb = np.unravel_index(val[0].argmax(), (P, P))
    assert yb < 8 and xb >= 11


def test_explicit_quarter_turn_is_rot_1():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 10001, (3, P, P)).astype(np.uint16)
    neigh = [R.window_neighbourhood(img, MARGIN + 4)]
    for geom in [(0, 4, 4, 0), (1, 2, 7, 3), (0, 8, 0, 2)]:
        turned = (geom[0], geom[1], geom[2], (geom[3] + 1) % 4)
        got = R.transform(neigh, P, [geom], 1.0, [(0.0, 1.0)], MARGIN)
        assert np.array_equal(got, R.transform(neigh, P, [turned], 1.0))
        assert np.array_equal(R.transform(neigh, P, [geom], 1.0, [(1.0, 0.0)], MARGIN), R.transform(neigh, P, [geom], 1.0))


@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_uniforms_stay_inside_their_ranges(seed, step):
    pol = R.Policy(**FULL)
    theta, sigma, g = R.image_draws(seed, step, GEOM_B, pol)
    assert theta.dtype == sigma.dtype == g.dtype == np.float32
    one, ulp = np.float32(1), 2.0 ** -23                            # [lo, hi) up to the rounding of the last fma

    def inside(v, lo, hi, fill):
        """All of v in [lo, hi + ulp], and its extremes within `fill` of the range's width from both ends."""
        lo, hi = float(lo), float(hi)
        return lo <= v.min() < lo + fill * (hi - lo) and hi - fill * (hi - lo) < v.max() <= hi + ulp * max(1.0, abs(hi))

    assert inside(theta, -pol.rotate, pol.rotate, 0.05)
    assert inside(sigma, one - pol.scale, one + pol.scale, 0.05)
    assert inside(g, one - pol.gain, one + pol.gain, 0.05)
    gains, offs = R.band_draws(seed, step, GEOM_B, 13, pol)
    assert inside(gains, one - pol.band_gain, one + pol.band_gain, 0.05)
    assert inside(offs, -pol.offset, pol.offset, 0.05)
    # the draws of different bands, of gains and offsets, and of different images are different words (n = 53235 values among the
    # m = 2.5 million fp32 numbers of [0.9, 1.1) meet by chance in about n / 2m = 1.1 % of the cases; repeated words would halve n)
    assert len(np.unique(gains)) > 0.98 * gains.size and len(np.unique(offs)) > 0.98 * offs.size
    assert abs(np.corrcoef(gains.reshape(-1), offs.reshape(-1))[0, 1]) < 0.02
    ab = R.affine_array(seed, step, GEOM_B, pol)
    assert np.allclose(np.hypot(ab[:, 0], ab[:, 1]), 1.0 / sigma, rtol=1e-6)
    assert np.allclose(np.degrees(np.arctan2(ab[:, 1], ab[:, 0])), theta, atol=1e-4)
    # a zero range gives the neutral value exactly
    off = R.Policy()
    th0, sg0, g0 = R.image_draws(seed, step, 64, off)
    gc0, oc0 = R.band_draws(seed, step, 64, 5, off)
    assert not th0.any() and (sg0 == 1).all() and (g0 == 1).all() and (gc0 == 1).all() and not oc0.any()


def test_the_three_call_families_never_share_a_philox_input():
    """Geometric, noise and policy calls differ in their keys for every seed, so no counter of one can meet one of another."""
    for seed in (0, 3, 2 ** 40 + 7, 2 ** 64 - 1):
        lo, hi = S._split(seed)
        keys = {(lo, hi), (lo, ~hi & 0xFFFFFFFF), (~lo & 0xFFFFFFFF, hi)}
        assert len(keys) == 3
    assert len({R.TAG_IMAGE, R.TAG_GAIN, R.TAG_OFFSET}) == 3 and max(R.TAG_IMAGE, R.TAG_GAIN, R.TAG_OFFSET) < 1 << 16


def test_affine_cases_cover_both_crops_and_dtypes():
    assert {(c, d) for c, d, _ in AFFINE_CASES} == {(c, d) for c in ("window", "scene") for d in ("uint16", "float32")}
