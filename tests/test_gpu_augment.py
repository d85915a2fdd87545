"""The augmentation policy of the staging calls (`eae_amd.Augment`; include/eae.h, "augmentation policy") against its NumPy
restatement (augment_ref.py): `augment_batch`, `stage_bands`, `stage_scene_windows` and `SceneLoader`.

  a. the quarter turn drawn in Philox mode, bit for bit, at B = 4095 on position-coded 12 x 12 images;
  b. explicit (flip, top, left, rot): all of D4 times a few crops, bit for bit, for every source and both scene crops;
  c. gain and offset: explicit, and the Philox draws at C = 1, 4, 5, 13, 16, bit for bit;
  d. explicit (a, b): within 8 x 2^-24 x max|raw| / divisor of the float64 bilinear value at the reference's fp32 fractions;
  e. (a, b) drawn in Philox mode against the explicit call with the reference's (a, b);
  f. the images do not depend on where in a scene the window lies;
  g. no policy, an all-zero policy and train=False are the plain calls; an id out of range gives a NaN image at its position only;
  h. `SceneLoader(augment=)`;  i. `fit_autoencoder` from such loaders.

The conditions (a) relies on -- every (flip, rot) occurs with every top and with every left at B = 4095 -- are asserted on the
reference alone in test_augment_reference.py, which imports the cases below.

Bound of (d).  lerp(p, q, t) = fma(t, fl(q - p), p) has two roundings of at most half an ulp of 2 max|raw| and of max|raw|: 1.5 x
2^-24 max|raw|.  The two lerps along x enter the one along y with weights that sum to 1, which adds its own 1.5, and the division half
an ulp more: below 4 x 2^-24 max|raw| / divisor, doubled to 8.  A wrong tap on coded data misses by a code step, 2^24 / 8 times that.

Deviation of (e).  The drawn (a, b) differ from the reference's float64 ones by the device's sincosf and division, and a sample
moves with them.  AFFINE_DEV_MEASURED = 1.860e-6 is the largest |Philox-mode value - explicit-call value| / (max|raw| / divisor) over
AFFINE_CASES measured on an MI355X (per case 1.20e-6 .. 1.86e-6); the bound is 8 x that, 1.488e-5, and must stay below
AFFINE_BOUND_CAP = 1e-3 of the value range (a wrong word, sign or centre moves samples by a fraction of a pixel: orders of
magnitude more on these random scenes)."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as R
import stage_ref as S

pytestmark = pytest.mark.gpu

SEED_STEPS = [(3, 5), (0, 0), (2 ** 40 + 7, 2 ** 33 + 1)]
HW = 12                             # square, >= 9: every offset 0..8 moves real pixels; 144 pixels: the draws are made per thread
GEOM_B = 4095                       # 4095 * 144 pixels: the last workgroup of 256 is partial
GEOM_N = 3
NOISE_STD = 0.03
CROPS = [(0, 0), (8, 8), (4, 8), (2, 5), (4, 4)]
FULL = dict(dihedral=True, rotate=12.0, scale=0.1, gain=0.2, band_gain=0.1, offset=0.05)
RADIO = dict(gain=0.2, band_gain=0.1, offset=0.05)
MARGIN = 16                         # of the reference's extended image: rotations up to 12 degrees, scales down to 0.9, P <= 16

AFFINE_CASES = [("window", "uint16", 0), ("scene", "uint16", 1), ("scene", "float32", 2), ("window", "float32", 0)]
AFFINE_DEV_MEASURED = 1.860e-6      # MI355X, ROCm 7: 1.20e-6 .. 1.86e-6 over AFFINE_CASES, the largest at the third case
AFFINE_BOUND_CAP = 1e-3


# ---------------------------------------------------------------------------------------------------- inputs
def coded_bands():
    """uint16 [3,1,12,12], data[n,0,y,x] = 1 + 144 n + 12 y + x: every (n, flip, top, left, rot) gives another output."""
    return (1 + np.arange(GEOM_N * HW * HW)).reshape(GEOM_N, 1, HW, HW).astype(np.uint16)


def coded_hwc(b):
    """uint8 HWC [b,12,12,3] with (y, x, b % 251) in the three channels."""
    u8 = np.empty((b, HW, HW, 3), np.uint8)
    u8[..., 0] = np.arange(HW)[None, :, None]
    u8[..., 1] = np.arange(HW)[None, None, :]
    u8[..., 2] = (np.arange(b) % 251)[:, None, None]
    return u8


def d4_geom():
    """int32 [40,4]: the eight (flip, rot) times CROPS."""
    return np.array([(f, t, le, r) for f in (0, 1) for r in range(4) for t, le in CROPS], np.int32)


def _dev_uint(a):
    return torch.from_numpy(a.astype(np.int32)).to(torch.uint16 if a.dtype == np.uint16 else torch.uint8).cuda()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _window_ref(imgs, geom, div, affine=None):
    """`augment_ref.transform` of planar images [B,C,P,P] (zeros around each)."""
    e = MARGIN + 4
    return R.transform([R.window_neighbourhood(im, e) for im in imgs], imgs.shape[-1], geom, div, affine, MARGIN)


def _assert_images_equal(got, ref, geom):
    if np.array_equal(got, ref):
        return
    bad = np.nonzero((got != ref).reshape(len(ref), -1).any(axis=1))[0]
    b = int(bad[0])
    pytest.fail(f"{len(bad)} of {len(ref)} batch positions differ; the first is b = {b}, whose reference (flip, top, left, rot) is "
                f"{tuple(int(v) for v in geom[b])}")


@functools.lru_cache(maxsize=None)
def _scene_case(dtype):
    """Case "D" of test_gpu_scene_train.py (C = 5, 37 x 41, P = 16, S = 5), as uint16 or with fp32 values: scene (device), its NumPy
    copy, divisor, P, S, grid, 10 window ids with the four corners."""
    import eae_amd
    from scene_util import _scene, _divisor
    from test_gpu_scene_train import CASES, _ids
    c, h, w, _, p, s, grid = CASES["D"]
    td = {"uint16": torch.uint16, "float32": torch.float32}[dtype]
    scene = _scene(c, h, w, td, seed=ord("D"))
    assert eae_amd.window_grid(h, w, p, s, any_patch=True) == grid
    n_h, n_w = grid
    n = n_h * n_w
    ids = [0, n_w - 1, (n_h - 1) * n_w, n - 1] + _ids(n, 6, seed=8)
    arr = _np(scene)
    arr.setflags(write=False)
    return scene, arr, _divisor(c, td), p, s, grid, ids


def _scene_neighs(arr, ids, n_w, p, s, crop):
    e = MARGIN + 4
    if crop == "scene":
        return [R.scene_neighbourhood(arr, (n // n_w) * s, (n % n_w) * s, p, e) for n in ids]
    return [R.window_neighbourhood(arr[:, (n // n_w) * s:(n // n_w) * s + p, (n % n_w) * s:(n % n_w) * s + p], e) for n in ids]


def _ids_dev(ids):
    return torch.tensor(ids, dtype=torch.int64, device="cuda")


# ---------------------------------------------------------------------------------------------------- a. D4 draws, Philox mode
@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_stage_bands_d4_draws(seed, step):
    import eae_amd
    data = coded_bands()
    idx = np.arange(GEOM_B) % GEOM_N
    geom = R.geom_array(seed, step, GEOM_B)
    neigh = [R.window_neighbourhood(im, 4) for im in data]
    ref = np.stack([R.integer_image(neigh[idx[b]], HW, geom[b]) for b in range(GEOM_B)]).astype(np.float32)
    got = eae_amd.stage_bands(_dev_uint(data), 1.0, index=torch.from_numpy(idx), noise_std=0.0, seed=seed, step=step,
                              augment=eae_amd.Augment(dihedral=True))
    assert got.shape == (GEOM_B, 1, HW, HW) and got.dtype == torch.float32
    _assert_images_equal(_np(got), ref, geom)
    # (flip, top, left) of a batch position are what they are without the policy: undo the turn
    plain = _np(eae_amd.stage_bands(_dev_uint(data), 1.0, index=torch.from_numpy(idx), noise_std=0.0, seed=seed, step=step))
    back = np.stack([np.rot90(g, -int(r), axes=(-2, -1)) for g, r in zip(_np(got), geom[:, 3])])
    assert np.array_equal(back, plain)


@pytest.mark.parametrize("seed,step", SEED_STEPS)
def test_augment_batch_d4_draws(seed, step):
    import eae_amd
    u8 = coded_hwc(GEOM_B)
    geom = R.geom_array(seed, step, GEOM_B)
    planar = R.hwc_windows(u8)
    ref = np.stack([R.integer_image(R.window_neighbourhood(planar[b], 4), HW, geom[b]) for b in range(GEOM_B)])
    ref = ref.astype(np.float32) / np.float32(255)
    got = eae_amd.augment_batch(torch.from_numpy(u8).cuda(), noise_std=0.0, seed=seed, step=step, augment=eae_amd.Augment(dihedral=True))
    assert got.shape == (GEOM_B, 3, HW, HW)
    _assert_images_equal(_np(got), ref, geom)


# ---------------------------------------------------------------------------------------------------- b. explicit geometry
@pytest.mark.parametrize("c,dtype", [(5, "uint8"), (13, "uint16"), (5, "uint16"), (13, "uint8")])
def test_stage_bands_explicit_geometry(c, dtype):
    import eae_amd
    geom = d4_geom()
    b = len(geom)
    hi = 256 if dtype == "uint8" else 10001
    data = np.random.default_rng(c).integers(1, hi, (b, c, HW, HW)).astype(np.dtype(dtype))
    div = np.linspace(2000, 12000, c).astype(np.float32)
    ref = _window_ref(data, geom, div).astype(np.float32)
    got = eae_amd.stage_bands(_dev_uint(data), div, noise_std=0.0, geom=_t(geom))
    _assert_images_equal(_np(got), ref, geom)
    assert len({_np(got[i * len(CROPS) + 4]).tobytes() for i in range(8)}) == 8          # the centred crops: eight different images


def test_augment_batch_explicit_geometry():
    import eae_amd
    geom = d4_geom()
    u8 = np.random.default_rng(7).integers(0, 256, (len(geom), HW, HW, 3)).astype(np.uint8)
    ref = _window_ref(R.hwc_windows(u8), geom, np.float32(255)).astype(np.float32)
    got = eae_amd.augment_batch(torch.from_numpy(u8).cuda(), noise_std=0.0, geom=_t(geom))
    _assert_images_equal(_np(got), ref, geom)


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("crop", ["window", "scene"])
def test_scene_explicit_geometry(crop, dtype):
    import eae_amd
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case(dtype)
    geom = d4_geom()[3::4][:len(ids)]
    assert len(geom) == len(ids) and len({(f, r) for f, _, _, r in geom.tolist()}) == 8
    ref = R.transform(_scene_neighs(arr, ids, n_w, p, s, crop), p, geom, div).astype(np.float32)
    got = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), noise_std=0.0, geom=_t(geom), crop=crop)
    _assert_images_equal(_np(got), ref, geom)


def test_scene_crops_are_stage_bands_on_cut_windows():
    """crop="window" is `stage_bands` on the materialised windows; crop="scene" is the window crop with (flip, 4, 4, rot) on the
    shifted windows cut from the scene zero-padded by 4 (the identity of include/eae.h), with noise."""
    import eae_amd
    from test_gpu_scene_train import _scene_crop_case, _cut, _noise
    scene, div, p, s, n_w, ids, params, wins, mask = _scene_crop_case("D")
    b = len(ids)
    rot = [(3 * i + 1) % 4 for i in range(b)]
    geom = torch.tensor([(f, t, le, r) for (f, t, le), r in zip(params, rot)], dtype=torch.int32)
    centred = torch.tensor([(f, 4, 4, r) for (f, _, _), r in zip(params, rot)], dtype=torch.int32)
    noise = _noise((b, scene.shape[0], p, p), seed=22)
    kw = dict(noise=noise, noise_std=NOISE_STD)
    plain = torch.from_numpy(_cut(_np(scene), ids, n_w, p, s)).cuda()
    got_w = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), geom=geom, **kw)
    assert torch.equal(got_w, eae_amd.stage_bands(plain, div, geom=geom, **kw))
    got_s = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), geom=geom, crop="scene", **kw)
    assert (mask.reshape(b, -1) == 0).any(axis=1).sum() >= 1
    assert torch.equal(got_s, eae_amd.stage_bands(torch.from_numpy(wins).cuda(), div, geom=centred, **kw))
    assert not torch.equal(got_s, got_w)


# ---------------------------------------------------------------------------------------------------- c. radiometric
def test_explicit_radio_then_noise():
    import eae_amd
    rng = np.random.default_rng(41)
    geom = d4_geom()[::5]
    b, c = len(geom), 5
    data = rng.integers(1, 10001, (b, c, HW, HW)).astype(np.uint16)
    div = np.linspace(2000, 12000, c).astype(np.float32)
    radio = np.stack([rng.uniform(0.7, 1.3, (b, c)), rng.uniform(-0.1, 0.1, (b, c))], 2).astype(np.float32)
    noise = rng.standard_normal((b, c, HW, HW)).astype(np.float32)
    base = _window_ref(data, geom, div).astype(np.float32)
    ref = S.add_noise(R.apply_radio(base, radio), noise, NOISE_STD)
    got = eae_amd.stage_bands(_dev_uint(data), div, geom=_t(geom), radio=_t(radio), noise=_t(noise), noise_std=NOISE_STD)
    assert np.array_equal(_np(got), ref)
    u8 = rng.integers(0, 256, (b, HW, HW, 3)).astype(np.uint8)
    base = _window_ref(R.hwc_windows(u8), geom, np.float32(255)).astype(np.float32)
    ref = S.add_noise(R.apply_radio(base, radio[:, :3]), noise[:, :3], NOISE_STD)
    got = eae_amd.augment_batch(torch.from_numpy(u8).cuda(), geom=_t(geom), radio=_t(radio[:, :3]), noise=_t(noise[:, :3]),
                                noise_std=NOISE_STD)
    assert np.array_equal(_np(got), ref)


@pytest.mark.parametrize("c,pair", [(1, 0), (4, 1), (5, 2), (13, 0), (16, 2)])
def test_radiometric_draws(c, pair):
    import eae_amd
    seed, step = SEED_STEPS[pair]
    b = 9
    pol = R.Policy(**RADIO)
    data = np.random.default_rng(c + 50).integers(1, 10001, (b, c, HW, HW)).astype(np.uint16)
    div = np.linspace(2000, 12000, c).astype(np.float32)
    radio = R.radio_array(seed, step, b, c, pol)
    assert len(np.unique(radio[:, :, 0])) == b * c and len(np.unique(radio[:, :, 1])) == b * c
    ref = R.apply_radio(S.stage_transform(data, S.stage_params(seed, step, b), div), radio)
    got = eae_amd.stage_bands(_dev_uint(data), div, noise_std=0.0, seed=seed, step=step, augment=eae_amd.Augment(**pol.kwargs()))
    assert np.array_equal(_np(got), ref)
    # one part of the policy at a time draws the same values as all three together
    for part in ("gain", "band_gain", "offset"):
        one = R.Policy(**{part: RADIO[part]})
        ref = R.apply_radio(S.stage_transform(data, S.stage_params(seed, step, b), div), R.radio_array(seed, step, b, c, one))
        got = eae_amd.stage_bands(_dev_uint(data), div, noise_std=0.0, seed=seed, step=step, augment=eae_amd.Augment(**one.kwargs()))
        assert np.array_equal(_np(got), ref), part


def test_radiometric_draws_augment_batch_and_scene():
    import eae_amd
    seed, step = SEED_STEPS[2]
    pol = R.Policy(**RADIO)
    u8 = np.random.default_rng(43).integers(0, 256, (5, HW, HW, 3)).astype(np.uint8)
    ref = R.apply_radio(S.stage_transform_hwc(u8, S.stage_params(seed, step, 5)), R.radio_array(seed, step, 5, 3, pol))
    got = eae_amd.augment_batch(torch.from_numpy(u8).cuda(), noise_std=0.0, seed=seed, step=step, augment=eae_amd.Augment(**RADIO))
    assert np.array_equal(_np(got), ref)
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case("uint16")
    b = len(ids)
    kw = dict(noise_std=NOISE_STD, seed=seed, step=step, crop="scene")
    base = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), **dict(kw, noise_std=0.0))
    z = _np(eae_amd.stage_scene_windows(torch.zeros_like(scene), 1.0, p, s, _ids_dev(ids), **dict(kw, noise_std=1.0)))
    ref = S.add_noise(R.apply_radio(_np(base), R.radio_array(seed, step, b, scene.shape[0], pol)), z, NOISE_STD)
    got = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), augment=eae_amd.Augment(**RADIO), **kw)
    assert np.array_equal(_np(got), ref)


# ---------------------------------------------------------------------------------------------------- d. affine, explicit (a, b)
def _affine_cases(b):
    """float32 [b,2]: rotations of -12 .. 12 degrees with scales 0.9 .. 1.1."""
    th = np.deg2rad(np.linspace(-12, 12, b))
    sg = np.linspace(0.9, 1.1, b)[::-1]
    return np.stack([np.cos(th) / sg, np.sin(th) / sg], 1).astype(np.float32)


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
@pytest.mark.parametrize("crop", ["window", "scene"])
def test_scene_explicit_affine(crop, dtype):
    import eae_amd
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case(dtype)
    geom = d4_geom()[3::4][:len(ids)]
    affine = _affine_cases(len(ids))
    ref = R.transform(_scene_neighs(arr, ids, n_w, p, s, crop), p, geom, div, affine, MARGIN)
    got = _np(eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), noise_std=0.0, geom=_t(geom), affine=_t(affine), crop=crop))
    bound = 8 * 2.0 ** -24 * float(np.abs(arr).max()) / np.asarray(div, np.float64)
    err = np.abs(got.astype(np.float64) - ref).max(axis=(0, 2, 3))
    print(f"affine {crop} {dtype}: largest error / bound per band {np.round(err / bound, 3).tolist()}")
    assert (err <= bound).all()
    assert np.abs(got - R.transform(_scene_neighs(arr, ids, n_w, p, s, crop), p, geom, div)).max() > 1e-3       # and it does turn


def test_stage_bands_explicit_affine():
    import eae_amd
    geom = d4_geom()[::3][:12]
    b, c = len(geom), 5
    data = np.random.default_rng(44).integers(1, 10001, (b, c, HW, HW)).astype(np.uint16)
    div = np.linspace(2000, 12000, c).astype(np.float32)
    affine = _affine_cases(b)
    ref = _window_ref(data, geom, div, affine)
    got = _np(eae_amd.stage_bands(_dev_uint(data), div, noise_std=0.0, geom=_t(geom), affine=_t(affine)))
    bound = 8 * 2.0 ** -24 * 10000.0 / div.astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref).max(axis=(0, 2, 3)) <= bound).all()
    u8 = np.random.default_rng(45).integers(0, 256, (b, HW, HW, 3)).astype(np.uint8)
    ref = _window_ref(R.hwc_windows(u8), geom, np.float32(255), affine)
    got = _np(eae_amd.augment_batch(torch.from_numpy(u8).cuda(), noise_std=0.0, geom=_t(geom), affine=_t(affine)))
    assert np.abs(got.astype(np.float64) - ref).max() <= 8 * 2.0 ** -24


@pytest.mark.parametrize("crop", ["window", "scene"])
def test_affine_identity_and_quarter_turn(crop):
    import eae_amd
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case("uint16")
    b = len(ids)
    geom = d4_geom()[3::4][:b]
    args = (scene, div, p, s, _ids_dev(ids))
    kw = dict(noise_std=0.0, crop=crop)
    plain = eae_amd.stage_scene_windows(*args, geom=_t(geom), **kw)
    ident = torch.tensor([(1.0, 0.0)] * b)
    assert torch.equal(eae_amd.stage_scene_windows(*args, geom=_t(geom), affine=ident, **kw), plain)
    # (a, b) = (0, 1) is one more quarter turn: exact, every tap fraction being 0
    turned = geom.copy()
    turned[:, 3] = (turned[:, 3] + 1) % 4
    quarter = torch.tensor([(0.0, 1.0)] * b)
    assert torch.equal(eae_amd.stage_scene_windows(*args, geom=_t(geom), affine=quarter, **kw),
                       eae_amd.stage_scene_windows(*args, geom=_t(turned), **kw))


# ---------------------------------------------------------------------------------------------------- e. affine, Philox mode
@pytest.mark.parametrize("crop,dtype,pair", AFFINE_CASES)
def test_affine_philox_mode(crop, dtype, pair):
    """Largest |Philox-mode value - explicit call with the reference's (a, b)| over the value range, measured on an MI355X over
    AFFINE_CASES: 1.860e-6 (AFFINE_DEV_MEASURED); the bound is 8 x that, 1.488e-5, under the cap of 1e-3."""
    import eae_amd
    seed, step = SEED_STEPS[pair]
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case(dtype)
    b = 4 * len(ids)
    ids = ids * 4
    pol = R.Policy(dihedral=True, rotate=12.0, scale=0.1)
    affine = R.affine_array(seed, step, b, pol)
    assert np.abs(affine[:, 1]).max() > 0.1 and np.ptp(np.hypot(affine[:, 0], affine[:, 1])) > 0.1
    args = (scene, div, p, s, _ids_dev(ids))
    got = eae_amd.stage_scene_windows(*args, noise_std=0.0, seed=seed, step=step, crop=crop, augment=eae_amd.Augment(**pol.kwargs()))
    ref = eae_amd.stage_scene_windows(*args, noise_std=0.0, crop=crop, geom=_t(R.geom_array(seed, step, b)), affine=_t(affine))
    scale = float(np.abs(arr).max()) / np.asarray(div, np.float64)
    dev = float((np.abs(_np(got).astype(np.float64) - _np(ref)).max(axis=(0, 2, 3)) / scale).max())
    print(f"affine deviation {crop} {dtype} seed={seed} step={step}: {dev:.3e} of the value range")
    bound = 8 * AFFINE_DEV_MEASURED
    assert bound <= AFFINE_BOUND_CAP
    assert dev <= bound


# ---------------------------------------------------------------------------------------------------- f. origin independence
def test_images_do_not_depend_on_the_window_origin():
    import eae_amd
    p, s, sur = 16, 4, 12
    rng = np.random.default_rng(46)
    arr = rng.integers(0, 10001, (1, p + 2 * sur, 3100)).astype(np.uint16)
    block = rng.integers(0, 10001, (p + 2 * sur, p + 2 * sur)).astype(np.uint16)
    far = 2988                                                     # the far window starts at column 3000
    arr[0, :, :p + 2 * sur] = block
    arr[0, :, far:far + p + 2 * sur] = block
    scene = _dev_uint(arr)
    n_w = (3100 - p) // s + 1
    row = sur // s
    ids = [row * n_w + sur // s, row * n_w + (far + sur) // s] * 8
    b = len(ids)
    geom = np.repeat(d4_geom()[3::5], 2, axis=0)[:b]
    affine = np.repeat(_affine_cases(8), 2, axis=0)
    radio = np.repeat(rng.uniform(0.8, 1.2, (8, 1, 2)), 2, axis=0).astype(np.float32)
    noise = np.repeat(rng.standard_normal((8, 1, p, p)), 2, axis=0).astype(np.float32)
    got = eae_amd.stage_scene_windows(scene, 10000.0, p, s, _ids_dev(ids), crop="scene", geom=_t(geom), affine=_t(affine),
                                      radio=_t(radio), noise=_t(noise), noise_std=NOISE_STD, augment=eae_amd.Augment(**FULL))
    assert torch.equal(got[0::2], got[1::2])
    assert len({_np(g).tobytes() for g in got[0::2]}) == 8


# ---------------------------------------------------------------------------------------------------- g. off means off
def test_no_policy_is_the_plain_call():
    """Plain and no-policy calls run the same kernel (but for the scene), so the plain result is also anchored: to the NumPy restatement (stage_ref.py)
    with the draws of `stage_params`, and train=False to the division alone."""
    import eae_amd
    rng = np.random.default_rng(47)
    full = eae_amd.Augment(**FULL)
    data_np = rng.integers(0, 10001, (6, 5, HW, HW)).astype(np.uint16)
    u8_np = rng.integers(0, 256, (6, HW, HW, 3)).astype(np.uint8)
    data, u8 = _dev_uint(data_np), torch.from_numpy(u8_np).cuda()
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case("uint16")
    origins = [((n // n_w) * s, (n % n_w) * s) for n in ids]
    calls = [(lambda **kw: eae_amd.stage_bands(data, 10000.0, **kw), lambda g: S.stage_transform(data_np, g, 10000.0)),
             (lambda **kw: eae_amd.augment_batch(u8, **kw), lambda g: S.stage_transform_hwc(u8_np, g)),
             (lambda **kw: eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), crop="scene", **kw),
              lambda g: S.scene_transform(arr, origins, p, g, div, "scene")),
             (lambda **kw: eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), **kw),
              lambda g: S.scene_transform(arr, origins, p, g, div, "window"))]
    for call, ref in calls:
        plain = call(seed=9, step=4)
        assert torch.equal(call(seed=9, step=4, augment=None), plain)
        assert torch.equal(call(seed=9, step=4, augment=eae_amd.Augment()), plain)
        assert not torch.equal(call(seed=9, step=4, augment=full), plain)
        assert torch.equal(call(seed=9, step=4, train=False, augment=full), call(train=False))
        b = len(plain)
        assert np.array_equal(_np(call(seed=9, step=4, noise_std=0.0)), ref(S.stage_params(9, 4, b)))
        assert np.array_equal(_np(call(seed=9, step=4, train=False, augment=full)), ref(np.array([(0, 4, 4)] * b)))


@pytest.mark.parametrize("crop", ["window", "scene"])
def test_out_of_range_ids_give_nan_images_with_the_policy(crop):
    import eae_amd
    scene, arr, div, p, s, (n_h, n_w), good = _scene_case("uint16")
    n = n_h * n_w
    ids = [good[0], -1, good[1], good[2], n, good[3]]
    kw = dict(seed=77, step=3, noise_std=NOISE_STD, crop=crop, augment=eae_amd.Augment(**FULL))
    got = eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), **kw)
    keep = [0, 2, 3, 5]
    assert torch.isnan(got[1]).all() and torch.isnan(got[4]).all() and not torch.isnan(got[keep]).any()
    ids_ok = list(ids)
    ids_ok[1], ids_ok[4] = good[0], good[1]
    assert torch.equal(got[keep], eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids_ok), **kw)[keep])
    data = _dev_uint(np.random.default_rng(48).integers(1, 10001, (4, 5, HW, HW)).astype(np.uint16))
    idx, idx_ok = [0, -1, 2, 4, 1, 2 ** 40], [0, 3, 2, 1, 1, 0]
    kw.pop("crop")
    got = eae_amd.stage_bands(data, 10000.0, index=torch.tensor(idx), **kw)
    assert torch.isnan(got[[1, 3, 5]]).all() and not torch.isnan(got[[0, 2, 4]]).any()
    assert torch.equal(got[[0, 2, 4]], eae_amd.stage_bands(data, 10000.0, index=torch.tensor(idx_ok), **kw)[[0, 2, 4]])


def test_draw_placement_does_not_change_the_values():
    """The per-image draws made by every thread and made once per workgroup through LDS are the same words."""
    import eae_amd
    scene, arr, div, p, s, (n_h, n_w), ids = _scene_case("uint16")
    ids = ids + ids[:3]                                            # 13 images of 256 pixels
    outs = [eae_amd.stage_scene_windows(scene, div, p, s, _ids_dev(ids), seed=5, step=6, crop="scene",
                                        augment=eae_amd.Augment(_draw_mode=m, **FULL)) for m in (0, 1, 2)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    data = _dev_uint(np.random.default_rng(49).integers(1, 10001, (7, 13, 20, 20)).astype(np.uint16))      # 400 pixels: two images a workgroup
    outs = [eae_amd.stage_bands(data, 10000.0, seed=5, step=6, augment=eae_amd.Augment(_draw_mode=m, **FULL)) for m in (0, 1, 2)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


# ---------------------------------------------------------------------------------------------------- h. SceneLoader
def _labelled_a():
    from test_gpu_scene_train import _labelled_a as base
    return base()


def test_scene_loader_batches_with_a_policy():
    import eae_amd
    scene, div, p, s, label, purity = _labelled_a()
    pol = eae_amd.Augment(**FULL)
    loader = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=4, seed=5, noise_std=0.05, crop="scene",
                                 augment=pol)
    plain = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=4, seed=5, noise_std=0.05, crop="scene")
    for e in (0, 1):
        sched = loader.schedule(e)
        batches, ordinary = list(loader), list(plain)
        assert len(batches) == len(sched) == 2
        for i, (x, y) in enumerate(batches):
            ids = loader.windows[sched[i].cuda()]
            ref = eae_amd.stage_scene_windows(scene, div, p, s, ids, seed=5, step=e * 2 + i, noise_std=0.05, crop="scene", augment=pol)
            assert torch.equal(x, ref) and torch.equal(y, label.reshape(-1)[ids])
            assert torch.equal(y, ordinary[i][1]) and not torch.equal(x, ordinary[i][0])


def test_scene_loader_epoch_with_a_policy_does_not_synchronise():
    """torch's sync debug mode raises on a synchronising call (the control below shows that it does here)."""
    import warnings
    import eae_amd
    scene, div, p, s, label, purity = _labelled_a()
    loader = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=2, crop="scene", seed=1,
                                 augment=eae_amd.Augment(**FULL))
    ref = [(x.clone(), y.clone()) for x, y in loader]              # epoch 0, also the warm-up
    loader.set_epoch(0)
    torch.cuda.synchronize()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.cuda.set_sync_debug_mode("error")
    try:
        got = list(loader)
        with pytest.raises(RuntimeError):
            got[0][0][0, 0, 0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(got) == len(ref) == 3 and all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(got, ref))


# ---------------------------------------------------------------------------------------------------- i. fit
def test_fit_autoencoder_from_loaders_with_a_policy():
    import eae_amd
    from scene_util import _scene
    scene = _scene(3, 128, 128, torch.uint8, seed=50)
    r = np.random.default_rng(51).integers(0, 10, (128, 128)).astype(np.uint8)
    label, purity, _ = eae_amd.window_labels(torch.from_numpy(r).cuda(), 64, 32, 10)

    def fit():
        kw = dict(divisor=255.0, patch=64, stride=32, batch_size=8, seed=2)
        train = eae_amd.SceneLoader(scene, label, train=True, crop="scene", augment=eae_amd.Augment(**FULL), **kw)
        val = eae_amd.SceneLoader(scene, label, train=False, **kw)
        torch.manual_seed(0)
        return eae_amd.fit_autoencoder(train, val, alpha=30, lr=1e-3, num_epochs=2, verbose=False)

    a, b = fit(), fit()
    assert a["epochs"] == b["epochs"] == 2
    assert np.isfinite(a["train_curve"]).all() and np.isfinite(a["val_curve"]).all()
    assert a["train_curve"] == b["train_curve"] and a["val_curve"] == b["val_curve"]
    sa, sb = a["model"].state_dict(), b["model"].state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
