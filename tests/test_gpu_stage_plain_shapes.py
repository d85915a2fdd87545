"""Plain staging calls (no policy) at the shapes where the one staging kernel (csrc/eae_stage.hip) can go wrong, bit for bit against
the NumPy restatement (stage_ref.py) with noise_std = 0 and the geometric draws of the Philox stream:

  12 x 20  240 pixels: several images per workgroup;
  16 x 16  256 pixels: one image per workgroup, the size from which a policy's draws go through LDS;
  13 x 20  260 pixels: every workgroup straddles two images, the last is partial;
   9 x 40  360 pixels: not square;

through `augment_batch` (C = 3), `stage_bands` (C = 5 uint16, C = 16 uint8, an index that repeats and permutes) and
`stage_scene_windows` (both crops, uint16 and fp32, P = 16 and P = 12), B = 5.  Also explicit `params` [B,3] with pairwise different
rows (a table read with another stride is wrong from b = 1 on), `train=False` (the division only, whatever seed, step and noise_std
say) and explicit `noise` as one fma."""
import numpy as np
import pytest
import torch

import stage_ref as S

pytestmark = pytest.mark.gpu

B = 5
SHAPES = [(12, 20), (16, 16), (13, 20), (9, 40)]
SEED_STEPS = [(11, 2), (2 ** 40 + 7, 2 ** 33 + 1)]
PARAMS5 = np.array([(0, 0, 0), (1, 8, 8), (1, 0, 8), (0, 8, 0), (1, 4, 2)], np.int32)        # both flips, offsets 0 and 8
CENTRED = np.array([(0, 4, 4)] * B, np.int32)                                                 # train=False
INDEX = [3, 0, 3, 1, 2]
BANDS = [(np.uint16, 5), (np.uint8, 16)]
SCENE_HW, SCENE_S = (37, 41), 5
NOISE_STD = 0.03


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev(a):
    """A NumPy array on the device; uint16 by way of int32."""
    return _t(a.astype(np.int32)).to(torch.uint16) if a.dtype == np.uint16 else _t(a)


def _hwc(h, w):
    return np.random.default_rng(h * 100 + w).integers(0, 256, (B, h, w, 3)).astype(np.uint8)


def _bands(dtype, c, h, w):
    hi = 10001 if dtype == np.uint16 else 256
    data = np.random.default_rng(c * 10000 + h * 100 + w).integers(0, hi, (4, c, h, w)).astype(dtype)
    div = (np.float32(hi - 1) * (1 + 0.1 * np.arange(c))).astype(np.float32)
    return data, div


def _scene(dtype, p):
    """(scene [5,37,41], divisor, ids: the four corner windows and one inside, window columns) for P x P windows at stride 5."""
    h, w = SCENE_HW
    rng = np.random.default_rng(p)
    arr = rng.integers(0, 10001, (5, h, w)).astype(np.uint16) if dtype == np.uint16 else (rng.random((5, h, w)) * 3).astype(np.float32)
    div = ((10000.0 if dtype == np.uint16 else 1.5) * (1 + 0.1 * np.arange(5))).astype(np.float32)
    n_h, n_w = (h - p) // SCENE_S + 1, (w - p) // SCENE_S + 1
    ids = [0, n_h * n_w - 1, n_w - 1, (n_h - 1) * n_w, n_w + 2]
    return arr, div, ids, n_w


def _scene_ref(arr, div, ids, n_w, p, params, crop):
    return S.scene_transform(arr, [((n // n_w) * SCENE_S, (n % n_w) * SCENE_S) for n in ids], p, params, div, crop)


def _stage_scene(arr, div, ids, p, crop, **kw):
    import eae_amd
    return eae_amd.stage_scene_windows(_dev(arr), [float(d) for d in div], p, SCENE_S, torch.tensor(ids, dtype=torch.int64).cuda(),
                                       crop=crop, **kw).cpu().numpy()


def test_the_drawn_rows_differ():
    """What the Philox cases rely on: both flips occur and no two batch positions draw the same row."""
    for seed, step in SEED_STEPS:
        rows = S.params_array(seed, step, B)
        assert len({tuple(r) for r in rows}) == B and set(rows[:, 0]) == {0, 1}
    assert len({tuple(r) for r in PARAMS5}) == B


# ---------------------------------------------------------------------------------------------------- Philox geometry
@pytest.mark.parametrize("hw", SHAPES)
def test_augment_batch_philox(hw):
    import eae_amd
    u8 = _hwc(*hw)
    for seed, step in SEED_STEPS:
        got = eae_amd.augment_batch(_t(u8), seed=seed, step=step, noise_std=0.0).cpu().numpy()
        assert np.array_equal(got, S.stage_transform_hwc(u8, S.stage_params(seed, step, B)))


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("dtype,c", BANDS)
def test_stage_bands_philox(dtype, c, hw):
    import eae_amd
    data, div = _bands(dtype, c, *hw)
    for seed, step in SEED_STEPS:
        got = eae_amd.stage_bands(_dev(data), _t(div), index=torch.tensor(INDEX), seed=seed, step=step, noise_std=0.0).cpu().numpy()
        assert np.array_equal(got, S.stage_ref(data, INDEX, div, S.stage_params(seed, step, B), None, 0.0))


@pytest.mark.parametrize("p", [16, 12])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("crop", ["window", "scene"])
def test_stage_scene_windows_philox(crop, dtype, p):
    arr, div, ids, n_w = _scene(dtype, p)
    for seed, step in SEED_STEPS:
        got = _stage_scene(arr, div, ids, p, crop, seed=seed, step=step, noise_std=0.0)
        assert np.array_equal(got, _scene_ref(arr, div, ids, n_w, p, S.stage_params(seed, step, B), crop))


# ---------------------------------------------------------------------------------------------------- explicit params [B,3]
@pytest.mark.parametrize("hw", SHAPES)
def test_explicit_params_rows(hw):
    import eae_amd
    u8 = _hwc(*hw)
    got = eae_amd.augment_batch(_t(u8), params=_t(PARAMS5), noise_std=0.0, seed=11, step=2).cpu().numpy()
    assert np.array_equal(got, S.stage_transform_hwc(u8, PARAMS5))
    data, div = _bands(np.uint16, 5, *hw)
    got = eae_amd.stage_bands(_dev(data), _t(div), index=torch.tensor(INDEX), params=_t(PARAMS5), noise_std=0.0, seed=11, step=2)
    assert np.array_equal(got.cpu().numpy(), S.stage_ref(data, INDEX, div, PARAMS5, None, 0.0))


@pytest.mark.parametrize("p", [16, 12])
@pytest.mark.parametrize("crop", ["window", "scene"])
def test_explicit_params_rows_scene(crop, p):
    arr, div, ids, n_w = _scene(np.uint16, p)
    got = _stage_scene(arr, div, ids, p, crop, params=_t(PARAMS5), noise_std=0.0, seed=11, step=2)
    assert np.array_equal(got, _scene_ref(arr, div, ids, n_w, p, PARAMS5, crop))


# ---------------------------------------------------------------------------------------------------- train=False
@pytest.mark.parametrize("hw", [(16, 16), (13, 20)])
def test_eval_mode_is_the_division_only(hw):
    import eae_amd
    kw = dict(train=False, seed=11, step=2, noise_std=NOISE_STD)
    u8 = _hwc(*hw)
    assert np.array_equal(eae_amd.augment_batch(_t(u8), **kw).cpu().numpy(), S.stage_transform_hwc(u8, CENTRED))
    for dtype, c in BANDS:
        data, div = _bands(dtype, c, *hw)
        got = eae_amd.stage_bands(_dev(data), _t(div), index=torch.tensor(INDEX), **kw).cpu().numpy()
        assert np.array_equal(got, S.stage_ref(data, INDEX, div, CENTRED, None, 0.0))
    # explicit draws are ignored too
    got = eae_amd.stage_bands(_dev(data), _t(div), index=torch.tensor(INDEX), params=_t(PARAMS5),
                              noise=torch.ones((B, c) + hw).cuda(), **kw).cpu().numpy()
    assert np.array_equal(got, S.stage_ref(data, INDEX, div, CENTRED, None, 0.0))


@pytest.mark.parametrize("crop", ["window", "scene"])
def test_eval_mode_is_the_division_only_scene(crop):
    for dtype in (np.uint16, np.float32):
        arr, div, ids, n_w = _scene(dtype, 16)
        got = _stage_scene(arr, div, ids, 16, crop, train=False, seed=11, step=2, noise_std=NOISE_STD)
        assert np.array_equal(got, _scene_ref(arr, div, ids, n_w, 16, CENTRED, crop))


# ---------------------------------------------------------------------------------------------------- explicit noise
def test_explicit_noise_is_one_fma():
    import eae_amd
    h, w = 13, 20
    seed, step = SEED_STEPS[0]
    drawn = S.stage_params(seed, step, B)
    rng = np.random.default_rng(5)
    u8 = _hwc(h, w)
    noise = rng.standard_normal((B, 3, h, w)).astype(np.float32)
    got = eae_amd.augment_batch(_t(u8), seed=seed, step=step, noise=_t(noise), noise_std=NOISE_STD).cpu().numpy()
    assert np.array_equal(got, S.add_noise(S.stage_transform_hwc(u8, drawn), noise, NOISE_STD))
    for dtype, c in BANDS:
        data, div = _bands(dtype, c, h, w)
        noise = rng.standard_normal((B, c, h, w)).astype(np.float32)
        got = eae_amd.stage_bands(_dev(data), _t(div), index=torch.tensor(INDEX), seed=seed, step=step, noise=_t(noise),
                                  noise_std=NOISE_STD).cpu().numpy()
        assert np.array_equal(got, S.stage_ref(data, INDEX, div, drawn, noise, NOISE_STD))
    arr, div, ids, n_w = _scene(np.uint16, 16)
    noise = rng.standard_normal((B, 5, 16, 16)).astype(np.float32)
    got = _stage_scene(arr, div, ids, 16, "scene", seed=seed, step=step, noise=_t(noise), noise_std=NOISE_STD)
    assert np.array_equal(got, S.add_noise(_scene_ref(arr, div, ids, n_w, 16, drawn, "scene"), noise, NOISE_STD))
