"""Training from a scene on the device (eae_amd.scene): `stage_scene_windows` against `scene_windows` and against `stage_bands` on
windows cut on the host (explicit draws and the shared Philox stream, both crop modes), `window_labels` against a NumPy bincount
oracle, the batches of a `SceneLoader`, and one epoch of `fit_autoencoder` fed by loaders and by the same batches as plain lists.
Every comparison is bitwise."""

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import _stream, _ptr
from scene_util import _scene, _divisor

pytestmark = pytest.mark.gpu

#        name: (bands, H, W, dtype, P, S, grid)
CASES = {"A": (3, 100, 150, torch.uint8, 64, 32, (2, 3)),
         "B": (13, 70, 64, torch.uint16, 64, 3, (3, 1)),
         "C": (1, 64, 200, torch.float32, 64, 48, (1, 3)),
         "D": (5, 37, 41, torch.uint16, 16, 5, (5, 6))}           # a patch that is no multiple of the wave size
NOISE_STD = 0.03


def _case(name):
    c, h, w, dtype, p, s, grid = CASES[name]
    scene = _scene(c, h, w, dtype, seed=ord(name))
    assert eae_amd.window_grid(h, w, p, s, any_patch=True) == grid
    return scene, _divisor(c, dtype), p, s, grid


def _ids(n_windows, count, seed):
    """`count` window ids in shuffled order (wrapping round a small grid, so duplicates occur there)."""
    perm = torch.randperm(n_windows, generator=torch.Generator().manual_seed(seed)).tolist()
    return [perm[i % n_windows] for i in range(count)]


def _cut(arr, ids, n_w, p, s, shift=None):
    """[B,C,P,P] windows cut from a NumPy scene [C,H,W]; shift[b] = (dy, dx) moves the origin of window b."""
    out = []
    for b, n in enumerate(ids):
        oy, ox = (n // n_w) * s, (n % n_w) * s
        if shift is not None:
            oy, ox = oy + shift[b][0], ox + shift[b][1]
        assert 0 <= oy and oy + p <= arr.shape[1] and 0 <= ox and ox + p <= arr.shape[2]
        out.append(arr[:, oy:oy + p, ox:ox + p])
    return np.stack(out)


def _dev(ids):
    return torch.tensor(ids, dtype=torch.int64, device="cuda")


def _noise(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).cuda()


# flip 0/1, top / left in {0, 4, 8}; rows of (., 0, 0) and (., 8, 8)
PARAMS7 = [(0, 0, 0), (1, 8, 8), (1, 0, 0), (0, 8, 8), (0, 4, 8), (1, 8, 4), (1, 4, 0)]


# ---------------------------------------------------------------------------------------------------- 1. train=False
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_eval_mode_is_scene_windows(name):
    scene, div, p, s, (n_h, n_w) = _case(name)
    n = n_h * n_w
    ids = _ids(n, n, seed=3)
    ids.insert(1, ids[-1])                                        # one duplicate
    ref = eae_amd.scene_windows(scene, div, p, s)[_dev(ids)]
    for crop in ("window", "scene"):
        got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), train=False, crop=crop, seed=9, step=4)
        assert got.shape == (n + 1, scene.shape[0], p, p) and got.dtype == torch.float32
        assert torch.equal(got, ref)


# ---------------------------------------------------------------------------------------------------- 2. / 3. crop="window"
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_window_crop_explicit_draws(name):
    scene, div, p, s, (n_h, n_w) = _case(name)
    ids = _ids(n_h * n_w, 7, seed=5)
    params = torch.tensor(PARAMS7, dtype=torch.int32)
    noise = _noise((7, scene.shape[0], p, p), seed=21)
    wins = torch.from_numpy(_cut(scene.cpu().numpy(), ids, n_w, p, s)).cuda()
    ref = eae_amd.stage_bands(wins, div, params=params, noise=noise, noise_std=NOISE_STD)
    got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=params, noise=noise, noise_std=NOISE_STD)
    assert torch.equal(got, ref)
    # the draws matter: without the noise, and with other params, the batch is another one
    assert not torch.equal(got, eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=params, noise=noise, noise_std=0.0))
    assert not torch.equal(got, eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=params.flip(0), noise=noise,
                                                            noise_std=NOISE_STD))


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_window_crop_philox_stream_is_stage_bands(name):
    scene, div, p, s, (n_h, n_w) = _case(name)
    ids = _ids(n_h * n_w, 7, seed=6)
    got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), seed=1234, step=5, noise_std=NOISE_STD)
    other = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), seed=1234, step=6, noise_std=NOISE_STD)
    assert not torch.equal(got, other)                             # the comparison below can fail
    wins = torch.from_numpy(_cut(scene.cpu().numpy(), ids, n_w, p, s)).cuda()
    ref = eae_amd.stage_bands(wins, div, seed=1234, step=5, noise_std=NOISE_STD)
    assert torch.equal(got, ref)
    # and the geometric draws alone (no noise): the (flip, top, left) of every batch position
    assert torch.equal(eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), seed=1234, step=5, noise_std=0.0),
                       eae_amd.stage_bands(wins, div, seed=1234, step=5, noise_std=0.0))


# ---------------------------------------------------------------------------------------------------- 4. crop="scene"
def _scene_crop_case(name):
    """ids, params and the host oracle's shifted windows for crop="scene": the four corner windows with (top, left) = (0, 0) and
    (8, 8), both flips, and two windows with mixed offsets."""
    scene, div, p, s, (n_h, n_w) = _case(name)
    n = n_h * n_w
    corners = [0, n_w - 1, (n_h - 1) * n_w, n - 1]
    ids = corners + corners + _ids(n, 2, seed=8)
    params = [(0, 0, 0), (1, 0, 0), (0, 0, 0), (1, 0, 0), (1, 8, 8), (0, 8, 8), (1, 8, 8), (0, 8, 8), (1, 4, 8), (0, 2, 5)]
    shift = [(t - 4, -(le - 4) if f else le - 4) for f, t, le in params]
    arr = scene.cpu().numpy()
    padded = np.pad(arr, ((0, 0), (4, 4), (4, 4)))
    real = np.pad(np.ones(arr.shape[1:], dtype=np.uint8)[None], ((0, 0), (4, 4), (4, 4)))
    pshift = [(dy + 4, dx + 4) for dy, dx in shift]               # origins in the padded scene
    wins = _cut(padded, ids, n_w, p, s, pshift)
    mask = _cut(real, ids, n_w, p, s, pshift)[:, 0]
    return scene, div, p, s, n_w, ids, params, wins, mask


@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_scene_crop_is_stage_bands_on_shifted_windows(name):
    scene, div, p, s, n_w, ids, params, wins, mask = _scene_crop_case(name)
    b = len(ids)
    noise = _noise((b, scene.shape[0], p, p), seed=22)
    pt = torch.tensor(params, dtype=torch.int32)
    centred = torch.tensor([(f, 4, 4) for f, _, _ in params], dtype=torch.int32)
    ref = eae_amd.stage_bands(torch.from_numpy(wins).cuda(), div, params=centred, noise=noise, noise_std=NOISE_STD)
    # the oracle reads padded zeros, and is not the window crop
    assert (mask.reshape(b, -1) == 0).any(axis=1).sum() >= 1
    if name == "B":                                                # the grid reaches every edge of this scene
        sides = [mask[:, 0, :], mask[:, -1, :], mask[:, :, 0], mask[:, :, -1]]
        assert all((side == 0).any() for side in sides)
    plain = torch.from_numpy(_cut(scene.cpu().numpy(), ids, n_w, p, s)).cuda()
    ref_window = eae_amd.stage_bands(plain, div, params=pt, noise=noise, noise_std=NOISE_STD)
    assert (ref != ref_window).reshape(b, -1).any(dim=1).sum() >= 1
    got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=pt, noise=noise, noise_std=NOISE_STD, crop="scene")
    assert torch.equal(got, ref)
    assert torch.equal(eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=pt, noise=noise, noise_std=NOISE_STD), ref_window)


def test_scene_crop_fp32():
    scene, div, p, s, n_w, ids, params, wins, mask = _scene_crop_case("C")
    assert (mask == 0).any()
    x = torch.from_numpy(wins)
    for b, (f, _, _) in enumerate(params):
        if f:
            x[b] = x[b].flip(-1)
    ref = x / torch.tensor(div, dtype=torch.float32)[None, :, None, None]                # IEEE division on the host
    got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), params=torch.tensor(params, dtype=torch.int32), noise_std=0.0,
                                      crop="scene")
    assert torch.equal(got.cpu(), ref)


# ---------------------------------------------------------------------------------------------------- 5. ids outside the grid
@pytest.mark.parametrize("name,crop", [("A", "window"), ("D", "scene"), ("C", "window")])
def test_out_of_range_ids_give_nan_images(name, crop):
    scene, div, p, s, (n_h, n_w) = _case(name)
    n = n_h * n_w
    good = _ids(n, 4, seed=2)
    ids = [good[0], -1, good[1], good[2], n, good[3]]
    kw = dict(seed=77, step=3, noise_std=NOISE_STD, crop=crop)
    got = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids), **kw)
    assert torch.isnan(got[1]).all() and torch.isnan(got[4]).all()
    keep = [0, 2, 3, 5]
    assert not torch.isnan(got[keep]).any()
    # the neighbours are what they are with valid ids in those places (batch positions, and so the draws, unchanged)
    ids_ok = list(ids)
    ids_ok[1], ids_ok[4] = good[0], good[1]
    ref = eae_amd.stage_scene_windows(scene, div, p, s, _dev(ids_ok), **kw)
    assert torch.equal(got[keep], ref[keep])


# ---------------------------------------------------------------------------------------------------- 6. window labels
def _labels_oracle(r, p, s, k):
    h, w = r.shape
    n_h, n_w = (h - p) // s + 1, (w - p) // s + 1
    label = np.empty((n_h, n_w), np.int64)
    count = np.empty((n_h, n_w), np.int32)
    labelled = np.empty((n_h, n_w), np.int32)
    for i in range(n_h):
        for j in range(n_w):
            v = r[i * s:i * s + p, j * s:j * s + p].reshape(-1).astype(np.int64)
            hist = np.bincount(v[(v >= 0) & (v < k)], minlength=k)
            labelled[i, j] = hist.sum()
            label[i, j] = hist.argmax() if hist.sum() else -1              # argmax: the first, i.e. the lowest class
            count[i, j] = hist.max() if hist.sum() else 0
    return label, count, labelled


def _raw_labels(raster, p, s, k):
    """The C entry point itself: integer label, count and labelled."""
    lib = _lib.load()
    h, w = raster.shape
    n_h, n_w = eae_amd.window_grid(h, w, p, s, any_patch=True)
    label = torch.full((n_h, n_w), -7, dtype=torch.int64, device="cuda")
    count = torch.full((n_h, n_w), -7, dtype=torch.int32, device="cuda")
    labelled = torch.full((n_h, n_w), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.eae_scene_window_labels(_stream(), _ptr(raster), raster.element_size(), h, w, p, s, k, _ptr(label), _ptr(count),
                                           _ptr(labelled)))
    return label, count, labelled


def _check_labels(r, p, s, k, ignore=None, oracle_of=None):
    raster = torch.from_numpy(r).cuda()
    el, ec, en = _labels_oracle(r if oracle_of is None else oracle_of, p, s, k)
    if ignore is None:
        gl, gc, gn = _raw_labels(raster, p, s, k)
        assert np.array_equal(gl.cpu().numpy(), el) and np.array_equal(gc.cpu().numpy(), ec) and np.array_equal(gn.cpu().numpy(), en)
        only = torch.full_like(gl, -7)
        _lib.check(_lib.load().eae_scene_window_labels(_stream(), _ptr(raster), raster.element_size(), r.shape[0], r.shape[1], p, s, k,
                                                       _ptr(only), None, None))                    # count and labelled may be NULL
        assert torch.equal(only, gl)
    label, purity, labelled = eae_amd.window_labels(raster, p, s, k, ignore=ignore)
    assert label.dtype == torch.int64 and purity.dtype == torch.float32 and labelled.dtype == torch.float32
    pp = float(p * p)
    assert np.array_equal(label.cpu().numpy(), el)
    assert torch.equal(purity.cpu(), torch.from_numpy(ec.astype(np.float32)) / pp)
    assert torch.equal(labelled.cpu(), torch.from_numpy(en.astype(np.float32)) / pp)
    again = eae_amd.window_labels(raster, p, s, k, ignore=ignore)
    assert all(torch.equal(a, b) for a, b in zip(again, (label, purity, labelled)))              # identical over two runs
    return el, ec, en


def _raster_a():
    r = np.random.default_rng(41).integers(0, 10, (100, 150)).astype(np.uint8)
    r[20:60, 50:90] = 255
    return r


def test_window_labels_seeded_raster():
    r = _raster_a()
    el, ec, en = _check_labels(r, 64, 32, 10)
    assert el.shape == (2, 3) and (en < 64 * 64).any() and (el >= 0).all()
    # ignore=[3]: class 3 counts as unlabelled; values outside [0, K) in the list change nothing
    gone = r.copy()
    gone[gone == 3] = 255
    _check_labels(r, 64, 32, 10, ignore=[3, 99, -2], oracle_of=gone)
    _check_labels(r, 64, 32, 10, ignore=3, oracle_of=gone)


def test_window_labels_tie_and_empty_window():
    r = np.full((64, 128), 255, np.uint8)
    r[:, :32], r[:, 32:64] = 7, 2
    el, ec, en = _check_labels(r, 64, 64, 10)
    assert el.tolist() == [[2, -1]] and ec.tolist() == [[2048, 0]] and en.tolist() == [[4096, 0]]


def test_window_labels_int32_values_outside_the_classes():
    r = np.random.default_rng(42).choice(np.array([-3, 0, 63, 64, 1000], np.int32), (37, 41))
    el, ec, en = _check_labels(r, 16, 5, 64)
    assert el.shape == (5, 6) and set(np.unique(el)) <= {-1, 0, 63} and (en < 256).all()
    # other integer dtypes go through int32
    wide = torch.from_numpy(r.astype(np.int64)).cuda()
    wide[0, 0] = 2**40 + 5                                         # would alias class 5 if it were merely truncated
    r2 = r.copy()
    r2[0, 0] = -1
    got = eae_amd.window_labels(wide, 16, 5, 64)
    ref = eae_amd.window_labels(torch.from_numpy(r2).cuda(), 16, 5, 64)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))


def test_window_labels_one_class():
    r = np.random.default_rng(43).integers(0, 3, (70, 64)).astype(np.uint8)
    el, ec, en = _check_labels(r, 64, 3, 1)
    assert (el == 0).all() and np.array_equal(ec, en)


# ---------------------------------------------------------------------------------------------------- 7. SceneLoader
def _labelled_a():
    scene, div, p, s, grid = _case("A")
    r = _raster_a()
    r[0:64, 64:128] = 255                                          # window (0, 2) has no labelled pixel
    label, purity, labelled = eae_amd.window_labels(torch.from_numpy(r).cuda(), p, s, 10)
    assert label.shape == grid and label[0, 2] == -1 and (label >= 0).sum() == 5
    return scene, div, p, s, label, purity


def test_scene_loader_batches_are_stage_scene_windows():
    scene, div, p, s, label, purity = _labelled_a()
    kw = dict(divisor=div, patch=p, stride=s, batch_size=4, seed=5, noise_std=0.05, crop="scene")
    loader = eae_amd.SceneLoader(scene, label, **kw)
    assert loader.batch_size == 4 and len(loader) == 2 and loader.windows.tolist() == [0, 1, 3, 4, 5]
    assert loader.windows.device == scene.device
    seen = []
    for e in (0, 1):
        sched = loader.schedule(e)
        assert [b.numel() for b in sched] == [4, 1]                # a short last batch
        batches = list(loader)
        assert len(batches) == 2
        for i, (x, y) in enumerate(batches):
            ids = loader.windows[sched[i].cuda()]
            ref = eae_amd.stage_scene_windows(scene, div, p, s, ids, train=True, seed=5, step=e * 2 + i, noise_std=0.05, crop="scene")
            assert torch.equal(x, ref) and x.device == scene.device
            assert y.dtype == torch.int64 and torch.equal(y, label.reshape(-1)[ids]) and (y >= 0).all()
            seen.append(ids.tolist())
    assert seen[:2] != seen[2:]                                    # epoch 1 is another order
    # set_epoch replays an epoch
    loader.set_epoch(0)
    x0, _ = next(iter(loader))
    assert torch.equal(x0, eae_amd.stage_scene_windows(scene, div, p, s, _dev(seen[0]), seed=5, step=0, noise_std=0.05, crop="scene"))
    # the epoch is taken by __iter__ itself: two iterators made before either is consumed run epochs 0 and 1
    loader.set_epoch(0)
    it0, it1 = iter(loader), iter(loader)
    loader.set_epoch(7)                                            # a later set_epoch does not move them
    assert loader.epoch == 7
    (xb, _), (xa, _) = next(it1), next(it0)
    assert torch.equal(xa, x0)
    assert torch.equal(xb, eae_amd.stage_scene_windows(scene, div, p, s, _dev(seen[2]), seed=5, step=2, noise_std=0.05, crop="scene"))
    # drop_last drops the short batch
    cut = eae_amd.SceneLoader(scene, label, drop_last=True, **kw)
    got = list(cut)
    assert len(cut) == 1 and len(got) == 1 and got[0][0].shape[0] == 4 and torch.equal(got[0][0], x0)


def test_scene_loader_purity_and_eval_order():
    scene, div, p, s, label, purity = _labelled_a()
    thr = float(purity[label >= 0].median())
    want = [n for n in range(label.numel()) if label.reshape(-1)[n] >= 0 and float(purity.reshape(-1)[n]) >= thr]
    assert 0 < len(want) < 5
    loader = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=2, purity=purity, min_purity=thr, train=False)
    assert loader.windows.tolist() == want and loader.shuffle is False
    allw = eae_amd.scene_windows(scene, div, p, s)
    for _ in range(2):                                             # every epoch: ascending ids, scene_windows batches
        got_ids = []
        for i, (x, y) in enumerate(loader):
            ids = want[2 * i:2 * i + 2]
            assert torch.equal(x, allw[_dev(ids)]) and y.tolist() == label.reshape(-1)[_dev(ids)].tolist()
            got_ids += ids
        assert got_ids == want
    # windows= restricts the set and keeps its order when not shuffling
    sub = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=8, windows=_dev([5, 2, 0]), train=False)
    assert sub.windows.tolist() == [5, 0]
    (x, y), = list(sub)
    assert torch.equal(x, allw[_dev([5, 0])])


def test_scene_loader_epoch_does_not_synchronise():
    """torch's sync debug mode raises on a synchronising call (the control below shows that it does here)."""
    import warnings
    scene, div, p, s, label, purity = _labelled_a()
    loader = eae_amd.SceneLoader(scene, label, divisor=div, patch=p, stride=s, batch_size=2, crop="scene", seed=1)
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


# ---------------------------------------------------------------------------------------------------- 8. end to end
def test_fit_autoencoder_from_scene_loaders():
    scene = _scene(3, 128, 128, torch.uint8, seed=50)
    r = np.random.default_rng(51).integers(0, 10, (128, 128)).astype(np.uint8)
    label, purity, _ = eae_amd.window_labels(torch.from_numpy(r).cuda(), 64, 32, 10)
    assert label.shape == (3, 3) and (label >= 0).all()

    def loaders():
        kw = dict(divisor=255.0, patch=64, stride=32, batch_size=8, seed=2)
        return eae_amd.SceneLoader(scene, label, train=True, **kw), eae_amd.SceneLoader(scene, label, train=False, **kw)

    def fit(train, val):
        torch.manual_seed(0)
        return eae_amd.fit_autoencoder(train, val, alpha=30, lr=1e-3, num_epochs=1, verbose=False)

    a = fit(*loaders())
    train, val = loaders()
    b = fit([(x, y) for x, y in train], [(x, y) for x, y in val])
    assert a["epochs"] == b["epochs"] == 1
    assert a["train_curve"] == b["train_curve"] and a["val_curve"] == b["val_curve"]
    assert np.isfinite(a["train_curve"]).all() and np.isfinite(a["val_curve"]).all()
    sa, sb = a["model"].state_dict(), b["model"].state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    # the features and labels the classifier stage reads come through the same loader
    feats, ys = eae_amd.extract_features(loaders()[1], a["model"].enc)
    assert feats.shape == (9, 64) and ys.tolist() == label.reshape(-1).tolist()
