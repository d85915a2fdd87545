"""Nodata- and mask-aware scene classification (eae_amd.scene): the per-window invalid-pixel counts against a NumPy brute force, the
compaction of valid window ids, the index-driven encoder / classifier against the staged and plain paths (bitwise), the
validity-aware blend, an all-invalid scene, a scene beyond 2^31 elements and the argument checks."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import scene as S
from eae_amd.engine import engine_for
from scene_util import _MAX, _scene, _divisor, _model as _encoder, _mlp

pytestmark = pytest.mark.gpu

P = 64
_NP = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32}


# ---------------------------------------------------------------------------------------------------------------- scenes with holes
def _holey_scene(c, h, w, dtype, s, seed, nodata, p=P, frac=0.004):
    """NumPy scene [C,H,W] without accidental nodata, then: whole-pixel nodata at random, single-band nodata at random (counts only
    for rule="any"), and whole-pixel nodata exactly at columns / rows j*S + P - 1 and j*S + P (window edges, one past them)."""
    g = np.random.default_rng(seed)
    if dtype == torch.float32:
        x = (g.random((c, h, w), dtype=np.float32) * 3.0 + 0.5).astype(np.float32)
    else:
        x = g.integers(1, _MAX[dtype], (c, h, w)).astype(_NP[dtype])
    full = g.random((h, w)) < frac
    for j in range((w - p) // s + 1):
        for col in (j * s + p - 1, j * s + p):
            if col < w:
                full[(j * 37 + 5) % h, col] = True
    for i in range((h - p) // s + 1):
        for row in (i * s + p - 1, i * s + p):
            if row < h:
                full[row, (i * 53 + 3) % w] = True
    part = g.random((c, h, w)) < frac / 2
    x[part] = nodata
    x[:, full] = nodata
    return x


def _inv_np(x, nodata, rule, mask=None):
    if nodata is None:
        inv = np.zeros(x.shape[1:], dtype=bool)
    else:
        eq = np.isnan(x) if isinstance(nodata, float) and np.isnan(nodata) else x == nodata
        inv = eq.all(0) if rule == "all" else eq.any(0)
    if mask is not None:
        inv = inv | (mask != 0)
    return inv


def _counts_np(inv, p, s):
    h, w = inv.shape
    n_h, n_w = (h - p) // s + 1, (w - p) // s + 1
    out = np.zeros((n_h, n_w), dtype=np.int64)
    for i in range(n_h):
        for j in range(n_w):
            out[i, j] = inv[i * s:i * s + p, j * s:j * s + p].sum()
    return out


def _rand_mask(h, w, seed, frac=0.003):
    g = np.random.default_rng(seed)
    m = g.random((h, w)) < frac
    m[h // 3:h // 3 + 9, w // 2:w // 2 + 13] = True         # a small cloud
    return m


# ---------------------------------------------------------------------------------------------------------------- 1. counts
@pytest.mark.parametrize("dtype,c,s,w,nodata,rule,use_mask", [
    (torch.uint8, 1, 64, 131, 0, "all", False), (torch.uint8, 3, 32, 203, 0, "any", False), (torch.uint8, 13, 20, 171, 255, "all", True),
    (torch.uint8, 16, 7, 129, 0, "any", True), (torch.uint16, 13, 32, 257, 0, "all", False), (torch.uint16, 3, 7, 131, 65535, "any", False),
    (torch.uint16, 16, 20, 199, 0, "all", True), (torch.uint16, 1, 64, 203, 7, "any", True),
    (torch.float32, 3, 20, 97, float("nan"), "all", False), (torch.float32, 16, 7, 130, float("nan"), "any", True),
    (torch.float32, 13, 32, 161, -9999.0, "all", False), (torch.float32, 1, 64, 150, 0.0, "any", True),
    (torch.uint8, 3, 7, 149, None, "all", True), (torch.float32, 13, 32, 131, None, "any", True)])
def test_invalid_counts_match_brute_force(dtype, c, s, w, nodata, rule, use_mask):
    h = 157
    x = _holey_scene(c, h, w, dtype, s, seed=c * 31 + s + w, nodata=0 if nodata is None else nodata)
    mask = _rand_mask(h, w, seed=s + w) if use_mask else None
    scene = torch.from_numpy(x).cuda()
    mt = torch.from_numpy(mask).cuda() if use_mask else None
    got = eae_amd.window_invalid_counts(scene, P, s, nodata=nodata, mask=mt, rule=rule)
    ref = _counts_np(_inv_np(x, nodata, rule, mask), P, s)
    assert got.dtype == torch.int32 and tuple(got.shape) == ref.shape
    assert np.array_equal(got.cpu().numpy(), ref)
    assert ref.max() > 0 and (nodata is None or ref.min() < ref.max())
    if use_mask:                                  # a uint8 mask gives the same counts as the bool one
        got8 = eae_amd.window_invalid_counts(scene, P, s, nodata=nodata, mask=mt.to(torch.uint8) * 7, rule=rule)
        assert torch.equal(got8, got)


def test_invalid_counts_patch_128_and_unaligned_rows():
    """P = 128, a width whose rows start at every byte offset (W odd, uint8), mask only and nodata only."""
    c, h, w, s = 3, 300, 333, 20
    x = _holey_scene(c, h, w, torch.uint8, s, seed=9, nodata=0, p=128)
    mask = _rand_mask(h, w, seed=10)
    scene = torch.from_numpy(x).cuda()
    for nodata, m in ((0, None), (None, mask), (0, mask)):
        got = eae_amd.window_invalid_counts(scene, 128, s, nodata=nodata, mask=None if m is None else torch.from_numpy(m).cuda())
        assert np.array_equal(got.cpu().numpy(), _counts_np(_inv_np(x, nodata, "all", m), 128, s))


# ---------------------------------------------------------------------------------------------------------------- 2. selection
def test_valid_windows_is_flatnonzero():
    c, h, w, s = 4, 250, 301, 7
    x = _holey_scene(c, h, w, torch.uint16, s, seed=21, nodata=0, frac=0.0005)
    scene = torch.from_numpy(x).cuda()
    counts = _counts_np(_inv_np(x, 0, "all"), P, s)
    for mi in (0.0, 1 / 4096, 2.5 / 4096, 0.01, 0.5):
        t = S.invalid_threshold(P, mi)
        ids = eae_amd.valid_windows(scene, P, s, nodata=0, max_invalid=mi)
        assert ids.dtype == torch.int64 and ids.device == scene.device
        assert np.array_equal(ids.cpu().numpy(), np.flatnonzero(counts.reshape(-1) <= t))
    empty = eae_amd.valid_windows(torch.zeros((c, 100, 100), dtype=torch.uint16, device="cuda"), P, 8, nodata=0)
    assert empty.numel() == 0 and empty.dtype == torch.int64


def test_valid_windows_millions():
    """A grid of 2.6 M windows (S = 1): the one-workgroup compaction against NumPy."""
    h, w = 1677, 1663
    g = np.random.default_rng(3)
    mask = g.random((h, w)) < 2e-5
    ids = eae_amd.valid_windows(torch.ones((1, h, w), dtype=torch.uint8, device="cuda"), P, 1,
                                mask=torch.from_numpy(mask).cuda(), max_invalid=1 / 4096)
    n_h, n_w = h - P + 1, w - P + 1
    assert n_h * n_w > 2_500_000
    ii = np.pad(mask.astype(np.int64).cumsum(0).cumsum(1), ((1, 0), (1, 0)))
    cnt = ii[P:, P:] - ii[:-P, P:] - ii[P:, :-P] + ii[:-P, :-P]
    assert np.array_equal(ids.cpu().numpy(), np.flatnonzero(cnt.reshape(-1) <= 1))


# ---------------------------------------------------------------------------------------------------------------- 3. index-driven encoder
@pytest.mark.parametrize("dtype,c,s,batch", [(torch.uint8, 3, 20, 64), (torch.uint16, 13, 32, 48), (torch.uint16, 4, 7, 96)])
def test_encode_windows_bitwise_staged(dtype, c, s, batch):
    scene = _scene(c, 157, 211, dtype, seed=400 + c)
    div = _divisor(c, dtype)
    model = _encoder(c, seed=c + 1, batch=batch)
    n_h, n_w = eae_amd.window_grid(157, 211, P, s)
    g = torch.Generator().manual_seed(c)
    idx = torch.randint(0, n_h * n_w, (2 * batch + 17,), generator=g)
    idx[5] = idx[100] = n_h * n_w - 1                             # duplicates and the last window
    idx[7] = 0
    z = eae_amd.encode_scene(scene, model, divisor=div, stride=s, batch=batch, windows=idx.cuda())
    assert z.shape == (len(idx), 64)
    mb = engine_for(model.enc).max_batch
    host = scene.cpu()
    ref = []
    with torch.no_grad():
        for b0 in range(0, len(idx), mb):
            wins = []
            for n in idx[b0:b0 + mb].tolist():
                y, x0 = S.window_origin(n, n_w, s)
                wins.append(host[:, y:y + P, x0:x0 + P])
            ref.append(model.enc(eae_amd.stage_bands(torch.stack(wins).cuda(), div, train=False)))
    ref = torch.cat(ref)
    assert torch.isfinite(ref).all()
    assert torch.equal(z, ref)


# ---------------------------------------------------------------------------------------------------------------- 4. no nodata present
@pytest.mark.parametrize("s", [64, 32])
def test_classify_nodata_absent_equals_plain(s):
    c = 3
    scene = (_scene(c, 170, 203, torch.uint8, seed=500 + s) | 1)              # no zero anywhere
    model, mlp = _encoder(c, seed=7, batch=64), _mlp(64, 10)
    div = _divisor(c, torch.uint8)
    for blend in (False, True):
        p0, l0 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, blend=blend)
        p1, l1 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, blend=blend, nodata=0)
        assert torch.equal(p0, p1) and torch.equal(l0, l1)


# ---------------------------------------------------------------------------------------------------------------- 5. swath edge + cloud
def _swath(c, h, w, dtype, seed):
    """Scene with a diagonal nodata (0) region, the swath edge, in the bottom-left, and a cloud mask."""
    x = _scene(c, h, w, dtype, seed).cpu().numpy()
    x[x == 0] = 1
    yy, xx = np.mgrid[0:h, 0:w]
    x[:, yy > xx * 0.8 + h * 0.35] = 0
    cloud = np.zeros((h, w), dtype=bool)
    cloud[20:60, w - 90:w - 40] = True
    return x, cloud


@pytest.mark.parametrize("dtype,c,s", [(torch.uint16, 4, 16), (torch.uint8, 3, 32)])
def test_classify_swath_and_cloud(dtype, c, s):
    h, w = 230, 260
    x, cloud = _swath(c, h, w, dtype, seed=600 + s)
    scene, mt = torch.from_numpy(x).cuda(), torch.from_numpy(cloud).cuda()
    div = _divisor(c, dtype)
    model, mlp = _encoder(c, seed=9, batch=64), _mlp(64, 12)
    p0, l0 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64)
    counts = _counts_np(_inv_np(x, 0, "all", cloud), P, s)
    for mi in (0.0, 0.1):
        t = S.invalid_threshold(P, mi)
        gen = engine_for(model.enc).generation()
        p1, l1 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, nodata=0, mask=mt, max_invalid=mi)
        assert engine_for(model.enc).generation() != gen
        valid = torch.from_numpy(counts <= t).cuda()
        assert 0 < int(valid.sum()) < valid.numel()
        assert torch.equal(l1 >= 0, valid)                              # exactly the windows with counts <= t
        assert (l1[~valid] == -1).all() and (p1[:, ~valid] == 0).all()
        assert torch.equal(l1[valid], l0[valid])
        assert torch.equal(p1[:, valid], p0[:, valid])
    # the same through windows= (the valid ids)
    ids = eae_amd.valid_windows(scene, P, s, nodata=0, mask=mt)
    p2, l2 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, windows=ids)
    p3, l3 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, nodata=0, mask=mt)
    assert torch.equal(p2, p3) and torch.equal(l2, l3)


# ---------------------------------------------------------------------------------------------------------------- 6. blend
@pytest.mark.parametrize("s", [32, 16])
def test_blend_valid_is_the_masked_mean(s):
    c, classes, h, w = 4, 6, 230, 260
    x, cloud = _swath(c, h, w, torch.uint16, seed=700 + s)
    scene, mt = torch.from_numpy(x).cuda(), torch.from_numpy(cloud).cuda()
    div = _divisor(c, torch.uint16)
    model, mlp = _encoder(c, seed=13, batch=64), _mlp(64, classes)
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, nodata=0, mask=mt)
    cprobs, clabels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, nodata=0, mask=mt, blend=True)
    n_h, n_w = labels.shape
    k = P // s
    valid = (labels >= 0).cpu()
    p = probs.double().cpu().numpy()
    ref = np.zeros((classes, n_h + k - 1, n_w + k - 1))
    for i in range(n_h):
        for j in range(n_w):
            if valid[i, j]:
                ref[:, i:i + k, j:j + k] += p[:, i:i + 1, j:j + 1]
    cov = S.valid_coverage(valid, k).numpy()
    has = cov > 0
    assert 0 < has.sum() < has.size
    ref[:, has] /= cov[has]
    got = cprobs.cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-6
    cl = clabels.cpu().numpy()
    assert (cl[~has] == -1).all() and (got[:, ~has] == 0).all()
    assert np.array_equal(cl[has], got.argmax(0)[has])


# ---------------------------------------------------------------------------------------------------------------- 7. all invalid
def test_all_invalid_scene_launches_nothing():
    c = 3
    model, mlp = _encoder(c, seed=17, batch=64), _mlp(64, 10)
    scene = torch.zeros((c, 150, 170), dtype=torch.uint8, device="cuda")
    eng = engine_for(model.enc)
    eae_amd.encode_scene(_scene(c, 64, 64, torch.uint8, 1), model, batch=64)      # the engine exists and has run once
    gen = eng.generation()
    probs, labels = eae_amd.classify_scene(scene, model, mlp, stride=16, batch=64, nodata=0)
    assert (labels == -1).all() and (probs == 0).all()
    cprobs, clabels = eae_amd.classify_scene(scene, model, mlp, stride=16, batch=64, nodata=0, blend=True)
    assert (clabels == -1).all() and (cprobs == 0).all()
    p2, l2 = eae_amd.classify_scene(scene, model, mlp, stride=16, batch=64, windows=torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert (l2 == -1).all() and (p2 == 0).all()
    assert eng.generation() == gen


# ---------------------------------------------------------------------------------------------------------------- 8. 64-bit offsets
def test_nodata_scene_beyond_2g_elements():
    """uint8 16 x 11 600 x 11 600 (> 2^31 elements) with nodata in the bottom-right corner."""
    c, h, w, s, batch = 16, 11600, 11600, 64, 512
    gen = torch.Generator(device="cuda").manual_seed(2)
    scene = torch.randint(1, 256, (c, h, w), dtype=torch.uint8, device="cuda", generator=gen)
    assert scene.numel() > 2 ** 31
    scene[:, h - 300:, w - 250:] = 0
    scene[:5, h - 400:h - 300, w - 250:] = 0                  # some bands only: valid for rule="all"
    div = _divisor(c, torch.uint8)
    model, mlp = _encoder(c, seed=43), _mlp(64, 10)
    n_h, n_w = eae_amd.window_grid(h, w, P, s)
    counts = eae_amd.window_invalid_counts(scene, P, s, nodata=0)
    bottom = scene[:, (n_h - 1) * s:(n_h - 1) * s + P, :].cpu().numpy()
    ref = _counts_np(_inv_np(bottom, 0, "all"), P, s)[0]
    assert np.array_equal(counts[-1].cpu().numpy(), ref) and ref[-1] == P * P and ref[0] == 0
    assert int(counts[:-5].sum()) == 0
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=batch, nodata=0)
    p0, l0 = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=batch)
    valid = (counts == 0)
    assert torch.equal(labels >= 0, valid)
    assert torch.equal(labels[valid], l0[valid])
    last = torch.nonzero(valid.reshape(-1)).reshape(-1)[-300:]
    assert torch.equal(labels.reshape(-1)[last], l0.reshape(-1)[last])
    assert torch.equal(probs.reshape(10, -1)[:, last], p0.reshape(10, -1)[:, last])
    del scene
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- 9. errors
def test_rejected_arguments_raise():
    c = 3
    model, mlp = _encoder(c, seed=51, batch=64), _mlp(64, 10)
    ok = _scene(c, 100, 130, torch.uint8, seed=1)
    okf = _scene(c, 100, 130, torch.float32, seed=1)
    m_ok = torch.zeros((100, 130), dtype=torch.bool, device="cuda")
    n = 37 * 67                                                      # grid at stride 1
    ids = torch.arange(5, dtype=torch.int64, device="cuda")
    bad = [
        lambda: eae_amd.classify_scene(ok, model, mlp, mask=torch.zeros((100, 129), dtype=torch.bool, device="cuda")),
        lambda: eae_amd.classify_scene(ok, model, mlp, mask=torch.zeros((100, 130), dtype=torch.float32, device="cuda")),
        lambda: eae_amd.classify_scene(ok, model, mlp, mask=m_ok.cpu()),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=256),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=-1),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=float("nan")),
        lambda: eae_amd.classify_scene(ok.to(torch.int32).to(torch.uint16), model, mlp, nodata=70000),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=0, max_invalid=1.0),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=0, max_invalid=-0.1),
        lambda: eae_amd.classify_scene(ok, model, mlp, nodata=0, rule="most"),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=ids, nodata=0),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=ids, mask=m_ok),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=ids.to(torch.int32)),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=ids.cpu()),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=ids.reshape(1, 5)),
        lambda: eae_amd.classify_scene(ok, model, mlp, stride=1, windows=torch.tensor([0, n], device="cuda")),
        lambda: eae_amd.classify_scene(ok, model, mlp, windows=torch.tensor([-1], device="cuda")),
        lambda: eae_amd.encode_scene(ok, model, windows=torch.zeros(0, dtype=torch.int64, device="cuda")),
        lambda: eae_amd.encode_scene(ok, model, stride=1, windows=torch.tensor([n], device="cuda")),
        lambda: eae_amd.encode_scene(ok, model, windows=ids.float()),
        lambda: eae_amd.window_invalid_counts(ok, P, 8, nodata=300),
        lambda: eae_amd.window_invalid_counts(ok, P, 8, nodata=0, rule="none"),
        lambda: eae_amd.window_invalid_counts(ok, P, 8, mask=m_ok[:, :-1]),
        lambda: eae_amd.window_invalid_counts(okf, P, 8, mask=m_ok.to(torch.int16)),
        lambda: eae_amd.valid_windows(ok, P, 8, nodata=0, max_invalid=1.5),
        lambda: eae_amd.valid_windows(ok, P, 8, nodata=0, max_invalid=float("nan")),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
    # fp32 scenes accept any float nodata, NaN included
    assert eae_amd.window_invalid_counts(okf, P, 8, nodata=float("nan")).sum() == 0
    torch.cuda.synchronize()
