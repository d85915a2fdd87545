"""Scene classification on the device (eae_amd.scene): the window gather, conv1 reading the scene directly, the MLP predict epilogue,
blending, 64-bit indexing and the argument checks.  The staged path is composed from public pieces: scene_windows -> eval-mode
Encoder -> eae_mlp_eval_step."""
import ctypes as C

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import engine_for, _stream, _ptr
from eae_amd.mlp_engine import mlp_engine_for
from helpers import ae_state_np, mlp_state_np, load_state_np
from scene_util import _scene, _divisor, _model as _encoder, _mlp, _desc

pytestmark = pytest.mark.gpu


def _host_windows(scene, p, s):
    """[N,C,P,P] windows cut on the host (CPU), in window order."""
    x = scene.cpu()
    c, h, w = x.shape
    n_h, n_w = (h - p) // s + 1, (w - p) // s + 1
    return torch.stack([x[:, i * s:i * s + p, j * s:j * s + p] for i in range(n_h) for j in range(n_w)]), n_h, n_w


def _staged_z(scene, div, model, stride, batch, first=0, count=None):
    """scene_windows -> eval encoder, in the fused path's batches (windows first.., `batch` per pass)."""
    p = model.enc.image_size
    n_h, n_w = eae_amd.window_grid(scene.shape[1], scene.shape[2], p, stride)
    count = n_h * n_w - first if count is None else count
    out = []
    with torch.no_grad():
        for b0 in range(first, first + count, batch):
            nb = min(batch, first + count - b0)
            out.append(model.enc(eae_amd.scene_windows(scene, div, p, stride, first=b0, count=nb)))
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("dtype,c,s,w", [(torch.uint8, 1, 64, 131), (torch.uint8, 3, 20, 203), (torch.uint16, 4, 32, 150),
                                         (torch.uint16, 13, 7, 131), (torch.float32, 16, 20, 97), (torch.float32, 3, 7, 130),
                                         (torch.uint8, 13, 32, 129), (torch.uint16, 16, 64, 257)])
def test_scene_windows_bitwise_stage_bands(dtype, c, s, w):
    scene = _scene(c, 101, w, dtype, seed=c * 7 + s)
    div = _divisor(c, dtype)
    got = eae_amd.scene_windows(scene, div, 64, s)
    wins, n_h, n_w = _host_windows(scene, 64, s)
    assert got.shape == (n_h * n_w, c, 64, 64)
    if dtype == torch.float32:
        ref = wins / torch.tensor(div, dtype=torch.float32)[None, :, None, None]        # IEEE division on the host
    else:
        ref = eae_amd.stage_bands(wins.cuda(), div, train=False).cpu()
    assert torch.equal(got.cpu(), ref)
    # a sub-range is the same rows
    part = eae_amd.scene_windows(scene, div, 64, s, first=n_h * n_w - 2, count=1)
    assert torch.equal(part.cpu(), ref[-2:-1])


# ---------------------------------------------------------------------------------------------------------------- fused encoder
@pytest.mark.parametrize("dtype,c,s,batch", [(torch.uint8, 3, 20, 64), (torch.uint16, 13, 32, 48), (torch.float32, 4, 7, 96),
                                             (torch.uint8, 1, 64, 8), (torch.uint16, 16, 13, 64), (torch.float32, 3, 32, 64)])
def test_encode_scene_bitwise_staged(dtype, c, s, batch):
    """All three dtypes and CP forms (C = 3 -> 4, 1 / 4 -> 8, 13 / 16 -> 16), odd scene widths, a last partial batch, and windows on
    the last row and column (the whole grid is compared)."""
    scene = _scene(c, 157, 211, dtype, seed=100 + c + s)
    div = _divisor(c, dtype)
    model = _encoder(c, seed=c, batch=batch)
    z = eae_amd.encode_scene(scene, model, divisor=div, stride=s, batch=batch)
    n_h, n_w = eae_amd.window_grid(157, 211, 64, s)
    assert z.shape == (n_h * n_w, 64)
    assert (n_h * n_w) % batch != 0 or batch == 8
    assert engine_for(model.enc).max_batch == batch
    ref = _staged_z(scene, div, model, s, batch)
    assert torch.isfinite(ref).all()
    assert torch.equal(z, ref)
    # an Encoder module works the same way as its SupervisedAutoencoder
    assert torch.equal(eae_amd.encode_scene(scene, model.enc, divisor=div, stride=s, batch=batch), z)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_encode_scene_halo_stays_zero(dtype):
    """Windows surrounded by large non-zero scene pixels: the conv padding at the window border must stay zero (a leak of the
    neighbouring pixels would change z)."""
    c = 3
    big = {torch.uint8: 255, torch.uint16: 65535, torch.float32: 1e4}[dtype]
    scene = torch.full((c, 192, 192), big, dtype=dtype)
    g = torch.Generator().manual_seed(5)
    centre = torch.randint(0, 100, (c, 64, 64), generator=g).to(dtype)
    scene[:, 64:128, 64:128] = centre
    scene = scene.cuda()
    div = _divisor(c, dtype)
    model = _encoder(c, seed=11, batch=16)
    z = eae_amd.encode_scene(scene, model, divisor=div, stride=64, batch=16)
    ref = _staged_z(scene, div, model, 64, engine_for(model.enc).max_batch)
    assert torch.equal(z, ref)
    # the centre window alone, staged as an isolated image, is the same latent
    with torch.no_grad():
        iso = model.enc(eae_amd.stage_bands(centre[None].cuda(), div, train=False)) if dtype != torch.float32 else \
            model.enc((centre[None] / torch.tensor(div)[None, :, None, None]).cuda())
    assert torch.equal(z[4:5], iso)


# ---------------------------------------------------------------------------------------------------------------- predict
@pytest.mark.parametrize("dtype,c,s,classes", [(torch.uint8, 3, 20, 10), (torch.uint16, 13, 32, 16), (torch.float32, 4, 16, 3)])
def test_classify_scene_matches_staged_logits(dtype, c, s, classes):
    scene = _scene(c, 150, 203, dtype, seed=200 + c)
    div = _divisor(c, dtype)
    model, mlp = _encoder(c, seed=21, batch=64), _mlp(64, classes)
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64)
    n_h, n_w = eae_amd.window_grid(150, 203, 64, s)
    assert probs.shape == (classes, n_h, n_w) and labels.shape == (n_h, n_w) and labels.dtype == torch.int64
    z = _staged_z(scene, div, model, s, engine_for(model.enc).max_batch)
    meng = mlp_engine_for(mlp)
    logits = torch.cat([meng.eval_step(z[b:b + 256], torch.zeros(min(256, len(z) - b), dtype=torch.int64, device="cuda"),
                                       want_logits=True) for b in range(0, len(z), 256)])
    assert torch.equal(labels.reshape(-1), logits.argmax(1))
    ref = torch.softmax(logits, 1).t().reshape(classes, n_h, n_w)
    assert (probs - ref).abs().max().item() <= 1e-6
    assert (probs.flatten(1).std(1) > 0).all()    # windows differ: a constant map would hide an indexing error


def test_classify_scene_reference_parity():
    """Small RGB scene against the NumPy oracle: ae_forward(train=False) z -> mlp_forward(train=False), the tolerances of
    test_gpu_mlp.py::test_extract_features_and_module_forward."""
    from oracle import ae_numpy as O
    torch.manual_seed(0)
    m = eae_amd.SupervisedAutoencoder(64)
    sd = ae_state_np()
    load_state_np(m, sd)
    clf = eae_amd.MLP(64, 10)
    msd = mlp_state_np()
    load_state_np(clf, msd)
    m, clf = m.cuda().eval(), clf.cuda().eval()
    scene = _scene(3, 128, 160, torch.uint8, seed=9)
    probs, labels = eae_amd.classify_scene(scene, m, clf, divisor=255.0, stride=32, batch=16)
    z = eae_amd.encode_scene(scene, m, divisor=255.0, stride=32, batch=16).cpu().numpy()
    wins, n_h, n_w = _host_windows(scene, 64, 32)
    x = (wins.float() / 255.0).numpy()
    zr = O.ae_forward(sd, x, train=False)["z"]
    assert np.abs(z - zr).max() <= 0.02 * np.abs(zr).max()
    lr = O.mlp_forward(msd, zr, train=False)["logits"]
    pr = np.exp(lr - lr.max(1, keepdims=True))
    pr /= pr.sum(1, keepdims=True)
    got = probs.cpu().numpy().reshape(10, -1).T
    assert np.abs(got - pr).max() < 2e-2
    agree = (labels.cpu().numpy().reshape(-1) == lr.argmax(1)).mean()
    assert agree >= 0.9, agree


# ---------------------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("s", [64, 32, 16])
def test_blend_is_the_box_mean(s):
    c, classes = 4, 6
    scene = _scene(c, 170, 190, torch.uint16, seed=300 + s)
    div = _divisor(c, torch.uint16)
    model, mlp = _encoder(c, seed=31, batch=64), _mlp(64, classes)
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64)
    cprobs, clabels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=64, blend=True)
    n_h, n_w = labels.shape
    k = 64 // s
    assert cprobs.shape == (classes, n_h + k - 1, n_w + k - 1) and clabels.shape == (n_h + k - 1, n_w + k - 1)
    p = probs.double().cpu().numpy()
    ref = np.zeros((classes, n_h + k - 1, n_w + k - 1))
    cnt = np.zeros((n_h + k - 1, n_w + k - 1))
    for i in range(n_h):
        for j in range(n_w):
            ref[:, i:i + k, j:j + k] += p[:, i:i + 1, j:j + 1]
            cnt[i:i + k, j:j + k] += 1
    ref /= cnt
    assert np.abs(cprobs.cpu().numpy() - ref).max() < 1e-6
    got_l = clabels.cpu().numpy()
    ref_l = cprobs.cpu().numpy().argmax(0)
    assert np.array_equal(got_l, ref_l)
    if k == 1:
        assert torch.equal(cprobs, probs) and torch.equal(clabels, labels)


# ---------------------------------------------------------------------------------------------------------------- 64-bit offsets
def test_scene_beyond_2g_elements():
    """uint8 scene of 16 x 11 600 x 11 600 (2.15e9 elements > 2^31): the last windows of the fused path match the staged path."""
    c, h, w, s, batch = 16, 11600, 11600, 64, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    scene = torch.randint(0, 256, (c, h, w), dtype=torch.uint8, device="cuda", generator=gen)
    assert scene.numel() > 2 ** 31
    div = _divisor(c, torch.uint8)
    model, mlp = _encoder(c, seed=41), _mlp(64, 10)
    n_h, n_w = eae_amd.window_grid(h, w, 64, s)
    n = n_h * n_w
    z = eae_amd.encode_scene(scene, model, divisor=div, stride=s, batch=batch)
    mb = engine_for(model.enc).max_batch
    last0 = (n - 1) // mb * mb                              # the fused path's last batch
    ref = _staged_z(scene, div, model, s, mb, first=last0, count=n - last0)
    assert torch.equal(z[last0:], ref)
    # the staged windows themselves: the last window's pixels are the scene's bottom-right corner
    lastwin = eae_amd.scene_windows(scene, div, 64, s, first=n - 1, count=1)
    y0, x0 = eae_amd.scene.window_origin(n - 1, n_w, s)
    corner = scene[:, y0:y0 + 64, x0:x0 + 64].cpu()
    assert torch.equal(lastwin.cpu(), eae_amd.stage_bands(corner[None].cuda(), div, train=False).cpu())
    probs, labels = eae_amd.classify_scene(scene, model, mlp, divisor=div, stride=s, batch=batch)
    logits = mlp_engine_for(mlp).eval_step(ref[-200:], torch.zeros(200, dtype=torch.int64, device="cuda"), want_logits=True)
    assert torch.equal(labels.reshape(-1)[-200:], logits.argmax(1))
    del scene
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- errors
def test_rejected_arguments_raise():
    model, mlp = _encoder(3, seed=51), _mlp(64, 10)
    ok = _scene(3, 100, 100, torch.uint8, seed=1)
    bad = [
        lambda: eae_amd.encode_scene(_scene(4, 100, 100, torch.uint8, 1), model),          # C != in_channels
        lambda: eae_amd.encode_scene(_scene(3, 63, 100, torch.uint8, 1), model),           # smaller than one window
        lambda: eae_amd.encode_scene(ok, model, stride=0),
        lambda: eae_amd.encode_scene(ok, model, stride=65),
        lambda: eae_amd.encode_scene(ok.cpu(), model),                                     # host scene
        lambda: eae_amd.classify_scene(ok, model, eae_amd.MLP(32, 10).cuda()),            # MLP width
        lambda: eae_amd.classify_scene(ok, model, mlp, stride=24, blend=True),
        lambda: eae_amd.scene_windows(ok, 1.0, 64, 8, first=20, count=10),                  # outside the grid
    ]
    for fn in bad:
        with pytest.raises(RuntimeError):
            fn()
    # the C entry points check on their own: NULL divisor, C mismatch, bad stride, a scene smaller than P, the wrong patch, quant=1
    eng, meng = engine_for(model.enc), mlp_engine_for(mlp)
    lib = _lib.load()
    div = torch.ones(3, device="cuda")
    z = torch.empty((8, 64), device="cuda")
    probs = torch.empty((10, 8), device="cuda")
    labels = torch.empty(8, dtype=torch.int64, device="cuda")
    ok4 = _scene(4, 100, 100, torch.uint8, seed=2)
    small = _scene(3, 63, 100, torch.uint8, seed=3)
    descs = [_desc(ok, None), _desc(ok4, torch.ones(4, device="cuda")), _desc(ok, div, stride=0), _desc(ok, div, stride=65),
             _desc(small, div), _desc(_scene(3, 130, 130, torch.uint8, seed=4), div, patch=128), _desc(ok, div, dtype=7)]
    for d in descs:
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_scene_encode(eng.ctx, _stream(), C.byref(d), 0, 1, _ptr(z)))
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_scene_classify(eng.ctx, meng.ctx, _stream(), C.byref(d), 0, 1, _ptr(probs), _ptr(labels)))
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_windows(_stream(), C.byref(_desc(ok, None)), 0, 1, _ptr(z)))
    torch.cuda.synchronize()


def test_range_entry_points_from_a_later_first_window():
    """The range form with first > 0 (the Python layer always passes 0): windows 5..11 of a 3 x 4 grid at max_batch 4, two batch
    boundaries and a ragged last batch of 3.  They equal the whole-grid call's rows bitwise (eval mode mixes no rows), nothing in
    front of them is written, and the index form over the same ids agrees."""
    model, mlp = _encoder(3, seed=71, batch=4), _mlp(64, 10)
    scene = _scene(3, 128, 160, torch.uint8, seed=11)
    eng, meng = engine_for(model.enc), mlp_engine_for(mlp)
    assert eng.max_batch == 4 and eae_amd.window_grid(128, 160, 64, 32) == (3, 4)
    d = _desc(scene, torch.full((3,), 255.0, device="cuda"), stride=32)
    lib, n = eng.lib, 12

    def run(first, count):
        z = torch.full((count, 64), -7.0, device="cuda")
        probs, err = torch.full((10, n), -7.0, device="cuda"), torch.full((n,), -7.0, device="cuda")
        labels = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.eae_scene_encode(eng.ctx, _stream(), C.byref(d), first, count, _ptr(z)))
        _lib.check(lib.eae_scene_classify(eng.ctx, meng.ctx, _stream(), C.byref(d), first, count, _ptr(probs), _ptr(labels)))
        _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d), first, count, _ptr(err), None))
        return z, probs, labels, err

    z0, p0, l0, e0 = run(0, n)
    z1, p1, l1, e1 = run(5, 7)
    assert torch.isfinite(z0).all() and (z0.std(0) > 0).any() and (e0 > 0).all() and (l0 >= 0).all()
    assert torch.equal(z1, z0[5:])
    assert torch.equal(p1[:, 5:], p0[:, 5:]) and torch.equal(l1[5:], l0[5:])
    assert (p1[:, :5] == -7).all() and (l1[:5] == -7).all()
    assert torch.equal(e1[5:], e0[5:]) and (e1[:5] == -7).all()
    ids = torch.arange(5, n, dtype=torch.int64, device="cuda")
    zi = torch.empty((7, 64), device="cuda")
    _lib.check(lib.eae_scene_encode_windows(eng.ctx, _stream(), C.byref(d), _ptr(ids), 7, _ptr(zi)))
    assert torch.equal(zi, z0[5:])


def test_quant_fp8_context_rejected():
    torch.manual_seed(0)
    m = eae_amd.SupervisedAutoencoder(64, 10, image_size=256).cuda().eval()
    m._eae_quant, m._eae_max_batch = "fp8", 8
    eng = engine_for(m.enc)
    assert eng.quant == 1
    scene = _scene(3, 256, 256, torch.uint8, seed=4)
    with pytest.raises(RuntimeError):
        eae_amd.encode_scene(scene, m, divisor=255.0)
    lib = _lib.load()
    div = torch.ones(3, device="cuda")
    z = torch.empty((1, 64), device="cuda")
    d = _desc(scene, div, patch=256, stride=256)
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_encode(eng.ctx, _stream(), C.byref(d), 0, 1, _ptr(z)))


def test_backward_after_scene_is_refused():
    """classify_scene replaces the resident forward: a backward that uses a generation taken before it is refused."""
    torch.manual_seed(0)
    enc = eae_amd.Encoder(64, 64).cuda().train()
    mlp = _mlp(64, 10)
    x = torch.rand((4, 3, 64, 64), device="cuda")
    z = enc(x)
    eng = engine_for(enc)
    gen = eng.generation()
    scene = _scene(3, 96, 96, torch.uint8, seed=6)
    d = _desc(scene, torch.full((3,), 255.0, device="cuda"), stride=32)
    probs = torch.empty((10, 4), device="cuda")
    labels = torch.empty(4, dtype=torch.int64, device="cuda")
    _lib.check(eng.lib.eae_scene_classify(eng.ctx, mlp_engine_for(mlp).ctx, _stream(), C.byref(d), 0, 4, _ptr(probs), _ptr(labels)))
    assert eng.generation() != gen
    with pytest.raises(RuntimeError):
        z.sum().backward()
    torch.cuda.synchronize()
