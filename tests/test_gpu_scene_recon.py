"""Scene reconstruction on the device (eae_amd.scene_reconstruction_error / reconstruct_scene): deconv4's scene-target epilogue
against the staged composition of public pieces (scene_windows -> eval-mode SupervisedAutoencoder -> a float64 MSE), batch
independence, the NumPy oracle, nodata / mask / window lists, the stitched raster's ownership rule, 64-bit offsets and refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd.engine import engine_for, _stream, _ptr
from helpers import ae_state_np, load_state_np
from scene_util import _scene, _divisor, _desc, _model as _build

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                     # unit roundoff of fp32
_model = functools.partial(_build, all_halves=True)    # non-trivial running statistics in BOTH halves


def _staged(scene, div, model, stride, batch, first=0, count=None):
    """(x, x_hat) [N,C,P,P] fp32: scene_windows -> eval autoencoder, in the fused path's batches."""
    p = model.enc.image_size
    n_h, n_w = eae_amd.window_grid(scene.shape[1], scene.shape[2], p, stride)
    count = n_h * n_w - first if count is None else count
    xs, hs = [], []
    with torch.no_grad():
        for b0 in range(first, first + count, batch):
            nb = min(batch, first + count - b0)
            x = eae_amd.scene_windows(scene, div, p, stride, first=b0, count=nb)
            xs.append(x)
            hs.append(model(x)[0])
    return torch.cat(xs), torch.cat(hs)


def _ref_err(x, xh):
    """float64 means of (x_hat - x)^2 per window [N] and per window and band [N,C]."""
    d2 = (xh.double() - x.double()) ** 2
    return d2.mean(dim=(1, 2, 3)), d2.mean(dim=(2, 3))


def _rel_tol(c, p):
    # Depth of the fp32 summation as implemented (csrc/eae_edge.hip.h, deconv4_scene_body): each thread chains its 2 pixels
    # (`bsum[co] = fmaf(d, d, bsum[co])`, i = 0, 1), 6 xor-shuffle levels (`bsum[k] += __shfl_xor(bsum[k], o)`), 3 additions over the
    # four waves (`((redb[0] + redb[1]) + redb[2]) + redb[3]`), and C for the band sum of scene_err_finalize_kernel
    # (csrc/eae_edge_launch.hip, `tot += __shfl(s, base + k)`): d = 2 + 6 + 3 + C; the window's tiles add 8 (P/64)^2 more.
    d = 2 + 6 + 3 + c
    tiles = 8 * (p // 64) ** 2
    return 2 * (d + tiles) * U


# ---------------------------------------------------------------------------------------------------------------- fused vs staged
@pytest.mark.parametrize("dtype,c,s,batch,p", [(torch.uint8, 3, 20, 16, 64), (torch.uint16, 13, 32, 4, 64), (torch.float32, 4, 7, 96, 64),
                                               (torch.uint8, 1, 64, 4, 64), (torch.uint16, 16, 13, 64, 64),
                                               (torch.float32, 3, 32, 8, 64), (torch.uint8, 3, 64, 8, 128)])
def test_error_maps_match_staged_float64(dtype, c, s, batch, p):
    """All three dtypes and CP forms (C = 3 -> 4, 1 / 4 -> 8, 13 / 16 -> 16), odd scene sizes, a partial last batch, the whole grid.
    x_hat is bit-identical by construction, so only the fp32 summation differs from the float64 reference."""
    h, w = (157, 211) if p == 64 else (300, 333)
    scene = _scene(c, h, w, dtype, seed=100 + c + s)
    div = _divisor(c, dtype)
    model = _model(c, seed=c, batch=batch, image_size=p)
    err, band = eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=s, batch=batch, per_band=True)
    n_h, n_w = eae_amd.window_grid(h, w, p, s)
    assert err.shape == (n_h, n_w) and band.shape == (c, n_h, n_w) and err.dtype == torch.float32
    assert (n_h * n_w) % batch != 0 and engine_for(model.enc).max_batch == batch
    x, xh = _staged(scene, div, model, s, batch)
    ref, ref_band = _ref_err(x, xh)
    tol = _rel_tol(c, p)
    got, got_band = err.reshape(-1).double(), band.reshape(c, -1).t().double()
    rel = ((got - ref).abs() / ref).max().item()
    rel_band = ((got_band - ref_band).abs() / ref_band).max().item()
    print(f"rel err {rel:.3e} band {rel_band:.3e} tol {tol:.3e}")
    assert torch.isfinite(got).all() and (ref > 0).all()
    assert rel <= tol and rel_band <= tol
    assert err.std().item() > 0                      # windows differ: a constant map would hide an indexing error
    # without per_band the same map
    assert torch.equal(eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=s, batch=batch), err)


def test_batch_independent_and_deterministic():
    c, s = 4, 16
    scene = _scene(c, 150, 203, torch.uint16, seed=7)
    div = _divisor(c, torch.uint16)
    out = []
    for batch in (8, 64, 64):
        model = _model(c, seed=3, batch=batch)
        assert engine_for(model.enc).max_batch == batch
        out.append(eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=s, batch=batch, per_band=True))
        out.append(eae_amd.reconstruct_scene(scene, model, divisor=div, stride=s, batch=batch, residual=True))
    for k in range(2):
        for t8, t64, t64b in zip(out[k], out[2 + k], out[4 + k]):
            assert torch.equal(t8, t64) and torch.equal(t64, t64b)


# ---------------------------------------------------------------------------------------------------------------- oracle
def _two_group_scene():
    """2 x 4 windows of 64 x 64, alternating low contrast around mid-grey and full-range noise; group[n] True = low contrast."""
    g = torch.Generator().manual_seed(77)
    s = torch.empty((3, 128, 256), dtype=torch.uint8)
    low = []
    for n in range(8):
        i, j = divmod(n, 4)
        low.append((i + j) % 2 == 0)
        w = torch.randint(124, 133, (3, 64, 64), generator=g) if low[-1] else torch.randint(0, 256, (3, 64, 64), generator=g)
        s[:, i * 64:(i + 1) * 64, j * 64:(j + 1) * 64] = w.to(torch.uint8)
    return s, np.array(low)


def test_oracle_parity_on_a_two_group_scene():
    """Against the NumPy oracle.  The project's x_hat tolerances (max-abs 3e-2, mean-abs 3e-3: SURVEY section 8c) bound a window's
    error by |mean((a + e)^2) - mean(a^2)| <= 2 max|a| mean|e| + max|e|^2 = 6.9e-3 with |a| < 1."""
    from oracle import ae_numpy as O
    bound = 2 * 1.0 * 3e-3 + 3e-2 ** 2
    sd = ae_state_np()
    scene, low = _two_group_scene()
    x = torch.stack([scene[:, i * 64:(i + 1) * 64, j * 64:(j + 1) * 64] for i in range(2) for j in range(4)])
    x = (x.float() / 255.0).numpy()
    xr = O.ae_forward(sd, x, train=False)["x_hat"]
    ref = ((xr.astype(np.float64) - x) ** 2).mean(axis=(1, 2, 3))
    # the scene separates the groups by far more than the bound, so the bound cannot hide a failure
    assert ref[~low].min() - ref[low].max() >= 5 * bound
    torch.manual_seed(0)
    m = load_state_np(eae_amd.SupervisedAutoencoder(64), sd).cuda().eval()
    got = eae_amd.scene_reconstruction_error(scene.cuda(), m, divisor=255.0, stride=64, batch=8).cpu().numpy().reshape(-1)
    print("oracle", ref, "fused", got)
    assert np.abs(got - ref).max() <= bound
    assert got[~low].min() > got[low].max()


# ---------------------------------------------------------------------------------------------------------------- nodata / mask / windows
def _holed_scene():
    g = torch.Generator().manual_seed(21)
    s = torch.randint(1, 256, (3, 170, 230), generator=g, dtype=torch.int64).to(torch.uint8)
    s[:, 40:75, 100:140] = 0                      # a nodata hole
    s[0, 150:, :30] = 0                           # one band only: not nodata under rule="all"
    mask = torch.zeros((170, 230), dtype=torch.bool)
    mask[120:124, 200:] = True
    return s.cuda(), mask.cuda()


def test_nodata_mask_and_window_lists():
    scene, mask = _holed_scene()
    s, batch = 32, 8
    model = _model(3, seed=5, batch=batch)
    full, full_band = eae_amd.scene_reconstruction_error(scene, model, divisor=255.0, stride=s, batch=batch, per_band=True)
    n_h, n_w = full.shape
    for kw in (dict(nodata=0), dict(mask=mask), dict(nodata=0, mask=mask, rule="any"), dict(nodata=0, mask=mask, max_invalid=0.2)):
        ids = eae_amd.valid_windows(scene, 64, s, **kw)
        valid = torch.zeros(n_h * n_w, dtype=torch.bool, device="cuda")
        valid[ids] = True
        valid = valid.reshape(n_h, n_w)
        assert 0 < int(valid.sum()) < n_h * n_w
        err, band = eae_amd.scene_reconstruction_error(scene, model, divisor=255.0, stride=s, batch=batch, per_band=True, **kw)
        assert torch.equal(torch.isnan(err), ~valid) and torch.equal(torch.isnan(band), ~valid.expand(3, -1, -1))
        assert torch.equal(err[valid], full[valid]) and torch.equal(band[:, valid], full_band[:, valid])
        if "max_invalid" in kw:                   # partly invalid windows are kept and scored with their pixels as stored
            cnt = eae_amd.window_invalid_counts(scene, 64, s, nodata=0, mask=mask)
            assert bool(((cnt > 0) & valid).any())
    # a window list: any order, duplicates
    ids = torch.tensor([n_h * n_w - 1, 3, 0, 3, 7, n_h * n_w - 1], dtype=torch.int64, device="cuda")
    listed = torch.zeros(n_h * n_w, dtype=torch.bool, device="cuda")
    listed[ids] = True
    listed = listed.reshape(n_h, n_w)
    err = eae_amd.scene_reconstruction_error(scene, model, divisor=255.0, stride=s, batch=4, windows=ids)
    assert torch.equal(torch.isnan(err), ~listed) and torch.equal(err[listed], full[listed])
    # the stitched raster: NaN exactly on the pixels owned by windows that were not run
    rfull, resfull = eae_amd.reconstruct_scene(scene, model, divisor=255.0, stride=s, batch=batch, residual=True)
    rec, res = eae_amd.reconstruct_scene(scene, model, divisor=255.0, stride=s, batch=4, residual=True, windows=ids)
    own = torch.zeros(rfull.shape[1:], dtype=torch.bool, device="cuda")
    for n in set(ids.tolist()):
        i, j = divmod(n, n_w)
        (y0, y1), (x0, x1) = eae_amd.owned_span(i, n_h, 64, s), eae_amd.owned_span(j, n_w, 64, s)
        own[y0:y1, x0:x1] = True
    assert torch.equal(torch.isnan(res), ~own) and torch.equal(torch.isnan(rec), ~own.expand(3, -1, -1))
    assert torch.equal(res[own], resfull[own]) and torch.equal(rec[:, own], rfull[:, own])
    # no valid window: nothing is launched (the engine's forward generation does not move)
    eng = engine_for(model.enc)
    gen = eng.generation()
    empty = eae_amd.scene_reconstruction_error(torch.zeros_like(scene), model, divisor=255.0, stride=s, batch=batch, nodata=0)
    assert torch.isnan(empty).all() and eng.generation() == gen
    none = eae_amd.reconstruct_scene(scene, model, divisor=255.0, stride=s, windows=torch.empty(0, dtype=torch.int64, device="cuda"))
    assert torch.isnan(none).all() and eng.generation() == gen
    with pytest.raises(RuntimeError):
        eae_amd.scene_reconstruction_error(scene, model, windows=torch.tensor([n_h * n_w], device="cuda"))


# ---------------------------------------------------------------------------------------------------------------- stitching
@pytest.mark.parametrize("dtype,c,s", [(torch.uint8, 3, 64), (torch.uint16, 13, 32), (torch.float32, 4, 58), (torch.uint8, 1, 62)])
def test_stitched_raster_is_the_owned_spans_pasted(dtype, c, s):
    """stride = P is plain tiling, P/2 the common overlap, 58 and 62 give m = 3 and m = 1 (owned spans off every vector alignment)."""
    h, w, p, batch = 157, 211, 64, 8
    scene = _scene(c, h, w, dtype, seed=300 + s)
    div = _divisor(c, dtype)
    model = _model(c, seed=13, batch=batch)
    rec, res = eae_amd.reconstruct_scene(scene, model, divisor=div, stride=s, batch=batch, residual=True)
    n_h, n_w = eae_amd.window_grid(h, w, p, s)
    h_g, w_g = (n_h - 1) * s + p, (n_w - 1) * s + p
    assert rec.shape == (c, h_g, w_g) and res.shape == (h_g, w_g)
    x, xh = _staged(scene, div, model, s, batch)
    ref, x32 = torch.full_like(rec, float("nan")), torch.full_like(rec, float("nan"))
    for n in range(n_h * n_w):
        i, j = divmod(n, n_w)
        (y0, y1), (x0, x1) = eae_amd.owned_span(i, n_h, p, s), eae_amd.owned_span(j, n_w, p, s)
        ref[:, y0:y1, x0:x1] = xh[n][:, y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s]
        x32[:, y0:y1, x0:x1] = x[n][:, y0 - i * s:y1 - i * s, x0 - j * s:x1 - j * s]
        if s == p:
            assert (y0, y1, x0, x1) == (i * p, (i + 1) * p, j * p, (j + 1) * p)
    assert torch.isfinite(rec).all() and torch.isfinite(res).all()
    assert torch.equal(rec, ref)
    # the residual: band mean of (recon - x)^2 with x the fp32 value the encoder read (scene / divisor: scene_windows), a chain of C fused multiply-adds and one division
    ref_res = ((rec.double() - x32.double()) ** 2).mean(dim=0)
    rel = ((res.double() - ref_res).abs() / ref_res.clamp_min(1e-300)).max().item()
    print(f"residual rel err {rel:.3e} tol {2 * (c + 1) * U:.3e}")
    assert rel <= 2 * (c + 1) * U
    assert torch.equal(eae_amd.reconstruct_scene(scene, model, divisor=div, stride=s, batch=batch), rec)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_reconstruction_halo_stays_zero(dtype):
    """A window surrounded by huge scene values: its owned pixels equal the x_hat of the window staged as an isolated image (a leak
    of the neighbours into the encoder's padding, or a target or store outside the window, would show)."""
    c = 3
    big = {torch.uint8: 255, torch.uint16: 65535, torch.float32: 1e4}[dtype]
    scene = torch.full((c, 192, 192), big, dtype=dtype)
    g = torch.Generator().manual_seed(5)
    centre = torch.randint(0, 100, (c, 64, 64), generator=g).to(dtype)
    scene[:, 64:128, 64:128] = centre
    scene = scene.cuda()
    div = _divisor(c, dtype)
    model = _model(c, seed=11, batch=16)
    rec = eae_amd.reconstruct_scene(scene, model, divisor=div, stride=64, batch=16)
    err = eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=64, batch=16)
    iso_x = eae_amd.stage_bands(centre[None].cuda(), div, train=False) if dtype != torch.float32 else \
        (centre[None] / torch.tensor(div)[None, :, None, None]).cuda()
    with torch.no_grad():
        iso = model(iso_x)[0]
    assert torch.equal(rec[:, 64:128, 64:128], iso[0])
    ref, _ = _ref_err(iso_x, iso)
    assert abs(err[1, 1].item() - ref.item()) <= _rel_tol(c, 64) * ref.item()


# ---------------------------------------------------------------------------------------------------------------- 64-bit offsets
def test_error_map_beyond_2g_elements():
    """uint8 scene of 16 x 11 600 x 11 600 (2.15e9 elements > 2^31): the errors of the fused path's last batch match the staged
    computation.  Only the error map is computed here (the stitched raster of this scene would take 8.6 GB)."""
    c, h, w, s, batch = 16, 11600, 11600, 64, 512
    gen = torch.Generator(device="cuda").manual_seed(1)
    scene = torch.randint(0, 256, (c, h, w), dtype=torch.uint8, device="cuda", generator=gen)
    assert scene.numel() > 2 ** 31
    div = _divisor(c, torch.uint8)
    model = _model(c, seed=41)
    n_h, n_w = eae_amd.window_grid(h, w, 64, s)
    n = n_h * n_w
    err = eae_amd.scene_reconstruction_error(scene, model, divisor=div, stride=s, batch=batch)
    mb = engine_for(model.enc).max_batch
    last0 = (n - 1) // mb * mb                              # the fused path's last batch
    x, xh = _staged(scene, div, model, s, mb, first=last0, count=n - last0)
    ref, _ = _ref_err(x, xh)
    got = err.reshape(-1)[last0:].double()
    assert torch.isfinite(err).all()
    assert ((got - ref).abs() / ref).max().item() <= _rel_tol(c, 64)
    del scene, x, xh
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_rejected_arguments_raise():
    model = _model(3, seed=51, batch=8)
    ok = _scene(3, 100, 100, torch.uint8, seed=1)
    ids = torch.zeros(1, dtype=torch.int64, device="cuda")
    for fn in (eae_amd.scene_reconstruction_error, eae_amd.reconstruct_scene):
        for bad in (lambda: fn(_scene(4, 100, 100, torch.uint8, 1), model), lambda: fn(ok, model, stride=0),
                    lambda: fn(ok, model, stride=65), lambda: fn(ok.cpu(), model), lambda: fn(ok, model.enc),
                    lambda: fn(ok, model, windows=ids, nodata=0), lambda: fn(ok, model, windows=ids.cpu())):
            with pytest.raises(RuntimeError):
                bad()
    with pytest.raises(RuntimeError):
        eae_amd.reconstruct_scene(ok, model, stride=33)
    # the C entry points check on their own
    eng = engine_for(model.enc)
    lib = _lib.load()
    div = torch.ones(3, device="cuda")
    err = torch.empty(4, device="cuda")
    rec = torch.empty((3, 100, 100), device="cuda")
    ok4 = _scene(4, 100, 100, torch.uint8, seed=2)
    d_ok = _desc(ok, div, stride=36)
    _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d_ok), 0, 4, _ptr(err), None))      # the good call passes
    for d in (_desc(ok, None), _desc(ok4, torch.ones(4, device="cuda")), _desc(ok, div, stride=0), _desc(ok, div, stride=65)):
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d), 0, 1, _ptr(err), None))
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_scene_recon_error_windows(eng.ctx, _stream(), C.byref(d), _ptr(ids), 1, _ptr(err), None))
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_scene_reconstruct(eng.ctx, _stream(), C.byref(d), None, 1, _ptr(rec), None))
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d_ok), 0, 4, None, None))         # NULL outputs
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_recon_error_windows(eng.ctx, _stream(), C.byref(d_ok), _ptr(ids), 1, None, None))
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_recon_error_windows(eng.ctx, _stream(), C.byref(d_ok), None, 1, _ptr(err), None))
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_reconstruct(eng.ctx, _stream(), C.byref(d_ok), None, 4, None, None))
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d_ok), 2, 3, _ptr(err), None))      # outside the grid
    with pytest.raises(RuntimeError):                                                                        # odd patch - stride
        _lib.check(lib.eae_scene_reconstruct(eng.ctx, _stream(), C.byref(_desc(ok, div, stride=35)), None, 4, _ptr(rec), None))
    # the engine of a stand-alone Encoder has no decoder
    torch.manual_seed(0)
    enc = eae_amd.Encoder(64, 64).cuda().eval()
    eenc = engine_for(enc)
    for call in (lambda: lib.eae_scene_recon_error(eenc.ctx, _stream(), C.byref(d_ok), 0, 4, _ptr(err), None),
                 lambda: lib.eae_scene_recon_error_windows(eenc.ctx, _stream(), C.byref(d_ok), _ptr(ids), 1, _ptr(err), None),
                 lambda: lib.eae_scene_reconstruct(eenc.ctx, _stream(), C.byref(_desc(ok, div, stride=36)), None, 4, _ptr(rec), None)):
        with pytest.raises(RuntimeError):
            _lib.check(call())
    torch.cuda.synchronize()


def test_quant_fp8_context_rejected():
    torch.manual_seed(0)
    m = eae_amd.SupervisedAutoencoder(64, 10, image_size=256).cuda().eval()
    m._eae_quant, m._eae_max_batch = "fp8", 8
    eng = engine_for(m.enc)
    assert eng.quant == 1
    scene = _scene(3, 256, 256, torch.uint8, seed=4)
    with pytest.raises(RuntimeError):
        eae_amd.scene_reconstruction_error(scene, m, divisor=255.0)
    with pytest.raises(RuntimeError):
        eae_amd.reconstruct_scene(scene, m, divisor=255.0)
    lib = _lib.load()
    d = _desc(scene, torch.ones(3, device="cuda"), patch=256, stride=256)
    err = torch.empty(1, device="cuda")
    with pytest.raises(RuntimeError):
        _lib.check(lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d), 0, 1, _ptr(err), None))


def test_backward_after_scene_reconstruction_is_refused():
    """The scene calls replace the resident forward: a backward that uses a generation taken before one is refused."""
    model = _model(3, seed=61, batch=8).train()
    x = torch.rand((4, 3, 64, 64), device="cuda")
    x_hat, logits, z = model(x)
    eng = engine_for(model)
    gen = eng.generation()
    scene = _scene(3, 96, 96, torch.uint8, seed=6)
    d = _desc(scene, torch.full((3,), 255.0, device="cuda"), stride=32)
    err = torch.empty(4, device="cuda")
    _lib.check(eng.lib.eae_scene_recon_error(eng.ctx, _stream(), C.byref(d), 0, 4, _ptr(err), None))
    assert eng.generation() != gen
    with pytest.raises(RuntimeError):
        x_hat.sum().backward()
    torch.cuda.synchronize()
