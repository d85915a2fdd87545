"""The NumPy reference of the global gradient-norm clipping (tests/grad_clip_ref.py) equals torch.nn.utils.clip_grad_norm_ on CPU
tensors laid out by eae_ae_layout -- configurations with and without padding, norms above and below max_norm, and inf."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_clip_ref as R

# (latent, bands, classes): the golden shape; a padded latent with 3 padding floats behind deconv4's bias and 2 behind the classifier's;
# 13 bands and 7 classes
CONFIGS = [(64, 3, 10), (48, 1, 10), (128, 13, 7)]


@pytest.mark.parametrize("latent,bands,classes", CONFIGS)
def test_layout_of_the_reference_is_the_librarys(latent, bands, classes):
    from eae_amd import _lib
    lib = _lib.load()
    cfg = _lib.EaeConfig(latent, classes, 64, 64, 8, 0, 0, bands)
    poff = (C.c_longlong * 39)()
    boff = (C.c_longlong * 15)()
    _lib.check(lib.eae_ae_layout(C.byref(cfg), poff, boff))
    sizes = R.ae_param_sizes(latent, classes, 64, bands)
    assert list(poff) == R.layout_offsets(sizes)
    pad = R.padding_index(list(poff), sizes)
    if (latent, bands, classes) == (48, 1, 10):
        assert len(pad) == 3 + 2 and list(pad[:3]) == [poff[33] + 1, poff[33] + 2, poff[33] + 3]
    if (latent, bands, classes) == (64, 3, 10):
        assert len(pad) == 1 + 2


@pytest.mark.parametrize("latent,bands,classes", CONFIGS)
@pytest.mark.parametrize("rel", [0.5, 2.0, float("inf")])
@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_reference_equals_torch_clip_grad_norm(latent, bands, classes, rel, scale):
    sizes = R.ae_param_sizes(latent, classes, 64, bands)
    poff = R.layout_offsets(sizes)
    rng = np.random.default_rng(latent + bands)
    arena = (rng.standard_normal(poff[38]) * 1e-2).astype(np.float32)
    arena[R.padding_index(poff, sizes)] = 1e4            # the arenas are the caller's: padding need not be zero
    total = R.grad_norm(arena, poff, sizes, scale)
    params = []
    for s, n in enumerate(sizes):
        p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
        p.grad = torch.from_numpy(arena[poff[s]: poff[s] + n].astype(np.float64)) * scale       # (DDP averages before it clips)
        params.append(p)
    want = torch.cat([p.grad for p in params]).norm().item()
    assert abs(total - want) <= 1e-12 * want
    max_norm = rel * total
    got = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2).item()
    assert abs(total - got) <= 1e-12 * got
    coef = R.clip_coef(total, max_norm)
    assert (coef == 1.0) == (rel >= 2.0)
    for s, n in enumerate(sizes):
        ref = arena[poff[s]: poff[s] + n].astype(np.float64) * scale * coef
        assert np.allclose(params[s].grad.numpy(), ref, rtol=1e-12, atol=0.0), s
    c32 = float(R.clip_coef_f32(total, max_norm))
    assert abs(c32 - coef) <= 4 * 2.0 ** -24
