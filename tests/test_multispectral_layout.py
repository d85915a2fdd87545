"""Multispectral inputs (in_channels 1..16): module shells, default initialisation and the C ABI's arena layout agree (no GPU)."""
import ctypes as C
import math
import os

import pytest
import torch

import eae_amd
from eae_amd import _lib

EDGE = {"enc.encoder.0.weight": lambda c: (32, c, 3, 3), "dec.decoder.10.weight": lambda c: (32, c, 3, 3),
        "dec.decoder.10.bias": lambda c: (c,)}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from eae_amd import build
        build.build(verbose=False)
    return _lib.load()


def _layout(lib, latent, in_channels, quant=0):
    cfg = _lib.EaeConfig(latent, 10, 64, 64, 8, quant, 0, in_channels)
    poff = (C.c_longlong * 39)()
    boff = (C.c_longlong * 15)()
    rc = lib.eae_ae_layout(C.byref(cfg), poff, boff)
    return rc, list(poff), list(boff)


@pytest.mark.parametrize("c", [1, 4, 13, 16])
def test_state_dict_keys_and_edge_shapes(c):
    ref = eae_amd.SupervisedAutoencoder(64).state_dict()
    sd = eae_amd.SupervisedAutoencoder(64, in_channels=c).state_dict()
    assert list(sd) == list(ref) and len(sd) == 59
    for k in ref:
        if k in EDGE:
            assert tuple(sd[k].shape) == EDGE[k](c) and tuple(ref[k].shape) == EDGE[k](3), k
        else:
            assert sd[k].shape == ref[k].shape, k
    m = eae_amd.SupervisedAutoencoder(64, in_channels=c)
    assert m.in_channels == c and m.enc.in_channels == c and m.dec.out_channels == c


@pytest.mark.parametrize("c", [1, 13, 16])
def test_default_init_follows_torch_fan_in(c):
    torch.manual_seed(0)
    m = eae_amd.SupervisedAutoencoder(64, in_channels=c)
    bound = 1.0 / math.sqrt(9 * c)          # kaiming_uniform(a=sqrt(5)) on fan_in = 9C gives U(-1/sqrt(fan_in), +)
    for w, b in ((m.enc.encoder[0].weight, m.enc.encoder[0].bias), (m.dec.decoder[10].weight, m.dec.decoder[10].bias)):
        assert w.abs().max().item() <= bound and w.abs().max().item() > 0.8 * bound
        assert b.abs().max().item() <= bound
    # deconv4's bias has fan_in 9C as well (ConvTranspose2d computes it from weight [Cin, Cout, 3, 3])
    assert m.dec.decoder[10].bias.abs().max().item() > 0.5 * bound or c == 1


@pytest.mark.parametrize("c", [1, 3, 4, 13, 16])
def test_layout_matches_module_parameters(lib, c):
    for latent in (64, 100):
        rc, poff, boff = _layout(lib, latent, c)
        assert rc == 0
        sizes = [p.numel() for p in eae_amd.SupervisedAutoencoder(latent, in_channels=c).parameters()]
        assert len(sizes) == 38
        for i, n in enumerate(sizes):
            assert poff[i] % 4 == 0 and poff[i + 1] - poff[i] >= n and poff[i + 1] - poff[i] < n + 4, (c, i)
        assert boff[14] == 2 * (32 + 64 + 128 + 256 + 128 + 64 + 32)


def test_in_channels_zero_means_three(lib):
    assert _layout(lib, 64, 0) == _layout(lib, 64, 3)
    cfg = _lib.EaeConfig(64, 10, 64, 64, 8)           # the positional form of the older callers leaves the field 0
    poff = (C.c_longlong * 39)()
    assert lib.eae_ae_layout(C.byref(cfg), poff, None) == 0
    assert list(poff) == _layout(lib, 64, 3)[1]


@pytest.mark.parametrize("c,quant", [(17, 0), (-1, 0), (13, 1)])
def test_layout_rejects_bad_band_counts(lib, c, quant):
    rc, _, _ = _layout(lib, 64, c, quant)
    assert rc == -2 and b"in_channels" in lib.eae_last_error()


def test_fp8_still_takes_rgb(lib):
    cfg = _lib.EaeConfig(64, 10, 128, 256, 8, 1, 0, 3)
    assert lib.eae_ae_layout(C.byref(cfg), None, None) == 0


@pytest.mark.parametrize("bad", [0, 17, -3, 2.5, True])
def test_constructors_reject_out_of_range(bad):
    for ok in (1, 16):        # the keyword exists and takes the band range ...
        eae_amd.SupervisedAutoencoder(64, in_channels=ok)
        eae_amd.Encoder(64, in_channels=ok)
        eae_amd.Decoder(64, out_channels=ok)
    with pytest.raises(ValueError, match="in_channels"):      # ... and refuses what is outside it
        eae_amd.SupervisedAutoencoder(64, in_channels=bad)
    with pytest.raises(ValueError, match="in_channels"):
        eae_amd.Encoder(64, in_channels=bad)
    with pytest.raises(ValueError, match="out_channels"):
        eae_amd.Decoder(64, out_channels=bad)


def test_fit_functions_take_in_channels():
    import inspect
    from eae_amd import train
    for fn in (train.fit_autoencoder, train.fit_autoencoder_group, train.grid_search_autoencoder):
        p = inspect.signature(fn).parameters["in_channels"]
        assert p.default == 3
