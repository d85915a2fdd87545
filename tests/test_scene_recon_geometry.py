"""Ownership arithmetic of the stitched reconstruction (eae_amd.scene.owned_span) against brute-force enumeration, and the argument
checks of the reconstruction functions that run before any device work (no GPU needed)."""
import pytest
import torch

import eae_amd
from eae_amd import scene as S

_PS = [(64, 64), (64, 32), (64, 2), (128, 64), (64, 62), (64, 20), (128, 2)]


@pytest.mark.parametrize("p,s", _PS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_owned_spans_partition_the_extent(n, p, s):
    extent = (n - 1) * s + p
    owners = [0] * extent
    prev_hi = 0
    for i in range(n):
        lo, hi = S.owned_span(i, n, p, s)
        assert lo == prev_hi and lo < hi                       # no gap, no overlap, never empty
        assert i * s <= lo and hi <= i * s + p                 # inside the window itself
        for y in range(lo, hi):
            owners[y] += 1
        prev_hi = hi
    assert prev_hi == extent
    assert owners == [1] * extent
    # interior windows own the centred S pixels
    m = (p - s) // 2
    for i in range(1, n - 1):
        assert S.owned_span(i, n, p, s) == (i * s + m, i * s + m + s)


@pytest.mark.parametrize("p,s", _PS)
def test_a_single_window_owns_its_whole_patch(p, s):
    assert S.owned_span(0, 1, p, s) == (0, p)


@pytest.mark.parametrize("p,s", [(64, 63), (64, 1), (64, 33), (128, 65)])
def test_odd_patch_minus_stride_raises(p, s):
    with pytest.raises(RuntimeError):
        S.owned_span(0, 3, p, s)


@pytest.mark.parametrize("i,n,p,s", [(3, 3, 64, 32), (-1, 3, 64, 32), (0, 0, 64, 32), (0, 2, 64, 0), (0, 2, 64, 66)])
def test_owned_span_rejects(i, n, p, s):
    with pytest.raises(RuntimeError):
        S.owned_span(i, n, p, s)


def test_exports():
    for name in ("scene_reconstruction_error", "reconstruct_scene", "owned_span"):
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))


def test_bad_arguments_rejected_before_device_work():
    torch.manual_seed(0)
    model = eae_amd.SupervisedAutoencoder(64, 10, in_channels=3)
    enc = eae_amd.Encoder(64, 64, in_channels=3)
    ok = torch.zeros((3, 96, 96), dtype=torch.uint8)
    ids = torch.zeros(1, dtype=torch.int64)
    for fn in (eae_amd.scene_reconstruction_error, eae_amd.reconstruct_scene):
        bad = [
            lambda: fn(ok, enc),                                        # an Encoder has no decoder
            lambda: fn(ok, model.enc),
            lambda: fn(ok, "not a model"),
            lambda: fn(ok, model),                                      # a host tensor: the scene must be on the device
            lambda: fn(ok, model, windows=ids, nodata=0),               # windows= with nodata= / mask=
            lambda: fn(ok, model, windows=ids, mask=torch.zeros((96, 96), dtype=torch.bool)),
            lambda: fn(ok, model, rule="some"),
            lambda: fn(ok, model, max_invalid=1.0),
            lambda: fn(ok, model, stride=0),
            lambda: fn(ok, model, stride=65),
            lambda: fn(torch.zeros((4, 96, 96), dtype=torch.uint8), model),        # C != in_channels
            lambda: fn(torch.zeros((3, 96, 96), dtype=torch.int32), model),        # dtype
            lambda: fn(ok, model, nodata=300),                           # outside the dtype's range
        ]
        for f in bad:
            with pytest.raises(RuntimeError):
                f()
    with pytest.raises(RuntimeError):
        eae_amd.reconstruct_scene(ok, model, stride=33)                 # odd patch - stride
