"""Window-grid and blend-coverage arithmetic of eae_amd.scene against brute-force enumeration, and the argument checks that run
before any device work (no GPU needed)."""
import pytest
import torch

import eae_amd
from eae_amd import scene as S


def _brute_windows(h, w, p, s):
    return [(y, x) for y in range(0, h - p + 1, s) for x in range(0, w - p + 1, s)]


@pytest.mark.parametrize("h,w,p,s", [(64, 64, 64, 64), (64, 64, 64, 1), (130, 203, 64, 7), (150, 97, 64, 20), (256, 200, 128, 32),
                                     (127, 191, 64, 64), (100, 64, 64, 13)])
def test_window_grid_matches_enumeration(h, w, p, s):
    n_h, n_w = S.window_grid(h, w, p, s)
    wins = _brute_windows(h, w, p, s)
    assert n_h * n_w == len(wins)
    for n, org in enumerate(wins):
        assert S.window_origin(n, n_w, s) == org
    # every window lies inside the scene, and one more step on either axis would not
    assert (n_h - 1) * s + p <= h < n_h * s + p
    assert (n_w - 1) * s + p <= w < n_w * s + p


@pytest.mark.parametrize("n_h,n_w,p,s", [(1, 1, 64, 64), (3, 5, 64, 32), (4, 2, 64, 16), (6, 7, 64, 8), (2, 9, 128, 64)])
def test_cell_coverage_matches_enumeration(n_h, n_w, p, s):
    c_h, c_w, k = S.cell_grid(n_h, n_w, p, s)
    assert k == p // s and (c_h, c_w) == (n_h + k - 1, n_w + k - 1)
    cov = S.cell_coverage(n_h, n_w, k)
    assert cov.shape == (c_h, c_w)
    brute = torch.zeros((c_h, c_w), dtype=torch.int64)
    members = {}
    for i in range(n_h):
        for j in range(n_w):
            # window (i, j) spans pixels [i*s, i*s + p): cells i .. i + k - 1
            for ci in range(i, i + k):
                for cj in range(j, j + k):
                    brute[ci, cj] += 1
                    members.setdefault((ci, cj), []).append((i, j))
    assert torch.equal(cov, brute)
    for (ci, cj), ws in members.items():
        i0, i1, j0, j1 = S.cell_windows(ci, cj, n_h, n_w, k)
        assert sorted(ws) == [(i, j) for i in range(i0, i1 + 1) for j in range(j0, j1 + 1)]
    # the cell map covers the pixels of the window grid exactly
    assert c_h * s == (n_h - 1) * s + p and c_w * s == (n_w - 1) * s + p


@pytest.mark.parametrize("h,w,p,s", [(63, 100, 64, 8), (100, 63, 64, 8), (100, 100, 64, 0), (100, 100, 64, 65), (100, 100, 64, -1),
                                     (100, 100, 48, 8), (100, 100, 0, 1)])
def test_window_grid_rejects(h, w, p, s):
    with pytest.raises(RuntimeError):
        S.window_grid(h, w, p, s)


@pytest.mark.parametrize("p,s", [(64, 24), (64, 48), (128, 96), (64, 0)])
def test_blend_needs_a_dividing_stride(p, s):
    with pytest.raises(RuntimeError):
        S.cell_grid(4, 4, p, s)


def test_exports():
    for name in ("scene_windows", "encode_scene", "classify_scene", "window_grid"):
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))


def test_bad_arguments_rejected_before_device_work():
    """CPU tensors, wrong ranks and dtypes, band-count and divisor mismatches, bad strides and an MLP of the wrong width all raise
    before anything touches a device (these run on a machine without one)."""
    torch.manual_seed(0)
    enc = eae_amd.Encoder(64, 64, in_channels=3)
    mlp = eae_amd.MLP(64, 10)
    ok = torch.zeros((3, 96, 96), dtype=torch.uint8)
    bad = [
        lambda: eae_amd.encode_scene(ok, enc),                                          # a host tensor: the scene must be on the device
        lambda: eae_amd.encode_scene(torch.zeros((1, 3, 96, 96), dtype=torch.uint8), enc),          # not planar [C,H,W]
        lambda: eae_amd.encode_scene(torch.zeros((3, 96, 96), dtype=torch.int32), enc),             # dtype
        lambda: eae_amd.encode_scene(torch.zeros((4, 96, 96), dtype=torch.uint8), enc),             # C != in_channels
        lambda: eae_amd.encode_scene(ok, enc, stride=0),
        lambda: eae_amd.encode_scene(ok, enc, stride=65),
        lambda: eae_amd.encode_scene(torch.zeros((3, 63, 96), dtype=torch.uint8), enc),             # smaller than one window
        lambda: eae_amd.encode_scene(ok, enc, divisor=[1.0, 2.0]),                                  # one divisor per band
        lambda: eae_amd.encode_scene(ok, "not an encoder"),
        lambda: eae_amd.classify_scene(ok, enc, eae_amd.MLP(32, 10)),                              # MLP width != latent_dim
        lambda: eae_amd.classify_scene(ok, enc, mlp, stride=24, blend=True),                        # blend: S must divide P
        lambda: eae_amd.scene_windows(ok, 1.0, 64, 8),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
