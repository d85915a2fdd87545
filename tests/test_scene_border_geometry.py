"""Border arithmetic of eae_amd.scene (no GPU needed): `border_source` against numpy.pad, `border_grid` against the sizes it must
cover, and the border argument checks, which run before anything touches a device."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import scene as S

MODES = ("constant", "edge", "reflect")


@pytest.mark.parametrize("mode", MODES)
def test_border_source_is_numpy_pad(mode):
    """np.pad of arange(n) holds the source index of every padded position (constant: the fill -1 marks None).  The sweep takes every
    n in 1..7 with every pad pair the mode allows; for reflect that is p, q <= n - 1, the single reflection, p = n - 1 included."""
    cases = 0
    for n in range(1, 8):
        top = n - 1 if mode == "reflect" else 9
        for p in range(top + 1):
            for q in range(top + 1):
                kw = {"constant_values": -1} if mode == "constant" else {}
                ref = np.pad(np.arange(n), (p, q), mode, **kw)
                got = [S.border_source(v, p, n, mode) for v in range(p + n + q)]
                assert [-1 if g is None else g for g in got] == ref.tolist(), (n, p, q)
                cases += 1
    assert cases >= 140
    if mode == "reflect":
        assert S.border_source(0, 4, 5, mode) == 4 and S.border_source(8, 0, 5, mode) == 0        # p = n - 1 on either side
        with pytest.raises(RuntimeError):
            S.border_source(0, 5, 5, mode)                                                        # a second reflection
        with pytest.raises(RuntimeError):
            S.border_source(9, 0, 5, mode)


def test_border_source_rejects_an_unknown_mode():
    for mode in ("symmetric", "wrap", None):
        with pytest.raises(RuntimeError, match="border must be"):
            S.border_source(0, 1, 4, mode)


# the GPU cases (tests/test_gpu_scene_border.py), an exact fit, a strip lower than the patch, one window per axis, the 10980-px tile
SHAPES = [(100, 150, 64, 32, (3, 4), (14, 14, 5, 5)), (70, 64, 64, 64, (2, 1), (29, 29, 0, 0)), (40, 200, 64, 48, (1, 4), (12, 12, 4, 4)),
          (128, 192, 64, 64, (2, 3), (0, 0, 0, 0)), (96, 160, 64, 32, (2, 4), (0, 0, 0, 0)), (1, 1, 64, 64, (1, 1), (31, 32, 31, 32)),
          (65, 64, 64, 1, (2, 1), (0, 0, 0, 0)), (10980, 10980, 64, 64, (172, 172), (14, 14, 14, 14)), (129, 200, 128, 96, (2, 2), (47, 48, 12, 12))]


@pytest.mark.parametrize("h,w,p,s,grid,pads", SHAPES)
def test_border_grid_covers_the_scene(h, w, p, s, grid, pads):
    n_h, n_w, got = S.border_grid(h, w, p, s, "center")
    assert (n_h, n_w) == grid and got == pads
    for anchor in ("center", "origin"):
        n_h, n_w, (pt, pb, pl, pr) = S.border_grid(h, w, p, s, anchor)
        assert (n_h, n_w) == grid
        # the extent of the grid is the padded size exactly, every pad is below the patch size, and no window lies in padding alone
        assert (n_h - 1) * s + p == h + pt + pb and (n_w - 1) * s + p == w + pl + pr
        assert all(0 <= v < p for v in (pt, pb, pl, pr))
        assert n_h == 1 or (n_h - 2) * s + p < h + pt
        assert n_w == 1 or (n_w - 2) * s + p < w + pl
        if anchor == "origin":
            assert pt == 0 and pl == 0
        else:
            assert pb - pt in (0, 1) and pr - pl in (0, 1)
        # the borderless grid of the padded size is this grid
        assert S.window_grid(h + pt + pb, w + pl + pr, p, s) == (n_h, n_w)
    assert S.border_grid(100, 150, 64, 32, "origin")[2] == (0, 28, 0, 10)


@pytest.mark.parametrize("args", [(100, 100, 48, 8), (100, 100, 64, 0), (100, 100, 64, 65), (0, 100, 64, 8), (100, 0, 64, 8)])
def test_border_grid_rejects(args):
    with pytest.raises(RuntimeError):
        S.border_grid(*args)
    with pytest.raises(RuntimeError, match="anchor"):
        S.border_grid(100, 100, 64, 32, "centre")


def test_exports():
    for name in ("border_grid", "border_source"):
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))


def test_border_arguments_rejected_before_device_work():
    """Each call fails on its border argument (the message names it), not on the host tensor it is given: the border checks come
    first, on a machine without a device."""
    torch.manual_seed(0)
    enc = eae_amd.Encoder(64, 64, in_channels=3)
    ae = eae_amd.SupervisedAutoencoder(64, 10, in_channels=3)
    mlp = eae_amd.MLP(64, 10)
    u8 = torch.zeros((3, 96, 100), dtype=torch.uint8)
    u16 = torch.zeros((3, 96, 100), dtype=torch.uint16)
    f32 = torch.zeros((3, 96, 100), dtype=torch.float32)
    low = torch.zeros((3, 20, 200), dtype=torch.uint8)          # 20 rows: centre pads 22 / 22 >= 20
    bad = [
        ("border must be", lambda: eae_amd.scene_windows(u8, 1.0, 64, 32, border="wrap")),
        ("border must be", lambda: eae_amd.encode_scene(u8, enc, stride=32, border="symmetric")),
        ("border must be", lambda: eae_amd.classify_scene(u8, enc, mlp, stride=32, border=2)),
        ("anchor must be", lambda: eae_amd.encode_scene(u8, enc, stride=32, border="edge", anchor="centre")),
        ("mirrors once", lambda: eae_amd.encode_scene(low, enc, border="reflect")),
        ("mirrors once", lambda: eae_amd.window_invalid_counts(low, 64, 64, nodata=0, border="reflect")),
        ("mirrors once", lambda: eae_amd.reconstruct_scene(torch.zeros((3, 200, 20), dtype=torch.uint8), ae, border="reflect")),
        ("fill of a uint8", lambda: eae_amd.encode_scene(u8, enc, stride=32, border="constant", fill=1.5)),
        ("fill of a uint8", lambda: eae_amd.encode_scene(u8, enc, stride=32, border="constant", fill=256)),
        ("fill of a uint8", lambda: eae_amd.valid_windows(u8, 64, 32, nodata=0, border="constant", fill=-1)),
        ("fill of a uint16", lambda: eae_amd.scene_reconstruction_error(u16, ae, stride=32, border="constant", fill=65536)),
        ("fill of a uint16", lambda: eae_amd.scene_windows(u16, 1.0, 64, 32, border="constant", fill=float("nan"))),
        ("fill must be a number", lambda: eae_amd.scene_windows(f32, 1.0, 64, 32, border="constant", fill="0")),
        ("fill is the value of border='constant'", lambda: eae_amd.encode_scene(u8, enc, stride=32, fill=7)),
        ("fill is the value of border='constant'", lambda: eae_amd.classify_scene(u8, enc, mlp, stride=32, border="edge", fill=7)),
        ("fill is the value of border='constant'", lambda: eae_amd.scene_windows(f32, 1.0, 64, 32, fill=0.5)),
    ]
    for msg, fn in bad:
        with pytest.raises(RuntimeError, match=msg):
            fn()
    # what passes the border checks fails later, on the host tensor: an edge strip lower than the patch, a float fill of an fp32 scene
    for fn in (lambda: eae_amd.encode_scene(low, enc, border="edge"),
               lambda: eae_amd.scene_windows(f32, 1.0, 64, 32, border="constant", fill=0.5),
               lambda: eae_amd.encode_scene(u8, enc, stride=32, border="constant", fill=255.0)):
        with pytest.raises(RuntimeError, match="HIP device"):
            fn()
    # border=None still refuses a scene smaller than one window
    with pytest.raises(RuntimeError, match="smaller than one"):
        eae_amd.encode_scene(low, enc)
