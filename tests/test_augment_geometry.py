"""The augmentation policy (`eae_amd.Augment`, ``augment=`` / ``geom=`` / ``affine=`` / ``radio=`` of the staging calls): the three
entry points in the header, the library and the ctypes table, and the argument errors raised on the host, in Python and behind the
C ABI.  No GPU needed."""
import ctypes as C
import os
import re

import pytest
import torch

import eae_amd
from eae_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eae_augment_aug", "eae_stage_bands_aug", "eae_scene_stage_windows_aug")


def test_new_symbols_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.EXPORTS
    assert re.search(r"typedef\s+struct\s+eae_aug\s*\{", src)
    assert "Augment" in eae_amd.__all__ and callable(eae_amd.Augment)
    # the struct of the ctypes table is the header's: an int, five floats, an int
    fields = re.search(r"typedef\s+struct\s+eae_aug\s*\{(.*?)\}\s*eae_aug\s*;", src, flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.EaeAug._fields_]
    assert C.sizeof(_lib.EaeAug) == 28


def test_augment_validates_its_fields():
    a = eae_amd.Augment()
    assert (a.dihedral, a.rotate, a.scale, a.gain, a.band_gain, a.offset) == (False, 0.0, 0.0, 0.0, 0.0, 0.0)
    a = eae_amd.Augment(dihedral=True, rotate=10, scale=0.1, gain=0.2, band_gain=0.1, offset=0.05)
    assert "rotate=10.0" in repr(a) and a.dihedral is True
    for name in ("rotate", "scale", "gain", "band_gain", "offset"):
        with pytest.raises(RuntimeError, match=f"{name} must not be negative"):
            eae_amd.Augment(**{name: -0.1})
        for bad in (float("nan"), float("inf"), "0.1", None, True):
            with pytest.raises(RuntimeError, match=f"{name} must be a finite number"):
                eae_amd.Augment(**{name: bad})
    for name in ("scale", "gain", "band_gain"):
        for bad in (1.0, 1.5):
            with pytest.raises(RuntimeError, match=f"{name} must be below 1"):
                eae_amd.Augment(**{name: bad})
    with pytest.raises(RuntimeError, match="at most 180"):
        eae_amd.Augment(rotate=181)
    with pytest.raises(RuntimeError, match="dihedral must be a bool"):
        eae_amd.Augment(dihedral="yes")
    eae_amd.Augment(offset=3.0)                                     # an offset has no upper limit


def _host_calls(w=12):
    """The three staging calls on host tensors: images of 12 x w, windows of 16 x 16 (everything else in order)."""
    bands = torch.zeros((4, 5, 12, w), dtype=torch.uint16)
    hwc = torch.zeros((4, 12, w, 3), dtype=torch.uint8)
    scene = torch.zeros((5, 37, 41), dtype=torch.uint16)
    ids = torch.tensor([0, 3, 1, 2], dtype=torch.int64)
    return {"stage_bands": (lambda **kw: eae_amd.stage_bands(bands, 10000.0, **kw), 5, False),
            "augment_batch": (lambda **kw: eae_amd.augment_batch(hwc, **kw), 3, False),
            "stage_scene_windows": (lambda **kw: eae_amd.stage_scene_windows(scene, 10000.0, 16, 5, ids, **kw), 5, True)}


@pytest.mark.parametrize("name", ["stage_bands", "augment_batch", "stage_scene_windows"])
def test_staging_calls_host_errors(name):
    call, c, scene = _host_calls()[name]
    if not scene:
        wide = _host_calls(w=20)[name][0]
        with pytest.raises(RuntimeError, match="need square images, got 12 x 20"):
            wide(augment=eae_amd.Augment(dihedral=True))
        with pytest.raises(RuntimeError, match="need square images"):
            wide(geom=torch.zeros((4, 4), dtype=torch.int32))
        with pytest.raises(RuntimeError, match=r"affine must be float32 \[B,2\]"):      # the other parts take any H x W
            wide(augment=eae_amd.Augment(rotate=5.0, gain=0.1), affine=torch.zeros((3, 2)))
    with pytest.raises(RuntimeError, match="augment must be an eae_amd.Augment"):
        call(augment=dict(rotate=5.0))
    with pytest.raises(RuntimeError, match=r"geom must be int32 \[B,4\]"):
        call(geom=torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"geom must be int32 \[B,4\]"):
        call(geom=torch.zeros((3, 4), dtype=torch.int32))
    with pytest.raises(RuntimeError, match=r"geom must be int32 \[B,4\].*dtype"):
        call(geom=torch.zeros((4, 4), dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"affine must be float32 \[B,2\]"):
        call(affine=torch.zeros((4, 3)))
    with pytest.raises(RuntimeError, match=r"affine must be float32 \[B,2\].*dtype"):
        call(affine=torch.zeros((4, 2), dtype=torch.float64))
    with pytest.raises(RuntimeError, match=r"radio must be float32 \[B,C,2\]"):
        call(radio=torch.zeros((4, c + 1, 2)))
    with pytest.raises(RuntimeError, match=r"radio must be float32 \[B,C,2\]"):
        call(radio=torch.zeros((4, c)))
    with pytest.raises(RuntimeError, match=r"radio must be float32 \[B,C,2\].*dtype"):
        call(radio=torch.zeros((4, c, 2), dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"geom int32 \[B,4\].*not params"):
        call(augment=eae_amd.Augment(gain=0.1), params=torch.zeros((4, 3), dtype=torch.int32))
    with pytest.raises(RuntimeError):                               # everything is in order but the data is a host tensor
        call(augment=eae_amd.Augment(rotate=5.0, gain=0.1), affine=torch.zeros((4, 2)), radio=torch.zeros((4, c, 2)))


def test_scene_loader_takes_a_policy_only():
    sc = torch.zeros((3, 100, 150), dtype=torch.uint8)
    label = torch.tensor([[0, 1, -1], [2, -1, 1]], dtype=torch.int64)
    with pytest.raises(RuntimeError, match="augment must be an eae_amd.Augment"):
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, augment="d4")
    with pytest.raises(RuntimeError):                               # everything is in order but the scene is a host tensor
        eae_amd.SceneLoader(sc, label, patch=64, stride=32, augment=eae_amd.Augment(dihedral=True))


# ---------------------------------------------------------------------------------------------------- behind the C ABI
def _c_bands(lib, aug, h=12, w=12, geom=None):
    """eae_stage_bands_aug with pointers that are never read: an argument error is found before anything is launched."""
    fake = C.c_void_p(4096)
    return lib.eae_stage_bands_aug(None, fake, 2, 4, 5, h, w, None, 4, fake, fake, 1, 0.0, 0, 0, aug, geom, None, None, None)


def test_c_abi_rejects_bad_policies():
    lib = _lib.load()
    bad = [_lib.EaeAug(0, -1.0, 0, 0, 0, 0, 0), _lib.EaeAug(0, 181.0, 0, 0, 0, 0, 0), _lib.EaeAug(0, float("nan"), 0, 0, 0, 0, 0),
           _lib.EaeAug(0, 0, 1.0, 0, 0, 0, 0), _lib.EaeAug(0, 0, -0.5, 0, 0, 0, 0), _lib.EaeAug(0, 0, 0, 1.0, 0, 0, 0),
           _lib.EaeAug(0, 0, 0, 0, 1.5, 0, 0), _lib.EaeAug(0, 0, 0, 0, 0, -0.01, 0), _lib.EaeAug(0, 0, 0, 0, 0, float("inf"), 0),
           _lib.EaeAug(0, 0, 0, 0, 0, 0, 3), _lib.EaeAug(1, 0, 0, 0, 0, 0, 2)]                   # the last: LDS draws, 144 pixels
    for aug in bad:
        assert _c_bands(lib, aug) == -2, list(aug._fields_)
        assert b"stage_bands: augment:" in lib.eae_last_error()
    assert _c_bands(lib, _lib.EaeAug(1, 0, 0, 0, 0, 0, 0), h=12, w=20) == -2 and b"square" in lib.eae_last_error()
    assert _c_bands(lib, None, h=12, w=20, geom=C.c_void_p(4096)) == -2 and b"square" in lib.eae_last_error()
    with pytest.raises(_lib.EaeError, match="rotate"):
        _lib.check(_c_bands(lib, bad[0]))
    # the other two entry points share the check
    fake = C.c_void_p(4096)
    assert lib.eae_augment_aug(None, fake, fake, 4, 12, 12, 1, 0.0, 0, 0, bad[3], None, None, None, None) == -2
    assert b"augment: augment: scale" in lib.eae_last_error()
    div = (C.c_float * 5)(*[1.0] * 5)
    desc = _lib.EaeScene(fake, C.cast(div, C.c_void_p), 1, 5, 37, 41, 16, 5)
    assert lib.eae_scene_stage_windows_aug(None, C.byref(desc), fake, 4, fake, 1, 0.0, 0, 0, bad[5], None, None, None, None, 0) == -2
    assert b"scene_stage_windows: augment: gain" in lib.eae_last_error()
