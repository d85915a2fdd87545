"""eae_mlp_layout_ex / eae_mlp_create_ex on the host: the offset tables against NumPy, the default architecture against
eae_mlp_layout, and every rejected argument (EAE_ERR_ARG before anything is allocated: no GPU is needed to be refused)."""
import ctypes as C

import pytest

import mlp_arch_ref as A
from eae_amd import _lib

ERR_ARG = -2
ARCHS = [(37, (24,), 16), (16, (12, 20, 6, 10), 3), (64, (48, 32, 16), 10), (64, (256, 128, 64), 10), (256, (512, 384), 10),
         (48, (40, 72, 8, 136), 1), (16, (1, 1, 1, 1), 2), (1024, (512, 512, 512, 512), 16), (1, (1,), 1)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _layout(lib, IN, hidden, Cn):
    nh = len(hidden)
    poff, boff = (C.c_longlong * (4 * nh + 3))(), (C.c_longlong * (2 * nh + 1))()
    rc = lib.eae_mlp_layout_ex(IN, Cn, nh, (C.c_int * max(nh, 1))(*hidden), poff, boff)
    return rc, list(poff), list(boff)


@pytest.mark.parametrize("IN,hidden,Cn", ARCHS, ids=[f"in{a[0]}-{'x'.join(map(str, a[1]))}-c{a[2]}" for a in ARCHS])
def test_layout_matches_numpy(lib, IN, hidden, Cn):
    rc, poff, boff = _layout(lib, IN, hidden, Cn)
    assert rc == 0
    want_p, want_b = A.Arch(hidden, 0.0).layout(IN, Cn)
    assert poff == want_p and boff == want_b
    assert all(o % 4 == 0 for o in poff) and boff[-1] == 2 * sum(hidden)
    assert lib.eae_mlp_layout_ex(IN, Cn, len(hidden), (C.c_int * len(hidden))(*hidden), None, None) == 0      # tables are optional


@pytest.mark.parametrize("IN,Cn", [(64, 10), (1, 1), (1024, 16), (37, 5)])
def test_default_architecture_matches_eae_mlp_layout(lib, IN, Cn):
    p0, b0 = (C.c_longlong * 11)(), (C.c_longlong * 5)()
    assert lib.eae_mlp_layout(IN, Cn, p0, b0) == 0
    rc, poff, boff = _layout(lib, IN, (128, 64), Cn)
    assert rc == 0 and poff == list(p0) and boff == list(b0)


BAD = [(0, (128, 64), 10), (1025, (128, 64), 10), (64, (128, 64), 0), (64, (128, 64), 17), (64, (), 10), (64, (8, 8, 8, 8, 8), 10),
       (64, (0,), 10), (64, (128, 513), 10), (64, (-4, 64), 10)]


@pytest.mark.parametrize("IN,hidden,Cn", BAD)
def test_bad_architecture_is_err_arg(lib, IN, hidden, Cn):
    rc, _, _ = _layout(lib, IN, hidden, Cn)
    assert rc == ERR_ARG and lib.eae_last_error()
    h = C.c_void_p()
    nh = len(hidden)
    rates = (C.c_float * max(nh, 1))(*([0.0] * nh))
    assert lib.eae_mlp_create_ex(IN, Cn, nh, (C.c_int * max(nh, 1))(*hidden), rates, 64, C.byref(h)) == ERR_ARG and not h.value


def test_bad_rates_batch_and_pointers_are_err_arg(lib):
    h = C.c_void_p()
    widths = (C.c_int * 2)(128, 64)
    for rates in ((1.0, 0.0), (0.3, -0.1), (0.3, 1.5), (float("nan"), 0.0)):
        assert lib.eae_mlp_create_ex(64, 10, 2, widths, (C.c_float * 2)(*rates), 64, C.byref(h)) == ERR_ARG and not h.value
    ok = (C.c_float * 2)(0.3, 0.0)
    for mb in (0, -1):
        assert lib.eae_mlp_create_ex(64, 10, 2, widths, ok, mb, C.byref(h)) == ERR_ARG and not h.value
    assert lib.eae_mlp_create_ex(64, 10, 2, widths, None, 64, C.byref(h)) == ERR_ARG and not h.value
    assert lib.eae_mlp_create_ex(64, 10, 2, None, ok, 64, C.byref(h)) == ERR_ARG and not h.value
    assert lib.eae_mlp_create_ex(64, 10, 2, widths, ok, 64, None) == ERR_ARG
    assert lib.eae_mlp_layout_ex(64, 10, 2, None, None, None) == ERR_ARG
    with pytest.raises(_lib.EaeError):
        _lib.check(lib.eae_mlp_layout_ex(64, 10, 0, widths, None, None))
