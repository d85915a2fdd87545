"""The tile plan of the stride-2 conv launches (csrc/eae_conv_plan.h) through eae_op_conv_s2_ntiles, against the closed form
ceil(B / NI) * (Hpos / TH) * (Wpos / TW) with the geometries from a literal table (host code only: no GPU)."""
import os

import pytest

import conv_ref as R
from conv_ref import GRIDS, IGEMM_EXACT_CASES
from eae_amd import _lib
from test_gpu_ops_path import IGEMM_CASES


def _expected(kind, cin, cout, B, hin, win=None):
    """the closed form for the geometry of conv_ref's literal table (the one copy the tests hold), under this process's settings"""
    win = hin if win is None else win
    hp, wp = (hin // 2, win // 2) if kind == 0 else (hin, win)
    return R.expected_ntiles(kind, cin, cout, hp, wp, B, R.ig_small_setting())


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from eae_amd import build
        build.build(verbose=False)
    return _lib.load()


def test_ntiles_is_the_closed_form(lib):
    assert len(IGEMM_CASES) == 12
    for kind, cin, cout, hin, _, _, _ in IGEMM_CASES:
        for scale in (1, 4):                                       # the layer's map at 64x64 and at 256x256 images
            for B in range(1, 601):
                got = lib.eae_op_conv_s2_ntiles(kind, cin, B, hin * scale, hin * scale)
                assert got == _expected(kind, cin, cout, B, hin * scale), (kind, cin, B, hin * scale)


def test_ntiles_on_rectangular_and_multi_tile_grids(lib):
    """The position grids of the bit-exact kernel tests (conv_ref.GRIDS: 4x4, 8x8, one tile, 2x2 tiles, two across, three down)."""
    assert [g[:2] for g in GRIDS] == [(4, 4), (8, 8), (8, 16), (16, 32), (8, 32), (24, 16)]
    for kind, cin, cout, _, _, _, _ in IGEMM_CASES:
        for hp, wp, _ in GRIDS:
            hin, win = (2 * hp, 2 * wp) if kind == 0 else (hp, wp)
            for B in range(1, 601):
                got = lib.eae_op_conv_s2_ntiles(kind, cin, B, hin, win)
                assert got == _expected(kind, cin, cout, B, hin, win), (kind, cin, B, hin, win)
    # rows and columns are not interchangeable: 16 rows x 8 columns has no geometry, 8 rows x 16 columns is one tile per image
    assert _expected(1, 64, 32, 3, 16, 8) == -1 and lib.eae_op_conv_s2_ntiles(1, 64, 3, 16, 8) == -1
    assert _expected(1, 64, 32, 3, 8, 16) == 3 and lib.eae_op_conv_s2_ntiles(1, 64, 3, 8, 16) == 3
    assert lib.eae_op_conv_s2_ntiles(0, 32, 1, 48, 32) == 3 and lib.eae_op_conv_s2_ntiles(0, 32, 1, 16, 64) == 2


def test_every_bit_exact_case_hits_the_geometry_it_names(lib):
    """What test_gpu_conv_geometry.py asserts per case on the GPU, here for the whole table at once."""
    for kind, cin, cout, smode, epi, hp, wp, B in IGEMM_EXACT_CASES:
        hin, win = (2 * hp, 2 * wp) if kind == 0 else (hp, wp)
        assert lib.eae_op_conv_s2_ntiles(kind, cin, B, hin, win) == _expected(kind, cin, cout, B, hin, win), (kind, cin, hp, wp, B)


def test_conv_kind_boundary_at_4x4(lib):
    # 128 -> 256 on a 4x4 output: (B + 3) / 4 tiles of 4 images while the 8-image grid has fewer than 256 workgroups, (B + 7) / 8 after
    assert lib.eae_op_conv_s2_ntiles(0, 128, 504, 8, 8) == 126
    assert lib.eae_op_conv_s2_ntiles(0, 128, 505, 8, 8) == 64


def test_unsupported_map_is_the_error_value(lib):
    assert lib.eae_op_conv_s2_ntiles(0, 64, 8, 12, 12) == -1       # 6x6 output
    assert lib.eae_op_conv_s2_ntiles(1, 128, 8, 6, 6) == -1        # 6x6 input
    assert lib.eae_op_conv_s2_ntiles(1, 64, 8, 16, 12) == -1       # 12 columns
