"""The tile plan of the stride-2 conv launches (csrc/eae_conv_plan.h) through eae_op_conv_s2_ntiles, against the closed form
ceil(B / NI) * (Hpos / TH) * (Wpos / TW) with the geometries from a literal table (host code only: no GPU)."""
import os

import pytest

from eae_amd import _lib
from test_gpu_ops_path import IGEMM_CASES

# (TW, TH, NI): tile width x height in positions (conv: of the output map, transposed: of the input map), images per tile
WIDE = (16, 8, 1)                                                 # position grids that are multiples of 8 rows x 16 columns
NARROW = {(0, 8): ((8, 8, 2), (8, 8, 1)), (0, 4): ((4, 4, 8), (4, 4, 4)),      # (kind, side): (large tiles, small tiles)
          (1, 8): ((8, 8, 1), (8, 8, 1)), (1, 4): ((4, 4, 4), (4, 4, 4))}     # (transposed kind: small = narrower channel blocks)


def _cdiv(a, b):
    return -(-a // b)


def _tiles(geo, B, pos):
    tw, th, ni = geo
    return _cdiv(B, ni) * (pos // th) * (pos // tw)


def _expected(kind, cin, cout, B, hin):
    pos = hin // 2 if kind == 0 else hin
    if pos % 16 == 0:
        return _tiles(WIDE, B, pos)
    if (kind, pos) not in NARROW:
        return -1
    large, small = NARROW[kind, pos]
    takes_small = kind == 1 or cin >= 64                           # the conv kind has small tiles from 64 input channels on
    is_small = _tiles(large, B, pos) * (cout // 64) < 256          # the large-tile grid leaves CUs empty (EAE_IG_SMALL unset)
    return _tiles(small if takes_small and is_small else large, B, pos)


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


def test_conv_kind_boundary_at_4x4(lib):
    # 128 -> 256 on a 4x4 output: (B + 3) / 4 tiles of 4 images while the 8-image grid has fewer than 256 workgroups, (B + 7) / 8 after
    assert lib.eae_op_conv_s2_ntiles(0, 128, 504, 8, 8) == 126
    assert lib.eae_op_conv_s2_ntiles(0, 128, 505, 8, 8) == 64


def test_unsupported_map_is_the_error_value(lib):
    assert lib.eae_op_conv_s2_ntiles(0, 64, 8, 12, 12) == -1       # 6x6 output
    assert lib.eae_op_conv_s2_ntiles(1, 128, 8, 6, 6) == -1        # 6x6 input
    assert lib.eae_op_conv_s2_ntiles(1, 64, 8, 16, 12) == -1       # 12 columns
