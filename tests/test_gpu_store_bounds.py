"""Output stores through per-workgroup buffer windows (OutRsrc, csrc/eae_common.hip.h): nothing dropped, nothing outside the tensor.

Every case calls an op of the C ABI with each output placed inside a larger allocation, guard bands in front and behind, twice
with two different sentinel fills, and once into plain buffers.  It asserts that
  * the guard bands still hold the sentinel (no store landed outside the tensor),
  * the two sentinel runs are bitwise equal (so every in-range byte was written: a byte left alone would keep its fill),
  * they are bitwise equal to the run into plain buffers.
A scratch area the op need not fill completely is checked for its guard bands only.  The shapes are the smallest that reach each
edge: a last tile with one valid image, a second M-block with one valid row, a last window with one valid piece.

eae_op_adam takes arena lengths that are multiples of 4 floats only (4099 is refused with EAE_ERR_ARG, asserted below), so the
optimizer case runs n = 4100: 1025 pieces of 16 bytes, the second workgroup's window holds one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_gpu_ops_path import IGEMM_CASES, WGRAD_CASES, Src, _pack

pytestmark = pytest.mark.gpu

GUARD = 4096            # bytes in front of and behind every output (keeps the 256-byte alignment of the allocation)
FILLS = (0x5A, 0xA5)


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


def _banded(run, sizes, full=None, init=None):
    """run(ptrs) launches the op with its outputs at ptrs; sizes = bytes per output; full[i] False: guard bands only;
    init[i]: a uint8 tensor the output holds before the call (in/out arenas), None: the sentinel."""
    full = full or [True] * len(sizes)
    init = init or [None] * len(sizes)
    results = []
    for fill in FILLS + (None,):
        bufs = []
        for nb, ini in zip(sizes, init):
            lo = 0 if fill is None else GUARD
            whole = torch.full((lo + nb + lo,), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
            if ini is not None:
                whole[lo:lo + nb] = ini
            bufs.append((whole, lo, nb))
        run([C.c_void_p(w.data_ptr() + lo) for w, lo, _ in bufs])
        torch.cuda.synchronize()
        for i, (w, lo, nb) in enumerate(bufs):
            if fill is not None:
                assert bool((w[:lo] == fill).all()), f"output {i}: front guard band overwritten"
                assert bool((w[lo + nb:] == fill).all()), f"output {i}: rear guard band overwritten"
        results.append([w[lo:lo + nb].clone() for w, lo, nb in bufs])
    for i, (a, b, p) in enumerate(zip(*results)):
        if full[i]:
            assert torch.equal(a, b), f"output {i}: {int((a != b).sum())} bytes keep their sentinel (store dropped)"
            assert torch.equal(a, p), f"output {i}: differs from the run into a plain buffer"
    return results[2]


# ---------------------------------------------------------------------------------------------------- stride-2 conv family
def _case(kind, cin, cout, smode, epi):
    """the row of test_gpu_ops_path.IGEMM_CASES for this instantiation: (kind, cin, cout, hin, smode, epi, B)"""
    rows = [c for c in IGEMM_CASES if (c[0], c[1], c[2], c[4], c[5]) == (kind, cin, cout, smode, epi)]
    assert len(rows) == 1, (kind, cin, cout, smode, epi)
    return rows[0]


def _run_conv(lib, kind, cin, cout, smode, epi, hin=None, B=None):
    import gpu_util as G
    from eae_amd._lib import check
    row = _case(kind, cin, cout, smode, epi)
    hin = hin or row[3]
    B = B or row[6]
    rng = np.random.default_rng(7000 + 37 * cin + 11 * kind + smode + 3 * epi + B)
    src = Src(smode, (B, cin, hin, hin), rng)
    hout = hin // 2 if kind == 0 else hin * 2
    shape = (cout, cin, 3, 3) if kind == 0 else (cin, cout, 3, 3)
    w = (rng.standard_normal(shape) / np.sqrt(9 * cin)).astype(np.float32)
    buf, p1, p2 = _pack(lib, w)
    wp = p1 if kind == 0 else p2
    bd = G.f32(rng.standard_normal(cout).astype(np.float32)) if epi == 0 else None
    nt = lib.eae_op_conv_s2_ntiles(kind, cin, B, hin, hin)
    assert nt > 0
    yprev_d = pcoef_d = None
    if epi == 1:
        yprev_d = G.to_nhwc_bf16(rng.standard_normal((B, cout, hout, hout)).astype(np.float32))
        pcoef_d = G.f32(np.stack([1.0 + 0.2 * rng.standard_normal(cout), 0.3 * rng.standard_normal(cout),
                                  0.1 * rng.standard_normal(cout), 1.0 + 0.2 * rng.random(cout)]).astype(np.float32))
    sizes = [B * hout * hout * cout * 2] + ([2 * cout * nt * 4] if epi != 2 else [])

    def run(ptrs):
        check(lib.eae_op_conv_s2(G.stream(), kind, src.src, cin, cout, B, hin, hin, G.ptr(wp), G.ptr(bd), ptrs[0],
                                 ptrs[1] if epi != 2 else None, epi, G.ptr(yprev_d), G.ptr(pcoef_d)))
    out = _banded(run, sizes)[0]
    assert bool((out.view(torch.int16) != 0).any())


# (kind, cin, cout, source mode, epilogue, input size, batch): the position grid is 4x4 / 8x8 / 16 wide
CONV_CASES = [
    (0, 128, 256, 1, 0, 8, 1), (0, 128, 256, 1, 0, 8, 9),      # conv kind on a 4x4 grid: one image; a last tile with one valid image
    (1, 256, 128, 2, 1, 4, 5),                                  # transposed kind on 4x4 (one-role kernel: mask epilogue)
    (1, 128, 64, 1, 0, 8, 3),                                   # transposed kind on 8x8
    (0, 32, 64, 1, 0, 32, 1),                                   # 16-wide conv tile, forward
    (1, 64, 32, 2, 1, 16, 1),                                   # 16-wide transposed tile, mask epilogue with yprev: two passes, paired px rows
    (1, 256, 128, 0, 0, 4, 5),                                  # wave-specialised kernel, transposed 256 -> 128 forward (its default layer)
]


@pytest.mark.parametrize("kind,cin,cout,smode,epi,hin,B", CONV_CASES)
def test_conv_s2_output_window(lib, kind, cin, cout, smode, epi, hin, B):
    _run_conv(lib, kind, cin, cout, smode, epi, hin, B)


# run in a child with EAE_IG_SMALL=0 (read once per process): the 8-images-per-tile geometry of the conv kind at 4x4 that large batches
# take -- forward on the wave-specialised kernel (its default layer), backward-data of dec.deconv1 on the one-role kernel
LARGE_TILE_CASES = [(0, 128, 256, 1, 0, 8, 1), (0, 128, 256, 1, 0, 8, 9), (0, 128, 256, 2, 2, 8, 9)]


def _large_tile_child():
    from eae_amd import _lib
    lib_ = _lib.load()
    assert lib_.eae_op_conv_s2_ntiles(0, 128, 9, 8, 8) == 2      # 8 images per tile
    for c in LARGE_TILE_CASES:
        _run_conv(lib_, *c)
    print("large-tile cases ok")


def test_conv_s2_output_window_8_images_per_tile():
    env = dict(os.environ, EAE_IG_SMALL="0")
    code = "import conftest, test_gpu_store_bounds as t; t._large_tile_child()"
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "large-tile cases ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------- latent projections
@pytest.mark.parametrize("M", [1, 129])
def test_fc_bias_bf16_output_window(lib, M):
    import gpu_util as G
    from eae_amd._lib import check
    L, Pn = 64, 16
    K = 256 * Pn
    g = torch.Generator(device="cuda").manual_seed(M)
    zd = torch.randn((M, L), device="cuda", generator=g)
    wd = (torch.randn((K, L), device="cuda", generator=g) * 0.1).to(torch.bfloat16)
    bd = torch.randn((K,), device="cuda", generator=g)
    _banded(lambda p: check(lib.eae_op_fc_bias_bf16(G.stream(), G.ptr(zd), G.ptr(wd), M, K, L, G.ptr(bd), p[0])), [M * K * 2])


@pytest.mark.parametrize("M", [1, 129])
def test_fc_splitk_output_window(lib, M):
    import gpu_util as G
    from eae_amd._lib import check
    N, Pn = 64, 16
    K = 256 * Pn
    g = torch.Generator(device="cuda").manual_seed(100 + M)
    ad = torch.randn((M, K), device="cuda", generator=g).to(torch.bfloat16)
    wd = (torch.randn((N, K), device="cuda", generator=g) * 0.02).to(torch.bfloat16)
    bd = torch.randn((N,), device="cuda", generator=g)
    need = (K // 128) * M * N
    # outputs: the result and the split-K partials (exactly `need` floats, every one written)
    _banded(lambda p: check(lib.eae_op_fc_splitk(G.stream(), G.src(0, ad), G.ptr(wd), M, N, K, G.ptr(bd), None, p[1], need, p[0])),
            [M * N * 4, need * 4])


# ---------------------------------------------------------------------------------------------------- edge layers
def _pack_edge(lib, w, c, cp):
    import gpu_util as G
    kp = (9 * cp + 31) // 32 * 32
    wd = G.f32(w)
    wpack = torch.zeros(32 * kp, dtype=torch.bfloat16, device="cuda")
    wjoint = torch.zeros(4 * cp * 128, dtype=torch.bfloat16, device="cuda")
    assert lib.eae_op_pack_edge(G.stream(), G.ptr(wd), c, G.ptr(wpack), G.ptr(wjoint)) == 0, lib.eae_last_error()
    return wpack, wjoint


EDGE_C, EDGE_CP, EDGE_H, EDGE_W = 3, 4, 8, 64       # the smallest image the edge kernels take: one 4 x 32 tile of the 32-channel map


def test_edge_conv_output_window(lib):
    import gpu_util as G
    from eae_amd._lib import check
    rng = np.random.default_rng(31)
    x = G.f32(rng.random((1, EDGE_C, EDGE_H, EDGE_W), dtype=np.float32))
    wpack, _ = _pack_edge(lib, (rng.standard_normal((32, EDGE_C, 3, 3)) * 0.2).astype(np.float32), EDGE_C, EDGE_CP)
    bd = G.f32((rng.standard_normal(32) * 0.1).astype(np.float32))
    ho, wo = EDGE_H // 2, EDGE_W // 2
    nt = (ho // 4) * (wo // 32)
    _banded(lambda p: check(lib.eae_op_edge_conv_c(G.stream(), 0, G.ptr(x), EDGE_C, 1, EDGE_H, EDGE_W, G.ptr(wpack), G.ptr(bd), p[0], p[1],
                                                   0, None, None)), [ho * wo * 32 * 2, 2 * 32 * nt * 4])


def test_deconv4_loss_output_windows(lib):
    import gpu_util as G
    from eae_amd import _lib as L
    from eae_amd._lib import check
    rng = np.random.default_rng(32)
    hin, win = EDGE_H // 2, EDGE_W // 2
    a3 = G.to_nhwc_bf16(rng.standard_normal((1, 32, hin, win)).astype(np.float32))
    _, wjoint = _pack_edge(lib, (rng.standard_normal((32, EDGE_C, 3, 3)) * 0.2).astype(np.float32), EDGE_C, EDGE_CP)
    bd = G.f32((rng.standard_normal(EDGE_C) * 0.1).astype(np.float32))
    xd = G.f32(rng.random((1, EDGE_C, EDGE_H, EDGE_W), dtype=np.float32))
    ntiles = (hin // 4) * (win // 32)
    lps = (EDGE_C + 4) // 4 * 4
    src = L.EaeSrc(a3.data_ptr(), None, None, 0)
    gscale = 2.0 / (EDGE_C * EDGE_H * EDGE_W)
    # outputs: x_hat fp32 NCHW, g bf16 NHWC-CP, loss partials
    _banded(lambda p: check(lib.eae_op_deconv4_loss_c(G.stream(), src, EDGE_C, 1, hin, win, G.ptr(wjoint), G.ptr(bd), G.ptr(xd),
                                                      C.c_float(gscale), p[0], p[1], p[2])),
            [EDGE_C * EDGE_H * EDGE_W * 4, EDGE_H * EDGE_W * EDGE_CP * 2, ntiles * lps * 4])


def test_edge_wgrad_output_windows(lib):
    import gpu_util as G
    from eae_amd import _lib as L
    from eae_amd._lib import check
    rng = np.random.default_rng(33)
    x = G.f32(rng.random((1, EDGE_C, EDGE_H, EDGE_W), dtype=np.float32))
    side_d = G.to_nhwc_bf16((rng.standard_normal((1, 32, EDGE_H // 2, EDGE_W // 2)) * 0.1).astype(np.float32))
    side = L.EaeSrc(side_d.data_ptr(), None, None, 0)
    nsc = 1 << 16                                    # >= 288 * C floats per workgroup; the op need not fill it
    _banded(lambda p: check(lib.eae_op_edge_wgrad_c(G.stream(), 0, G.ptr(x), EDGE_C, 1, EDGE_H, EDGE_W, side, p[0], nsc, p[1])),
            [nsc * 4, 32 * EDGE_C * 9 * 4], full=[False, True])


# ---------------------------------------------------------------------------------------------------- 3x3 weight gradient
def test_wgrad_s2_output_windows(lib):
    import gpu_util as G
    from eae_amd._lib import check
    cs, cb, hs, smode, bmode, B = [c for c in WGRAD_CASES if (c[0], c[1], c[2]) == (256, 128, 4)][0]
    rng = np.random.default_rng(34)
    small = Src(smode, (B, cs, hs, hs), rng)
    big = Src(bmode, (B, cb, 2 * hs, 2 * hs), rng)
    nsc = 6 * 1024 * 1024                            # what the parity tests hand in; the op need not fill it
    _banded(lambda p: check(lib.eae_op_wgrad_s2(G.stream(), small.src, big.src, cs, cb, B, hs, hs, p[0], nsc, p[1])),
            [nsc * 4, cs * cb * 9 * 4], full=[False, True])


# ---------------------------------------------------------------------------------------------------- optimizer, packs
def test_adam_output_windows(lib):
    import gpu_util as G
    from eae_amd._lib import check
    n = 4100                                         # 1025 pieces: the second workgroup's window holds one
    g = torch.Generator(device="cuda").manual_seed(35)
    p0 = torch.randn((n,), device="cuda", generator=g) + 3.0
    gd = torch.randn((n,), device="cuda", generator=g) + 2.0
    zero = torch.zeros((n,), device="cuda")
    init = [p0.view(torch.uint8), zero.view(torch.uint8), zero.view(torch.uint8)]
    got = _banded(lambda p: check(lib.eae_op_adam(G.stream(), p[0], G.ptr(gd), p[1], p[2], n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1)),
                  [n * 4] * 3, init=init)
    # in/out arenas: a dropped store would leave the old value -- every element of p, m and v changes in this step
    for new, old in zip(got, init):
        assert bool((new.view(torch.int32) != old.view(torch.int32)).all())
    # an arena length that is no multiple of 4 floats is refused and nothing is written
    pd, md, vd = p0.clone(), zero.clone(), zero.clone()
    assert lib.eae_op_adam(G.stream(), G.ptr(pd), G.ptr(gd), G.ptr(md), G.ptr(vd), 4099, 1e-3, 0.9, 0.999, 1e-8, 1e-4, 1) == -2
    torch.cuda.synchronize()
    assert torch.equal(pd, p0) and torch.equal(md, zero) and torch.equal(vd, zero)


def test_pack3x3_output_windows(lib):
    import gpu_util as G
    from eae_amd._lib import check
    a, b = 64, 32
    wd = torch.randn((a, b, 3, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(36))
    _banded(lambda p: check(lib.eae_op_pack3x3(G.stream(), G.ptr(wd), a, b, p[0], p[1])), [a * b * 9 * 2] * 2)
