"""tests/pack_ref.py (the whole-array NumPy layouts the GPU pack tests compare bytes against) pinned to an independent restatement:
for every destination index i of a pack, the source index the layout's definition names -- flat integer arithmetic, one formula per
pack, no reshape or transpose.  Sources hold distinct non-zero numbers, so "every source element exactly once, all padding zero"
is checked too.  Small shapes, with L < Lp and C < CP.  No GPU."""
import numpy as np
import pytest
import torch

import pack_ref as R


def _numbered(shape):
    """fp32 tensor whose elements are 1, 2, 3, ... (distinct, non-zero, exact in fp32)."""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return np.arange(1, n + 1, dtype=np.float32).reshape(shape)


def _gather(src, idx):
    """dst[i] = src.flat[idx[i]], 0 where idx[i] < 0."""
    flat = src.ravel()
    return np.where(idx >= 0, flat[np.maximum(idx, 0)], np.float32(0.0))


def _check(got, src, idx, shape):
    got = np.asarray(got)
    assert got.shape == tuple(shape), (got.shape, shape)
    ref = _gather(src, idx).reshape(shape)
    assert np.array_equal(got, ref)
    # a permutation with zero padding: every source element exactly once, nothing else
    nz = got[got != 0]
    assert nz.size == src.size and np.array_equal(np.sort(nz), np.sort(src.ravel()))
    assert int((got == 0).sum()) == got.size - src.size


@pytest.mark.parametrize("a,b", [(4, 2), (5, 3), (8, 16)])
def test_3x3_layouts(a, b):
    w = _numbered((a, b, 3, 3))
    i = np.arange(a * b * 9)
    # p1 [A][9][B]: i = (ai * 9 + tap) * B + bi
    bi, tap, ai = i % b, (i // b) % 9, i // (9 * b)
    _check(R.p1_3x3(w), w, (ai * b + bi) * 9 + tap, (a, 9, b))
    # p2 [B][9][A]: i = (bi * 9 + tap) * A + ai
    ai, tap, bi = i % a, (i // a) % 9, i // (9 * a)
    _check(R.p2_3x3(w), w, (ai * b + bi) * 9 + tap, (b, 9, a))


@pytest.mark.parametrize("c", [1, 3, 5, 8, 13, 16])
def test_kcp_layout(c):
    cp = R.edge_cp(c)
    kp = R.ceil_to(9 * cp, 32)
    assert (cp, kp) == {1: (8, 96), 3: (4, 64), 5: (8, 96), 8: (8, 96), 13: (16, 160), 16: (16, 160)}[c]
    w = _numbered((32, c, 3, 3))
    i = np.arange(32 * kp)
    k, a = i % kp, i // kp
    tap, ch = k // cp, k % cp
    idx = np.where((tap < 9) & (ch < c), (a * c + np.minimum(ch, c - 1)) * 9 + np.minimum(tap, 8), -1)
    _check(R.kcp(w), w, idx, (32, kp))


@pytest.mark.parametrize("c", [1, 3, 7, 16])
def test_deconv4_joint_layout(c):
    cp = R.edge_cp(c)
    w = _numbered((32, c, 3, 3))
    idx = np.full(4 * cp * 128, -1, np.int64)
    for n in range(4 * c):
        ph, co = divmod(n, c)
        py, px = ph >> 1, ph & 1
        for k in range(128):
            nb, ci = k >> 5, k & 31
            dy, dx = nb >> 1, nb & 1
            # output row 2 y + py of a stride-2, pad-1, 3-tap transposed conv reads input row y + dy through tap ky = py + 1 - 2 dy
            ky, kx = py + 1 - 2 * dy, px + 1 - 2 * dx
            if ky < 0 or kx < 0:
                continue
            idx[n * 128 + k] = (ci * c + co) * 9 + ky * 3 + kx
    _check(R.deconv4_joint(w), w, idx, (4 * cp, 128))


@pytest.mark.parametrize("L,P", [(5, 2), (64, 3), (70, 1)])
def test_fc_layouts(L, P):
    K, Lp = 256 * P, R.ceil_to(L, 64)
    we, wd, b = _numbered((L, K)), _numbered((K, L)), _numbered((K,))
    i = np.arange(Lp * K)
    # we1 [Lp][K'], k' = p * 256 + c  <-  We[r][c * P + p]
    k2, r = i % K, i // K
    c, p = k2 % 256, k2 // 256
    _check(R.we1(we), we, np.where(r < L, np.minimum(r, L - 1) * K + c * P + p, -1), (Lp, K))
    # we2 [K'][Lp]
    r, k2 = i % Lp, i // Lp
    c, p = k2 % 256, k2 // 256
    _check(R.we2(we), we, np.where(r < L, np.minimum(r, L - 1) * K + c * P + p, -1), (K, Lp))
    # wd1 [K'][Lp], row j' = p * 256 + c  <-  Wd[c * P + p][l]
    l, j2 = i % Lp, i // Lp
    c, p = j2 % 256, j2 // 256
    _check(R.wd1(wd), wd, np.where(l < L, (c * P + p) * L + np.minimum(l, L - 1), -1), (K, Lp))
    # wd2 [Lp][K']
    j2, l = i % K, i // K
    c, p = j2 % 256, j2 // 256
    _check(R.wd2(wd), wd, np.where(l < L, (c * P + p) * L + np.minimum(l, L - 1), -1), (Lp, K))
    # bd [K']
    j2 = np.arange(K)
    _check(R.bd(b), b, (j2 % 256) * P + j2 // 256, (K,))
    # w1p [128][Lp], bep [Lp]
    w1, be = _numbered((128, L)), _numbered((L,))
    j = np.arange(128 * Lp)
    _check(R.pad_cols(w1, Lp), w1, np.where(j % Lp < L, (j // Lp) * L + np.minimum(j % Lp, L - 1), -1), (128, Lp))
    j = np.arange(Lp)
    _check(R.pad_cols(be, Lp), be, np.where(j < L, np.minimum(j, L - 1), -1), (Lp,))


def test_bf16_bits_match_torch():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.standard_normal(4096).astype(np.float32) * s for s in (1e-3, 1.0, 300.0)])
    # exact ties between two bf16 neighbours (round to even) and their fp32 neighbours
    ties = (np.arange(0x3F800000, 0x3F800000 + 64 * 0x8000, 0x8000, dtype=np.uint32)).view(np.float32)
    a = np.concatenate([a, ties, np.nextafter(ties, np.float32(4.0)), np.nextafter(ties, np.float32(0.0)), -ties, [0.0]]).astype(np.float32)
    ref = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_bits(a), ref)


def _e4m3_values():
    """value of each non-negative finite OCP e4m3 byte 0x00..0x7E (0x7F is NaN)."""
    b = np.arange(0x7F)
    e, m = b >> 3, b & 7
    return np.where(e == 0, m * 2.0 ** -9, (1 + m / 8.0) * 2.0 ** (e.astype(np.float64) - 7))


def test_fp8_bytes_match_a_table_search():
    vals = _e4m3_values()
    assert vals[-1] == 448.0 and vals[8] == 2.0 ** -6 and vals[1] == 2.0 ** -9
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.standard_normal(2048) * s for s in (2e-3, 0.05, 1.0, 40.0, 600.0)]).astype(np.float32)
    mid = ((vals[:-1] + vals[1:]) / 2).astype(np.float32)           # exact ties between neighbours (representable in fp32)
    a = np.concatenate([a, mid, -mid, vals.astype(np.float32), [1000.0, -1000.0, 448.0, -448.0, 464.0, -464.0]]).astype(np.float32)
    for s_w in (1.0, 0.125, 512.0):
        v = np.clip(a.astype(np.float32) * np.float32(s_w), -448.0, 448.0).astype(np.float64)
        d = np.abs(np.abs(v)[:, None] - vals[None, :])
        best = d.min(1)
        cand = d == best[:, None]                                    # one candidate, or two at a tie: take the even byte
        lo = cand.argmax(1)
        hi = cand.shape[1] - 1 - cand[:, ::-1].argmax(1)
        byte = np.where(lo % 2 == 0, lo, hi).astype(np.uint8)
        byte |= (np.signbit(v).astype(np.uint8) << 7)
        got = R.fp8_bytes(a, s_w)
        assert np.array_equal(got, byte), np.flatnonzero(got != byte)[:8]
    assert R.fp8_bytes(np.float32([1000.0, -1000.0]), 1.0).tolist() == [0x7E, 0xFE]


def test_fp8_scale():
    assert R.fp8_scale(1000.0) == 2.0 ** -3 and R.fp8_scale(0.25) == 512.0 and R.fp8_scale(224.0) == 1.0 and R.fp8_scale(225.0) == 0.5


def test_packs_of_a_small_model():
    """packs(): the right keys, lengths and dtypes; names and shapes agree with the module shells."""
    import eae_amd
    m = eae_amd.SupervisedAutoencoder(latent_dim=50, num_classes=7, image_size=64, in_channels=5)
    names = [n for n, _ in m.named_parameters()]
    assert names == list(R.PARAM_NAMES)
    shapes = R.param_shapes(64, 64, 50, 7, 5)
    assert {n: tuple(p.shape) for n, p in m.named_parameters()} == shapes
    rng = np.random.default_rng(2)
    sd = {n: rng.standard_normal(s).astype(np.float32) for n, s in shapes.items()}
    pk = R.packs(sd, quant_scales=[1.0] * 6)
    assert sorted(pk) == list(range(34))
    K = 256 * 16
    assert pk[R.CONV1].shape == (32, 96) and pk[R.DECONV4_KCP].shape == (32, 96) and pk[R.DECONV4_JOINT].shape == (32, 128)
    assert pk[R.WE1].shape == (64, K) and pk[R.WE2].shape == (K, 64) and pk[R.WD1].shape == (K, 64) and pk[R.WD2].shape == (64, K)
    assert pk[R.W1P].shape == (128, 64) and pk[R.BEP].shape == (64,) and pk[R.BD].shape == (K,)
    for i in range(6):
        assert pk[R.P1 + i].dtype == np.uint16 and pk[R.FP8_P1 + i].dtype == np.uint8 and pk[R.FP8_P1 + i].shape == pk[R.P1 + i].shape
    assert pk[R.W1P].dtype == np.uint32 and pk[R.WE1].dtype == np.uint16
    sd64 = dict(sd)
    shapes64 = R.param_shapes(64, 64, 64, 7, 5)
    for n in ("enc.encoder.13.weight", "enc.encoder.13.bias", "dec.decoder_input.weight", "classifier.0.weight"):
        sd64[n] = rng.standard_normal(shapes64[n]).astype(np.float32)
    assert sorted(R.packs(sd64)) == [i for i in range(22) if i not in (R.W1P, R.BEP)]
