"""NumPy restatement of every weight pack the engine derives from its parameters (pack_all_kernel; the enumeration of
include/eae.h, EAE_DEBUG_PACK), as whole-array operations on the state_dict tensors.  A pack is a permutation plus one rounding,
so the result is exact: `packs()` returns the bytes the pack arena must hold.  tests/test_pack_reference.py pins every formula
to an element-by-element restatement of the index arithmetic.

Shapes: CP = padded band count (4 / 8 / 16), KP = 9 * CP rounded up to 32, P = positions of the 256-channel map (h / 16 * w / 16),
K = 256 * P, Lp = latent width rounded up to 64.
"""
import numpy as np

from oracle import ae_numpy as O

# state_dict names of the 38 parameter tensors in arena order (model.parameters() order of SupervisedAutoencoder)
PARAM_NAMES = (
    [f"enc.encoder.{i}.{k}" for i in (0, 1, 3, 4, 6, 7, 9, 10) for k in ("weight", "bias")]
    + ["enc.encoder.13.weight", "enc.encoder.13.bias", "dec.decoder_input.weight", "dec.decoder_input.bias"]
    + [f"dec.decoder.{i}.{k}" for i in (1, 2, 4, 5, 7, 8, 10) for k in ("weight", "bias")]
    + [f"classifier.{i}.{k}" for i in (0, 2) for k in ("weight", "bias")])
# the six 3x3 layers with p1 / p2 (and fp8) packs: conv2, conv3, conv4, deconv1, deconv2, deconv3
W3_NAMES = ("enc.encoder.3.weight", "enc.encoder.6.weight", "enc.encoder.9.weight",
            "dec.decoder.1.weight", "dec.decoder.4.weight", "dec.decoder.7.weight")

# pack indices (include/eae.h)
CONV1, P1, P2, DECONV4_JOINT, DECONV4_KCP, WE1, WE2, WD1, WD2, W1P, BEP, BD, FP8_P1, FP8_P2 = 0, 1, 7, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 28
PACK_LABEL = {CONV1: "conv1", DECONV4_JOINT: "deconv4_joint", DECONV4_KCP: "deconv4_kcp", WE1: "we1", WE2: "we2", WD1: "wd1",
              WD2: "wd2", W1P: "w1p", BEP: "bep", BD: "bd"}
for _i in range(6):
    PACK_LABEL[P1 + _i], PACK_LABEL[P2 + _i] = f"p1[{_i}]", f"p2[{_i}]"
    PACK_LABEL[FP8_P1 + _i], PACK_LABEL[FP8_P2 + _i] = f"fp8_p1[{_i}]", f"fp8_p2[{_i}]"


def edge_cp(c):
    return 4 if c == 3 else 8 if c <= 8 else 16


def ceil_to(n, m):
    return (n + m - 1) // m * m


def param_shapes(h, w, latent, classes, bands):
    """Shapes of the 38 tensors, keyed by state_dict name."""
    K = 256 * (h // 16) * (w // 16)
    s = {}
    for i, (co, ci) in zip((0, 3, 6, 9), ((32, bands), (64, 32), (128, 64), (256, 128))):
        s[f"enc.encoder.{i}.weight"], s[f"enc.encoder.{i}.bias"] = (co, ci, 3, 3), (co,)
        s[f"enc.encoder.{i + 1}.weight"], s[f"enc.encoder.{i + 1}.bias"] = (co,), (co,)
    s["enc.encoder.13.weight"], s["enc.encoder.13.bias"] = (latent, K), (latent,)
    s["dec.decoder_input.weight"], s["dec.decoder_input.bias"] = (K, latent), (K,)
    for i, (ci, co) in zip((1, 4, 7, 10), ((256, 128), (128, 64), (64, 32), (32, bands))):
        s[f"dec.decoder.{i}.weight"], s[f"dec.decoder.{i}.bias"] = (ci, co, 3, 3), (co,)
        if i != 10:
            s[f"dec.decoder.{i + 1}.weight"], s[f"dec.decoder.{i + 1}.bias"] = (co,), (co,)
    s["classifier.0.weight"], s["classifier.0.bias"] = (128, latent), (128,)
    s["classifier.2.weight"], s["classifier.2.bias"] = (classes, 128), (classes,)
    return {n: s[n] for n in PARAM_NAMES}


# ---------------------------------------------------------------------------------------------------------------
# layouts (values, fp32; no rounding yet)
# ---------------------------------------------------------------------------------------------------------------
def p1_3x3(w):
    """[A][B][3][3] -> [A][9][B]"""
    a, b = w.shape[:2]
    return w.reshape(a, b, 9).transpose(0, 2, 1)


def p2_3x3(w):
    """[A][B][3][3] -> [B][9][A]"""
    a, b = w.shape[:2]
    return w.reshape(a, b, 9).transpose(1, 2, 0)


def kcp(w):
    """[32][C][3][3] -> [32][KP], k = tap * CP + c; zero for c >= C and k >= 9 * CP."""
    a, c = w.shape[:2]
    cp = edge_cp(c)
    t = np.zeros((a, 9, cp), w.dtype)
    t[:, :, :c] = w.reshape(a, c, 9).transpose(0, 2, 1)
    out = np.zeros((a, ceil_to(9 * cp, 32)), w.dtype)
    out[:, :9 * cp] = t.reshape(a, 9 * cp)
    return out


_D4_TAP = {(0, 0): 1, (1, 0): 2, (1, 1): 0}       # (output parity, neighbour) -> kernel tap; (0, 1) has none


def deconv4_joint(w):
    """[32 ci][C co][3][3] -> [4 * CP][128]: row n = (py * 2 + px) * C + co (rows >= 4 C zero), column k = (dy * 2 + dx) * 32 + ci."""
    ci_n, c = w.shape[:2]
    out = np.zeros((4 * edge_cp(c), 128), w.dtype)
    for py in (0, 1):
        for px in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    if (py, dy) not in _D4_TAP or (px, dx) not in _D4_TAP:
                        continue
                    ky, kx = _D4_TAP[(py, dy)], _D4_TAP[(px, dx)]
                    r0, k0 = (py * 2 + px) * c, (dy * 2 + dx) * 32
                    out[r0:r0 + c, k0:k0 + ci_n] = w[:, :, ky, kx].T
    return out


def pad_rows(a, n):
    out = np.zeros((n,) + a.shape[1:], a.dtype)
    out[:a.shape[0]] = a
    return out


def pad_cols(a, n):
    out = np.zeros(a.shape[:-1] + (n,), a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def we1(we):
    """enc.fc weight [L][c * P + p] -> [Lp][p * 256 + c]"""
    L, K = we.shape
    return pad_rows(we.reshape(L, 256, K // 256).transpose(0, 2, 1).reshape(L, K), ceil_to(L, 64))


def we2(we):
    return we1(we).T


def wd1(wd):
    """dec.fc weight [c * P + p][L] -> [p * 256 + c][Lp]"""
    K, L = wd.shape
    return pad_cols(wd.reshape(256, K // 256, L).transpose(1, 0, 2).reshape(K, L), ceil_to(L, 64))


def wd2(wd):
    return wd1(wd).T


def bd(b):
    """dec.fc bias [c * P + p] -> [p * 256 + c]"""
    return b.reshape(256, -1).T.ravel()


# ---------------------------------------------------------------------------------------------------------------
# bytes
# ---------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """uint16 bits of the bf16 rounding (to nearest even) of fp32 values."""
    r = O.bf16_round(np.ascontiguousarray(a, dtype=np.float32))
    return (r.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def fp8_bytes(a, s_w):
    """e4m3 bytes of sat(w * s_w): the product in fp32, clipped to +-448, rounded to nearest even."""
    v = np.clip(np.ascontiguousarray(a, dtype=np.float32) * np.float32(s_w), np.float32(-448.0), np.float32(448.0))
    return O.fp8_bytes_e4m3(O.fp8_round(v, "e4m3"))


def fp8_scale(amax):
    """The weight scale delayed scaling derives from a reported max |w|: 2^floor(log2(448 / (2 amax)))."""
    return float(2.0 ** np.floor(np.log2(448.0 / (2.0 * float(amax)))))


def packs(sd, quant_scales=None):
    """{pack index: contiguous array of the pack's bits (uint16 bf16 / uint32 fp32 / uint8 e4m3)} for a state_dict of fp32 arrays.
    w1p and bep appear only when the latent width is no multiple of 64, the fp8 packs only with quant_scales (s_w of the six layers)."""
    out = {CONV1: bf16_bits(kcp(sd["enc.encoder.0.weight"]))}
    for i, n in enumerate(W3_NAMES):
        out[P1 + i], out[P2 + i] = bf16_bits(p1_3x3(sd[n])), bf16_bits(p2_3x3(sd[n]))
    out[DECONV4_JOINT] = bf16_bits(deconv4_joint(sd["dec.decoder.10.weight"]))
    out[DECONV4_KCP] = bf16_bits(kcp(sd["dec.decoder.10.weight"]))
    we, wd = sd["enc.encoder.13.weight"], sd["dec.decoder_input.weight"]
    out[WE1], out[WD1] = bf16_bits(we1(we)), bf16_bits(wd1(wd))
    out[WE2], out[WD2] = np.ascontiguousarray(out[WE1].T), np.ascontiguousarray(out[WD1].T)
    L = we.shape[0]
    if L % 64:
        out[W1P] = f32_bits(pad_cols(sd["classifier.0.weight"], ceil_to(L, 64)))
        out[BEP] = f32_bits(pad_cols(sd["enc.encoder.13.bias"], ceil_to(L, 64)))
    out[BD] = f32_bits(bd(sd["dec.decoder_input.bias"]))
    if quant_scales is not None:
        for i, n in enumerate(W3_NAMES):
            out[FP8_P1 + i] = np.ascontiguousarray(fp8_bytes(p1_3x3(sd[n]), quant_scales[i]))
            out[FP8_P2 + i] = np.ascontiguousarray(fp8_bytes(p2_3x3(sd[n]), quant_scales[i]))
    return {k: np.ascontiguousarray(v) for k, v in out.items()}
