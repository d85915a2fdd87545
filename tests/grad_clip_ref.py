"""NumPy fp64 reference of the engine's global gradient-norm clipping (include/eae.h eae_set_grad_clip), pinned to
torch.nn.utils.clip_grad_norm_(norm_type=2) by tests/test_grad_clip_reference.py:

    total = s * sqrt(sum g_i^2)  over the 38 gradient tensors of the arena (the padding eae_ae_layout leaves behind a tensor excluded)
    coef  = min(1, max_norm / (total + 1e-6))
"""
import numpy as np


def ae_param_sizes(latent, classes, size=64, bands=3):
    """Elements of the 38 parameter tensors in arena order (named_parameters() order of SupervisedAutoencoder)."""
    P = (size // 16) * (size // 16)
    K, L, C, N = 256 * P, latent, classes, bands
    return [32 * 9 * N, 32, 32, 32, 64 * 32 * 9, 64, 64, 64, 128 * 64 * 9, 128, 128, 128, 256 * 128 * 9, 256, 256, 256,
            L * K, L, K * L, K, 256 * 128 * 9, 128, 128, 128, 128 * 64 * 9, 64, 64, 64, 64 * 32 * 9, 32, 32, 32,
            32 * 9 * N, N, 128 * L, 128, C * 128, C]


def layout_offsets(sizes):
    """eae_ae_layout's offsets: every tensor rounded up to 4 elements; 39 values, the last one = the arena length."""
    off = [0]
    for n in sizes:
        off.append(off[-1] + (n + 3) // 4 * 4)
    return off


def padding_index(poff, sizes):
    """Arena indices of the padding elements."""
    idx = []
    for s, n in enumerate(sizes):
        idx.extend(range(poff[s] + n, poff[s + 1]))
    return np.asarray(idx, dtype=np.int64)


def grad_norm(arena, poff, sizes, grad_scale=1.0):
    """s * L2 norm over the 38 tensors of a flat gradient arena, fp64."""
    a = np.asarray(arena, dtype=np.float64)
    ss = 0.0
    for s, n in enumerate(sizes):
        t = a[poff[s]: poff[s] + n]
        ss += float(np.dot(t, t))
    return float(grad_scale) * float(np.sqrt(ss))


def clip_coef(total, max_norm):
    """torch's clip coefficient, fp64."""
    return float(min(1.0, float(max_norm) / (float(total) + 1e-6)))


def clip_coef_f32(total, max_norm):
    """The same expression evaluated in float32 (what the optimizer kernel computes from its float32 total)."""
    with np.errstate(over="ignore"):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(total) + np.float32(1e-6)))
