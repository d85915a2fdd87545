"""Plain fp64 NumPy references for the kernels between the convolutions: BatchNorm statistics / coefficients, and the
classification head.  Each function restates what torch computes (nn.BatchNorm2d, native_batch_norm_backward,
nn.Linear-ReLU-nn.Linear + CrossEntropyLoss); tests/test_ops_reference.py pins them against torch on the CPU in float64.
No GPU, no torch import: the GPU tests import this module for their expected values."""
import numpy as np

F64 = np.float64


def _f64(a):
    return np.asarray(a, dtype=F64)


# ------------------------------------------------------------------------------------------------ BatchNorm
def bn_from_moments(mean, var, count, gamma, beta, rm, rv, momentum, eps):
    """Training-mode BatchNorm of a channel with batch mean `mean` and BIASED batch variance `var` over `count` elements:
    invstd, the apply coefficients s, t (BN(y) = s*y + t) and the momentum update of the running statistics (unbiased
    variance for count > 1; a single element has no unbiased variance, the biased one, 0, is used)."""
    mean, var, gamma, beta = _f64(mean), _f64(var), _f64(gamma), _f64(beta)
    invstd = 1.0 / np.sqrt(var + F64(eps))
    s = gamma * invstd
    t = beta - mean * s
    unb = var * (F64(count) / (F64(count) - 1.0)) if count > 1 else var
    out = {"mean": mean, "var": var, "invstd": invstd, "s": s, "t": t}
    if rm is not None:
        out["running_mean"] = (1.0 - F64(momentum)) * _f64(rm) + F64(momentum) * mean
        out["running_var"] = (1.0 - F64(momentum)) * _f64(rv) + F64(momentum) * unb
    return out


def bn_train_ref(y, gamma, beta, rm, rv, momentum, eps):
    """y [N][C] (N = batch * pixels of one channel): nn.BatchNorm2d in training mode."""
    y = _f64(y)
    return bn_from_moments(y.mean(0), y.var(0), y.shape[0], gamma, beta, rm, rv, momentum, eps)


def moments_from_partials(part, count):
    """mean and biased variance (never negative) from partial sums part [2][C][ntiles] = (sum y, sum y^2) of row chunks."""
    p = _f64(part).sum(2)
    mean = p[0] / F64(count)
    return mean, np.maximum(p[1] / F64(count) - mean * mean, 0.0)


def bn_eval_ref(gamma, beta, rm, rv, eps):
    """nn.BatchNorm2d in eval mode: the affine map of the running statistics."""
    invstd = 1.0 / np.sqrt(_f64(rv) + F64(eps))
    s = _f64(gamma) * invstd
    return {"mean": _f64(rm), "invstd": invstd, "s": s, "t": _f64(beta) - _f64(rm) * s}


def bn_bwd_coef_ref(sum_g, sum_gxhat, count, gamma, mean, invstd):
    """dy = A*g + B*y + C, the way native_batch_norm_backward combines its two sums:
    dy = (g - sum_g / N - xhat * sum_gxhat / N) * gamma * invstd  with  xhat = (y - mean) * invstd."""
    sum_g, sum_gxhat, gamma, mean, invstd = (_f64(a) for a in (sum_g, sum_gxhat, gamma, mean, invstd))
    n = F64(count)
    A = gamma * invstd
    B = -A * invstd * sum_gxhat / n
    C = -A * sum_g / n + A * invstd * mean * sum_gxhat / n
    return A, B, C


def bn_bwd_ref(g, y, gamma, mean, invstd):
    """Training-mode BatchNorm backward on g, y [N][C]: dgamma, dbeta and the exact input gradient dy."""
    g, y, gamma, mean, invstd = (_f64(a) for a in (g, y, gamma, mean, invstd))
    n = F64(y.shape[0])
    xhat = (y - mean) * invstd
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dy = (g - dbeta / n - xhat * dgamma / n) * (gamma * invstd)
    return {"dgamma": dgamma, "dbeta": dbeta, "dy": dy, "xhat": xhat}


def splits_for(n_rows, ntiles, rng):
    """Start rows of `ntiles` non-empty, unequal chunks of n_rows rows."""
    assert 1 <= ntiles <= n_rows
    cuts = np.sort(rng.choice(np.arange(1, n_rows), size=ntiles - 1, replace=False)) if ntiles > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts]).astype(np.int64)


def partials2(u, v, splits):
    """[2][C][ntiles] fp32: per chunk (rows splits[i] .. splits[i+1]) the fp64 sums of u and of v, rounded once to fp32."""
    su = np.add.reduceat(_f64(u), splits, axis=0)
    sv = np.add.reduceat(_f64(v), splits, axis=0)
    return np.ascontiguousarray(np.stack([su.T, sv.T]).astype(np.float32))


def partials(y, splits):
    """[2][C][ntiles] fp32 partial sums (sum y, sum y^2) of arbitrary unequal row chunks of y [N][C]."""
    y = _f64(y)
    return partials2(y, y * y, splits)


# ------------------------------------------------------------------------------------------------ head
def head_ref(z, w1, b1, w2, b2, labels=None):
    """Linear(L,128)-ReLU-Linear(128,C) + CrossEntropyLoss(mean) and its whole backward, fp64.
    Returns logits, and with labels: loss (log-sum-exp form), correct (argmax = first maximum), dz, dw1, db1, dw2, db2."""
    z, w1, b1, w2, b2 = (_f64(a) for a in (z, w1, b1, w2, b2))
    h = np.maximum(z @ w1.T + b1, 0.0)
    lg = h @ w2.T + b2
    out = {"logits": lg, "argmax": lg.argmax(1)}        # np.argmax returns the first maximum
    if labels is None:
        return out
    labels = np.asarray(labels, np.int64)
    nb = lg.shape[0]
    m = lg.max(1, keepdims=True)
    lse = m + np.log(np.exp(lg - m).sum(1, keepdims=True))
    logp = lg - lse
    out["loss"] = float(-logp[np.arange(nb), labels].mean())
    out["correct"] = int((out["argmax"] == labels).sum())
    dl = np.exp(logp)
    dl[np.arange(nb), labels] -= 1.0
    dl /= nb
    dh = (dl @ w2) * (h > 0)
    out.update(dz=dh @ w1, dw1=dh.T @ z, db1=dh.sum(0), dw2=dl.T @ h, db2=dl.sum(0))
    return out
