"""Exact restatement of csrc/eae_bn_acc.h: the fixed-point arithmetic of the folded BatchNorm finalize.

Python integers carry the sums (with the wrap modulo 2^64 of the unsigned atomic add and the SIGNED read of the consumers made
explicit), numpy.float32 / numpy.float64 scalars carry every floating-point operation in the order the header has them, one rounding
per operation (no fused multiply-add: the check program is built with -ffp-contract=off).  test_bn_acc_reference.py holds the C++ to
this bit for bit; test_gpu_bn_range.py takes the limits from here.

accumulate() is the one vectorised function: the conversion of many contributions at once, in NumPy's float32 / int64 arithmetic,
which is exact too (rint rounds to nearest even like llrintf, and a float32 below 2^62 in magnitude converts to int64 exactly).
accumulate_ints() is the same with Python integers, one contribution at a time; the test compares the two."""
import numpy as np

F32, F64 = np.float32, np.float64
SCALE_FWD = F32(2.0 ** 24)
SCALE_BWD = F32(2.0 ** 42)
TOTAL = 2.0 ** 62
PARENT_LIMIT = F32(9.0e18)        # the rule of the commits before eae_bn_acc.h: one constant, whatever the launch


def limit(contributions, world=1):
    """bn_acc_limit: what |v * scale| of one contribution must stay below"""
    n = F64(max(int(contributions), 1)) * F64(max(int(world), 1))
    return F32(F64(TOTAL) / n)


def value_limit(scale, contributions, world=1):
    return limit(contributions, world) / F32(scale)


def parent_limit(contributions, world=1):
    return PARENT_LIMIT


def signed(total):
    """the consumers' read of an accumulator word: two's complement"""
    total &= (1 << 64) - 1
    return total - (1 << 64) if total >> 63 else total


def accumulate(values, scale, lim):
    """values: float32 array of one channel's contributions -> (accumulator word as an unsigned Python int, flag)"""
    with np.errstate(over="ignore", invalid="ignore"):
        sv = np.asarray(values, F32) * F32(scale)
        fits = np.abs(sv) < F32(lim)
        fixed = np.rint(sv[fits]).astype(np.int64)
    word = int(fixed.view(np.uint64).sum(dtype=np.uint64)) if fixed.size else 0      # uint64 sums wrap
    return word, bool((~fits).any())


def accumulate_ints(values, scale, lim):
    """the same, one contribution at a time with Python integers; also returns the sum that did not wrap"""
    word, true_sum, flag = 0, 0, False
    for v in np.asarray(values, F32):
        with np.errstate(over="ignore", invalid="ignore"):
            sv = F32(v) * F32(scale)
        if abs(sv) < F32(lim):
            q = int(np.rint(F64(sv)))                   # (a float32 is a float64: the same round-to-nearest-even integer)
            true_sum += q
            word = (word + q) & ((1 << 64) - 1)
        else:
            flag = True
    return word, flag, true_sum


def fwd_finish(w1, w2, flag, scale, count, eps, gamma, beta):
    """accumulator words -> dict(s, t, mean, invstd: float32; var: float64)    (bn_acc_fwd_finish)"""
    inv_scale, count = F32(1.0) / F32(scale), F32(count)
    with np.errstate(all="ignore"):
        a = F64(np.nan) if flag else F64(signed(w1)) * F64(inv_scale)
        b = F64(signed(w2)) * F64(inv_scale)
        mean = a / F64(count)
        var = b / F64(count) - mean * mean
        if var < 0.0:
            var = F64(0.0)
        invstd = F32(1.0) / np.sqrt(F32(var) + F32(eps))
        s = F32(gamma) * invstd
        t = F32(beta) - F32(mean) * s
    return dict(s=s, t=t, mean=F32(mean), invstd=invstd, var=var)


def running(o, count, momentum, rm, rv):
    """(bn_acc_running) -> new running mean, running variance"""
    count, momentum = F32(count), F32(momentum)
    with np.errstate(all="ignore"):
        unb = o["var"] * F64(count) / (F64(count) - F64(1.0)) if count > 1 else o["var"]
        rm = (F32(1.0) - momentum) * F32(rm) + momentum * o["mean"]
        rv = (F32(1.0) - momentum) * F32(rv) + momentum * F32(unb)
    return rm, rv


def bwd_finish(w1, w2, flag, scale, count, gamma, mean, invstd):
    """accumulator words -> dict(A, Bc, Cc, dgamma, dbeta)    (bn_acc_bwd_finish)"""
    inv_scale, count, mean, invstd = F32(1.0) / F32(scale), F32(count), F32(mean), F32(invstd)
    with np.errstate(all="ignore"):
        db = F32(np.nan) if flag else F32(F64(signed(w1)) * F64(inv_scale))
        dg = F32(np.nan) if flag else F32(F64(signed(w2)) * F64(inv_scale))
        A = F32(gamma) * invstd
        Bc = -A * invstd * dg / count
        Cc = -A * db / count - Bc * mean
    return dict(A=A, Bc=Bc, Cc=Cc, dgamma=dg, dbeta=db)


def bits(x):
    return int(np.asarray(x, F32).view(np.uint32))
