"""NumPy reference of the optimizer unit (csrc/eae_optim.hip) with every fp32 rounding spelled out: the Adam update of adam_body /
adam_update, the fp64 sum-of-squares partials of grad_sumsq_body in the kernel's own order, and the (total, coef) pair of clip_coef.
tests/test_adam_reference.py ties it to exact rational arithmetic, to oracle.ae_numpy.adam_step and to tests/grad_clip_ref.py;
tests/test_gpu_adam_exact.py compares the kernels with it bit for bit.

Assumed of the device: IEEE fp32 and fp64 sqrt, IEEE fp32 division, fused multiply-add with one rounding, subnormals kept (DESIGN.md
section 19).  Assumed of NumPy: one float32 / float64 ufunc call (add, subtract, multiply, divide, sqrt) on arrays of that type is the
correctly rounded IEEE operation with subnormals kept; no expression below holds more than one operation per call, and
tests/test_adam_reference.py checks the assumption on subnormal operands and results."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
EAE_CLIP_MAX_PARTS = 512
ADAM_MAX_BLOCKS = 2048


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == F32, a.dtype
    return a


def _op(fn, a, b):
    """One fp32 operation: both operands fp32, the result fp32."""
    r = fn(_f32(a), _f32(b))
    assert r.dtype == F32
    return r


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding.  a * b is exact in fp64 (48 significant bits, exponents within range); c is added with a
    TwoSum that yields the error of the fp64 sum; an inexact sum whose last mantissa bit is even is stepped to its fp64 neighbour in
    the direction of the error (round to odd: 53 bits >= 24 + 2, so the final rounding to fp32 cannot double-round)."""
    a, b, c = np.broadcast_arrays(_f32(a), _f32(b), _f32(c))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        p = np.multiply(a.astype(F64), b.astype(F64))
        c64 = c.astype(F64)
        s = np.add(p, c64)
        bb = np.subtract(s, p)
        err = np.add(np.subtract(p, np.subtract(s, bb)), np.subtract(c64, bb))
        fix = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        # toward the error: up when err > 0, down when err < 0 (s != 0 here: an inexact fp64 sum is never zero)
        up = np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf))
        s = np.where(fix, up, s)
        return s.astype(F32)


def _exact(x):
    return Fraction(float(x))


def _round_fraction_to_f32(q, zero_sign_negative):
    """Round-to-nearest-even of the rational q to fp32 (subnormals kept, overflow to inf)."""
    if q == 0:
        return F32(-0.0) if zero_sign_negative else F32(0.0)
    sign = -1 if q < 0 else 1
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()      # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                       # 2^e <= q < 2^(e+1)
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    n = q / ulp
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (k & 1)):
        k += 1
    val = k * ulp
    if val >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(val))                                    # exact: at most 24 significant bits, within fp64's range


def fma32_exact(a, b, c):
    """Scalar fl32(a * b + c) on fractions.Fraction: the slow form fma32 is checked against (finite operands only)."""
    a, b, c = F32(a), F32(b), F32(c)
    q = _exact(a) * _exact(b) + _exact(c)
    # an exact zero: -0 only when the product and the addend are both negative zeros (round to nearest)
    prod_neg = bool(np.signbit(a)) != bool(np.signbit(b))
    return _round_fraction_to_f32(q, prod_neg and bool(np.signbit(c)))


def launch_scalars(lr, b1, b2, step):
    """The host side of eae_launch_adam: (step_size, bc2_sqrt, b1f, b2f) as float32.  lr, b1, b2 are the doubles the launcher sees (a
    caller that goes through a C `float` argument rounds to float32 first)."""
    bc1 = 1.0 - math.pow(float(b1), float(step))
    bc2 = 1.0 - math.pow(float(b2), float(step))
    return F32(float(lr) / bc1), F32(math.sqrt(bc2)), F32(b1), F32(b2)


def adam_update(p, g, m, v, *, scalars, eps, wd, geff):
    """One launch of adam_body over fp32 arrays: the new (p, m, v).  geff = fl32(gscale) without clipping, fl32(gscale * coef) with."""
    step_size, bc2_sqrt, b1f, b2f = (F32(s) for s in scalars)
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    eps32, wd32, geff32 = F32(eps), F32(wd), F32(geff)
    one = F32(1.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
        wp = _op(np.multiply, np.full_like(p, wd32), p)                              # wd * P[j]
        gj = fma32(g, np.full_like(g, geff32), wp)                                   # fma(G[j], geff, wp)
        omb1 = _op(np.subtract, one, b1f)                                            # 1.f - b1
        m1 = fma32(np.full_like(m, omb1), _op(np.subtract, gj, m), m)                # fma(1 - b1, gj - m, m)
        omb2 = _op(np.subtract, one, b2f)                                            # 1.f - b2
        t = _op(np.multiply, np.full_like(gj, omb2), gj)                             # (1 - b2) * gj
        v1 = fma32(np.full_like(v, b2f), v, _op(np.multiply, gj, t))                 # fma(b2, v, gj * t)
        root = np.sqrt(v1)
        assert root.dtype == F32
        denom = _op(np.add, _op(np.divide, root, np.full_like(root, bc2_sqrt)), np.full_like(root, eps32))
        q = _op(np.divide, m1, denom)
        p1 = fma32(np.full_like(p, -step_size), q, p)                                # fma(-step_size, m / denom, p)
    return p1, m1, v1


def grad_sumsq_nparts(n):
    """eae_grad_sumsq_parts: one workgroup per 4096 elements, 1 .. 512."""
    return int(min(max((n + 4095) // 4096, 1), EAE_CLIP_MAX_PARTS))


def adam_blocks(n):
    """Workgroups of the optimizer launch over n elements (eae_launch_adam without max_blocks or a group)."""
    return int(min((n // 4 + 255) // 256, ADAM_MAX_BLOCKS))


def piece_valid(poff, sizes):
    """Valid elements of every 16-byte piece of the arena: 4, or the tensor's remainder in the tensor's last piece."""
    valid = np.full(poff[len(sizes)] // 4, 4, dtype=np.int64)
    for s, n in enumerate(sizes):
        if n % 4:
            valid[(poff[s] + n) // 4] = n % 4
    return valid


def block_sum_fixed(v):
    """block_sum_fixed over [blocks, 256] fp64 values: the xor butterfly 32, 16, ..., 1 over the 64 lanes of each wave (the same value
    must end up in every lane), then ((w0 + w1) + w2) + w3."""
    v = np.asarray(v, dtype=F64).reshape(-1, 4, 64).copy()
    lane = np.arange(64)
    o = 32
    while o > 0:
        v = np.add(v, v[:, :, lane ^ o])
        o >>= 1
    assert (v.view(np.int64) == v[:, :, :1].view(np.int64)).all(), "the butterfly left different values in the lanes of a wave"
    w = v[:, :, 0]
    return np.add(np.add(np.add(w[:, 0], w[:, 1]), w[:, 2]), w[:, 3])


def grad_sumsq_parts(arena, poff, sizes):
    """The fp64 partials of grad_sumsq_kernel, in the kernel's order: grid = grad_sumsq_nparts(n) workgroups of 256 threads, T = 256 *
    grid; thread t takes the pieces t + u*T + r*4T (rounds r, and u = 0..3 within a round), adds x^2, y^2, z^2, w^2 of a piece in that
    order, counts only the valid elements of a padded tail piece and nothing of a slot past the end; then block_sum_fixed."""
    g = _f32(arena)
    n = int(poff[len(sizes)])
    assert g.shape == (n,) and n % 4 == 0
    n4 = n // 4
    grid = grad_sumsq_nparts(n)
    T = 256 * grid
    valid = piece_valid(poff, sizes)
    g4 = g.reshape(n4, 4).astype(F64)
    t = np.arange(T)
    acc = np.zeros(T, dtype=F64)
    with np.errstate(over="ignore", invalid="ignore"):
        slot = 0
        while slot * T < n4:                                  # slot = u + 4 r
            i = t + slot * T
            inside = i < n4
            ic = np.where(inside, i, n4 - 1)                  # (past the end: piece n4 - 1 again, with 0 valid elements)
            cnt = np.where(inside, valid[ic], 0)
            q = g4[ic]
            for j in range(4):
                x = np.where(cnt > j, q[:, j], 0.0)           # selected to zero, never multiplied
                acc = np.add(acc, np.multiply(x, x))
            slot += 1
    return block_sum_fixed(acc.reshape(grid, 256))


def clip_total_coef(parts, gscale, max_norm):
    """clip_coef: (total, coef) as float32.  Thread i adds part[i], part[i + 256] onto 0.0, block_sum_fixed, total = fl32(fp64(gscale) *
    sqrt(ss)), coef = min(1, fl32(max_norm / fl32(total + 1e-6f)))."""
    parts = np.asarray(parts, dtype=F64)
    assert 1 <= parts.size <= EAE_CLIP_MAX_PARTS
    v = np.zeros(256, dtype=F64)
    for k in range(0, parts.size, 256):
        chunk = parts[k: k + 256]
        v[: chunk.size] = np.add(v[: chunk.size], chunk)
    ss = block_sum_fixed(v.reshape(1, 256))[0]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        total = F32(np.multiply(F64(F32(gscale)), np.sqrt(F64(ss))))
        den = np.add(np.asarray([total], dtype=F32), np.asarray([1e-6], dtype=F32))
        ratio = np.divide(np.asarray([max_norm], dtype=F32), den)
        assert ratio.dtype == F32
        coef = F32(min(F32(1.0), ratio[0]))                   # fminf(1, x); x is never NaN for max_norm > 0 and total >= 0 finite
    return total, coef


def geff_clipped(gscale, coef):
    """fl32(gscale * coef), the multiplier the clipping kernels feed to the gradient fma."""
    return np.multiply(np.asarray([gscale], dtype=F32), np.asarray([coef], dtype=F32))[0]


def bits(a):
    return np.ascontiguousarray(_f32(a)).view(np.int32)
