"""The NumPy reference of the optimizer unit (tests/adam_ref.py) against independent statements of the same arithmetic: its fused
multiply-add against exact rational arithmetic bit for bit, its Adam update against oracle.ae_numpy.adam_step (the torch semantics the
oracle is pinned to), its sum-of-squares partials and clip coefficient against tests/grad_clip_ref.py on the four arena layouts of
tests/test_gpu_adam_exact.py, and the partition property of the partials exactly."""
import numpy as np
import pytest

import adam_ref as A
import grad_clip_ref as R
from oracle import ae_numpy as O

F32 = np.float32
# (latent, bands, classes): elements, norm workgroups, norm rounds of 4 slots, optimizer workgroups -- the last one reaches the
# 512-workgroup cap of the norm kernel, a second round of its loop, and the 2048-workgroup cap of the optimizer
LAYOUTS = {(64, 3, 10): (1316048, 322, 1, 1286), (48, 1, 10): (1181760, 289, 1, 1155), (128, 13, 7): (1853976, 453, 1, 1811),
           (256, 3, 10): (2913680, 512, 2, 2048)}


def _fma_cases():
    rng = np.random.default_rng(2024)
    a, b, c = [], [], []

    def add(x, y, z):
        a.append(np.asarray(x, dtype=F32)); b.append(np.asarray(y, dtype=F32)); c.append(np.asarray(z, dtype=F32))

    n = 3000
    # random normals over many binades
    sc = lambda: (rng.standard_normal(n) * 10.0 ** rng.uniform(-12, 12, n)).astype(F32)
    add(sc(), sc(), sc())
    # total and near-total cancellation: c = -fl32(a * b), the next fp32 on either side, and the exact case of a short product
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    z = -(x * y)
    add(x, y, z)
    add(x, y, np.nextafter(z, F32(np.inf)))
    add(x, y, np.nextafter(z, F32(-np.inf)))
    xs, ys = rng.integers(-4096, 4096, n).astype(F32), rng.integers(-4096, 4096, n).astype(F32)
    add(xs, ys, -(xs * ys))
    # products on fp32 midpoints with a tiny c of either sign: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24, and odd k: (1 + k 2^-12)^2
    k = rng.integers(0, 2048, n) * 2 + 1
    mid = (1.0 + k * 2.0 ** -12).astype(F32)
    mid[:64] = F32(1.0 + 2.0 ** -12)
    assert (mid.astype(np.float64) == 1.0 + np.where(np.arange(n) < 64, 1, k) * 2.0 ** -12).all()
    tiny = (2.0 ** -rng.integers(60, 91, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)).astype(F32)
    add(mid, mid, tiny)
    add(mid, mid, np.zeros(n, dtype=F32))
    add(mid * F32(2.0 ** -70), mid * F32(2.0 ** -70), (tiny * np.float64(2.0 ** -50)).astype(F32))      # the same on subnormal results
    # subnormal results and operands
    add(sc() * F32(1e-20), sc() * F32(1e-20), (rng.standard_normal(n) * 1e-40).astype(F32))
    add((rng.standard_normal(n) * 1e-39).astype(F32), rng.standard_normal(n).astype(F32), (rng.standard_normal(n) * 1e-39).astype(F32))
    # overflow
    add(sc() * F32(1e25), sc() * F32(1e10), sc())
    # signed zeros
    zs = np.asarray([0.0, -0.0, 1.5, -1.5], dtype=F32)
    g = np.stack(np.meshgrid(zs, zs, np.asarray([0.0, -0.0], dtype=F32), indexing="ij"), -1).reshape(-1, 3)
    add(g[:, 0], g[:, 1], g[:, 2])
    add(np.asarray([1.5, -1.5, 1.5, -1.5], dtype=F32), np.asarray([2.0, 2.0, -2.0, -2.0], dtype=F32), np.asarray([-3.0, 3.0, 3.0, -3.0], dtype=F32))
    return np.concatenate(a), np.concatenate(b), np.concatenate(c)


def test_fma32_equals_exact_rational_arithmetic_bit_for_bit():
    a, b, c = _fma_cases()
    assert a.size >= 10000 and np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()
    got = A.fma32(a, b, c)
    want = np.asarray([A.fma32_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=F32)
    bad = np.flatnonzero(A.bits(got) != A.bits(want))
    assert bad.size == 0, [(a[i], b[i], c[i], got[i], want[i]) for i in bad[:5]]
    # the cases bite: the product rounded in fp64 and again in fp32 differs from the fused result somewhere, results are subnormal,
    # infinite and zero of both signs somewhere
    with np.errstate(over="ignore"):
        naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (A.bits(naive) != A.bits(want)).sum() > 0
    tiny = np.finfo(F32).tiny
    assert ((want != 0) & (np.abs(want) < tiny)).sum() > 100 and np.isinf(want).sum() > 10
    assert ((want == 0) & np.signbit(want)).sum() > 0 and ((want == 0) & ~np.signbit(want)).sum() > 100


def test_numpy_float32_operations_keep_subnormals_and_round_once():
    """What adam_ref assumes of NumPy: a float32 ufunc call is the IEEE operation.  Checked against the fp64 result rounded once (for
    one + - * / or sqrt of fp32 operands the fp64 rounding in between is harmless: 53 >= 2 * 24 + 2) on operands and results in the
    subnormal range."""
    rng = np.random.default_rng(7)
    n = 20000
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-44, -30, n)).astype(F32)
    y = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)).astype(F32)
    y[y == 0] = 1
    assert ((x != 0) & (np.abs(x) < np.finfo(F32).tiny)).sum() > 1000
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for got, want in ((x * y, x64 * y64), (x / y, x64 / y64), (x + x[::-1], x64 + x64[::-1]), (x - x[::-1], x64 - x64[::-1]),
                      (np.sqrt(np.abs(x)), np.sqrt(np.abs(x64)))):
        assert got.dtype == F32 and (A.bits(got) == A.bits(want.astype(F32))).all()


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_adam_update_follows_the_oracles_adam_step(wd):
    """5 steps from zero moments on the same inputs, at the tolerance tests/test_gpu_ops.py::test_adam_kernel grants the kernel against
    this oracle."""
    n = 4099
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(n).astype(F32)
    po = {"w": p0.copy()}
    st = O.new_adam_state()
    p, m, v = p0.copy(), np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    for step in range(1, 6):
        g = rng.standard_normal(n).astype(F32)
        O.adam_step(po, {"w": g}, st, 1e-3, weight_decay=wd)
        p, m, v = A.adam_update(p, g, m, v, scalars=A.launch_scalars(1e-3, 0.9, 0.999, step), eps=1e-8, wd=wd, geff=1.0)
    assert st["step"] == 5
    np.testing.assert_allclose(p, po["w"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m, st["m"]["w"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v, st["v"]["w"], rtol=1e-5, atol=1e-6)
    assert np.abs(p - p0).max() > 1e-3


def test_clipped_multiplier_and_scalars():
    s = A.launch_scalars(float(F32(5e-3)), 0.9, 0.999, 2)
    assert all(isinstance(x, F32) for x in s)
    assert s[0] == F32(float(F32(5e-3)) / (1.0 - 0.9 ** 2)) and s[1] == F32(np.sqrt(1.0 - 0.999 ** 2))
    # at large step counts the bias corrections round to 1 (step 100000) or sit next to it (step 1000: 1 - 0.999^1000 = 0.632...)
    big = A.launch_scalars(1e-3, 0.9, 0.999, 100000)
    assert big[0] == F32(1e-3) and big[1] == F32(1.0)
    assert A.launch_scalars(1e-3, 0.9, 0.999, 1000)[0] == F32(1e-3)
    assert A.geff_clipped(0.5, F32(0.3)) == F32(0.5) * F32(0.3)


@pytest.fixture(scope="module", params=list(LAYOUTS), ids=lambda c: "L%d-N%d-C%d" % c)
def layout(request):
    cfg = request.param
    sizes = R.ae_param_sizes(cfg[0], cfg[2], 64, cfg[1])
    return cfg, sizes, R.layout_offsets(sizes)


def test_launch_geometry_of_the_four_layouts(layout):
    cfg, sizes, poff = layout
    n, parts, rounds, blocks = LAYOUTS[cfg]
    assert poff[38] == n
    assert A.grad_sumsq_nparts(n) == parts and A.adam_blocks(n) == blocks
    T = 256 * parts
    assert -(-(n // 4) // (4 * T)) == rounds
    assert -(-(n // 4) // (256 * blocks)) == rounds      # the optimizer's grid-stride loop
    valid = A.piece_valid(poff, sizes)
    assert int(valid.sum()) == sum(sizes) and (valid > 0).all()


def test_partials_and_coefficient_against_the_fp64_reference(layout):
    """Two fp64 summation orders of n non-negative terms differ by 2 n 2^-53 relative at the most (each of at most n - 1 additions
    errs by 2^-53 relative of a partial sum that is no larger than the total, in either order)."""
    cfg, sizes, poff = layout
    n = poff[38]
    rng = np.random.default_rng(n)
    arena = (rng.standard_normal(n) * 1e-2).astype(F32)
    arena[R.padding_index(poff, sizes)] = 1e4
    parts = A.grad_sumsq_parts(arena, poff, sizes)
    assert parts.dtype == np.float64 and parts.shape == (LAYOUTS[cfg][1],)
    ss = float(parts.sum())
    for gs in (1.0, 0.5):
        ref = R.grad_norm(arena, poff, sizes, gs)
        want_ss = (ref / gs) ** 2
        assert abs(ss - want_ss) <= 2 * n * 2.0 ** -53 * want_ss
        max_norm = 0.5 * ref
        total, coef = A.clip_total_coef(parts, gs, max_norm)
        assert total.dtype == F32 and coef.dtype == F32
        assert abs(float(total) - ref) <= 2.0 ** -24 * ref * (1 + 1e-6)
        assert A.bits(np.asarray([coef]))[0] == A.bits(np.asarray([R.clip_coef_f32(total, max_norm)]))[0]
        assert 0.4 < coef < 0.6
        assert A.clip_total_coef(parts, gs, float("inf"))[1] == 1.0 and A.clip_total_coef(parts, gs, 4 * ref)[1] == 1.0


def test_partials_count_every_valid_element_exactly_once(layout):
    cfg, sizes, poff = layout
    n = poff[38]
    arena = np.ones(n, dtype=F32)
    pad = R.padding_index(poff, sizes)
    arena[pad] = 1e4
    parts = A.grad_sumsq_parts(arena, poff, sizes)
    assert float(parts.sum()) == float(sum(sizes)) == float(n - len(pad))
    assert (parts == np.floor(parts)).all() and parts.min() >= 0
    total, coef = A.clip_total_coef(parts, 0.5, float("inf"))
    assert total == F32(0.5 * np.sqrt(np.float64(sum(sizes)))) and coef == 1.0
    # one hot: every other element contributes nothing, a padding element nothing at all
    arena[:] = 0
    arena[poff[17] + sizes[17] - 1] = 2.0 ** -3
    assert A.clip_total_coef(A.grad_sumsq_parts(arena, poff, sizes), 1.0, float("inf"))[0] == F32(2.0 ** -3)
    arena[:] = 0
    arena[pad] = 1e4
    assert A.clip_total_coef(A.grad_sumsq_parts(arena, poff, sizes), 1.0, float("inf")) == (F32(0.0), F32(1.0))
