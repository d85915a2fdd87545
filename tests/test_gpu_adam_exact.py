"""The optimizer kernels (csrc/eae_optim.hip: adam_body, grad_sumsq_body, clip_coef) against the NumPy reference tests/adam_ref.py, bit
for bit: every element of the parameters and of both moments compared as int32, the (total, coef) pair of the clipping launch
compared as bits, and the norm's "every element exactly once" probed with values whose sums are exact.

  a. the kernel alone through eae_op_adam: lengths around the store window, four workgroups and past the 2048-workgroup grid; weight
     decay off / on; steps 1, 2, 3, 1000, 100000; random normals plus blocks of signed zeros, subnormals, underflowing and overflowing
     squares, second moments around the square root's scaling thresholds, zero parameters under weight decay and m = g;
  b. the engine's arenas at the three shapes of tests/test_gpu_grad_clip.py (64x64 images, batch 8) after a train step and a gradient
     step, clipping off and on, weight decay and grad_scale off / on; and one synthetic case at latent 256, where the norm kernel
     reaches its 512-workgroup cap and a second round of its loop and the clipped optimizer its 2048-workgroup cap;
  c. all-ones and one-hot gradients under max_norm = inf and lr = 0 at those four shapes.

The replayed step (adam_dyn_*, eae_launch_set_dyn) and the grouped twins (*_g) are held to these bits by the equality tests of
tests/test_gpu_graph_optimizer.py and tests/test_gpu_grad_clip.py."""
import functools

import numpy as np
import pytest
import torch

import adam_ref as A
import grad_clip_ref as R
import test_gpu_grad_clip as GC
from test_gpu_grad_clip import ALPHA, CONFIGS, LR

pytestmark = pytest.mark.gpu
F32 = np.float32
BIG = (256, 3, 10)
B1, B2, EPS = 0.9, 0.999, 1e-8                       # AdamLaunch's defaults: what the engine steps with
LENGTHS = [4, 1020, 1024, 1028, 4096, 2 * 1024 * 1024 + 4 * 257]
STEPS = [1, 2, 3, 1000, 100000]
NSPECIAL = 7 * 64


def _assert_same_bits(got, want, inputs, what):
    """got, want: name -> fp32 array.  Every element, as int32; on a mismatch the first few elements with their inputs."""
    msgs = []
    for k in want:
        assert got[k].shape == want[k].shape and got[k].dtype == F32
        bad = np.flatnonzero(A.bits(got[k]) != A.bits(want[k]))
        print(f"{what}: {k}: {bad.size} of {want[k].size} elements differ")
        if bad.size:
            for i in bad[:6]:
                ins = ", ".join(f"{n}={float(a[i])!r}" for n, a in inputs.items())
                msgs.append(f"{k}[{i}]: kernel {float(got[k][i])!r} ({A.bits(got[k])[i]:#x}) reference {float(want[k][i])!r} "
                            f"({A.bits(want[k])[i]:#x}) from {ins}")
            msgs.append(f"{k}: {bad.size} elements differ")
    assert not msgs, what + "\n" + "\n".join(msgs)


def _no_nan(ref):
    assert not any(np.isnan(a).any() for a in ref), "the reference itself yields NaN: the inputs are wrong"


# ----------------------------------------------------------------------------------------------------------- a. the kernel alone
def _special_blocks(rng):
    """(p, g, m, v) of 7 blocks of 64 elements, one per class (module docstring)."""
    n = 64
    nrm = lambda s=1.0: (rng.standard_normal(n) * s).astype(F32)
    sgn = lambda: rng.choice([-1.0, 1.0], n).astype(F32)
    pos = lambda s: (np.abs(rng.standard_normal(n)) * s + s * 1e-3).astype(F32)
    zero4 = np.asarray([0.0, -0.0, 0.0, -0.0] * 16, dtype=F32), np.asarray([0.0, 0.0, -0.0, -0.0] * 16, dtype=F32)
    blocks = []
    # 1. g = +-0 with p = +-0 (the signed zero of wd * p and of g + wd * p)
    blocks.append((zero4[1], zero4[0], nrm(0.1), pos(1e-2)))
    # 2. subnormal g
    g = (sgn() * rng.integers(1, 1 << 23, n).astype(np.float64) * 2.0 ** -149).astype(F32)
    assert ((g != 0) & (np.abs(g) < np.finfo(F32).tiny)).all()
    blocks.append((nrm(), g, nrm(0.1), pos(1e-2)))
    # 3. |g| ~ 1e-23: g * t underflows to 0; with v = 0 denom is eps alone (p = 0 in the first half, so that weight decay keeps gj tiny)
    p = nrm(); p[:32] = 0
    blocks.append((p, (sgn() * rng.uniform(0.5e-23, 2e-23, n)).astype(F32), nrm(0.1), np.zeros(n, dtype=F32)))
    # 4. |g| ~ 1e21: g * t overflows, v' = inf, m' / denom = 0 and the parameter stays
    blocks.append((nrm(), (sgn() * rng.uniform(1e21, 4e21, n)).astype(F32), nrm(0.1), pos(1e-2)))
    # 5. v around the thresholds of sqrtf: subnormal v, the smallest normal, the expansion's scaling threshold 2^-96; g = p = 0
    v = np.concatenate([rng.integers(1, 1 << 23, 16).astype(np.float64) * 2.0 ** -149,
                        2.0 ** -126 * (1 + rng.integers(-3, 4, 16) * 2.0 ** -24),
                        2.0 ** -96 * (1 + rng.integers(-8, 9, 16) * 2.0 ** -23),
                        10.0 ** rng.uniform(-44, -28, 16)]).astype(F32)
    assert (v > 0).all()
    blocks.append((np.zeros(n, dtype=F32), np.zeros(n, dtype=F32), nrm(1e-12), v))
    # 6. p = +-0 with wd > 0
    blocks.append((zero4[0], nrm(1e-2), nrm(0.1), pos(1e-2)))
    # 7. m = g: the lerp is exact
    g = nrm(1e-2)
    blocks.append((nrm(), g, g.copy(), pos(1e-4)))
    return [np.concatenate([b[k] for b in blocks]) for k in range(4)]


@functools.lru_cache(maxsize=None)
def _kernel_inputs(n):
    """Random normals over several binades with non-zero first moments and v >= 0; the special blocks end 8 elements in front of the
    end (inside the last store window), and at a length too short for them every (length / 448)-th of their elements is taken."""
    rng = np.random.default_rng(1000 + n)
    p = rng.standard_normal(n).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)).astype(F32)
    m = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1, n)).astype(F32)
    v = (np.square(rng.standard_normal(n)) * 10.0 ** rng.uniform(-8, -2, n)).astype(F32)
    sp = _special_blocks(rng)
    assert sp[0].size == NSPECIAL
    if n >= NSPECIAL + 64:
        at = n - 8 - NSPECIAL
        for a, s in zip((p, g, m, v), sp):
            a[at: at + NSPECIAL] = s
    else:
        pick = np.linspace(0, NSPECIAL - 1, n).astype(np.int64)
        for a, s in zip((p, g, m, v), sp):
            a[:] = s[pick]
    assert (v >= 0).all() and np.abs(m).max() > 0
    for a in (p, g, m, v):
        a.setflags(write=False)
    return p, g, m, v


@pytest.fixture(scope="module")
def lib():
    from eae_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("n", LENGTHS)
def test_kernel_alone_equals_the_reference_bit_for_bit(lib, n, wd, step):
    import gpu_util as G
    from eae_amd._lib import check
    lr = 1e-3
    p, g, m, v = _kernel_inputs(n)
    ref = A.adam_update(p, g, m, v, scalars=A.launch_scalars(lr, B1, B2, step), eps=EPS, wd=wd, geff=1.0)
    _no_nan(ref)
    pd, gd, md, vd = (G.f32(a.copy()) for a in (p, g, m, v))          # fresh buffers for every call
    check(lib.eae_op_adam(G.stream(), G.ptr(pd), G.ptr(gd), G.ptr(md), G.ptr(vd), n, lr, B1, B2, EPS, wd, step))
    torch.cuda.synchronize()
    got = {"p": pd.cpu().numpy(), "m": md.cpu().numpy(), "v": vd.cpu().numpy()}
    assert np.array_equal(A.bits(gd.cpu().numpy()), A.bits(g))
    _assert_same_bits(got, dict(zip("pmv", ref)), {"p": p, "g": g, "m": m, "v": v}, f"n {n} wd {wd} step {step}")
    if n >= NSPECIAL + 64:      # the classes are what they claim to be
        at = n - 8 - NSPECIAL
        blk = lambda a, k: a[at + 64 * k: at + 64 * (k + 1)]
        assert np.isinf(blk(ref[2], 3)).all() and np.array_equal(A.bits(blk(ref[0], 3)), A.bits(blk(p, 3)))
        assert (blk(ref[2], 2)[:32] == 0).all() and (blk(ref[2], 4) > 0).all()
        assert np.array_equal(A.bits(blk(ref[1], 6)), A.bits(blk(g, 6))) == (wd == 0.0)


# ----------------------------------------------------------------------------------------------------------- b. the engine's arenas
def _snapshot(e):
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().copy() for k, t in (("p", e.params), ("g", e.grads), ("m", e.adam_m), ("v", e.adam_v))}


def _bits1(x):
    return int(A.bits(np.asarray([x], dtype=F32))[0])


def _check_engine_step(e, cfg, before, wd, gs, clip, what):
    """One adam_step(LR, wd, gs) of engine `e`, whose arenas hold `before`, against the reference: all three arenas, padding
    included; with `clip` the launch clips at half the reference's own norm and (total, coef) must be the reference's bits."""
    sizes = GC._sizes(cfg)
    assert list(e.poff) == R.layout_offsets(sizes)
    geff = F32(gs)
    if clip:
        parts = A.grad_sumsq_parts(before["g"], e.poff, sizes)
        norm, _ = A.clip_total_coef(parts, gs, float("inf"))
        assert np.isfinite(norm) and norm > 0
        max_norm = 0.5 * float(norm)
        total, coef = A.clip_total_coef(parts, gs, max_norm)            # (the engine hands max_norm on as a C float, as F32() does)
        assert total == norm and 0.4 < coef < 0.6
        geff = A.geff_clipped(gs, coef)
        e.set_grad_clip(max_norm)
    else:
        assert e.max_grad_norm is None
    e.adam_step(LR, weight_decay=wd, grad_scale=gs)
    step = int(e.lib.eae_get_adam_step(e.ctx))
    after = _snapshot(e)
    # eae_adam_step_scaled takes lr and weight_decay as C floats; the launcher widens them again
    scalars = A.launch_scalars(float(F32(LR)), B1, B2, step)
    ref = A.adam_update(before["p"], before["g"], before["m"], before["v"], scalars=scalars, eps=EPS, wd=float(F32(wd)), geff=geff)
    _no_nan(ref)
    assert np.array_equal(A.bits(after["g"]), A.bits(before["g"]))
    _assert_same_bits(after, dict(zip("pmv", ref)), before, what)
    if clip:
        t, c = e.read_grad_norm()
        print(f"{what}: total {t!r} (reference {float(total)!r}) coef {c!r} (reference {float(coef)!r})")
        assert (_bits1(t), _bits1(c)) == (_bits1(total), _bits1(coef))
        assert 0.4 < c < 0.6
    return step


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 1.0), (0.0, 0.5), (1e-4, 0.5)])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_engine_step_equals_the_reference_bit_for_bit(cfg, wd, gs):
    """A train step and a gradient step first (non-zero moments, real gradients, the optimizer's second launch); engine a steps
    without clipping, engine b from the same bits with it."""
    x, y = GC._batch(cfg)
    engs = [GC._engine(cfg)[1] for _ in range(2)]
    snaps = []
    for e in engs:
        e.train_step(x, y, ALPHA, LR)
        e.grad_step(x, y, ALPHA)
        snaps.append(_snapshot(e))
    assert all(np.array_equal(A.bits(snaps[0][k]), A.bits(snaps[1][k])) for k in "pgmv")
    assert np.abs(snaps[0]["m"]).max() > 0 and np.abs(snaps[0]["v"]).max() > 0
    for e, clip in zip(engs, (False, True)):
        assert _check_engine_step(e, cfg, snaps[0], wd, gs, clip, f"cfg {cfg} wd {wd} gs {gs} clip {clip}") == 2


def _synthetic_arenas(e, cfg, seed=77):
    """Random parameters, gradients and moments over the whole arena, padding included (Adam walks all of it; the norm must not)."""
    n = e.poff[38]
    rng = np.random.default_rng(seed)
    a = {"p": rng.standard_normal(n).astype(F32) * F32(0.1),
         "g": (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1, n)).astype(F32),
         "m": (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -2, n)).astype(F32),
         "v": (np.square(rng.standard_normal(n)) * 10.0 ** rng.uniform(-8, -3, n)).astype(F32)}
    a["g"][R.padding_index(e.poff, GC._sizes(cfg))] = 1e4
    for k, t in (("p", e.params), ("g", e.grads), ("m", e.adam_m), ("v", e.adam_v)):
        t.copy_(torch.from_numpy(a[k]))
    return a


def test_engine_step_at_both_grid_caps_equals_the_reference_bit_for_bit():
    """Latent 256: 2 913 680 elements, 728 420 pieces -- 512 norm workgroups (the cap) whose threads run a second round in which the
    slots u = 2, 3 lie past the end, and 2048 optimizer workgroups (the cap) whose grid-stride loop runs a second round, on the
    clipped path.  The optimizer launch needs the bound arenas only (no forward), so they are filled with synthetic values."""
    n = R.layout_offsets(GC._sizes(BIG))[38]
    assert A.grad_sumsq_nparts(n) == A.EAE_CLIP_MAX_PARTS and 4 * 256 * 512 < n // 4 < 6 * 256 * 512
    assert A.adam_blocks(n) == A.ADAM_MAX_BLOCKS and n // 4 > 256 * 2048
    _, e = GC._engine(BIG)
    assert e.poff[38] == n
    before = _synthetic_arenas(e, BIG)
    assert _check_engine_step(e, BIG, before, 1e-4, 0.5, True, f"cfg {BIG} synthetic, clipped") == 1


# ----------------------------------------------------------------------------------------------------------- c. every element once
def _probe_positions(poff, sizes):
    """Arena indices of the one-hot probes: the first and last valid element of every tensor, every padding element, every element of
    the pieces T - 1, T, 4T - 1, 4T (where the arena has them) and of the arena's last piece."""
    n = poff[38]
    n4 = n // 4
    T = 256 * A.grad_sumsq_nparts(n)
    idx = []
    for s, k in enumerate(sizes):
        idx += [poff[s], poff[s] + k - 1]
    idx += list(R.padding_index(poff, sizes))
    for piece in (T - 1, T, 4 * T - 1, 4 * T, n4 - 1):
        if 0 <= piece < n4:
            idx += [4 * piece + j for j in range(4)]
    return sorted(set(int(i) for i in idx))


@pytest.mark.parametrize("cfg", CONFIGS + [BIG])
def test_norm_counts_every_element_exactly_once(cfg):
    """max_norm = inf and lr = 0: the launch measures and moves no parameter.  Every expected value is exact: a sum of ones, or one
    power of two among zeros.  One launch and one read-back of two floats per probe."""
    _, e = GC._engine(cfg)
    sizes, poff = GC._sizes(cfg), e.poff
    n = poff[38]
    pad = R.padding_index(poff, sizes)
    valid = np.ones(n, dtype=bool)
    valid[pad] = False
    count = int(valid.sum())
    assert count == sum(sizes)
    e.set_grad_clip(float("inf"))
    p0 = e.params.clone()

    def norm(gs):
        e.adam_step(0.0, 0.0, gs)
        return e.read_grad_norm()

    # all ones, 1e4 in the padding
    ones = np.where(valid, F32(1.0), F32(1e4)).astype(F32)
    e.grads.copy_(torch.from_numpy(ones))
    for gs in (1.0, 0.5):
        total, coef = norm(gs)
        want = F32(gs * np.sqrt(np.float64(count)))
        print(f"cfg {cfg} all ones gs {gs}: total {total!r} want {float(want)!r}")
        assert (_bits1(total), coef) == (_bits1(want), 1.0)
    # one hot
    e.grads.zero_()
    pos = _probe_positions(poff, sizes)
    assert set(pad) <= set(pos) and n - 1 in pos
    T = 256 * A.grad_sumsq_nparts(n)
    if cfg == BIG:
        assert 4 * (4 * T) in pos and 4 * (4 * T - 1) in pos
    wrong = []
    prev = None
    for j, i in enumerate(pos):
        k = i % 17 - 8
        gs = (1.0, 0.5)[j % 2]
        if prev is not None:
            e.grads[prev] = 0.0
        e.grads[i] = 2.0 ** k
        prev = i
        total, coef = norm(gs)
        want = gs * 2.0 ** k if valid[i] else 0.0
        if (_bits1(total), coef) != (_bits1(want), 1.0):
            wrong.append((i, bool(valid[i]), gs, k, total, coef, want))
    print(f"cfg {cfg}: {len(pos)} one-hot probes, {len(wrong)} wrong")
    assert not wrong, wrong[:8]
    torch.cuda.synchronize()
    assert torch.equal(e.params, p0)          # lr = 0: nothing moved
