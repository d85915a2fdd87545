"""GPU parity of the MLP classifier kernel (csrc/eae_mlp.hip, mlp_engine.py) across widths, class counts and batch shapes,
against the float64 reference of tests/mlp_ref.py.

Tolerances.  The kernel is fp32 with fmaf chains and its own summation order.  No bound is taken from its output: for every
compared quantity the deviation of the fp32 NumPy oracle (oracle.ae_numpy.mlp_*; an fp32 run of mlp_ref where the oracle lacks
the piece: an arbitrary dL/dlogits, the summed loss) from the float64 reference on the same inputs is the fp32 yardstick, computed
inside the test so that it adapts to the shape.  The bound is 8 x yardstick (a different accumulation order over up to 1500 rows
and 1024 inputs) + 4 ulp of the reference's max-abs.  For the biases in front of a BatchNorm (net.0.bias, net.4.bias), whose
gradient is analytically zero, the floor is 4 ulp of max_j sum_b |dh[b, j]|, the magnitude that cancels in that column sum.
Parameters after Adam: Adam divides each step by |g|, so an element whose gradient (with weight decay) is not far above the
gradient's own bound takes a noise-normalised step; each element is therefore allowed, on top of the bound, what its step moves
when its gradient moves by that bound (adam_sensitivity, from the reference alone; negligible elsewhere), and every parameter
additionally holds the tolerances of test_gpu_mlp.py::test_mlp_adam_trajectory.
ReLU ties: a pre-activation within fp32 error of zero flips a mask bit and moves gradients discontinuously, so each case asserts
on the reference, before launching, that no o1 (of a kept unit) or o2 lies within 16 x its yardstick of zero; the seeds below were
searched on the CPU for that.  For B >= 1024 the drop mask of offending layer-1 units is zeroed instead.

Known, untested limits: a label outside [0, C) is undefined behaviour in the kernel, and the autograd bridge provides no dx for
an input that requires grad.

Yardstick, bound and the kernel's measured deviation (MI355X), relative to the reference's max-abs (absolute where that is 0:
C = 1 has exactly zero gradients).  Per case the worst tensor of each group: fwd = logits, loss, running statistics, probs;
grad = the ten gradients; adam = parameters and both moments after the step.  `pytest -s` prints every tensor.
  case                       group  worst tensor (deviation / bound)   yardstick  bound     measured
  train-in1024-c16-b1500     fwd    buf/net.5.running_var               7.96e-08  1.11e-06  7.96e-08
  train-in1024-c16-b1500     grad   grad/net.7.weight                   2.61e-07  2.56e-06  8.89e-07
  train-in1024-c16-b1500     adam   v/net.7.weight                      4.16e-07  3.80e-06  1.46e-06
  train-in1-c1-b2            fwd    buf/net.1.running_var               7.79e-08  1.10e-06  7.79e-08
  train-in1-c1-b2            grad   grad/net.0.weight                   0.00e+00  0.00e+00  0.00e+00
  train-in1-c1-b2            adam   v/net.4.weight                      1.71e-07  1.84e-06  1.71e-07
  train-in37-c16-b3          fwd    buf/net.5.running_var               6.56e-08  1.00e-06  6.56e-08
  train-in37-c16-b3          grad   grad/net.0.bias                     3.80e-08  7.81e-07  2.09e-07
  train-in37-c16-b3          adam   m/net.0.bias                        1.20e-02  9.57e-02  6.58e-02
  train-in48-c10-b1025       fwd    buf/net.1.running_var               8.27e-08  1.14e-06  8.27e-08
  train-in48-c10-b1025       grad   grad/net.5.bias                     3.10e-08  7.25e-07  1.54e-07
  train-in48-c10-b1025       adam   v/net.4.weight                      4.59e-07  4.15e-06  1.20e-06
  train-in64-c10-b64         fwd    step3/loss                          3.37e-08  7.46e-07  1.70e-07
  train-in64-c10-b64         grad   step3/grad/net.0.weight             2.86e-07  2.76e-06  4.38e-07
  train-in64-c10-b64         adam   step3/v/net.7.bias                  3.35e-08  7.45e-07  2.56e-07
  train-in128-c2-b7          fwd    loss                                1.46e-09  4.88e-07  6.81e-08
  train-in128-c2-b7          grad   grad/net.4.weight                   2.36e-07  2.36e-06  7.14e-07
  train-in128-c2-b7          adam   v/net.5.weight                      1.39e-07  1.59e-06  5.69e-07
  train-in256-c10-b33        fwd    step2/logits                        3.67e-07  3.41e-06  3.78e-07
  train-in256-c10-b33        grad   step1/grad/net.7.weight             3.42e-07  3.21e-06  5.46e-07
  train-in256-c10-b33        adam   step1/v/net.7.bias                  1.59e-07  1.75e-06  4.88e-07
  train-in64-c2-b200         fwd    buf/net.1.running_var               8.46e-08  1.15e-06  8.30e-08
  train-in64-c2-b200         grad   grad/net.1.bias                     2.28e-07  2.30e-06  3.37e-07
  train-in64-c2-b200         adam   v/net.4.bias                        1.25e-03  9.99e-03  2.23e-03
  train-in1-c10-b64          fwd    buf/net.1.running_var               8.36e-08  1.15e-06  8.36e-08
  train-in1-c10-b64          grad   grad/net.7.bias                     1.67e-07  1.81e-06  3.49e-07
  train-in1-c10-b64          adam   m/net.7.bias                        1.89e-07  1.99e-06  4.26e-07
  train-in37-c2-b1024        fwd    buf/net.1.running_var               7.98e-08  1.11e-06  7.98e-08
  train-in37-c2-b1024        grad   grad/net.1.bias                     3.15e-07  3.00e-06  9.11e-07
  train-in37-c2-b1024        adam   v/net.1.bias                        4.32e-07  3.93e-06  1.62e-06
  train-in48-c1-b33          fwd    buf/net.5.running_var               7.69e-08  1.09e-06  7.69e-08
  train-in48-c1-b33          grad   grad/net.0.weight                   0.00e+00  0.00e+00  0.00e+00
  train-in48-c1-b33          adam   v/net.4.weight                      1.68e-07  1.82e-06  1.68e-07
  train-in128-c16-b200       fwd    step2/logits                        3.51e-07  3.29e-06  3.00e-07
  train-in128-c16-b200       grad   step2/grad/net.7.bias               2.10e-07  2.16e-06  5.66e-07
  train-in128-c16-b200       adam   step2/v/net.0.bias                  2.28e-04  1.82e-03  5.58e-04
  train-in256-c1-b1500       fwd    buf/net.1.running_mean              6.29e-08  9.80e-07  6.85e-08
  train-in256-c1-b1500       grad   grad/net.0.weight                   0.00e+00  0.00e+00  0.00e+00
  train-in256-c1-b1500       adam   v/net.4.weight                      1.66e-07  1.80e-06  1.66e-07
  train-in1024-c10-b7        fwd    loss                                3.46e-09  5.04e-07  1.28e-07
  train-in1024-c10-b7        grad   grad/net.5.weight                   4.85e-07  4.36e-06  1.36e-06
  train-in1024-c10-b7        adam   v/net.7.weight                      2.24e-07  2.26e-06  1.04e-06
  train-in1024-c2-b64        fwd    loss                                2.35e-08  6.65e-07  6.89e-08
  train-in1024-c2-b64        grad   grad/net.7.bias                     4.75e-08  8.57e-07  4.10e-07
  train-in1024-c2-b64        adam   v/net.5.bias                        9.13e-08  1.21e-06  5.65e-07
  train-in64-c16-b33         fwd    buf/net.1.running_var               7.68e-08  1.09e-06  7.68e-08
  train-in64-c16-b33         grad   grad/net.7.bias                     1.85e-07  1.96e-06  3.19e-07
  train-in64-c16-b33         adam   v/net.0.bias                        4.27e-04  3.42e-03  9.06e-04
  train-in37-c10-b200        fwd    buf/net.5.running_var               7.83e-08  1.10e-06  7.83e-08
  train-in37-c10-b200        grad   grad/net.5.bias                     5.67e-08  9.31e-07  1.76e-07
  train-in37-c10-b200        adam   v/net.0.weight                      2.67e-07  2.61e-06  1.20e-06
  train-in48-c16-b64         fwd    buf/net.5.running_var               7.91e-08  1.11e-06  7.91e-08
  train-in48-c16-b64         grad   grad/net.5.bias                     5.19e-08  8.92e-07  1.64e-07
  train-in48-c16-b64         adam   v/net.4.bias                        5.76e-04  4.61e-03  1.44e-03
  train-in128-c10-b64        fwd    buf/net.5.running_var               6.67e-08  1.01e-06  6.67e-08
  train-in128-c10-b64        grad   grad/net.7.weight                   3.13e-07  2.98e-06  3.70e-07
  train-in128-c10-b64        adam   v/net.4.bias                        8.90e-04  7.12e-03  1.50e-03
  train-in256-c16-b1024      fwd    buf/net.5.running_var               7.23e-08  1.06e-06  7.23e-08
  train-in256-c16-b1024      grad   grad/net.7.weight                   2.69e-07  2.63e-06  6.70e-07
  train-in256-c16-b1024      adam   v/net.7.weight                      3.27e-07  3.10e-06  1.00e-06
  train-in1-c2-b200          fwd    buf/net.1.running_var               7.46e-08  1.07e-06  7.46e-08
  train-in1-c2-b200          grad   grad/net.5.bias                     3.71e-08  7.74e-07  1.41e-07
  train-in1-c2-b200          adam   v/net.5.bias                        5.19e-08  8.92e-07  3.07e-07
  train-in64-c1-b1025        fwd    buf/net.1.running_var               7.53e-08  1.08e-06  7.53e-08
  train-in64-c1-b1025        grad   grad/net.0.weight                   0.00e+00  0.00e+00  0.00e+00
  train-in64-c1-b1025        adam   v/net.4.weight                      1.75e-07  1.87e-06  1.75e-07
  eval-in64-c10-b1           fwd    loss sum                            6.08e-09  5.25e-07  5.29e-08
  eval-in37-c16-b63          fwd    forward logits                      1.87e-07  1.97e-06  2.62e-07
  eval-in1-c1-b64            fwd    forward logits                      3.11e-07  2.96e-06  5.18e-07
  eval-in1024-c2-b65         fwd    forward logits                      3.90e-07  3.59e-06  7.90e-07
  eval-in48-c10-b200         fwd    forward logits                      2.51e-07  2.48e-06  2.44e-07
  eval-in128-c16-b1000       fwd    call1/eval_step logits              3.85e-07  3.56e-06  4.23e-07
  dropout-train-in64-b64-step0 fwd    buf/net.1.running_var               7.79e-08  1.10e-06  7.79e-08
  dropout-train-in64-b64-step0 grad   grad/net.5.bias                     5.06e-08  8.82e-07  1.54e-07
  dropout-train-in64-b64-step0 adam   m/net.4.bias                        5.12e-04  4.10e-03  1.34e-03
  dropout-train-in64-b64-step1 fwd    buf/net.1.running_var               7.79e-08  1.10e-06  7.79e-08
  dropout-train-in64-b64-step1 grad   grad/net.5.bias                     4.23e-08  8.15e-07  1.51e-07
  dropout-train-in64-b64-step1 adam   v/net.5.bias                        9.56e-08  1.24e-06  4.73e-07
  dropout-train-in48-b1500-step0 fwd    buf/net.1.running_var               7.21e-08  1.05e-06  7.83e-08
  dropout-train-in48-b1500-step0 grad   grad/net.7.weight                   2.11e-07  2.17e-06  9.66e-07
  dropout-train-in48-b1500-step0 adam   v/net.7.weight                      3.12e-07  2.97e-06  1.76e-06
  dropout-fwd-in64-b64-step0 fwd    buf/net.1.running_var               7.79e-08  1.10e-06  7.79e-08
  dropout-fwd-in37-b64-step0 fwd    buf/net.1.running_var               7.26e-08  1.06e-06  7.26e-08
  dropout-fwd-in128-b1500-step7 fwd    buf/net.1.running_var               7.55e-08  1.08e-06  7.55e-08
  dropout-fwd-in64-b1500-step158 fwd    buf/net.1.running_var               8.20e-08  1.13e-06  8.20e-08
  autograd-in37-c16-b33      fwd    call2/logits                        2.62e-07  2.57e-06  4.27e-07
  autograd-in37-c16-b33      grad   call1/grad/net.4.weight             2.94e-07  2.83e-06  3.84e-07
  autograd-in128-c2-b200     fwd    call2/logits                        4.12e-07  3.77e-06  3.60e-07
  autograd-in128-c2-b200     grad   call1/grad/net.7.weight             4.67e-07  4.21e-06  6.77e-07
  autograd-in48-c10-b7       fwd    call2/logits                        2.39e-07  2.39e-06  4.19e-07
  autograd-in48-c10-b7       grad   call1/grad/net.7.weight             2.47e-07  2.45e-06  5.34e-07
  scene-l48-c16              fwd    probs (windows=)                    1.91e-08  6.29e-07  1.81e-08
  scene-l128-c1              fwd    probs (windows=)                    0.00e+00  4.77e-07  0.00e+00
  scene-l48-c1               fwd    probs (windows=)                    0.00e+00  4.77e-07  0.00e+00
  scene-l128-c16             fwd    probs (windows=)                    2.14e-08  6.48e-07  2.56e-08
No case takes more than a second on the device; the whole file runs in about six seconds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_ref as R

pytestmark = pytest.mark.gpu

# lr: where fp32 noise decides the sign of an element's gradient, Adam's normalised step differs by 2 * lr from the reference's
# whatever the implementation; lr = 1e-5 keeps that inside the absolute tolerance of test_mlp_adam_trajectory (3e-5), while a
# step of 1e-5 is still a thousand times the bound on a parameter (a few 1e-8), and m and v are compared directly
LR, WD = 1e-5, 1e-4
HI_SEED = 0x9E3779B97F4A7C15          # dropout seed with non-zero high 32 bits

# (input_dim, classes, batch, consecutive steps, data seed): every value of each axis, the four corners of the issue.
# B = 2 and B = 3 appear in the corners only: BatchNorm over two or three rows leaves the gradients in front of it to heavy
# cancellation (at B = 2 they vanish but for eps), which fp32 statistics and the oracle's float64 statistics do not resolve alike.
CASES = [
    (1024, 16, 1500, 1, 0), (1, 1, 2, 1, 0), (37, 16, 3, 1, 0), (48, 10, 1025, 1, 1),
    (64, 10, 64, 3, 0), (128, 2, 7, 1, 0), (256, 10, 33, 2, 0), (64, 2, 200, 1, 1),
    (1, 10, 64, 1, 1), (37, 2, 1024, 1, 0), (48, 1, 33, 1, 0), (128, 16, 200, 2, 5),
    (256, 1, 1500, 1, 5), (1024, 10, 7, 1, 0), (1024, 2, 64, 1, 0), (64, 16, 33, 1, 0),
    (37, 10, 200, 1, 2), (48, 16, 64, 1, 0), (128, 10, 64, 1, 0), (256, 16, 1024, 1, 6),
    (1, 2, 200, 1, 2), (64, 1, 1025, 1, 2),
]
# kernel-generated dropout: (input_dim, classes, batch, dropout seed, Adam step before the call, data seed)
DROPOUT_TRAIN = [(64, 10, 64, 3, 0, 0), (64, 10, 64, 3, 1, 0), (48, 16, 1500, HI_SEED, 0, 30)]      # train_step keys on step + 1
# forward keys on the step itself.  (seed 3, step 158): u of element 113200 (row 884, unit 48) equals float32(0.3) exactly, the one
# place where `u >= p` and `u > p` differ
DROPOUT_FWD = [(64, 10, 64, 3, 0, 0), (37, 2, 64, 4, 0, 0), (128, 10, 1500, HI_SEED, 7, 0), (64, 10, 1500, 3, 158, 0)]
# autograd path: (input_dim, classes, batch, engine seed, data seed); call n of an engine uses dropout seed engine seed + n
AUTOGRAD = [(37, 16, 33, 11, 0), (128, 2, 200, HI_SEED, 0), (48, 10, 7, 5, 0)]
# every (seed, step, B) whose Philox mask a test here relies on (tests/test_mlp_reference.py checks the keep fractions)
PHILOX_TRIPLES = ([(s, st + 1, b) for _, _, b, s, st, _ in DROPOUT_TRAIN] + [(s, st, b) for _, _, b, s, st, _ in DROPOUT_FWD]
                  + [((s + n) & 0xFFFFFFFFFFFFFFFF, 0, b) for _, _, b, s, _ in AUTOGRAD for n in (1, 2)] + [(1, 0, 64)])


# ---------------------------------------------------------------------------------------------------------------- CPU side
def case_inputs(IN, Cn, B, steps, seed, philox=None):
    """State, batches [(x, labels, keep mask)] of a case.  philox = (seed, first step): Philox masks instead of drawn ones."""
    p0 = R.make_state(IN, Cn, 1000 * seed + IN + 7 * Cn)
    batches = []
    for s in range(steps):
        x, y = R.make_batch(B, IN, Cn, 77 * seed + 13 * B + IN + s)
        if philox is None:
            mask = (np.random.default_rng(5 * seed + B + s).random((B, R.H1)) >= 0.3).astype(np.float32)
        else:
            mask = R.philox_keep_mask(philox[0], philox[1] + s, B)
        batches.append((x, y, mask))
    return p0, batches


def prepare(IN, Cn, B, steps, seed, philox=None):
    """Reference and yardstick of a case.  Returns (p0, batches, ref, yard, ties): ref / yard are per-step dicts of named
    quantities (float64 reference, fp32 oracle); ties the number of ReLU ties left (must be 0)."""
    p0, batches = case_inputs(IN, Cn, B, steps, seed, philox)
    ref = R.run_reference(p0, batches, LR, WD)
    yard = R.run_oracle(p0, batches, LR, WD)
    if B >= 1024 and philox is None:
        # zero the drop mask of layer-1 units that tie (they then contribute nothing whatever their sign), and start again
        t1, _ = R.relu_ties(ref[0], yard[0], batches[0][2])
        if t1.any():
            x, y, mask = batches[0]
            batches[0] = (x, y, np.where(t1, np.float32(0), mask))
            ref = R.run_reference(p0, batches, LR, WD)
            yard = R.run_oracle(p0, batches, LR, WD)
    # the oracle's CrossEntropy works in float64 on its fp32 logits: the loss's fp32 yardstick is an fp32 run of the reference
    for o, r32 in zip(yard, R.run_reference(p0, batches, LR, WD, dtype=np.float32)):
        o["loss"] = r32["loss"]
    ties = 0
    for r, o, (_, _, mask) in zip(ref, yard, batches):
        t1, t2 = R.relu_ties(r, o, mask)
        ties += int(t1.sum()) + int(t2.sum())
    return p0, batches, ref, yard, ties


def start_of(p0):
    """The quantities before the first step: the initial parameters and zero moments."""
    q = {}
    for k in R.PARAMS:
        q["param/" + k] = np.asarray(p0[k], dtype=np.float64)
        q["m/" + k] = q["v/" + k] = np.zeros_like(q["param/" + k])
    return q


class Report:
    """Collects (quantity, yardstick, bound, deviation), prints them, and fails at the end with every miss."""

    def __init__(self, case):
        self.case, self.rows, self.bad = case, [], []

    def check(self, name, got, ref, yard_val, scale=None, floor_scale=None, extra=None):
        """extra: elementwise allowance on top of the bound (adam_sensitivity); the deviation reported is what exceeds it.
        Returns the bound."""
        ref = np.asarray(ref, dtype=np.float64)
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = float(np.abs(ref).max()) if scale is None else scale
        yv = R.deviation(yard_val, ref)
        bd = R.bound(yv, scale if floor_scale is None else floor_scale)
        if not np.isfinite(got).all():
            dv = float("inf")
        elif extra is None:
            dv = R.deviation(got, ref)
        else:
            dv = float(np.maximum(np.abs(got - ref) - extra, 0).max())
        s = scale if scale > 0 else 1.0
        self.rows.append((name, yv / s, bd / s, dv / s))
        print(f"MLPDEV case={self.case} q={name} scale={scale:.3e} yard={yv / s:.3e} bound={bd / s:.3e} dev={dv / s:.3e}")
        if not dv <= bd:
            self.bad.append(f"{name}: deviation {dv:.3e} > bound {bd:.3e} (yardstick {yv:.3e}, scale {scale:.3e})")
        return bd

    def done(self):
        assert not self.bad, f"case {self.case}:\n" + "\n".join(self.bad)


def adam_sensitivity(g, bg, p_prev, m_prev, v_prev, t):
    """How far Adam's step of each element can move when its gradient moves by +-bg (the gradient's own bound):
    max |u(g +- bg) - u(g)| with u = lr / bc1 * m' / (sqrt(v') / sqrt(bc2) + eps), m' and v' from the previous moments.
    Adam divides the step by |g|, so where |g + wd * p| is not far above bg (and 1e-8) the step is normalised noise: this is
    the room such elements need, computed from the reference alone.  Elsewhere it is negligible."""
    ss, bc = LR / (1.0 - 0.9 ** t), np.sqrt(1.0 - 0.999 ** t)

    def u(gg):
        gg = gg + WD * p_prev
        return ss * (0.9 * m_prev + 0.1 * gg) / (np.sqrt(0.999 * v_prev + 0.001 * gg * gg) / bc + 1e-8)

    return np.maximum(np.abs(u(g + bg) - u(g)), np.abs(u(g - bg) - u(g)))


# ---------------------------------------------------------------------------------------------------------------- GPU side
def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _clf(IN, Cn, p0, max_batch, train=True):
    import eae_amd
    from eae_amd.mlp_engine import mlp_engine_for
    from helpers import load_state_np
    clf = eae_amd.MLP(input_dim=IN, num_classes=Cn)
    load_state_np(clf, p0)
    clf = clf.cuda()
    clf.train(train)
    eng = mlp_engine_for(clf, max_batch=max(256, max_batch))
    return clf, eng


def _slot(eng, arena, i, p):
    return arena[eng.poff[i]: eng.poff[i] + p.numel()].view(p.shape).cpu().numpy()


def _set_step(eng, step):
    from eae_amd._lib import check
    check(eng.lib.eae_mlp_set_adam_step(eng.ctx, int(step)))


def _compare_step(rep, clf, eng, logits, stats_before, ref, yard, B, tag="", prev=None, t=1):
    """Everything a fused train_step leaves behind, against the reference of that step.  prev: the reference's quantities
    before the step (parameters, moments); t: the Adam step count of this step."""
    torch.cuda.synchronize()
    rep.check(tag + "logits", logits.cpu().numpy(), ref["logits"], yard["logits"])
    st = np.array(eng.stats.tolist()[:3]) - stats_before
    rep.check(tag + "loss", st[0] / B, ref["loss"], yard["loss"])
    assert st[1] == B and st[2] == ref["correct"], (rep.case, st, ref["correct"])
    names = [n for n, _ in clf.named_parameters()]
    assert tuple(names) == R.PARAMS
    for (p, i), name in zip(eng._slots, names):
        fs = ref["cancel/" + name] if name in R.PREBN_BIAS else None
        sc = ref["cancel/" + name] if name in R.PREBN_BIAS else None
        bg = rep.check(tag + "grad/" + name, _slot(eng, eng.grads, i, p), ref["grad/" + name], yard["grad/" + name], scale=sc, floor_scale=fs)
        rep.check(tag + "m/" + name, _slot(eng, eng.adam_m, i, p), ref["m/" + name], yard["m/" + name])
        rep.check(tag + "v/" + name, _slot(eng, eng.adam_v, i, p), ref["v/" + name], yard["v/" + name])
        got = p.detach().cpu().numpy()
        extra = adam_sensitivity(ref["grad/" + name], bg, prev["param/" + name], prev["m/" + name], prev["v/" + name], t)
        rep.check(tag + "param/" + name, got, ref["param/" + name], yard["param/" + name], extra=extra)
        # never looser than test_mlp_adam_trajectory for the same tensor
        np.testing.assert_allclose(got, ref["param/" + name], rtol=3e-3, atol=3e-4 if name in R.PREBN_BIAS else 3e-5,
                                   err_msg=f"{rep.case} {name}")
    sd = clf.state_dict()
    for k in R.BUFFERS:
        rep.check(tag + "buf/" + k, sd[k].cpu().numpy(), ref["buf/" + k], yard["buf/" + k])
    assert int(sd["net.1.num_batches_tracked"]) == ref["nbt"] and int(sd["net.5.num_batches_tracked"]) == ref["nbt"]


@pytest.mark.parametrize("IN,Cn,B,steps,seed", CASES, ids=[f"in{c[0]}-c{c[1]}-b{c[2]}-s{c[3]}" for c in CASES])
def test_train_step_shapes(IN, Cn, B, steps, seed):
    p0, batches, ref, yard, ties = prepare(IN, Cn, B, steps, seed)
    assert ties == 0, f"{ties} ReLU ties: search another data seed"
    for r in ref:       # the correct count is compared exactly: the top two logits of every row must be clearly apart
        if Cn > 1:
            top = np.sort(r["logits"], axis=1)
            assert (top[:, -1] - top[:, -2]).min() > R.TIE_FACTOR * R.deviation(yard[0]["logits"], ref[0]["logits"])
    clf, eng = _clf(IN, Cn, p0, B)
    rep = Report(f"train-in{IN}-c{Cn}-b{B}")
    for s, (x, y, mask) in enumerate(batches):
        before = np.array(eng.stats.tolist()[:3])
        logits = eng.train_step(_cuda(x), _cuda(y), lr=LR, weight_decay=WD, drop_mask=_cuda(mask), want_logits=True)
        _compare_step(rep, clf, eng, logits, before, ref[s], yard[s], B, tag=f"step{s + 1}/" if steps > 1 else "",
                      prev=ref[s - 1] if s else start_of(p0), t=s + 1)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- eval
EVAL = [(64, 10, 1), (37, 16, 63), (1, 1, 64), (1024, 2, 65), (48, 10, 200), (128, 16, 1000)]


@pytest.mark.parametrize("IN,Cn,B", EVAL, ids=[f"in{c[0]}-c{c[1]}-b{c[2]}" for c in EVAL])
def test_eval_across_blocks(IN, Cn, B):
    """One block per 64 rows: every row of the logits, the statistics accumulated by two calls without a reset (atomics across
    blocks), and running statistics / num_batches_tracked untouched."""
    from oracle import ae_numpy as O
    p0 = R.make_state(IN, Cn, 31 + IN + Cn)
    x, y = R.make_batch(B, IN, Cn, 17 + B)
    x2, y2 = R.make_batch(B, IN, Cn, 18 + B)
    clf, eng = _clf(IN, Cn, p0, B, train=False)
    rep = Report(f"eval-in{IN}-c{Cn}-b{B}")
    sd0 = {k: v.clone() for k, v in clf.state_dict().items()}
    eng.reset_stats()
    tot = np.zeros(3)
    ytot = np.zeros(3)
    for i, (xx, yy) in enumerate(((x, y), (x2, y2))):
        c = R.forward(p0, xx, False)
        c32 = R.forward(p0, xx, False, dtype=np.float32)
        yl = O.mlp_forward(p0, xx, train=False)["logits"]
        loss, _, correct = R.cross_entropy(c["logits"], yy)
        loss32, _, _ = R.cross_entropy(c32["logits"], yy)           # the oracle's CE is float64 inside: fp32 run of the reference
        if Cn > 1:
            top = np.sort(c["logits"], axis=1)
            assert (top[:, -1] - top[:, -2]).min() > R.TIE_FACTOR * R.deviation(yl, c["logits"])
        tot += (loss * B, B, correct)
        ytot += (float(np.float32(loss32) * np.float32(B)), B, correct)
        lg = eng.eval_step(_cuda(xx), _cuda(yy), want_logits=True)
        rep.check(f"call{i}/eval_step logits", lg.cpu().numpy(), c["logits"], yl)
        if i == 0:
            with torch.no_grad():
                rep.check("forward logits", eng.forward(_cuda(xx), train=False).cpu().numpy(), c["logits"], yl)
                rep.check("module logits", clf(_cuda(xx)).cpu().numpy(), c["logits"], yl)
    torch.cuda.synchronize()
    st = eng.stats.tolist()[:3]
    rep.check("loss sum", st[0], tot[0], ytot[0])
    assert st[1] == tot[1] and st[2] == tot[2], (st, tot)
    for k, v in clf.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- dropout
@pytest.mark.parametrize("IN,Cn,B,dseed,step0,seed", DROPOUT_TRAIN, ids=[f"in{c[0]}-b{c[2]}-step{c[4]}" for c in DROPOUT_TRAIN])
def test_kernel_dropout_train_step(IN, Cn, B, dseed, step0, seed):
    """train_step without a drop_mask: the kernel's own Philox mask, keyed on (seed, step count AFTER the increment), proven
    bit for bit through logits, gradients (the backward through that mask, 1/0.7 scale) and the update."""
    p0, batches, ref, yard, ties = prepare(IN, Cn, B, 1, seed, philox=(dseed, step0 + 1))
    assert ties == 0, f"{ties} ReLU ties: search another data seed"
    x, y, mask = batches[0]
    clf, eng = _clf(IN, Cn, p0, B)
    eng.seed = dseed
    _set_step(eng, step0)
    rep = Report(f"dropout-train-in{IN}-b{B}-step{step0}")
    before = np.array(eng.stats.tolist()[:3])
    logits = eng.train_step(_cuda(x), _cuda(y), lr=LR, weight_decay=WD, drop_mask=None, want_logits=True)
    if step0 > 0:
        # Adam at step > 1 starts here from zero moments: the reference's bias corrections must use the kernel's step count
        p = R.cast(p0, np.float64)
        state = {"step": step0, "m": {}, "v": {}}
        loss, correct, c, g = R.train_step(p, state, x, y, LR, WD, mask)
        for k in R.PARAMS:
            ref[0]["param/" + k], ref[0]["m/" + k], ref[0]["v/" + k] = p[k], state["m"][k], state["v"][k]
        from oracle import ae_numpy as O
        po = {k: np.asarray(v).copy() for k, v in p0.items()}
        so = {"step": step0, "m": {}, "v": {}}
        O.mlp_train_step(po, so, x, y, LR, drop_mask=mask, weight_decay=WD)
        for k in R.PARAMS:
            yard[0]["param/" + k], yard[0]["m/" + k], yard[0]["v/" + k] = po[k], so["m"][k], so["v"][k]
    _compare_step(rep, clf, eng, logits, before, ref[0], yard[0], B, prev=start_of(p0), t=step0 + 1)
    rep.done()
    # the mask of this (seed, step) is not that of the neighbouring step or seed
    assert not np.array_equal(mask, R.philox_keep_mask(dseed, step0 + 2, B))
    assert not np.array_equal(mask, R.philox_keep_mask(dseed + 1, step0 + 1, B))
    assert not np.array_equal(mask, R.philox_keep_mask(dseed ^ (1 << 40), step0 + 1, B))


@pytest.mark.parametrize("IN,Cn,B,dseed,step,seed", DROPOUT_FWD, ids=[f"in{c[0]}-b{c[2]}-step{c[4]}" for c in DROPOUT_FWD])
def test_kernel_dropout_forward(IN, Cn, B, dseed, step, seed):
    """forward(train=True) keys on the current step count.  One wrong mask bit moves a logit row by far more than the bound."""
    from oracle import ae_numpy as O
    p0, batches = case_inputs(IN, Cn, B, 1, seed, philox=(dseed, step))
    x, _, mask = batches[0]
    c = R.forward(p0, x, True, drop_mask=mask)
    yl = O.mlp_forward(p0, x, train=True, drop_mask=mask)
    clf, eng = _clf(IN, Cn, p0, B)
    eng.seed = dseed
    _set_step(eng, step)
    rep = Report(f"dropout-fwd-in{IN}-b{B}-step{step}")
    with torch.no_grad():
        lg = eng.forward(_cuda(x), train=True)
    rep.check("logits", lg.cpu().numpy(), c["logits"], yl["logits"])
    sd = clf.state_dict()
    for k in R.BUFFERS:                      # a train-mode forward is one BatchNorm update, like the reference module's
        rep.check("buf/" + k, sd[k].cpu().numpy(), c["new_buffers"][k], yl["new_buffers"][k])
    assert int(sd["net.1.num_batches_tracked"]) == int(p0["net.1.num_batches_tracked"]) + 1
    rep.done()
    # resolving power: the reference under the masks of the next step, another seed, or a threshold of 0.31 is far outside the bound
    bd = R.bound(R.deviation(yl["logits"], c["logits"]), float(np.abs(c["logits"]).max()))
    others = [R.philox_keep_mask(dseed, step + 1, B), R.philox_keep_mask(dseed + 1, step, B),
              (R.philox_uniform(dseed, step, B * R.H1) >= np.float32(0.31)).astype(np.float32).reshape(B, R.H1)]
    if (dseed, step) == (3, 158):
        u = R.philox_uniform(dseed, step, B * R.H1)
        assert u[113200] == np.float32(0.3) and mask[884, 48] == 1 and c["o1"][884, 48] > 0.1       # kept, and it matters
        others.append((u > np.float32(0.3)).astype(np.float32).reshape(B, R.H1))
    for m in others:
        assert not np.array_equal(m, mask)
        assert R.deviation(R.forward(p0, x, True, drop_mask=m)["logits"], c["logits"]) > 100 * bd


# ---------------------------------------------------------------------------------------------------------------- autograd
@pytest.mark.parametrize("IN,Cn,B,eseed,seed", AUTOGRAD, ids=[f"in{c[0]}-c{c[1]}-b{c[2]}" for c in AUTOGRAD])
def test_autograd_arbitrary_dlogits(IN, Cn, B, eseed, seed):
    """logits = clf(x); (W * logits).sum().backward(): eae_mlp_backward takes dL/dlogits, recomputes the forward under the same
    Philox mask and leaves running statistics alone.  Two calls: the dropout seed moves, the statistics advance once each."""
    p0 = R.make_state(IN, Cn, 1000 * seed + IN + 7 * Cn)
    clf, eng = _clf(IN, Cn, p0, B)
    eng.seed = eseed
    eng._autograd_calls = 0
    p = R.cast(p0, np.float64)
    p32 = R.cast(p0, np.float32)
    rep = Report(f"autograd-in{IN}-c{Cn}-b{B}")
    for call in (1, 2):
        x, _ = R.make_batch(B, IN, Cn, 77 * seed + 13 * B + IN + call)
        dl = np.random.default_rng(call + B).standard_normal((B, Cn)).astype(np.float32)
        mask = R.philox_keep_mask((eseed + call) & 0xFFFFFFFFFFFFFFFF, 0, B)
        c = R.forward(p, x, True, drop_mask=mask)
        g = R.backward(p, c, dl)
        c32 = R.forward(p32, x, True, drop_mask=mask, dtype=np.float32)
        g32 = R.backward(p32, c32, dl)
        ties = sum(int(t.sum()) for t in R.relu_ties(c, c32, mask))
        assert ties == 0, f"{ties} ReLU ties: search another data seed"
        for q in clf.parameters():
            q.grad = None
        logits = clf(_cuda(x))
        rep.check(f"call{call}/logits", logits.detach().cpu().numpy(), c["logits"], c32["logits"])
        after_fwd = {k: v.clone() for k, v in clf.state_dict().items()}
        for k in R.BUFFERS:
            rep.check(f"call{call}/buf/" + k, after_fwd[k].cpu().numpy(), c["new_buffers"][k], c32["new_buffers"][k])
        assert int(after_fwd["net.1.num_batches_tracked"]) == int(p0["net.1.num_batches_tracked"]) + call
        assert int(after_fwd["net.5.num_batches_tracked"]) == int(p0["net.5.num_batches_tracked"]) + call
        (logits * _cuda(dl)).sum().backward()
        torch.cuda.synchronize()
        for name, q in clf.named_parameters():
            cancel = float(np.abs(g["dh1" if name == "net.0.bias" else "dh2"]).sum(axis=0).max()) if name in R.PREBN_BIAS else None
            rep.check(f"call{call}/grad/" + name, q.grad.cpu().numpy(), g[name], g32[name], scale=cancel, floor_scale=cancel)
        for k, v in clf.state_dict().items():          # backward moved neither statistics nor parameters
            assert torch.equal(v, after_fwd[k]), k
        for d in (p, p32):
            src = c if d is p else c32
            for k, v in src["new_buffers"].items():
                d[k] = v
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- scene
@pytest.mark.parametrize("latent,Cn", [(48, 16), (128, 1), (48, 1), (128, 16)])
def test_predict_epilogue_through_classify_scene(latent, Cn):
    """The predict epilogue: strided input (latent 48 lives in rows of stride 64), split at the MLP engine's max_batch (256) inside
    encoder batches of 400 over 540 windows (neither a multiple of 64 nor of 256), softmax, first-maximum labels, and the
    index-driven form with a shuffled list that holds duplicates."""
    import eae_amd
    from eae_amd.engine import engine_for
    from eae_amd.mlp_engine import mlp_engine_for
    from oracle import ae_numpy as O
    torch.manual_seed(latent + Cn)
    model = eae_amd.SupervisedAutoencoder(latent, 10)
    model._eae_max_batch = 400
    with torch.no_grad():
        for mod in model.enc.modules():
            if getattr(mod, "running_mean", None) is not None:
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
    model = model.cuda().eval()
    p0 = R.make_state(latent, Cn, 900 + latent + Cn)
    clf, meng = _clf(latent, Cn, p0, 256, train=False)
    g = torch.Generator().manual_seed(latent * 3 + Cn)
    scene = torch.randint(0, 256, (3, 200, 300), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    probs, labels = eae_amd.classify_scene(scene, model, clf, divisor=255.0, stride=8, batch=400)
    n_h, n_w = eae_amd.window_grid(200, 300, 64, 8)
    n = n_h * n_w
    assert n == 540 and probs.shape == (Cn, n_h, n_w) and labels.shape == (n_h, n_w)
    eng = engine_for(model.enc)
    meng = mlp_engine_for(clf)
    assert meng.max_batch == 256 and eng.max_batch == 400 and n % 64 and n % meng.max_batch and meng.max_batch < eng.max_batch
    z = eae_amd.encode_scene(scene, model, divisor=255.0, stride=8, batch=400).cpu().numpy()
    assert z.shape == (n, latent)
    c = R.forward(p0, z, False)
    yl = O.mlp_forward(p0, z, train=False)["logits"]

    def softmax(l):
        e = np.exp(l - l.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    ref_p, yard_p = softmax(c["logits"]), softmax(yl.astype(np.float32)).astype(np.float32)
    rep = Report(f"scene-l{latent}-c{Cn}")
    got_p = probs.cpu().numpy().reshape(Cn, n).T
    rep.check("probs", got_p, ref_p, yard_p, scale=1.0)
    assert np.abs(got_p.astype(np.float64).sum(axis=1) - 1.0).max() <= 16 * R.EPS32       # at most 16 terms, each within an ulp of 1
    tol = R.bound(R.deviation(yl, c["logits"]), float(np.abs(c["logits"]).max()))
    ref_l = c["logits"].argmax(axis=1)                       # the first maximum
    if Cn > 1:
        top = np.sort(c["logits"], axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2 * tol
    else:
        clear = np.ones(n, dtype=bool)
    assert (~clear).mean() <= 0.01
    got_l = labels.cpu().numpy().reshape(-1)
    assert np.array_equal(got_l[clear], ref_l[clear])
    assert ((got_l >= 0) & (got_l < Cn)).all()
    # index-driven: a shuffled list with duplicates; the other windows stay at label -1 / probability 0
    rng = np.random.default_rng(latent + Cn)
    ids = rng.permutation(n)[:301]
    ids = np.concatenate([ids, ids[:50], ids[100:103]])
    rng.shuffle(ids)
    p2, l2 = eae_amd.classify_scene(scene, model, clf, divisor=255.0, stride=8, batch=400, windows=_cuda(ids.astype(np.int64)))
    assert len(ids) % 64 and len(ids) % 256
    listed = np.zeros(n, dtype=bool)
    listed[ids] = True
    got_p2, got_l2 = p2.cpu().numpy().reshape(Cn, n).T, l2.cpu().numpy().reshape(-1)
    assert (got_l2[~listed] == -1).all() and (got_p2[~listed] == 0).all()
    rep.check("probs (windows=)", got_p2[listed], ref_p[listed], yard_p[listed], scale=1.0)
    assert np.array_equal(got_l2[listed & clear], ref_l[listed & clear])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- arguments
def test_rejected_arguments_touch_nothing():
    from eae_amd import _lib
    from eae_amd.engine import _ptr, _stream
    p0 = R.make_state(37, 16, 1)
    clf, eng = _clf(37, 16, p0, 256)
    lib = eng.lib
    x, y = R.make_batch(300, 37, 16, 2)
    xd, yd = _cuda(x), _cuda(y)
    logits = torch.full((300, 16), 7.0, device="cuda")
    eng.reset_stats()
    snap = {k: v.clone() for k, v in clf.state_dict().items()}
    grads = eng.grads.clone()
    bad = [
        lambda: eng.forward(xd[:1], train=True),                                      # BatchNorm1d in train mode needs B > 1
        lambda: eng.train_step(xd[:1], yd[:1], lr=LR),
        lambda: eng.train_step(xd, yd, lr=LR),                                        # B > max_batch (Python check)
        lambda: eng.eval_step(xd, yd),
        lambda: clf(xd[:1]),                                                          # autograd path, B = 1
        # the C entry points check on their own
        lambda: _lib.check(lib.eae_mlp_train_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 1, LR, WD, 0, None, _ptr(logits), _ptr(eng.stats))),
        lambda: _lib.check(lib.eae_mlp_train_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 257, LR, WD, 0, None, _ptr(logits), _ptr(eng.stats))),
        lambda: _lib.check(lib.eae_mlp_eval_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 257, _ptr(logits), _ptr(eng.stats))),
        lambda: _lib.check(lib.eae_mlp_eval_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 0, _ptr(logits), _ptr(eng.stats))),
        lambda: _lib.check(lib.eae_mlp_forward(eng.ctx, _stream(), _ptr(xd), 1, 1, 0, None, _ptr(logits))),
        lambda: _lib.check(lib.eae_mlp_forward(eng.ctx, _stream(), _ptr(xd), 257, 0, 0, None, _ptr(logits))),
        lambda: _lib.check(lib.eae_mlp_backward(eng.ctx, _stream(), _ptr(xd), 1, 0, None, _ptr(logits))),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"call {i} was accepted")
    poff, boff = (C.c_longlong * 11)(), (C.c_longlong * 5)()
    for IN, Cn in ((0, 10), (1025, 10), (64, 0), (64, 17), (-1, 10), (64, -1)):
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_mlp_layout(IN, Cn, poff, boff))
        h = C.c_void_p()
        with pytest.raises(RuntimeError):
            _lib.check(lib.eae_mlp_create(IN, Cn, 64, C.byref(h)))
        assert not h.value
    for IN, Cn in ((1, 1), (1024, 16)):             # the edges themselves are accepted
        _lib.check(lib.eae_mlp_layout(IN, Cn, poff, boff))
        assert poff[10] >= 128 * IN + 64 * 128 + 64 * Cn + Cn + 3 * 128 + 3 * 64 and all(o % 4 == 0 for o in poff)
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and eng.stats.abs().sum().item() == 0 and torch.equal(eng.grads, grads)
    for k, v in clf.state_dict().items():
        assert torch.equal(v, snap[k]), k
    # and the engine still works
    lg = eng.eval_step(xd[:256], yd[:256], want_logits=True)
    assert torch.isfinite(lg).all()
