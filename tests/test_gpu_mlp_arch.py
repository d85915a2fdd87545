"""GPU parity of the layer-table MLP kernel (csrc/eae_mlp_arch.hip: MLP(hidden=, dropout=), eae_mlp_create_ex) against the float64
reference of tests/mlp_arch_ref.py, at the smallest shapes at which the layer loop, the lane split of the column reductions (widths
that do not divide 1024) and the block split of eval mode can go wrong.

Tolerances are those of tests/test_gpu_mlp_shapes.py (its Report, adam_sensitivity, LR and WD are used as they are): the yardstick of
a quantity is the deviation of a float32 run of the reference from the float64 run on the same inputs; bound = 8 x yardstick + 4 ulp
of the reference's max-abs; for the biases in front of a BatchNorm the scale and floor are max_j sum_b |dh[b, j]|, the magnitude that
cancels in their analytically zero gradient; parameters after Adam are allowed adam_sensitivity on top.  Each case asserts on the
reference alone, before launching, that no BN output of a kept unit lies within 16 x yardstick of zero and that the top two logits of
every row are further apart than that; the data seeds below were searched on the CPU for it, so no element is left out.
The same search takes a third condition, also from the reference alone (`conditioned`): in every step of a case, the bound of every
gradient is at least twice what that gradient moves when x and the parameters move by relative 2^-24 -- a proxy for the step's
conditioning, not an error of the inputs, which are exact float32 values.  Of seeds 0 .. 5 of the six train cases it turns away seeds
0 and 1 of the width-1 case (16, (1, 1, 1, 1), B = 7: BatchNorm over seven rows of a single column, 1 / std up to 9.8) and no other.
At that case's seed 0 the yardstick of one tensor, the third BatchNorm's beta gradient, was 2.9e-9 absolute (1.7e-6 of its max-abs;
the neighbouring tensors' 0.9e-8 to 2e-8), the sensitivity 1.6e-8, the bound 2.4e-8 and the kernel's deviation 4.0e-8; every other
tensor of that run held its bound.

Yardstick, bound and measured deviation (MI355X) per case, relative to the reference's max-abs, the worst tensor of each group
(fwd = logits, loss, running statistics, probs; grad = gradients; adam = parameters and moments).  `pytest -s` prints every tensor.
  case                                  group  worst tensor (deviation / bound)   yardstick  bound     measured
  train-in64-h128x64-c10-b64            fwd    step3/logits                       2.95e-07  2.83e-06  3.72e-07
  train-in64-h128x64-c10-b64            grad   step2/grad/net.1.weight            2.01e-07  2.08e-06  3.51e-07
  train-in64-h128x64-c10-b64            adam   step2/v/net.1.weight               1.78e-07  1.90e-06  6.61e-07
  train-in37-h24-c16-b3                 fwd    logits                             9.54e-08  1.24e-06  1.97e-07
  train-in37-h24-c16-b3                 grad   grad/net.0.weight                  2.00e-07  2.08e-06  1.10e-06
  train-in37-h24-c16-b3                 adam   v/net.0.weight                     4.71e-07  4.24e-06  2.27e-06
  train-in64-h256x128x64-c10-b33        fwd    step1/logits                       2.90e-07  2.80e-06  3.60e-07
  train-in64-h256x128x64-c10-b33        grad   step1/grad/net.1.weight            3.97e-07  3.65e-06  6.38e-07
  train-in64-h256x128x64-c10-b33        adam   step2/v/net.8.bias                 5.99e-04  4.79e-03  1.20e-03
  train-in16-h1x1x1x1-c2-b7             fwd    buf/net.4.running_mean             6.71e-08  1.01e-06  6.71e-08
  train-in16-h1x1x1x1-c2-b7             grad   grad/net.4.weight                  2.69e-05  2.16e-04  1.12e-04
  train-in16-h1x1x1x1-c2-b7             adam   v/net.4.bias                       1.22e-05  9.80e-05  5.10e-05
  train-in256-h512x384-c10-b65          fwd    logits                             5.14e-07  4.59e-06  5.55e-07
  train-in256-h512x384-c10-b65          grad   grad/net.5.weight                  6.12e-07  5.37e-06  9.51e-07
  train-in256-h512x384-c10-b65          adam   m/net.5.weight                     6.07e-07  5.33e-06  9.62e-07
  train-in48-h40x72x8x136-c1-b200       fwd    logits                             7.04e-07  6.10e-06  5.25e-07
  train-in48-h40x72x8x136-c1-b200       grad   grad/net.0.weight                  0.00e+00  0.00e+00  0.00e+00
  train-in48-h40x72x8x136-c1-b200       adam   v/net.3.weight                     1.94e-07  2.03e-06  1.94e-07
  masks-in48-h40x72x24-c5-b33           fwd    step1/logits                       2.13e-07  2.18e-06  3.59e-07
  masks-in48-h40x72x24-c5-b33           grad   step1/grad/net.8.weight            2.23e-07  2.26e-06  4.03e-07
  masks-in48-h40x72x24-c5-b33           adam   step1/v/net.7.bias                 3.40e-03  2.72e-02  6.55e-03
  kernels-default                       fwd    b200/loss sum                      5.65e-08  9.28e-07  2.10e-07
  eval-rows                             fwd    logits                             2.27e-07  2.29e-06  2.43e-07
  eval-blocks                           fwd    deep/weighted loss sum             9.38e-09  5.52e-07  9.17e-08
  weighted-in48-h40x72-c5-b33           fwd    logits                             2.12e-07  2.17e-06  2.34e-07
  weighted-in48-h40x72-c5-b33           grad   grad/net.1.bias                    2.30e-07  2.32e-06  2.96e-07
  weighted-in48-h40x72-c5-b33           adam   v/net.4.bias                       2.86e-03  2.29e-02  4.42e-03
  autograd-in37-h24x40-c16-b33          fwd    logits                             1.78e-07  1.90e-06  1.83e-07
  autograd-in37-h24x40-c16-b33          grad   grad/net.8.weight                  2.14e-07  2.19e-06  3.29e-07
  scene-h256x128x64                     fwd    probs                              1.95e-08  6.33e-07  1.74e-08
Every case takes well under a second on the device; the file runs in about four seconds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mlp_arch_ref as A
import mlp_ref as R
import test_gpu_mlp_shapes as S
import weighted_ce_ref as W
from test_gpu_mlp_shapes import HI_SEED, LR, WD, Report, adam_sensitivity, _cuda, _set_step

pytestmark = pytest.mark.gpu

# (input_dim, hidden, dropout, classes, batch, steps, dropout seed, force the layer-table kernel, data seed)
G1 = [
    (64, (128, 64), (0.3, 0.0), 10, 64, 3, 3, True, 0),
    (37, (24,), (0.0,), 16, 3, 1, 0, None, 0),
    (64, (256, 128, 64), (0.5, 0.3, 0.0), 10, 33, 2, HI_SEED, None, 0),
    (16, (1, 1, 1, 1), 0.0, 2, 7, 1, 0, None, 2),
    (256, (512, 384), (0.2, 0.2), 10, 65, 1, 5, None, 3),
    (48, (40, 72, 8, 136), (0.0, 0.1, 0.0, 0.4), 1, 200, 1, 6, None, 3),
]
G4 = (48, (40, 72), (0.1, 0.0), 5, 33, 7, 0)            # input_dim, hidden, dropout, classes, batch, dropout seed, data seed
G5 = (37, (24, 40), (0.3, 0.3), 16, 33, 11, 0)          # input_dim, hidden, dropout, classes, batch, engine seed, data seed


def _id(c):
    return f"in{c[0]}-h{'x'.join(map(str, c[1]))}-c{c[3]}-b{c[4]}"


# ---------------------------------------------------------------------------------------------------------------- CPU side
def prepare(IN, hidden, dropout, Cn, B, steps, dseed, seed, criterion=R.cross_entropy, labels_fn=None, first_step=1, drawn_masks=False):
    """State, batches [(x, labels, keep masks)], float64 reference, float32 yardstick, and whether the case is clear of ReLU ties and of
    top-two logit ties and well enough conditioned (`conditioned`).  The masks are the Philox masks of step first_step + s, or with
    drawn_masks random ones (handed to the kernel as its drop_mask argument)."""
    arch = A.Arch(hidden, dropout)
    p0 = A.make_state(arch, IN, Cn, 1000 * seed + IN + 7 * Cn + sum(arch.hidden))
    batches = []
    for s in range(steps):
        x, y = R.make_batch(B, IN, Cn, 77 * seed + 13 * B + IN + s)
        if labels_fn is not None:
            y = labels_fn(y, s)
        masks = A.random_keep_masks(arch, B, 5 * seed + B + s) if drawn_masks else A.philox_keep_masks(arch, dseed, first_step + s, B)
        batches.append((x, y, masks))
    ref = A.run_reference(arch, p0, batches, LR, WD, criterion=criterion)
    yard = A.run_reference(arch, p0, batches, LR, WD, dtype=np.float32, criterion=criterion)
    clear = True
    for s, (r, o, batch) in enumerate(zip(ref, yard, batches)):
        before = p0 if s == 0 else {**p0, **{k: ref[s - 1]["param/" + k] for k in arch.params}, **{k: ref[s - 1]["buf/" + k] for k in arch.buffers}}
        clear &= conditioned(arch, before, batch, r, o, criterion)
        clear &= A.relu_ties(r, o, batch[2]) == 0
        if Cn > 1:
            top = np.sort(r["logits"], axis=1)
            clear &= bool((top[:, -1] - top[:, -2]).min() > R.TIE_FACTOR * R.deviation(o["logits"], r["logits"]))
    return arch, p0, batches, ref, yard, clear


def conditioned(arch, before, batch, ref_q, yard_q, criterion, draws=16):
    """Whether the yardstick of every gradient of a step (from the state `before`) is representative of fp32 error in that step.
    x and the parameters are exact float32 values, so nothing is rounded on the way in; the relative perturbations of up to 2^-24 that
    are applied to them in the float64 reference here are a PROXY for conditioning: they show how far a gradient moves under a relative
    error of half an fp32 ulp at the first operation, the least any fp32 implementation commits somewhere along the way.  `sens` is
    the largest move of a gradient tensor over `draws` seeded perturbations.  A bound below 2 x sens says that the one fp32 run that is
    the yardstick came out unusually close in a badly conditioned case (BatchNorm over few rows of a narrow layer with a small
    variance), not that fp32 is that exact there; such a seed is not used.  From the reference alone, for every step of a case."""
    x, y, masks = batch
    rng = np.random.default_rng(12345)
    sens = {k: 0.0 for k in arch.params}
    for _ in range(draws):
        jit = lambda v: np.asarray(v, np.float64) * (1 + rng.uniform(-1, 1, np.shape(v)) * 2.0 ** -24)      # noqa: E731
        p = {k: (jit(v) if np.asarray(v).dtype.kind == "f" else v) for k, v in before.items()}
        c = A.forward(arch, p, jit(x), True, masks)
        g = A.backward(arch, p, c, criterion(c["logits"], y)[1])
        for k in arch.params:
            sens[k] = max(sens[k], R.deviation(g[k], ref_q["grad/" + k]))
    for k in arch.params:
        scale = ref_q["cancel/" + k] if k in arch.prebn_bias else float(np.abs(ref_q["grad/" + k]).max())
        if R.bound(R.deviation(yard_q["grad/" + k], ref_q["grad/" + k]), scale) < 2 * sens[k]:
            return False
    return True


def start_of(arch, p0):
    q = {}
    for k in arch.params:
        q["param/" + k] = np.asarray(p0[k], dtype=np.float64)
        q["m/" + k] = q["v/" + k] = np.zeros_like(q["param/" + k])
    return q


# ---------------------------------------------------------------------------------------------------------------- GPU side
def _clf(IN, Cn, arch, p0, max_batch=256, train=True, general=None):
    import eae_amd
    from eae_amd.mlp_engine import mlp_engine_for
    from helpers import load_state_np
    clf = eae_amd.MLP(IN, num_classes=Cn, hidden=arch.hidden, dropout=arch.dropout)
    load_state_np(clf, p0)
    clf = clf.cuda()
    clf.train(train)
    eng = mlp_engine_for(clf, max_batch=max_batch, general=general)
    assert eng.general == (True if general else (arch.hidden, arch.dropout) != A.DEFAULT)
    return clf, eng


def _compare_grads(rep, arch, clf, eng, ref, yard, tag=""):
    """Every gradient of the arena against the reference; returns {name: bound}."""
    names = [n for n, _ in clf.named_parameters()]
    assert tuple(names) == arch.params
    bounds = {}
    for (p, i), name in zip(eng._slots, names):
        sc = ref["cancel/" + name] if name in arch.prebn_bias else None
        bounds[name] = rep.check(tag + "grad/" + name, S._slot(eng, eng.grads, i, p), ref["grad/" + name], yard["grad/" + name], scale=sc,
                                 floor_scale=sc)
    return bounds


def _compare_step(rep, arch, clf, eng, logits, stats_before, ref, yard, B, tag, prev, t):
    torch.cuda.synchronize()
    rep.check(tag + "logits", logits.cpu().numpy(), ref["logits"], yard["logits"])
    st = np.array(eng.stats.tolist()[:3]) - stats_before
    rep.check(tag + "loss", st[0] / B, ref["loss"], yard["loss"])
    assert st[1] == B and st[2] == ref["correct"], (rep.case, st, ref["correct"])
    bounds = _compare_grads(rep, arch, clf, eng, ref, yard, tag)
    for (p, i), name in zip(eng._slots, arch.params):
        rep.check(tag + "m/" + name, S._slot(eng, eng.adam_m, i, p), ref["m/" + name], yard["m/" + name])
        rep.check(tag + "v/" + name, S._slot(eng, eng.adam_v, i, p), ref["v/" + name], yard["v/" + name])
        extra = adam_sensitivity(ref["grad/" + name], bounds[name], prev["param/" + name], prev["m/" + name], prev["v/" + name], t)
        rep.check(tag + "param/" + name, p.detach().cpu().numpy(), ref["param/" + name], yard["param/" + name], extra=extra)
    sd = clf.state_dict()
    for k in arch.buffers:
        rep.check(tag + "buf/" + k, sd[k].cpu().numpy(), ref["buf/" + k], yard["buf/" + k])
    assert [int(sd[bn + ".num_batches_tracked"]) for bn in arch.bn] == ref["nbt"]


# ---------------------------------------------------------------------------------------------------------------- G1
@pytest.mark.parametrize("IN,hidden,dropout,Cn,B,steps,dseed,general,seed", G1, ids=[_id(c) for c in G1])
def test_train_steps_against_reference(IN, hidden, dropout, Cn, B, steps, dseed, general, seed):
    """Fused train steps; in the rows with dropout the kernel draws its own masks (Philox keyed on the step count after the
    increment, the fourth counter word 0x9E3779B9 + layer) and the reference takes them from the NumPy Philox."""
    arch, p0, batches, ref, yard, clear = prepare(IN, hidden, dropout, Cn, B, steps, dseed, seed)
    assert clear, "ReLU ties, top-two ties or an unrepresentative yardstick: search another data seed"
    clf, eng = _clf(IN, Cn, arch, p0, max_batch=max(256, B), general=general)
    eng.seed = dseed
    rep = Report("train-" + _id((IN, arch.hidden, 0, Cn, B)))
    for s, (x, y, _) in enumerate(batches):
        before = np.array(eng.stats.tolist()[:3])
        logits = eng.train_step(_cuda(x), _cuda(y), lr=LR, weight_decay=WD, want_logits=True)
        _compare_step(rep, arch, clf, eng, logits, before, ref[s], yard[s], B, f"step{s + 1}/" if steps > 1 else "",
                      ref[s - 1] if s else start_of(arch, p0), s + 1)
    rep.done()


G1_MASKS = (48, (40, 72, 24), (0.1, 0.0, 0.4), 5, 33, 2, 0)            # input_dim, hidden, dropout, classes, batch, steps, data seed


def test_train_steps_with_caller_masks():
    """drop_mask: the caller's keep masks [B, w_l] of the layers with a rate above 0 (here layers 0 and 2, of different widths, with a
    layer without dropout between them), in layer order, back to back in one tensor."""
    IN, hidden, dropout, Cn, B, steps, seed = G1_MASKS
    arch, p0, batches, ref, yard, clear = prepare(IN, hidden, dropout, Cn, B, steps, 0, seed, drawn_masks=True)
    assert clear, "ReLU ties, top-two ties or an unrepresentative yardstick: search another data seed"
    clf, eng = _clf(IN, Cn, arch, p0)
    eng.seed = 1                    # the Philox masks of any seed differ from the drawn ones
    rep = Report("masks-" + _id(G1_MASKS))
    for s, (x, y, masks) in enumerate(batches):
        assert [m is None for m in masks] == [False, True, False]
        assert not np.array_equal(masks[0], A.philox_keep_masks(arch, eng.seed, s + 1, B)[0])
        flat = np.concatenate([m.ravel() for m in masks if m is not None])
        assert flat.size == B * (40 + 24)
        before = np.array(eng.stats.tolist()[:3])
        logits = eng.train_step(_cuda(x), _cuda(y), lr=LR, weight_decay=WD, drop_mask=_cuda(flat), want_logits=True)
        _compare_step(rep, arch, clf, eng, logits, before, ref[s], yard[s], B, f"step{s + 1}/", ref[s - 1] if s else start_of(arch, p0), s + 1)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G2
def _scene_model(latent, side=128):
    import eae_amd
    torch.manual_seed(latent)
    model = eae_amd.SupervisedAutoencoder(latent, 10)
    with torch.no_grad():
        for mod in model.enc.modules():
            if getattr(mod, "running_mean", None) is not None:
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 2.0)
    g = torch.Generator().manual_seed(latent + 1)
    scene = torch.randint(0, 256, (3, side, side), generator=g, dtype=torch.int64).to(torch.uint8).cuda()
    return model.cuda().eval(), scene


def test_default_architecture_is_the_same_classifier_on_either_kernel():
    """One state, hidden (128, 64): eval-mode logits of forward and eval_step, and probs / labels of classify_scene, are bitwise those of
    the fixed kernel (the per-row arithmetic is written alike; only the rows per block differ).  The eval loss sum crosses blocks by
    atomicAdd in either kernel: it holds the bound against the reference."""
    import eae_amd
    arch = A.Arch(*A.DEFAULT)
    IN, Cn = 64, 10
    p0 = A.make_state(arch, IN, Cn, 21)
    clf_f, fixed = _clf(IN, Cn, arch, p0, train=False)
    clf_g, table = _clf(IN, Cn, arch, p0, train=False, general=True)
    assert not fixed.general and table.general
    rep = Report("kernels-default")
    for B in (1, 63, 200):
        x, y = R.make_batch(B, IN, Cn, 5 + B)
        xd, yd = _cuda(x), _cuda(y)
        with torch.no_grad():
            lf, lg = fixed.forward(xd, train=False), table.forward(xd, train=False)
            assert torch.equal(lf, lg), B
            assert torch.equal(clf_f(xd), clf_g(xd))
        fixed.reset_stats(); table.reset_stats()
        ef, eg = fixed.eval_step(xd, yd, want_logits=True), table.eval_step(xd, yd, want_logits=True)
        assert torch.equal(ef, eg) and torch.equal(ef, lf), B
        torch.cuda.synchronize()
        c = A.forward(arch, p0, x, False)
        c32 = A.forward(arch, p0, x, False, dtype=np.float32)
        loss, _, _ = R.cross_entropy(c["logits"], y)
        loss32, _, _ = R.cross_entropy(c32["logits"], y)
        st = table.stats.tolist()[:3]
        rep.check(f"b{B}/loss sum", st[0], loss * B, float(np.float32(loss32) * np.float32(B)))
        assert st[1] == B and st[2] == fixed.stats.tolist()[2]
    model, scene = _scene_model(IN)
    pf, lf = eae_amd.classify_scene(scene, model, clf_f, divisor=255.0, stride=8, batch=64)
    pg, lg = eae_amd.classify_scene(scene, model, clf_g, divisor=255.0, stride=8, batch=64)
    assert pf.shape == (Cn, 9, 9) and torch.equal(pf, pg) and torch.equal(lf, lg)
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G3
def test_eval_rows_are_independent():
    """(64, (256, 128, 64)): a row of a B = 200 pass is bitwise the row computed alone, and the workspace size (max_batch 256 or 1024)
    does not enter.  (200 rows are one row per block on an MI355X; test_eval_blocks_of_several_rows has blocks of several rows.)"""
    arch = A.Arch((256, 128, 64), (0.5, 0.3, 0.0))
    IN, Cn, B = 64, 10, 200
    p0 = A.make_state(arch, IN, Cn, 33)
    x, _ = R.make_batch(B, IN, Cn, 44)
    xd = _cuda(x)
    _, e256 = _clf(IN, Cn, arch, p0, max_batch=256, train=False)
    _, e1024 = _clf(IN, Cn, arch, p0, max_batch=1024, train=False)
    assert (e256.max_batch, e1024.max_batch) == (256, 1024)
    with torch.no_grad():
        full = e256.forward(xd, train=False)
        assert torch.equal(full, e1024.forward(xd, train=False))
        for r in (0, 63, 64, 199):
            assert torch.equal(e256.forward(xd[r:r + 1], train=False)[0], full[r]), r
    c, c32 = A.forward(arch, p0, x, False), A.forward(arch, p0, x, False, dtype=np.float32)
    rep = Report("eval-rows")
    rep.check("logits", full.cpu().numpy(), c["logits"], c32["logits"])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G2 / G3, several rows per block
def _rows_per_block(B):
    """The launcher's eval-mode split: ceil(B / compute units), at most 64."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    return min(64, -(-B // ncu))


def _batch_of_three_row_blocks():
    """A batch that the launcher splits into blocks of 3 rows with a last block of 1 (640 on the 256 compute units of an MI355X)."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * ncu + ncu // 2
    while B % 3 != 1:
        B += 1
    assert _rows_per_block(B) == 3 and B % 3 == 1
    return B


def test_eval_blocks_of_several_rows():
    """Eval mode with more rows than compute units: blocks hold several rows (r0 = block x rows per block into x, the workspace, logits
    and labels) and the last block fewer.  Default architecture: logits of forward, eval_step and the module, bitwise those of the fixed
    kernel, with every row bitwise the row computed alone; the eval statistics; and an engine forced onto the layer-table kernel stays
    on it when a bigger batch rebuilds it.  (256, 128, 64): rows against the row alone and against the reference, and the weighted
    criterion, whose W every block sums over the whole batch."""
    B = _batch_of_three_row_blocks()
    probe = (0, 1, 2, 3, 4, 5, B // 2, B - 4, B - 3, B - 2, B - 1)        # both sides of block boundaries, and the one-row last block
    arch = A.Arch(*A.DEFAULT)
    IN, Cn = 64, 10
    p0 = A.make_state(arch, IN, Cn, 21)
    x, y = R.make_batch(B, IN, Cn, 5 + B)
    xd, yd = _cuda(x), _cuda(y)
    clf_f, fixed = _clf(IN, Cn, arch, p0, max_batch=max(1024, B), train=False)
    clf_g, small = _clf(IN, Cn, arch, p0, max_batch=256, train=False, general=True)
    rep = Report("eval-blocks")
    with torch.no_grad():
        lf = fixed.forward(xd, train=False)
        lg = clf_g(xd)                                                    # B > 256: the engine is rebuilt for the bigger batch
        from eae_amd.mlp_engine import mlp_engine_for
        table = mlp_engine_for(clf_g)
        assert table is not small and table.general and table.max_batch >= B
        assert torch.equal(lf, lg) and torch.equal(lf, table.forward(xd, train=False)) and torch.equal(lf, clf_f(xd))
        for r in probe:
            assert torch.equal(table.forward(xd[r:r + 1], train=False)[0], lg[r]), r
    fixed.reset_stats(); table.reset_stats()
    ef, eg = fixed.eval_step(xd, yd, want_logits=True), table.eval_step(xd, yd, want_logits=True)
    assert torch.equal(ef, eg) and torch.equal(eg, lf)
    torch.cuda.synchronize()
    c, c32 = A.forward(arch, p0, x, False), A.forward(arch, p0, x, False, dtype=np.float32)
    loss, _, correct = R.cross_entropy(c["logits"], y)
    loss32, _, _ = R.cross_entropy(c32["logits"], y)
    st = table.stats.tolist()[:3]
    rep.check("default/loss sum", st[0], loss * B, float(np.float32(loss32) * np.float32(B)))
    assert st[1] == B and st[2] == fixed.stats.tolist()[2]
    # a deeper classifier
    arch = A.Arch((256, 128, 64), (0.5, 0.3, 0.0))
    p0 = A.make_state(arch, IN, Cn, 33)
    _, eng = _clf(IN, Cn, arch, p0, max_batch=max(1024, B), train=False)
    with torch.no_grad():
        full = eng.forward(xd, train=False)
        for r in probe:
            assert torch.equal(eng.forward(xd[r:r + 1], train=False)[0], full[r]), r
    c, c32 = A.forward(arch, p0, x, False), A.forward(arch, p0, x, False, dtype=np.float32)
    rep.check("deep/logits", full.cpu().numpy(), c["logits"], c32["logits"])
    cw, ign = W.make_weights(np.random.default_rng(3), Cn), -100
    yw = W.ignore_some(np.random.default_rng(8), y, Cn, ign)
    eng.set_class_weights(cw, ign)
    eng.reset_stats()
    ew = eng.eval_step(xd, _cuda(yw), want_logits=True)
    assert torch.equal(ew, full)
    loss, _, correct = W.mlp_dlogits_w(c["logits"], yw, cw, ign)
    loss32, _, _ = W.mlp_dlogits_w(c32["logits"], yw, cw, ign)
    top = np.sort(c["logits"], axis=1)
    assert (top[:, -1] - top[:, -2]).min() > R.TIE_FACTOR * R.deviation(c32["logits"], c["logits"])
    st = eng.stats.tolist()[:3]
    rep.check("deep/weighted loss sum", st[0], float(loss) * B, float(np.float32(loss32) * np.float32(B)))
    assert st[1] == B and st[2] == correct and eng.read_valid() == int(W.counted_rows(yw, Cn, ign).sum())
    rep.done()


def test_predict_epilogue_in_blocks_of_several_rows():
    """classify_scene over 676 windows in one MLP launch (blocks of 3 rows, a last block of 1): probs and labels of the layer-table kernel
    at the default architecture are bitwise the fixed kernel's, over the grid and over a shuffled window list with duplicates."""
    import eae_amd
    from eae_amd.mlp_engine import mlp_engine_for
    arch = A.Arch(*A.DEFAULT)
    latent, Cn = 64, 10
    model, scene = _scene_model(latent, side=264)
    model._eae_max_batch = 676
    n_h, n_w = eae_amd.window_grid(264, 264, 64, 8)
    n = n_h * n_w
    assert n == 676 and _rows_per_block(n) > 1 and n % _rows_per_block(n)
    p0 = A.make_state(arch, latent, Cn, 21)
    clf_f, fixed = _clf(latent, Cn, arch, p0, max_batch=1024, train=False)
    clf_g, table = _clf(latent, Cn, arch, p0, max_batch=1024, train=False, general=True)
    pf, lf = eae_amd.classify_scene(scene, model, clf_f, divisor=255.0, stride=8, batch=676)
    pg, lg = eae_amd.classify_scene(scene, model, clf_g, divisor=255.0, stride=8, batch=676)
    assert mlp_engine_for(clf_g) is table and mlp_engine_for(clf_f) is fixed and table.general and not fixed.general
    assert pf.shape == (Cn, n_h, n_w) and torch.equal(pf, pg) and torch.equal(lf, lg)
    assert ((lg >= 0) & (lg < Cn)).all() and (pg.sum(dim=0) - 1).abs().max() <= 16 * R.EPS32
    rng = np.random.default_rng(4)
    ids = rng.permutation(n)[:340]
    ids = np.concatenate([ids, ids[:50], ids[100:103]])
    rng.shuffle(ids)
    assert _rows_per_block(len(ids)) > 1 and len(ids) % _rows_per_block(len(ids))
    wd = _cuda(ids.astype(np.int64))
    pf2, lf2 = eae_amd.classify_scene(scene, model, clf_f, divisor=255.0, stride=8, batch=676, windows=wd)
    pg2, lg2 = eae_amd.classify_scene(scene, model, clf_g, divisor=255.0, stride=8, batch=676, windows=wd)
    assert torch.equal(pf2, pg2) and torch.equal(lf2, lg2)
    listed = np.zeros(n, dtype=bool)
    listed[ids] = True
    got = lg2.cpu().numpy().reshape(-1)
    assert (got[~listed] == -1).all() and np.array_equal(got[listed], lg.cpu().numpy().reshape(-1)[listed])


# ---------------------------------------------------------------------------------------------------------------- G4
def test_weighted_cross_entropy():
    IN, hidden, dropout, Cn, B, dseed, seed = G4
    rng = np.random.default_rng(3)
    cw, ign = W.make_weights(rng, Cn), -100
    crit = lambda lg, y: W.mlp_dlogits_w(lg, y, cw, ign)                                  # noqa: E731
    arch, p0, batches, ref, yard, clear = prepare(IN, hidden, dropout, Cn, B, 1, dseed, seed, criterion=crit,
                                                  labels_fn=lambda y, s: W.ignore_some(np.random.default_rng(8 + s), y, Cn, ign))
    assert clear, "ReLU ties, top-two ties or an unrepresentative yardstick: search another data seed"
    x, y, _ = batches[0]
    counted = W.counted_rows(y, Cn, ign)
    assert 0 < counted.sum() < B and (y == ign).any()
    clf, eng = _clf(IN, Cn, arch, p0)
    eng.seed = dseed
    eng.set_class_weights(cw, ign)
    rep = Report("weighted-" + _id(G4))
    before = np.array(eng.stats.tolist()[:3])
    logits = eng.train_step(_cuda(x), _cuda(y), lr=LR, weight_decay=WD, want_logits=True)
    _compare_step(rep, arch, clf, eng, logits, before, ref[0], yard[0], B, "", start_of(arch, p0), 1)
    assert eng.read_valid() == int(counted.sum())
    # eval_step: the same criterion, W summed over the whole batch by every block
    sd = {k: v.cpu().numpy() for k, v in clf.state_dict().items()}
    eng.reset_stats()
    eng.eval_step(_cuda(x), _cuda(y))
    c, c32 = A.forward(arch, sd, x, False), A.forward(arch, sd, x, False, dtype=np.float32)
    loss, _, correct = crit(c["logits"], y)
    loss32, _, _ = crit(c32["logits"], y)
    st = eng.stats.tolist()[:3]
    rep.check("eval loss sum", st[0], float(loss) * B, float(np.float32(loss32) * np.float32(B)))
    assert st[1] == B and st[2] == correct and eng.read_valid() == int(counted.sum())
    # every row ignored: W == 0 gives zero loss and zero gradients
    eng.reset_stats()
    eng.grads.fill_(7.0)
    eng.train_step(_cuda(x), _cuda(np.full(B, ign, np.int64)), lr=LR, weight_decay=WD)
    torch.cuda.synchronize()
    assert eng.stats.tolist()[:3] == [0.0, float(B), 0.0] and eng.read_valid() == 0
    for (p, i) in eng._slots:
        assert not S._slot(eng, eng.grads, i, p).any()
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G5
def test_autograd_bridge():
    """logits = clf(x); (D * logits).sum().backward() with an arbitrary D: the backward recomputes the forward under the same per-layer
    Philox masks (dropout seed = engine seed + call number, step 0) and leaves the running statistics, advanced once, alone."""
    IN, hidden, dropout, Cn, B, eseed, seed = G5
    arch = A.Arch(hidden, dropout)
    p0 = A.make_state(arch, IN, Cn, 1000 * seed + IN + 7 * Cn)
    x, _ = R.make_batch(B, IN, Cn, 77 * seed + 13 * B + IN)
    dl = np.random.default_rng(B).standard_normal((B, Cn)).astype(np.float32)
    masks = A.philox_keep_masks(arch, eseed + 1, 0, B)
    c, c32 = A.forward(arch, p0, x, True, masks), A.forward(arch, p0, x, True, masks, dtype=np.float32)
    g, g32 = A.backward(arch, p0, c, dl), A.backward(arch, p0, c32, dl)
    assert A.relu_ties(c, c32, masks) == 0, "ReLU ties: search another data seed"
    clf, eng = _clf(IN, Cn, arch, p0)
    eng.seed = eseed
    eng._autograd_calls = 0
    rep = Report("autograd-" + _id(G5))
    logits = clf(_cuda(x))
    rep.check("logits", logits.detach().cpu().numpy(), c["logits"], c32["logits"])
    after_fwd = {k: v.clone() for k, v in clf.state_dict().items()}
    for k in arch.buffers:
        rep.check("buf/" + k, after_fwd[k].cpu().numpy(), c["new_buffers"][k], c32["new_buffers"][k])
    for bn in arch.bn:
        assert int(after_fwd[bn + ".num_batches_tracked"]) == int(p0[bn + ".num_batches_tracked"]) + 1
    (logits * _cuda(dl)).sum().backward()
    torch.cuda.synchronize()
    for l_name, q in clf.named_parameters():
        cancel = float(np.abs(g["dh"][arch.prebn_bias.index(l_name)]).sum(axis=0).max()) if l_name in arch.prebn_bias else None
        rep.check("grad/" + l_name, q.grad.cpu().numpy(), g[l_name], g32[l_name], scale=cancel, floor_scale=cancel)
    for k, v in clf.state_dict().items():          # statistics advanced once, not twice; parameters untouched
        assert torch.equal(v, after_fwd[k]), k
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G6
def test_fit_mlp_builds_and_trains_the_architecture():
    import eae_amd
    from eae_amd.train import MLPStepper
    g = torch.Generator().manual_seed(1)
    X, Y = torch.randn(256, 16, generator=g), torch.randint(0, 4, (256,), generator=g)
    train_dl = [(X[i:i + 64], Y[i:i + 64]) for i in range(0, 256, 64)]
    val_dl, test_dl = [(X[:50], Y[:50])], [(X[50:90], Y[50:90])]
    torch.manual_seed(9)
    r = eae_amd.fit_mlp(train_dl, val_dl, test_dl, 1e-3, input_dim=16, num_classes=4, num_epochs=3, verbose=False, hidden=(32,),
                        dropout=0.0)
    keys = {"clf", "best_val_acc", "test_acc", "best_state", "train_acc", "val_acc", "train_loss", "val_loss"}
    assert set(r) == keys and r["clf"].hidden == (32,) and r["clf"].dropout == (0.0,) and len(r["train_acc"]) == 3
    torch.manual_seed(9)
    clf = eae_amd.MLP(16, num_classes=4, hidden=(32,), dropout=0.0).cuda()
    st = MLPStepper(clf, 1e-3, 1e-4, max_batch=256)
    assert st.eng.general
    for _ in range(3):
        clf.train()
        st.begin()
        for xb, yb in train_dl:
            st.train_step(xb.cuda(), yb.cuda())
        st.end()
        clf.eval()
        st.begin()
        for xb, yb in val_dl:
            st.eval_step(xb.cuda(), yb.cuda())
        st.end()
    a, b = r["clf"].state_dict(), clf.state_dict()
    assert list(a) == list(b) == ["net.0.weight", "net.0.bias", "net.1.weight", "net.1.bias", "net.1.running_mean", "net.1.running_var",
                                  "net.1.num_batches_tracked", "net.3.weight", "net.3.bias"]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert int(a["net.1.num_batches_tracked"]) == 12


def test_classify_scene_with_a_deeper_classifier():
    import eae_amd
    arch = A.Arch((256, 128, 64), (0.5, 0.3, 0.0))
    latent, Cn = 64, 10
    model, scene = _scene_model(latent)
    p0 = A.make_state(arch, latent, Cn, 55)
    clf, _ = _clf(latent, Cn, arch, p0, train=False)
    probs, labels = eae_amd.classify_scene(scene, model, clf, divisor=255.0, stride=8, batch=64)
    n = 81
    assert probs.shape == (Cn, 9, 9) and labels.shape == (9, 9)
    z = eae_amd.encode_scene(scene, model, divisor=255.0, stride=8, batch=64).cpu().numpy()
    c, c32 = A.forward(arch, p0, z, False), A.forward(arch, p0, z, False, dtype=np.float32)

    def softmax(l):
        e = np.exp(l - l.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    rep = Report("scene-h256x128x64")
    rep.check("probs", probs.cpu().numpy().reshape(Cn, n).T, softmax(c["logits"]), softmax(c32["logits"]), scale=1.0)
    tol = R.bound(R.deviation(c32["logits"], c["logits"]), float(np.abs(c["logits"]).max()))
    top = np.sort(c["logits"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > tol
    assert clear.mean() >= 0.9
    assert np.array_equal(labels.cpu().numpy().reshape(-1)[clear], c["logits"].argmax(axis=1)[clear])
    rep.done()


# ---------------------------------------------------------------------------------------------------------------- G7
def test_rejected_calls_touch_nothing():
    from eae_amd import _lib
    from eae_amd.engine import _ptr, _stream
    arch = A.Arch((40, 72), (0.1, 0.0))
    IN, Cn = 48, 5
    p0 = A.make_state(arch, IN, Cn, 2)
    clf, eng = _clf(IN, Cn, arch, p0)
    lib = eng.lib
    x, y = R.make_batch(300, IN, Cn, 2)
    xd, yd = _cuda(x), _cuda(y)
    logits = torch.full((300, Cn), 7.0, device="cuda")
    eng.reset_stats()
    snap = {k: v.clone() for k, v in clf.state_dict().items()}
    grads = eng.grads.clone()
    args = (_ptr(logits), _ptr(eng.stats))
    bad = [
        lambda: eng.train_step(xd, yd, lr=LR),                                                       # B > max_batch (Python check)
        lambda: eng.forward(xd[:1], train=True),                                                     # BatchNorm1d in train mode, B = 1
        lambda: clf(xd[:1]),
        lambda: _lib.check(lib.eae_mlp_train_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 257, LR, WD, 0, None, *args)),
        lambda: _lib.check(lib.eae_mlp_eval_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 257, *args)),
        lambda: _lib.check(lib.eae_mlp_forward(eng.ctx, _stream(), _ptr(xd), 257, 0, 0, None, _ptr(logits))),
        lambda: _lib.check(lib.eae_mlp_train_step(eng.ctx, _stream(), _ptr(xd), _ptr(yd), 1, LR, WD, 0, None, *args)),
        lambda: _lib.check(lib.eae_mlp_forward(eng.ctx, _stream(), _ptr(xd), 1, 1, 0, None, _ptr(logits))),
        lambda: _lib.check(lib.eae_mlp_backward(eng.ctx, _stream(), _ptr(xd), 1, 0, None, _ptr(logits))),
    ]
    for i, fn in enumerate(bad):
        with pytest.raises(RuntimeError):
            fn()
            pytest.fail(f"call {i} was accepted")
    # a context that was never bound
    h = C.c_void_p()
    _lib.check(lib.eae_mlp_create_ex(IN, Cn, 2, (C.c_int * 2)(40, 72), (C.c_float * 2)(0.1, 0.0), 64, C.byref(h)))
    try:
        assert lib.eae_mlp_eval_step(h, _stream(), _ptr(xd), _ptr(yd), 33, *args) == -4          # EAE_ERR_STATE
        assert lib.eae_mlp_train_step(h, _stream(), _ptr(xd), _ptr(yd), 33, LR, WD, 0, None, *args) == -4
    finally:
        lib.eae_mlp_destroy(h)
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and eng.stats.abs().sum().item() == 0 and torch.equal(eng.grads, grads)
    for k, v in clf.state_dict().items():
        assert torch.equal(v, snap[k]), k
    lg = eng.eval_step(xd[:256], yd[:256], want_logits=True)            # and the engine still works
    assert torch.isfinite(lg).all()
