"""Global gradient-norm clipping on the device (include/eae.h eae_set_grad_clip; engine.AEEngine.set_grad_clip / read_grad_norm;
train.AEStepper(max_grad_norm=)): the norm against the fp64 reference (tests/grad_clip_ref.py), the clipped update bit for bit against
an unclipped engine fed the coefficient as grad_scale, the untouched arithmetic below the threshold, the layout's padding, every path the
setting reaches (fused step, graph replay, group, data parallel, fit) and the refusal of a non-finite norm.

Shapes: 64x64 images at batch 8; (latent, bands, classes) = the golden shape, a padded latent with 3 padding floats behind deconv4's
bias and 2 behind the classifier's, and 13 bands / 7 classes with a latent of 128."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

import golden_util as gu
import grad_clip_ref as R
from helpers import load_state_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(64, 3, 10), (48, 1, 10), (128, 13, 7)]
ALPHA, LR = 35.0, 5e-3


def _model(cfg, seed=5):
    import eae_amd
    latent, bands, classes = cfg
    torch.manual_seed(seed)
    m = eae_amd.SupervisedAutoencoder(latent_dim=latent, num_classes=classes, image_size=64, in_channels=bands)
    load_state_np(m, gu.perturb_bn({k: v.detach().numpy().copy() for k, v in m.state_dict().items()}))
    return m.to("cuda").train()


def _engine(cfg, seed=5):
    from eae_amd.engine import engine_for
    m = _model(cfg, seed)
    return m, engine_for(m, max_batch=8)


def _batch(cfg, seed=11):
    rng = np.random.default_rng(seed)
    x = rng.random((8, cfg[1], 64, 64), dtype=np.float32)
    y = rng.integers(0, cfg[2], 8).astype(np.int64)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _sizes(cfg):
    return R.ae_param_sizes(cfg[0], cfg[2], 64, cfg[1])


def _ref_norm(eng, cfg, scale=1.0):
    torch.cuda.synchronize()
    return R.grad_norm(eng.grads.cpu().numpy(), eng.poff, _sizes(cfg), scale)


def _state(eng):
    torch.cuda.synchronize()
    return [t.clone() for t in (eng.params, eng.adam_m, eng.adam_v)]


def _same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


# ---------------------------------------------------------------------------------------------------------------- 1. norm
@pytest.mark.parametrize("cfg", CONFIGS)
def test_norm_and_coefficient_against_the_fp64_reference(cfg):
    """norm_out[0] within 1e-5 relative of the fp64 reference: fp32 tree summation at the largest arena here would give
    (log2 n + 2) * 2^-24 ~ 1.6e-6, times a margin of six (the kernels sum in fp64 and sit far inside); norm_out[1] within 2 ulp of
    min(1, max_norm / (norm_out[0] + 1e-6)) evaluated in float32."""
    _, e = _engine(cfg)
    x, y = _batch(cfg)
    for rel in (0.5, 0.01):
        e.grad_step(x, y, ALPHA)
        ref = _ref_norm(e, cfg)                   # (reads the arena back)
        assert ref > 0 and np.isfinite(ref)
        max_norm = float(np.float32(rel * ref))
        e.set_grad_clip(max_norm)
        e.adam_step(LR)
        total, coef = e.read_grad_norm()
        print(f"cfg {cfg} rel {rel}: total {total!r} reference {ref!r} rel.err {abs(total - ref) / ref:.3e} coef {coef!r}")
        assert abs(total - ref) <= 1e-5 * ref
        want = R.clip_coef_f32(total, max_norm)
        assert _ulps(coef, want) <= 2, (coef, want)
        assert coef < 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. update, bitwise
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (1e-4, 1.0), (0.0, 0.5), (1e-4, 0.5)])
def test_clipped_update_is_the_unclipped_one_with_the_coefficient_as_grad_scale(cfg, wd, gs):
    """Engine A clips at half the norm; engine B (no clip) gets fl32(grad_scale * A's coefficient) as its grad_scale: parameters and
    both moments bitwise equal -- weight decay is added after the clip."""
    x, y = _batch(cfg)
    _, a = _engine(cfg)
    _, b = _engine(cfg)
    for e in (a, b):
        e.train_step(x, y, ALPHA, LR)             # non-zero moments first
        e.grad_step(x, y, ALPHA)
    assert torch.equal(a.grads, b.grads)
    a.set_grad_clip(0.5 * _ref_norm(a, cfg, gs))
    a.adam_step(LR, weight_decay=wd, grad_scale=gs)
    total, coef = a.read_grad_norm()
    assert 0.4 < coef < 0.6
    b.adam_step(LR, weight_decay=wd, grad_scale=float(np.float32(gs) * np.float32(coef)))
    assert _same(_state(a), _state(b))
    assert b.max_grad_norm is None


# ---------------------------------------------------------------------------------------------------------------- 3. below the threshold
@pytest.mark.parametrize("cfg", CONFIGS)
def test_no_clipping_below_the_threshold_and_switching_off(cfg):
    x, y = _batch(cfg)
    engs = [_engine(cfg)[1] for _ in range(3)]            # 2 x norm, inf, off
    for e in engs:
        e.grad_step(x, y, ALPHA)
    ref = _ref_norm(engs[0], cfg)
    engs[0].set_grad_clip(2.0 * ref)
    engs[1].set_grad_clip(float("inf"))
    for e in engs:
        e.adam_step(LR, weight_decay=1e-4)
    for e in engs[:2]:
        total, coef = e.read_grad_norm()
        assert coef == 1.0 and abs(total - ref) <= 1e-5 * ref
    want = _state(engs[2])
    assert _same(_state(engs[0]), want) and _same(_state(engs[1]), want)
    # fused steps with the feature on but never clipping, then off again: the bits of an engine that never had it
    engs[1].train_step(x, y, ALPHA, LR)
    engs[2].train_step(x, y, ALPHA, LR)
    assert engs[1].read_grad_norm()[1] == 1.0
    engs[1].set_grad_clip(None)
    assert engs[1].max_grad_norm is None
    for _ in range(2):
        engs[1].train_step(x, y, ALPHA, LR)
        engs[2].train_step(x, y, ALPHA, LR)
    assert _same(_state(engs[1]), _state(engs[2]))
    assert torch.equal(engs[1].bn_running, engs[2].bn_running) and torch.equal(engs[1].loss_accum, engs[2].loss_accum)
    with pytest.raises(RuntimeError):
        engs[1].read_grad_norm()


def test_bad_max_norm_is_refused():
    from eae_amd import _lib
    _, e = _engine(CONFIGS[0])
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            e.set_grad_clip(bad)
        with pytest.raises(_lib.EaeError, match="libeae error -2"):
            _lib.check(e.lib.eae_set_grad_clip(e.ctx, bad, None))


# ---------------------------------------------------------------------------------------------------------------- 4. padding
def test_padding_between_tensors_does_not_count():
    cfg = CONFIGS[1]
    x, y = _batch(cfg)
    _, a = _engine(cfg)
    _, b = _engine(cfg)
    for e in (a, b):
        e.grad_step(x, y, ALPHA)
        e.set_grad_clip(float("inf"))
    ref = _ref_norm(a, cfg)
    pad = R.padding_index(a.poff, _sizes(cfg))
    assert len(pad) == 5
    b.grads[torch.from_numpy(pad).cuda()] = 1e4
    a.adam_step(LR)
    b.adam_step(LR)
    ta, tb = a.read_grad_norm()[0], b.read_grad_norm()[0]
    assert ta == tb and abs(tb - ref) <= 1e-5 * ref
    keep = torch.ones(a.poff[38], dtype=torch.bool, device="cuda")
    keep[torch.from_numpy(pad).cuda()] = False           # (Adam walks the whole arena: b's padding elements moved, nothing else may differ)
    assert all(torch.equal(s[keep], t[keep]) for s, t in zip(_state(a), _state(b)))


# ---------------------------------------------------------------------------------------------------------------- 5. paths
@pytest.mark.parametrize("cfg", CONFIGS)
def test_fused_step_equals_grad_step_plus_adam_step(cfg):
    x, y = _batch(cfg)
    _, a = _engine(cfg)
    _, b = _engine(cfg)
    norms = [[], []]
    for e in (a, b):
        e.set_grad_clip(1e-2)
    for _ in range(3):
        a.train_step(x, y, ALPHA, LR)
        norms[0].append(a.read_grad_norm())
        b.grad_step(x, y, ALPHA)
        b.adam_step(LR)
        norms[1].append(b.read_grad_norm())
    assert norms[0] == norms[1] and all(c < 1.0 for _, c in norms[0])
    assert _same(_state(a), _state(b))


def test_graph_replay_equals_eager_with_clipping_on_every_step():
    """The pattern of test_gpu_ae.py::test_graph_replay_equals_eager: from the third call the step -- with the sum-of-squares launch and
    the clipping optimizer kernel in it -- is replayed from a captured graph; same bits as the eager sequence."""
    cfg = CONFIGS[0]
    x, y = _batch(cfg)
    res = []
    for graph in (True, False):
        if graph:
            os.environ["EAE_GRAPH"] = "1"
        else:
            os.environ.pop("EAE_GRAPH", None)
        try:
            _, e = _engine(cfg)
            e.set_grad_clip(1e-2)
            norms = []
            for _ in range(6):
                e.train_step(x, y, ALPHA, LR)
                norms.append(e.read_grad_norm())
            res.append((_state(e), e.bn_running.clone(), e.loss_accum.clone(), norms))
        finally:
            os.environ.pop("EAE_GRAPH", None)
    assert _same(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    assert res[0][3] == res[1][3] and all(c < 1.0 for _, c in res[0][3])
    assert torch.isfinite(res[0][0][0]).all()


# ---------------------------------------------------------------------------------------------------------------- 6. non-finite
def test_non_finite_norm_refuses_the_update():
    """A data value, not a fault: one inf among the gradients makes the step diverged -- nothing is updated, loss_last reads NaN."""
    cfg = CONFIGS[0]
    x, y = _batch(cfg)
    _, e = _engine(cfg)
    e.set_grad_clip(1.0)
    e.train_step(x, y, ALPHA, LR)
    e.grad_step(x, y, ALPHA)
    before = _state(e)
    assert before[1].abs().max() > 0
    e.grads[e.poff[4] + 5] = float("inf")
    e.adam_step(LR)
    total, coef = e.read_grad_norm()
    assert not np.isfinite(total)
    assert _same(_state(e), before)
    assert torch.isnan(e.loss_last[:3]).all()
    # the next step (finite gradients again) trains
    e.train_step(x, y, ALPHA, LR)
    assert np.isfinite(e.read_grad_norm()[0]) and not torch.equal(_state(e)[0], before[0])
    assert torch.isfinite(e.loss_last[:3]).all()


# ---------------------------------------------------------------------------------------------------------------- 7. group
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2]])      # (a padded latent has no grouped form: eae_group_train_step refuses it)
def test_group_members_clip_like_each_alone(cfg):
    """Two members with max_norm = (small, inf): each bitwise the single-context step under eae_set_geometry_mult(2) -- the partial sums
    of the norm do not depend on the optimizer's grid, which shrinks for a member of a group."""
    from eae_amd import _lib
    from eae_amd.engine import AEEngine
    lib = _lib.load()
    norms = (1e-2, float("inf"))
    data = [_batch(cfg, 700 + k) for k in range(2)]
    alphas, lrs = [35.0, 20.0], [5e-3, 1e-3]

    def fresh():
        es = [_engine(cfg, seed=40 + k)[1] for k in range(2)]
        for e, mn in zip(es, norms):
            e.set_grad_clip(mn)
        return es

    def snap(e):
        torch.cuda.synchronize()
        return [t.clone() for t in (e.params, e.adam_m, e.adam_v, e.bn_running, e.loss_accum, e.grad_norm)]

    grouped = fresh()
    for _ in range(3):
        AEEngine.group_train_step(grouped, [d[0] for d in data], [d[1] for d in data], alphas, lrs)
    got = [snap(e) for e in grouped]
    alone = fresh()
    _lib.check(lib.eae_set_geometry_mult(2))
    try:
        for k, e in enumerate(alone):
            for _ in range(3):
                e.train_step(data[k][0], data[k][1], alphas[k], lrs[k])
    finally:
        _lib.check(lib.eae_set_geometry_mult(1))
    want = [snap(e) for e in alone]
    for k in range(2):
        for a, w in zip(got[k], want[k]):
            assert torch.equal(a, w), k
    assert float(got[0][5][1]) < 1.0 and float(got[1][5][1]) == 1.0
    # on in one member only: refused
    grouped[1].set_grad_clip(None)
    with pytest.raises(_lib.EaeError, match="libeae error -2.*clipping"):
        AEEngine.group_train_step(grouped, [d[0] for d in data], [d[1] for d in data], alphas, lrs)


def test_group_stepper_takes_a_value_per_member():
    from eae_amd import train as T
    cfg = CONFIGS[0]
    ms = [_model(cfg, seed=60 + k) for k in range(2)]
    st = T.GroupAEStepper(ms, [35.0, 35.0], [1e-3, 1e-3], max_batch=8, max_grad_norm=[1e-2, None])
    assert [e.max_grad_norm for e in st.engs] == [1e-2, float("inf")]
    x, y = _batch(cfg)
    st.begin([0, 1])
    st.train_step(x, y, [0, 1])
    assert st.engs[0].read_grad_norm()[1] < 1.0 and st.engs[1].read_grad_norm()[1] == 1.0
    st = T.GroupAEStepper(ms, [35.0, 35.0], [1e-3, 1e-3], max_batch=8)           # the cached engines: switched off again
    assert [e.max_grad_norm for e in st.engs] == [None, None]


# ---------------------------------------------------------------------------------------------------------------- 8. data parallel
DP_STEPS, DP_B, DP_NORM = 3, 8, 1e-2


def _dp_model():
    sys.path.insert(0, ROOT)
    import eae_amd
    torch.manual_seed(4242)
    return eae_amd.SupervisedAutoencoder(64, 10).cuda()


def _dp_data(rank):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_util as g
    x, y = g.make_images(DP_B, 900 + rank)
    return torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()


def _dp_worker(rank, world, initfile, outdir):
    import torch.distributed as dist
    from eae_amd import dp
    from eae_amd.engine import engine_for
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    m = _dp_model(); m.train()
    eng = engine_for(m, max_batch=DP_B)
    eng.set_grad_clip(DP_NORM)
    tr = dp.DataParallelTrainer(eng)
    tr.broadcast_parameters()
    x, y = _dp_data(rank)
    norms = []
    for s in range(DP_STEPS):
        tr.train_step(x, y, ALPHA, LR)
        norms.append(eng.read_grad_norm())
    torch.cuda.synchronize()
    np.savez(os.path.join(outdir, f"r{rank}.npz"), params=eng.params.cpu().numpy(), m=eng.adam_m.cpu().numpy(), norms=np.asarray(norms))
    dist.barrier()
    dist.destroy_process_group()


def test_dp_world2_replicas_clip_the_averaged_gradient_alike(monkeypatch):
    """World 2 on one GPU in the manner of test_gpu_dp2.py: the norm is taken after the all-reduce, with grad_scale = 1/2 -- the norm of
    the AVERAGED gradient; both replicas derive the same coefficient and end bitwise equal."""
    import torch.multiprocessing as mp
    from eae_amd.engine import engine_for
    monkeypatch.setenv("EAE_DP_OVERLAP", "1")
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        got = [dict(np.load(os.path.join(d, f"r{r}.npz"))) for r in range(2)]
    assert np.array_equal(got[0]["params"], got[1]["params"]) and np.array_equal(got[0]["m"], got[1]["m"])
    assert np.array_equal(got[0]["norms"], got[1]["norms"])
    # single-process reference: the shards' gradients summed, the fp64 norm of their average, Adam with grad_scale 1/2 under the same clip
    cfg = CONFIGS[0]
    m = _dp_model(); m.train()
    eng = engine_for(m, max_batch=DP_B)
    eng.set_grad_clip(DP_NORM)
    shards = [_dp_data(0), _dp_data(1)]
    for s in range(DP_STEPS):
        g = None
        for x, y in shards:
            eng.grad_step(x, y, ALPHA)
            torch.cuda.synchronize()
            g = eng.grads.clone() if g is None else g + eng.grads
        eng.grads.copy_(g)
        ref = _ref_norm(eng, cfg, 0.5)
        eng.adam_step(LR, grad_scale=0.5)
        total, coef = got[0]["norms"][s]
        assert abs(total - ref) <= 1e-5 * ref, (s, total, ref)
        assert coef < 1.0 and (total, coef) == eng.read_grad_norm()
    torch.cuda.synchronize()
    assert np.array_equal(got[0]["params"], eng.params.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- 9. fit
def test_fit_autoencoder_with_clipping_and_a_cosine_schedule():
    from eae_amd import schedule as S
    from eae_amd import train as T
    from eae_amd.engine import engine_for
    cfg = CONFIGS[0]
    m = _model(cfg)
    tr = [_batch(cfg, 21), _batch(cfg, 22)]
    va = [_batch(cfg, 23)]
    logs = []
    r = T.fit_autoencoder(tr, va, 35.0, 5e-3, num_epochs=2, model=m, log=logs.append, max_grad_norm=1e-2, lr_schedule=lambda: S.cosine(2))
    eng = engine_for(m, max_batch=8)
    total, coef = eng.read_grad_norm()
    assert np.isfinite(total) and np.isfinite(coef) and 0.0 < coef <= 1.0
    assert r["epochs"] == 2 and np.isfinite(r["train_curve"]).all() and np.isfinite(r["val_curve"]).all()
    assert logs[0].endswith("| lr=5.000e-03") and logs[1].endswith("| lr=2.500e-03")
    # a stepper built without the argument switches the cached engine's clipping off
    T.AEStepper(m, 35.0, 5e-3, max_batch=8)
    assert eng.max_grad_norm is None
