"""The optimizer kernels of the replayed train step (csrc/eae_optim.hip: adam_dyn_kernel, adam_dyn_clip_kernel = adam_body<CLIP, true>)
against the eager step's (adam_kernel, adam_clip_kernel = adam_body<CLIP, false>), bit for bit: at three arena lengths with different
last store windows and padding tails, and on a step that both must refuse.

Shapes: 64x64 images at batch 8, the (latent, bands, classes) of tests/test_gpu_grad_clip.py."""
import os

import pytest
import torch

import test_gpu_grad_clip as GC
from test_gpu_grad_clip import ALPHA, CONFIGS, LR

pytestmark = pytest.mark.gpu


def _engine(cfg, graph, clip):
    """A fresh engine of `cfg` whose context replays captured steps (EAE_GRAPH=1 at creation) or runs them eagerly."""
    if graph:
        os.environ["EAE_GRAPH"] = "1"
    else:
        os.environ.pop("EAE_GRAPH", None)
    try:
        _, e = GC._engine(cfg)
    finally:
        os.environ.pop("EAE_GRAPH", None)
    if clip is not None:
        e.set_grad_clip(clip)
    return e


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(s), _bits(t)) for s, t in zip(a, b))


@pytest.mark.parametrize("clip", [None, 1e-2], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_graph_replay_equals_eager_at_every_arena_tail(cfg, clip):
    """7 steps on the same buffers: two eager warm-up steps, the capture, four replays -- against 7 eager steps."""
    x, y = GC._batch(cfg)
    res = []
    for graph in (True, False):
        e = _engine(cfg, graph, clip)
        norms = []
        for _ in range(7):
            e.train_step(x, y, ALPHA, LR)
            if clip is not None:
                norms.append(e.read_grad_norm())
        res.append((GC._state(e), e.bn_running.clone(), e.loss_accum.clone(), norms))
    (sg, bg, lg, ng), (se, be, le, ne) = res
    assert GC._same(sg, se) and torch.equal(bg, be) and torch.equal(lg, le)
    assert ng == ne
    assert all(torch.isfinite(t).all() for t in sg) and torch.isfinite(bg).all() and torch.isfinite(lg).all()
    if clip is not None:
        assert len(ng) == 7 and all(c < 1.0 for _, c in ng)


@pytest.mark.parametrize("clip", [None, 1.0], ids=["unclipped", "clipped"])
def test_a_refused_replay_equals_a_refused_eager_step(clip):
    """One element of the input becomes inf IN PLACE (same buffers: the captured graph is replayed on it): the step is diverged, with
    clipping on the norm is not finite either.  Replay and eager refuse alike -- nothing is updated, the loss scalars read NaN -- and
    train on alike once the element is restored."""
    cfg = CONFIGS[0]
    x0, y = GC._batch(cfg)
    ends = []
    for graph in (True, False):
        e = _engine(cfg, graph, clip)
        x = x0.clone()
        for _ in range(4):                    # graph: 2 eager warm-up steps, capture, 1 replay
            e.train_step(x, y, ALPHA, LR)
        before = GC._state(e)
        assert all(torch.isfinite(t).all() for t in before) and before[1].abs().max() > 0
        keep = x[3, 1, 10, 10].item()
        x[3, 1, 10, 10] = float("inf")
        e.train_step(x, y, ALPHA, LR)
        assert _same_bits(GC._state(e), before), graph
        assert torch.isnan(e.loss_last[:3]).all(), graph
        x[3, 1, 10, 10] = keep
        for _ in range(2):
            e.train_step(x, y, ALPHA, LR)
        after = GC._state(e)
        assert all(torch.isfinite(t).all() for t in after) and torch.isfinite(e.loss_last[:3]).all(), graph
        assert not any(torch.equal(s, t) for s, t in zip(after, before)), graph
        ends.append(after + [e.bn_running.clone(), e.loss_accum.clone(), e.loss_last.clone()])
    assert _same_bits(ends[0], ends[1])
