"""Per-epoch learning-rate schedules (eae_amd/schedule.py) against torch's schedulers, and how the fit loops drive them -- scripted
steppers in the style of tests/test_loops.py, no GPU needed."""
import math

import pytest
import torch

from eae_amd import schedule as S
from eae_amd import train as T

LOSSES = [2.0, 1.5, 1.2, 1.19995, 1.3, 1.25, 1.2, 1.21, 1.0, 0.99995, 0.9999, 1.1, 1.0, 1.2, 1.1, 0.8, 0.81, 0.82, 0.83, 0.84,
          0.85, 0.86, 0.87, 0.7, 0.71, 0.72, 0.73, 0.74, 0.75, 0.76, 0.77, 0.78, 0.79, 0.8, 0.81, 0.82, 0.83, 0.84, 0.85, 0.86]


def _opt(lr):
    return torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=lr)


@pytest.mark.parametrize("floor", [0.0, 1e-5])
def test_cosine_equals_torch_cosine_annealing(floor):
    base, n = 5e-3, 40
    opt = _opt(base)
    ref = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=n, eta_min=floor)
    s = S.cosine(n, warmup=0, floor=floor)
    for e in range(n):
        want = opt.param_groups[0]["lr"]
        got = s.lr(e, base)
        assert abs(got - want) <= 1e-12 * want, (e, got, want)
        opt.step(); ref.step()
        s.observe(LOSSES[e])


def test_cosine_warmup_then_anneal():
    s = S.cosine(10, warmup=4, floor=1e-4)
    lrs = [s.lr(e, 1e-2) for e in range(12)]
    assert lrs[:4] == [1e-2 * k / 4 for k in (1, 2, 3, 4)]
    assert lrs[4] == 1e-2                                            # t = 0
    assert abs(lrs[7] - (1e-4 + (1e-2 - 1e-4) * (1 + math.cos(math.pi * 3 / 6)) / 2)) < 1e-18
    assert all(a > b for a, b in zip(lrs[4:10], lrs[5:11])) and lrs[10] == lrs[11] == 1e-4
    with pytest.raises(ValueError):
        S.cosine(4, warmup=4)


@pytest.mark.parametrize("kw", [dict(factor=0.5, patience=2, threshold=1e-4, min_lr=0.0), dict(factor=0.1, patience=0, threshold=1e-2, min_lr=1e-6),
                                dict(factor=0.5, patience=5, threshold=1e-4, min_lr=0.0)])
def test_plateau_equals_torch_reduce_on_plateau(kw):
    base = 1e-2
    opt = _opt(base)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", threshold_mode="rel", **kw)
    s = S.plateau(**kw)
    seen = set()
    for e in range(40):
        want = opt.param_groups[0]["lr"]
        got = s.lr(e, base)
        assert abs(got - want) <= 1e-12 * want, (e, got, want)
        seen.add(got)
        ref.step(LOSSES[e]); s.observe(LOSSES[e])
    if kw["patience"] < 5:
        assert len(seen) > 2                                         # the sequence really reduces more than once


class ScriptedAE:
    device = None

    def __init__(self, train_losses, val_losses, lr=None):
        self.t, self.v, self.i = train_losses, val_losses, 0
        self.seen = []
        if lr is not None:
            self.lr = lr

    def begin(self):
        self.n = 0

    def train_step(self, x, y):
        self.n += len(x); self.seen.append(("t", self.i // 2, getattr(self, "lr", None)))

    def eval_step(self, x, y):
        self.n += len(x)

    def end(self):
        e = self.i // 2
        out = (self.t[e] if self.i % 2 == 0 else self.v[e]), self.n
        self.i += 1
        return out


class ScriptedGroup:
    device = None

    def __init__(self, members, lrs=None):
        self.m = members
        self.seen = []
        if lrs is not None:
            self.lrs = list(lrs)

    def begin(self, active):
        for k in active:
            self.m[k].begin()

    def train_step(self, x, y, active):
        self.seen.append(tuple(self.lrs[k] for k in active) if hasattr(self, "lrs") else None)
        for k in active:
            self.m[k].train_step(x, y)

    def eval_step(self, x, y, active):
        for k in active:
            self.m[k].eval_step(x, y)

    def end(self, active):
        return [self.m[k].end() for k in active]


def _loader(sizes):
    return [(torch.zeros(b, 1), torch.zeros(b, dtype=torch.int64)) for b in sizes]


def test_fit_autoencoder_sets_the_scheduled_lr_before_every_epoch():
    n = 6
    st = ScriptedAE(list(range(9, 9 - n, -1)), [5.0, 4.0, 3.5, 3.0, 2.5, 2.0], lr=1e-3)
    logs = []
    T.fit_autoencoder(_loader([8, 8]), _loader([8]), alpha=35, lr=1e-3, num_epochs=n, patience=15, stepper=st, model=None, log=logs.append,
                      lr_schedule=lambda: S.cosine(n, warmup=2))
    want = [S.cosine(n, warmup=2).lr(e, 1e-3) for e in range(n)]
    assert [lr for _, _, lr in st.seen] == [w for w in want for _ in range(2)]        # two train batches per epoch, the epoch's lr in both
    assert logs[0] == f"[AE α=35 LR=0.001] Epoch 1 | TrainLoss=9.0000 | ValLoss=5.0000 | lr={want[0]:.3e}"
    assert all(ln.endswith(f"| lr={w:.3e}") for ln, w in zip(logs, want))


def test_plateau_in_fit_autoencoder_sees_the_validation_losses():
    val = [5.0, 4.0, 4.0, 4.0, 4.0, 3.0, 3.0, 3.0]
    st = ScriptedAE([9.0] * 8, val, lr=1.0)
    T.fit_autoencoder(_loader([8]), _loader([8]), alpha=1, lr=0.1, num_epochs=8, patience=15, stepper=st, model=None, verbose=False,
                      lr_schedule=lambda: S.plateau(factor=0.5, patience=1))
    # bad epochs 3 and 4 (1-based) -> halved before epoch 5; improvement at 6; bad 7, 8 -> halved after the last epoch
    assert [lr for _, _, lr in st.seen] == [0.1, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05]


def test_group_members_keep_their_own_schedule_state():
    a = ScriptedAE([9.0] * 6, [5.0, 4.0, 3.0, 2.0, 1.0, 0.5])          # keeps improving
    b = ScriptedAE([9.0] * 6, [5.0, 5.0, 5.0, 5.0, 5.0, 5.0])          # plateaus from the second epoch on
    g = ScriptedGroup([a, b], lrs=[7.0, 7.0])
    logs = [[], []]
    T.fit_autoencoder_group(_loader([8]), _loader([8]), [(20, 0.1), (30, 0.2)], num_epochs=6, patience=15, stepper=g, models=None, logs=logs,
                            lr_schedule=lambda: S.plateau(factor=0.5, patience=1))
    assert g.seen == [(0.1, 0.2), (0.1, 0.2), (0.1, 0.2), (0.1, 0.1), (0.1, 0.1), (0.1, 0.05)]
    assert logs[0][3].endswith("| lr=1.000e-01") and logs[1][3].endswith("| lr=1.000e-01") and logs[1][5].endswith("| lr=5.000e-02")


def test_no_schedule_is_todays_loop_byte_for_byte():
    def run(**kw):
        st = ScriptedAE([9, 8, 7, 6], [5.0, 4.0, 4.5, 4.2], lr=123.0)
        logs = []
        r = T.fit_autoencoder(_loader([8, 4]), _loader([8]), alpha=35, lr=1e-3, num_epochs=4, patience=2, stepper=st, model=None,
                              log=logs.append, **kw)
        return st, logs, r
    st, logs, r = run(lr_schedule=None)
    st0, logs0, r0 = run()
    assert logs == logs0 == ["[AE α=35 LR=0.001] Epoch 1 | TrainLoss=9.0000 | ValLoss=5.0000",
                             "[AE α=35 LR=0.001] Epoch 2 | TrainLoss=8.0000 | ValLoss=4.0000",
                             "[AE α=35 LR=0.001] Epoch 3 | TrainLoss=7.0000 | ValLoss=4.5000",
                             "[AE α=35 LR=0.001] Epoch 4 | TrainLoss=6.0000 | ValLoss=4.2000", "Early stopping triggered."]
    assert r["train_curve"] == r0["train_curve"] == [9, 8, 7, 6] and r["val_curve"] == r0["val_curve"] and r["epochs"] == 4
    assert st.lr == 123.0 and all(lr == 123.0 for _, _, lr in st.seen)          # the stepper's lr is never touched
    # the group loop likewise
    ga = ScriptedGroup([ScriptedAE([9, 8], [5.0, 4.0]), ScriptedAE([7, 6], [3.0, 3.5])])
    gl = [[], []]
    rs = T.fit_autoencoder_group(_loader([8]), _loader([8]), [(20, 0.1), (30, 0.2)], num_epochs=2, patience=5, stepper=ga, models=None, logs=gl,
                                 lr_schedule=None)
    assert gl[0] == ["[AE α=20 LR=0.1] Epoch 1 | TrainLoss=9.0000 | ValLoss=5.0000", "[AE α=20 LR=0.1] Epoch 2 | TrainLoss=8.0000 | ValLoss=4.0000"]
    assert rs[1]["val_curve"] == [3.0, 3.5] and ga.seen == [None, None]


def test_a_stepper_without_lr_is_refused():
    with pytest.raises(RuntimeError, match=r"lr_schedule needs a stepper with a settable `\.lr`"):
        T.fit_autoencoder(_loader([8]), _loader([8]), alpha=35, lr=1e-3, num_epochs=2, stepper=ScriptedAE([9, 8], [5.0, 4.0]), model=None,
                          verbose=False, lr_schedule=lambda: S.cosine(2))
    g = ScriptedGroup([ScriptedAE([9], [5.0])])
    with pytest.raises(RuntimeError, match=r"`\.lrs`"):
        T.fit_autoencoder_group(_loader([8]), _loader([8]), [(20, 0.1)], num_epochs=1, stepper=g, models=None, lr_schedule=lambda: S.cosine(2))


class ScriptedMLP:
    device = None
    lr = 0.0

    def __init__(self, val_losses):
        self.v, self.i, self.seen = val_losses, 0, []

    def begin(self):
        pass

    def train_step(self, x, y):
        self.seen.append(self.lr)

    def eval_step(self, x, y):
        pass

    def end(self):
        e = min(self.i // 2, len(self.v) - 1)
        self.i += 1
        return self.v[e], 0.5, 8


def test_fit_mlp_and_the_grids_pass_the_schedule_on(tmp_path):
    st = ScriptedMLP([1.0, 1.0, 1.0, 1.0])
    logs = []
    T.fit_mlp(_loader([8]), _loader([8]), _loader([8]), lr=0.4, num_epochs=4, stepper=st, clf=None, log=logs.append,
              lr_schedule=lambda: S.plateau(factor=0.5, patience=0))
    assert st.seen == [0.4, 0.4, 0.2, 0.1]
    assert logs[2] == "Epoch 3/4 | TrainAcc=0.500 ValAcc=0.500 | lr=2.000e-01"
    got = {}

    def fake_fit(tr, va, alpha, lr, **kw):
        got[(alpha, lr)] = kw
        return {"model": None, "train_curve": [1.0], "val_curve": [1.0], "best_val_loss": 1.0, "epochs": 1}
    fac = lambda: S.cosine(3)      # noqa: E731
    T.grid_search_autoencoder([], [], alpha_values=(20,), lr_values=(0.1,), out_dir=str(tmp_path / "a"), verbose=False, fit_fn=fake_fit,
                              max_grad_norm=2.0, lr_schedule=fac)
    assert got[(20, 0.1)]["max_grad_norm"] == 2.0 and got[(20, 0.1)]["lr_schedule"] is fac
    T.grid_search_autoencoder([], [], alpha_values=(20,), lr_values=(0.1,), out_dir=str(tmp_path / "b"), verbose=False, fit_fn=fake_fit)
    assert "max_grad_norm" not in got[(20, 0.1)] and "lr_schedule" not in got[(20, 0.1)]


def test_group_grad_norms():
    inf = float("inf")
    assert T._group_grad_norms(None, 3) == [None, None, None]
    assert T._group_grad_norms(2.0, 2) == [2.0, 2.0]
    assert T._group_grad_norms([1.0, None, 0], 3) == [1.0, inf, inf]
    with pytest.raises(ValueError):
        T._group_grad_norms([1.0], 2)
