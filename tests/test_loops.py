"""Bookkeeping of the fit loops (sample-weighted epoch means are the stepper's job on the device; here: early stopping,
best tracking, grid JSON schema, the reference's aliasing quirk) with scripted steppers -- no GPU needed.
Expected values are computed by hand from R.md:656-711 and R.md:2639-2704."""
import json
import os

import torch

import eae_amd
from eae_amd import train as T


class ScriptedAE:
    device = None

    def __init__(self, train_losses, val_losses):
        self.t, self.v, self.i, self.phase = train_losses, val_losses, 0, None
        self.calls = []

    def begin(self):
        self.n = 0

    def train_step(self, x, y):
        self.phase = "t"; self.n += len(x); self.calls.append(("t", len(x)))

    def eval_step(self, x, y):
        self.phase = "v"; self.n += len(x); self.calls.append(("v", len(x)))

    def end(self):
        e = self.i // 2
        out = (self.t[e] if self.i % 2 == 0 else self.v[e]), self.n
        self.i += 1
        return out


def _loader(sizes):
    return [(torch.zeros(b, 1), torch.zeros(b, dtype=torch.int64)) for b in sizes]


def test_early_stopping_strict_improvement():
    # val: improves at epochs 1,2; equal value at epoch 3 is NOT an improvement (strict <, R.md:690); patience 3
    val = [5.0, 4.0, 4.0, 4.5, 4.2, 3.0, 1.0]
    st = ScriptedAE([9, 8, 7, 6, 5, 4, 3], val)
    logs = []
    r = T.fit_autoencoder(_loader([64, 48]), _loader([64, 56]), alpha=35, lr=1e-3, num_epochs=7, patience=3, stepper=st,
                          model=None, log=logs.append)
    assert r["epochs"] == 5                      # epochs 3,4,5 fail to improve -> stop after the 5th
    assert r["best_val_loss"] == 4.0
    assert r["val_curve"] == val[:5]
    assert logs[-1] == "Early stopping triggered."
    assert logs[0] == "[AE α=35 LR=0.001] Epoch 1 | TrainLoss=9.0000 | ValLoss=5.0000"      # print format R.md:686-687
    # every batch of both loaders visited once per epoch, train before val
    assert st.calls[:4] == [("t", 64), ("t", 48), ("v", 64), ("v", 56)]


def test_grid_search_bookkeeping(tmp_path):
    table = {(20, 0.1): 3.0, (20, 0.2): 2.5, (30, 0.1): 2.5, (30, 0.2): 2.7}

    def fake_fit(tr, va, alpha, lr, **kw):
        return {"model": None, "train_curve": [1.0], "val_curve": [table[(alpha, lr)]], "best_val_loss": table[(alpha, lr)], "epochs": 1}

    out = T.grid_search_autoencoder([], [], alpha_values=(20, 30), lr_values=(0.1, 0.2), out_dir=str(tmp_path), verbose=False, fit_fn=fake_fit)
    assert (out["best_alpha"], out["best_lr"]) == (20, 0.2)          # first strict minimum wins (R.md:702)
    js = json.load(open(os.path.join(tmp_path, "validation_losses.json")))
    assert js == {"alpha=20, lr=0.1": 3.0, "alpha=20, lr=0.2": 2.5, "alpha=30, lr=0.1": 2.5, "alpha=30, lr=0.2": 2.7}


def test_grid_search_concurrent_same_bookkeeping_and_log_order(tmp_path):
    """concurrent=K runs the configurations on K host threads (each on its own stream on a GPU): the results table, the winner
    (first strict minimum in GRID order, R.md:702) and the log (a configuration's lines together, in grid order) are those of the
    sequential loop, whatever order the threads finish in."""
    import threading
    import time
    table = {(20, 0.1): 3.0, (20, 0.2): 2.5, (30, 0.1): 2.5, (30, 0.2): 2.7}
    seen = []

    def fake_fit(tr, va, alpha, lr, log=print, **kw):
        time.sleep(0.05 if alpha == 20 else 0.0)              # the first row finishes LAST
        seen.append(threading.get_ident())
        log(f"[AE α={alpha} LR={lr}] Epoch 1 | TrainLoss=1.0000 | ValLoss={table[(alpha, lr)]:.4f}")
        return {"model": None, "train_curve": [1.0], "val_curve": [table[(alpha, lr)]], "best_val_loss": table[(alpha, lr)], "epochs": 1}

    logs = {}
    outs = {}
    for k in (1, 4):
        seen.clear()
        logs[k] = []
        d = tmp_path / f"k{k}"
        outs[k] = T.grid_search_autoencoder([], [], alpha_values=(20, 30), lr_values=(0.1, 0.2), out_dir=str(d), verbose=True, fit_fn=fake_fit,
                                            log=logs[k].append, concurrent=k, device="cpu")
        if k > 1:
            assert len(set(seen)) > 1                            # really ran on several threads
    assert logs[1] == logs[4]
    assert (outs[4]["best_alpha"], outs[4]["best_lr"]) == (outs[1]["best_alpha"], outs[1]["best_lr"]) == (20, 0.2)
    assert outs[4]["results"] == outs[1]["results"]
    assert json.load(open(tmp_path / "k4" / "validation_losses.json")) == json.load(open(tmp_path / "k1" / "validation_losses.json"))


class ScriptedGroup:
    """K scripted members behind the group-stepper interface (begin / train_step / eval_step / end with the active index list)."""
    device = None

    def __init__(self, members):
        self.m = members
        self.calls = []

    def begin(self, active):
        for k in active:
            self.m[k].begin()

    def train_step(self, x, y, active):
        self.calls.append(("t", len(x), tuple(active)))
        for k in active:
            self.m[k].train_step(x, y)

    def eval_step(self, x, y, active):
        self.calls.append(("v", len(x), tuple(active)))
        for k in active:
            self.m[k].eval_step(x, y)

    def end(self, active):
        return [self.m[k].end() for k in active]


def test_group_fit_is_the_sequential_fit_per_member_and_drops_stopped_members():
    """fit_autoencoder_group keeps every member's curves / best / early stopping exactly as fit_autoencoder does for it alone
    (R.md:686-697), walks the loaders once per epoch for the whole group, and stops stepping a member once it has stopped."""
    vals = [[5.0, 4.0, 4.0, 4.5, 4.2, 3.0, 1.0], [3.0, 3.5, 3.6, 3.7, 1.0, 1.0, 1.0], [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0]]
    trains = [[9, 8, 7, 6, 5, 4, 3], [1, 1, 1, 1, 1, 1, 1], [2, 2, 2, 2, 2, 2, 2]]
    cfgs = [(35, 1e-3), (20, 2e-3), (40, 5e-3)]
    alone, alone_logs = [], []
    for k in range(3):
        lg = []
        alone.append(T.fit_autoencoder(_loader([64, 48]), _loader([64, 56]), alpha=cfgs[k][0], lr=cfgs[k][1], num_epochs=7, patience=3,
                                       stepper=ScriptedAE(trains[k], vals[k]), model=None, log=lg.append))
        alone_logs.append(lg)
    st = ScriptedGroup([ScriptedAE(trains[k], vals[k]) for k in range(3)])
    lines = [[] for _ in range(3)]
    rs = T.fit_autoencoder_group(_loader([64, 48]), _loader([64, 56]), cfgs, num_epochs=7, patience=3, stepper=st, models=None, logs=lines)
    for k in range(3):
        for key in ("train_curve", "val_curve", "best_val_loss", "epochs"):
            assert rs[k][key] == alone[k][key], (k, key)
        assert lines[k] == alone_logs[k]
    assert [r["epochs"] for r in rs] == [5, 4, 7]
    # epoch 1: all three members on every batch; epoch 5: member 1 (stopped after 4) is no longer stepped; epoch 6: member 0 gone too
    assert st.calls[:4] == [("t", 64, (0, 1, 2)), ("t", 48, (0, 1, 2)), ("v", 64, (0, 1, 2)), ("v", 56, (0, 1, 2))]
    assert st.calls[16] == ("t", 64, (0, 2)) and st.calls[20] == ("t", 64, (2,))


def test_grid_search_grouped_same_bookkeeping_and_log_order(tmp_path):
    """grouped=K: the grid is cut into groups of K in grid order, results / JSON / winner / log order are those of the sequential grid."""
    table = {(20, 0.1): 3.0, (20, 0.2): 2.5, (30, 0.1): 2.5, (30, 0.2): 2.7, (40, 0.1): 2.4, (40, 0.2): 2.4}
    seen = []

    def fake_fit(tr, va, alpha, lr, log=print, **kw):
        log(f"fit {alpha} {lr}")
        return {"model": None, "train_curve": [1.0], "val_curve": [table[(alpha, lr)]], "best_val_loss": table[(alpha, lr)], "epochs": 1}

    def fake_group_fit(tr, va, cfgs, logs=None, **kw):
        seen.append(list(cfgs))
        out = []
        for k, (a, lr) in enumerate(cfgs):
            logs[k].append(f"fit {a} {lr}")
            out.append({"model": None, "train_curve": [1.0], "val_curve": [table[(a, lr)]], "best_val_loss": table[(a, lr)], "epochs": 1})
        return out

    seq_logs, grp_logs = [], []
    a = T.grid_search_autoencoder(None, None, alpha_values=(20, 30, 40), lr_values=(0.1, 0.2), out_dir=str(tmp_path / "seq"), fit_fn=fake_fit,
                                  log=seq_logs.append)
    b = T.grid_search_autoencoder(None, None, alpha_values=(20, 30, 40), lr_values=(0.1, 0.2), out_dir=str(tmp_path / "grp"), grouped=4,
                                  group_fit_fn=fake_group_fit, log=grp_logs.append)
    assert seen == [[(20, 0.1), (20, 0.2), (30, 0.1), (30, 0.2)], [(40, 0.1), (40, 0.2)]]
    assert a["results"] == b["results"] and (a["best_alpha"], a["best_lr"]) == (b["best_alpha"], b["best_lr"]) == (40, 0.1)
    assert seq_logs == grp_logs
    assert json.load(open(tmp_path / "seq" / "validation_losses.json")) == json.load(open(tmp_path / "grp" / "validation_losses.json"))
    # two groups at a time from two host threads: same bookkeeping, same log order
    seen.clear()
    par_logs = []
    c = T.grid_search_autoencoder(None, None, alpha_values=(20, 30, 40), lr_values=(0.1, 0.2), out_dir=str(tmp_path / "par"), grouped=2,
                                  concurrent_groups=2, group_fit_fn=fake_group_fit, log=par_logs.append, device="cpu")
    assert sorted(seen) == [[(20, 0.1), (20, 0.2)], [(30, 0.1), (30, 0.2)], [(40, 0.1), (40, 0.2)]]
    assert a["results"] == c["results"] and (c["best_alpha"], c["best_lr"]) == (40, 0.1) and par_logs == seq_logs


_TABLE = {(20, 0.1): 3.0, (20, 0.2): 2.5, (30, 0.1): 2.5, (30, 0.2): 2.7}
_DRIVERS = ({}, {"concurrent": 2, "device": "cpu"}, {"grouped": 2})


def _fake_fits(seen_kw=None, made=None, say=None):
    """(fit_fn, group_fit_fn) over _TABLE: each configuration returns a tiny Linear filled with alpha + lr as its "model"; they record
    the keywords they were called with in `seen_kw`, a weak reference to every model in `made`, and log `say(alpha, lr)`."""
    import weakref

    def result(alpha, lr):
        m = torch.nn.Linear(2, 1)
        with torch.no_grad():
            m.weight.fill_(alpha + lr); m.bias.fill_(alpha + lr)
        if made is not None:
            made.append(weakref.ref(m))
        return {"model": m, "train_curve": [1.0], "val_curve": [_TABLE[(alpha, lr)]], "best_val_loss": _TABLE[(alpha, lr)], "epochs": 1}

    def fit(tr, va, alpha, lr, log=print, **kw):
        if seen_kw is not None:
            seen_kw.append(dict(kw))
        for ln in (say(alpha, lr) if say else ()):
            log(ln)
        return result(alpha, lr)

    def group_fit(tr, va, cfgs, logs=None, **kw):
        if seen_kw is not None:
            seen_kw.append(dict(kw))
        for k, (a, lr) in enumerate(cfgs):
            logs[k].extend(say(a, lr) if say else ())
        return [result(a, lr) for a, lr in cfgs]
    return {"fit_fn": fit, "group_fit_fn": group_fit}


def _grid(tmp_path, **kw):
    return T.grid_search_autoencoder([], [], alpha_values=(20, 30), lr_values=(0.1, 0.2), out_dir=str(tmp_path), **kw)


def test_sequential_grid_streams_the_fit_functions_lines(tmp_path):
    """The sequential driver hands its `log` to the fit function: a configuration's lines appear while it trains, after its header and
    in front of "New best AE", not when the fit returns."""
    logs, at = [], []

    def fit(tr, va, alpha, lr, log=print, **kw):
        for i in (1, 2):
            at.append(list(logs))            # what the caller has seen when this line is written
            log(f"line {i} of {alpha} {lr}")
        return {"model": None, "train_curve": [1.0], "val_curve": [1.0], "best_val_loss": _TABLE[(alpha, lr)], "epochs": 1}

    _grid(tmp_path, fit_fn=fit, log=logs.append)
    header = ["\n=====================================", "Training AE for α=20, LR=0.1", "====================================="]
    assert at[0] == header and at[1] == header + ["line 1 of 20 0.1"]
    assert logs[:7] == header + ["line 1 of 20 0.1", "line 2 of 20 0.1", "\nNew best AE", "   α=20, LR=0.1, ValLoss=3.0000"]
    second = logs.index("Training AE for α=20, LR=0.2")
    assert at[2] == logs[:second + 2] and at[3] == logs[:second + 3]
    assert logs.index("line 2 of 20 0.2") < logs.index("   α=20, LR=0.2, ValLoss=2.5000")


def test_what_a_custom_fit_function_sees(tmp_path):
    """Optional arguments reach a custom fit_fn / group_fit_fn only when set (or not the default), in all three drivers, and the
    models the grid prebuilds for the project's own fit functions never do."""
    optional = ("in_channels", "num_classes", "class_weight", "ignore_index", "max_grad_norm", "lr_schedule", "model", "models")
    w = torch.arange(1.0, 8.0)
    fac = lambda: None      # noqa: E731
    given = dict(in_channels=4, num_classes=7, class_weight=w, ignore_index=-1, max_grad_norm=2.0, lr_schedule=fac)
    for i, driver in enumerate(_DRIVERS):
        seen = []
        _grid(tmp_path / f"d{i}", verbose=False, **_fake_fits(seen_kw=seen), **driver)
        assert len(seen) == (2 if "grouped" in driver else 4)
        for kw in seen:
            assert not set(optional) & set(kw), (driver, sorted(kw))
        seen.clear()
        _grid(tmp_path / f"s{i}", verbose=False, **_fake_fits(seen_kw=seen), **driver, **given)
        assert len(seen) == (2 if "grouped" in driver else 4)
        for kw in seen:
            assert kw["in_channels"] == 4 and kw["num_classes"] == 7 and kw["class_weight"] is w and kw["ignore_index"] == -1
            assert kw["max_grad_norm"] == 2.0 and kw["lr_schedule"] is fac
            assert "model" not in kw and "models" not in kw, (driver, sorted(kw))


def test_the_saved_state_is_the_winners(tmp_path):
    """AE_GLOBAL_BEST.pt holds the state of the first strict minimum in grid order, (20, 0.2), as CPU tensors of its own; the
    `concurrent` and `grouped` drivers keep only such a copy of every finished configuration and let its model go."""
    import gc
    for i, driver in enumerate(_DRIVERS):
        made, alive = [], []

        def log(line):
            if line.startswith("Training AE"):          # bookkeeping of one configuration begins
                if not alive:
                    gc.collect()
                alive.append(sum(r() is not None for r in made))
        out = _grid(tmp_path / f"d{i}", log=log, **_fake_fits(made=made), **driver)
        assert (out["best_alpha"], out["best_lr"]) == (20, 0.2)
        state = torch.load(out["best_path"])
        assert sorted(state) == ["bias", "weight"]
        assert all(v.device.type == "cpu" and not v.requires_grad for v in state.values())
        assert torch.equal(state["weight"], torch.full((1, 2), 20.2)) and torch.equal(state["bias"], torch.full((1,), 20.2))
        assert len(made) == 4
        if driver:
            assert alive == [0, 0, 0, 0], (driver, alive)          # every fit has finished, and no result kept its model


def test_the_grid_snapshot_does_not_alias_the_model(tmp_path):
    """The state the grid keeps of a new best is a clone: a fit function that goes on changing the model it returned (the reference
    returns the LIVE model) does not change what is saved."""
    for i, driver in enumerate(_DRIVERS):
        fits = _fake_fits()
        kept = []

        def keep(fn):
            def wrapped(*a, **kw):
                r = fn(*a, **kw)
                kept.extend(r if isinstance(r, list) else [r])
                return r
            return wrapped
        out = _grid(tmp_path / f"d{i}", verbose=False, fit_fn=keep(fits["fit_fn"]), group_fit_fn=keep(fits["group_fit_fn"]), **driver)
        saved = torch.load(out["best_path"])
        for r in kept:
            for p in r["model"].state_dict().values():
                assert all(p.data_ptr() != v.data_ptr() for v in saved.values())
            with torch.no_grad():
                r["model"].weight.zero_()
        assert torch.equal(torch.load(out["best_path"])["weight"], torch.full((1, 2), 20.2))


class PlainAE:
    """A plain stepper with nothing but the four calls: no `.lr`, no device."""
    device = None

    def __init__(self):
        self.calls = []

    def begin(self):
        self.calls.append("b")

    def train_step(self, x, y):
        self.calls.append("t")

    def eval_step(self, x, y):
        self.calls.append("v")

    def end(self):
        self.calls.append("e")
        return 1.0, 8


def test_a_plain_stepper_without_lr_runs_unscheduled_and_is_left_alone():
    st = PlainAE()
    before = dict(vars(st))
    r = T.fit_autoencoder(_loader([8, 8]), _loader([8]), alpha=35, lr=1e-3, num_epochs=2, patience=5, stepper=st, model=None, verbose=False)
    assert r["epochs"] == 2 and r["train_curve"] == [1.0, 1.0] and r["best_val_loss"] == 1.0 and r["model"] is None
    assert st.calls == ["b", "t", "t", "e", "b", "v", "e"] * 2
    assert set(vars(st)) == set(before) and not hasattr(st, "lr") and not hasattr(st, "lrs") and st.device is None


class ScriptedMLP:
    device = None

    def __init__(self, clf, val_acc):
        self.clf, self.val_acc, self.k, self.epoch = clf, val_acc, 0, 0

    def begin(self):
        pass

    def train_step(self, x, y):
        with torch.no_grad():
            self.clf.net[7].bias += 1.0           # "training" mutates the live weights

    def eval_step(self, x, y):
        pass

    def end(self):
        self.k += 1
        phase = (self.k - 1) % 2                   # 0 = train, 1 = val (the final test call comes last)
        e = (self.k - 1) // 2
        if phase == 1 and e < len(self.val_acc):
            return 0.5, self.val_acc[e], 10
        return 0.5, 0.25, 10


def test_mlp_best_state_aliasing_quirk():
    val = [0.3, 0.6, 0.5]
    for alias in (True, False):
        clf = eae_amd.MLP(64)
        with torch.no_grad():
            clf.net[7].bias.zero_()
        st = ScriptedMLP(clf, val)
        r = T.fit_mlp(_loader([4]), _loader([4]), _loader([4]), lr=1e-3, num_epochs=3, clf=clf, stepper=st, alias_best=alias,
                      verbose=False)
        assert r["best_val_acc"] == 0.6 and r["val_acc"] == val
        # one train batch per epoch -> bias = epoch count. Best epoch = 2.
        got = float(clf.net[7].bias[0])
        if alias:      # reference behaviour (R.md:2683): shallow copy aliases the live tensors -> final-epoch weights
            assert got == 3.0
        else:
            assert got == 2.0


def test_evaluate_and_extract_contract_on_cpu_raises():
    # no CPU fallback: calling the product path without a HIP device must fail loudly
    import pytest
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    clf = eae_amd.MLP(64)
    with pytest.raises(RuntimeError):
        eae_amd.evaluate(clf, _loader([4]))
    m = eae_amd.SupervisedAutoencoder(64)
    with pytest.raises(RuntimeError):
        with torch.no_grad():
            m(torch.zeros(2, 3, 64, 64))
