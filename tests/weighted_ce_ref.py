"""NumPy restatement of the class-weighted cross-entropy with ignored labels that the fused steps compute (include/eae.h,
eae_set_class_weights), pinned to torch.nn.functional.cross_entropy(weight=, ignore_index=, reduction="mean") by
tests/test_weighted_ce_reference.py.  float64 by default; dtype=np.float32 gives the fp32 yardstick of the same formula.

A row is COUNTED when its label is not ignore_index and lies in [0, C).  W = sum of w[y] over the counted rows (w = 1 without a
vector); loss = sum_counted w[y] (lse - logit[y]) / W; dlogits = (softmax - onehot) w[y] / W for a counted row, a zero row otherwise;
correct counts counted rows whose first maximum is the label.  The one deviation from torch: W = 0 gives loss 0 and zero
gradients instead of NaN."""
import numpy as np

import mlp_ref as M


def counted_rows(labels, num_classes, ignore_index=None):
    labels = np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < num_classes)
    if ignore_index is not None:
        ok &= labels != ignore_index
    return ok


def cross_entropy_w(logits, labels, class_w=None, ignore_index=None):
    """(loss, dL/dlogits, correct, W) in the dtype of `logits`."""
    dt = logits.dtype.type
    b, c = logits.shape
    labels = np.asarray(labels, np.int64)
    ok = counted_rows(labels, c, ignore_index)
    safe = np.where(ok, labels, 0)
    w = np.ones(c, logits.dtype) if class_w is None else np.asarray(class_w).astype(logits.dtype)
    wr = np.where(ok, w[safe], dt(0))
    wsum = wr.sum(dtype=logits.dtype)
    m = logits.max(axis=1, keepdims=True)
    ls = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    rows = np.arange(b)
    d = np.exp(ls)
    d[rows, safe] -= dt(1)
    correct = int(((logits.argmax(axis=1) == labels) & ok).sum())
    if not wsum > 0:
        return dt(0), np.zeros_like(logits), correct, dt(0)
    loss = (-(ls[rows, safe]) * wr).sum(dtype=logits.dtype) / wsum
    return loss, d * (wr / wsum)[:, None], correct, wsum


def head_ref_w(z, w1, b1, w2, b2, labels, class_w=None, ignore_index=None, dtype=np.float64):
    """Linear(L,128)-ReLU-Linear(128,C) + the weighted CE and the whole backward: logits, argmax, loss, correct, W, dz, dw1, db1, dw2,
    db2 (the layout of ops_ref.head_ref)."""
    z, w1, b1, w2, b2 = (np.asarray(a).astype(dtype) for a in (z, w1, b1, w2, b2))
    h = np.maximum(z @ w1.T + b1, 0)
    lg = h @ w2.T + b2
    loss, dl, correct, wsum = cross_entropy_w(lg, labels, class_w, ignore_index)
    dh = (dl @ w2) * (h > 0)
    return {"logits": lg, "argmax": lg.argmax(1), "loss": float(loss), "correct": correct, "W": float(wsum), "dlogits": dl,
            "dz": dh @ w1, "dw1": dh.T @ z, "db1": dh.sum(0), "dw2": dl.T @ h, "db2": dl.sum(0)}


def mlp_dlogits_w(logits, labels, class_w=None, ignore_index=None):
    """(loss, dL/dlogits, correct) of the MLP's weighted criterion: what mlp_ref.cross_entropy is to the plain one."""
    loss, d, correct, _ = cross_entropy_w(logits, labels, class_w, ignore_index)
    return loss, d, correct


def mlp_run_w(p0, batches, lr, weight_decay, class_w=None, ignore_index=None, dtype=np.float64):
    """mlp_ref.run_reference with the weighted criterion: mlp_ref.forward / mlp_ref.backward fed with the weighted dlogits, then the
    running statistics, num_batches_tracked and Adam as in mlp_ref.train_step.  One dict of named quantities per step."""
    dt = np.dtype(dtype).type
    p, state, out = M.cast(p0, dtype), M.new_adam_state(), []
    for x, y, mask in batches:
        c = M.forward(p, x, True, drop_mask=mask, dtype=dtype)
        loss, dlog, correct = mlp_dlogits_w(c["logits"], y, class_w, ignore_index)
        g = M.backward(p, c, dlog)
        for k, v in c["new_buffers"].items():
            p[k] = v
        for k in ("net.1.num_batches_tracked", "net.5.num_batches_tracked"):
            p[k] = p[k] + 1
        M.adam_step(p, g, state, lr, weight_decay=weight_decay, dtype=dtype)
        q = M._quantities(dt(loss), correct, c, g, p, state)
        q["cancel/net.0.bias"] = float(np.abs(g["dh1"]).sum(axis=0).max())
        q["cancel/net.4.bias"] = float(np.abs(g["dh2"]).sum(axis=0).max())
        q["nbt"] = int(p["net.1.num_batches_tracked"])
        out.append(q)
    return out


def make_weights(rng, num_classes):
    """The issue's weights: uniform(0.25, 4) with one class set to 0 where C > 2."""
    w = rng.uniform(0.25, 4.0, num_classes).astype(np.float32)
    if num_classes > 2:
        w[int(rng.integers(0, num_classes))] = 0.0
    return w


def ignore_some(rng, labels, num_classes, ignore_index, fraction=0.25):
    """About `fraction` of the rows get a label that does not count, drawn from {ignore_index, -1, C, 255}."""
    labels = np.array(labels, np.int64)
    pool = np.array([ignore_index, -1, num_classes, 255], np.int64)
    hit = rng.random(labels.size) < fraction
    labels[hit] = pool[rng.integers(0, pool.size, int(hit.sum()))]
    return labels
