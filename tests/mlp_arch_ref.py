"""Plain NumPy restatement of the classifier with a configurable architecture (eae_amd.MLP(hidden=, dropout=)): per hidden layer
Linear-BN1d-ReLU-Dropout(p_l), then the last Linear; its CrossEntropy, backward (with dx), running-statistics update, one coupled-L2
Adam step, and the per-layer Philox4x32-10 keep masks of the kernel's dropout.  The structure, and at hidden = (128, 64),
dropout = (0.3, 0) every operation and its order, are those of tests/mlp_ref.py (tests/test_mlp_arch_reference.py holds the two equal
bit for bit there).

Everything is computed in ``dtype`` (float64: the reference; float32: the yardstick).  Parameters are a dict with the module's
state_dict names, which follow from the construction: a hidden layer takes the Sequential indices of Linear, BatchNorm1d, ReLU and,
only where its rate is above 0, Dropout."""
import math

import numpy as np

import mlp_ref as M

BN_EPS, BN_MOM = M.BN_EPS, M.BN_MOM
DEFAULT = ((128, 64), (0.3, 0.0))


class Arch:
    """hidden / dropout as tuples (a scalar dropout: that rate after every hidden layer) and the state_dict names they give."""

    def __init__(self, hidden, dropout):
        self.hidden = tuple(int(w) for w in hidden)
        self.dropout = (float(dropout),) * len(self.hidden) if np.isscalar(dropout) else tuple(float(p) for p in dropout)
        assert len(self.dropout) == len(self.hidden)
        self.lin, self.bn, i = [], [], 0
        for p in self.dropout:
            self.lin.append(f"net.{i}")
            self.bn.append(f"net.{i + 1}")
            i += 4 if p > 0 else 3
        self.last = f"net.{i}"
        self.n = len(self.hidden)
        self.params = tuple(n + s for l in range(self.n) for n in (self.lin[l], self.bn[l]) for s in (".weight", ".bias")) + \
            (self.last + ".weight", self.last + ".bias")
        self.buffers = tuple(n + s for n in self.bn for s in (".running_mean", ".running_var"))
        self.prebn_bias = tuple(n + ".bias" for n in self.lin)      # analytically zero gradient: BatchNorm removes the column mean

    def shapes(self, input_dim, num_classes):
        """{state_dict key: shape}, num_batches_tracked included."""
        out, k = {}, input_dim
        for l, w in enumerate(self.hidden):
            out[self.lin[l] + ".weight"], out[self.lin[l] + ".bias"] = (w, k), (w,)
            for s in (".weight", ".bias", ".running_mean", ".running_var"):
                out[self.bn[l] + s] = (w,)
            out[self.bn[l] + ".num_batches_tracked"] = ()
            k = w
        out[self.last + ".weight"], out[self.last + ".bias"] = (num_classes, k), (num_classes,)
        return out

    def layout(self, input_dim, num_classes):
        """(param_off, bn_off) of eae_mlp_layout_ex: W, b, gamma, beta per hidden layer, the last W and b, each rounded up to 4 floats,
        then the total; running mean, running variance per layer, then the total."""
        sh = self.shapes(input_dim, num_classes)
        po, o = [], 0
        for k in self.params:
            po.append(o)
            o += (int(np.prod(sh[k])) + 3) // 4 * 4
        bo, b = [], 0
        for w in self.hidden:
            bo += [b, b + w]
            b += 2 * w
        return po + [o], bo + [b]


# ------------------------------------------------------------------------------------------------------------------ Philox
def philox_uniform(seed, step, n, layer=0):
    """mlp_ref.philox_uniform with the fourth counter word 0x9E3779B9 + layer (mod 2^32): the stream of hidden layer `layer`."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(n, dtype=np.uint64)
    w = M.philox4x32_10((idx, step & 0xFFFFFFFF, step >> 32, (M._W0 + layer) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_keep_masks(arch, seed, step, B):
    """Per hidden layer the keep mask [B, w_l] (float32 0/1) of the kernel's dropout, None where the rate is 0: element b * w_l + j is
    kept iff u >= float32(p_l)."""
    return [None if p <= 0 else (philox_uniform(seed, step, B * w, l) >= np.float32(p)).astype(np.float32).reshape(B, w)
            for l, (w, p) in enumerate(zip(arch.hidden, arch.dropout))]


def random_keep_masks(arch, B, seed):
    rng = np.random.default_rng(seed)
    return [None if p <= 0 else (rng.random((B, w)) >= p).astype(np.float32) for w, p in zip(arch.hidden, arch.dropout)]


# ------------------------------------------------------------------------------------------------------------------ model
def forward(arch, p, x, train, drop_masks=None, dtype=np.float64):
    """Returns a dict: logits, per hidden layer the lists h, o (BN output), a, xh, inv, keep (None without dropout) and, in train
    mode, the updated running statistics under their state_dict names in ``new_buffers``."""
    dtype = np.dtype(dtype).type
    p = M.cast(p, dtype)
    x = np.asarray(x).astype(dtype)
    c = {"x": x, "train": train, "dtype": dtype, "h": [], "o": [], "a": [], "xh": [], "inv": [], "keep": [], "new_buffers": {}}
    a = x
    for l in range(arch.n):
        lin, bn = arch.lin[l], arch.bn[l]
        h = a @ p[lin + ".weight"].T + p[lin + ".bias"]
        o, xh, inv, rm, rv = M._bn(h, p[bn + ".weight"], p[bn + ".bias"], p[bn + ".running_mean"], p[bn + ".running_var"], train, dtype)
        a = np.maximum(o, dtype(0))
        keep = None
        if train and arch.dropout[l] > 0:
            if drop_masks is None or drop_masks[l] is None:
                raise ValueError("train mode needs the keep mask of every layer with dropout")
            keep = np.asarray(drop_masks[l]).astype(dtype) / dtype(1 - arch.dropout[l])
            a = a * keep
        for k, v in zip(("h", "o", "a", "xh", "inv", "keep"), (h, o, a, xh, inv, keep)):
            c[k].append(v)
        if train:
            c["new_buffers"][bn + ".running_mean"], c["new_buffers"][bn + ".running_var"] = rm, rv
    c["logits"] = a @ p[arch.last + ".weight"].T + p[arch.last + ".bias"]
    return c


def backward(arch, p, c, dlogits):
    """Gradients of sum(dlogits * logits) for a forward ``c``: every parameter under its name, dx, and ``dh``: per hidden layer the
    per-row gradient in front of its BatchNorm (its column sums are the analytically zero bias gradients)."""
    dtype = c["dtype"]
    p = M.cast(p, dtype)
    g = {"dh": [None] * arch.n}
    gin = np.asarray(dlogits).astype(dtype)
    above = arch.last
    for l in range(arch.n - 1, -1, -1):
        g[above + ".weight"], g[above + ".bias"] = gin.T @ c["a"][l], gin.sum(axis=0)
        da = gin @ p[above + ".weight"]
        if c["keep"][l] is not None:
            da = da * c["keep"][l]
        do = da * (c["o"][l] > 0)
        bn = arch.bn[l]
        gin, g[bn + ".weight"], g[bn + ".bias"] = M._bn_bwd(do, p[bn + ".weight"], c["xh"][l], c["inv"][l])
        g["dh"][l] = gin
        above = arch.lin[l]
    g[above + ".weight"], g[above + ".bias"] = gin.T @ c["x"], gin.sum(axis=0)
    g["dx"] = gin @ p[above + ".weight"]
    return g


def adam_step(arch, p, g, state, lr, weight_decay=1e-4, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float64):
    """mlp_ref.adam_step over this architecture's parameters.  Mutates p and state."""
    dtype = np.dtype(dtype).type
    state["step"] += 1
    t = state["step"]
    step_size = dtype(lr / (1.0 - b1 ** t))
    bc2_sqrt = dtype(math.sqrt(1.0 - b2 ** t))
    for k in arch.params:
        pk = p[k].astype(dtype)
        gk = g[k].astype(dtype) + dtype(weight_decay) * pk
        m = state["m"].get(k, np.zeros_like(pk))
        v = state["v"].get(k, np.zeros_like(pk))
        m = dtype(b1) * m + dtype(1 - b1) * gk
        v = dtype(b2) * v + dtype(1 - b2) * gk * gk
        p[k] = pk - step_size * (m / (np.sqrt(v) / bc2_sqrt + dtype(eps)))
        state["m"][k], state["v"][k] = m, v


def train_step(arch, p, state, x, labels, lr, weight_decay=1e-4, drop_masks=None, dtype=np.float64, criterion=M.cross_entropy):
    """One fused iteration (forward, criterion, backward, running statistics, num_batches_tracked, Adam).  Mutates p and state;
    returns (loss, number correct, forward dict, gradients).  criterion(logits, labels) -> (loss, dL/dlogits, correct)."""
    c = forward(arch, p, x, True, drop_masks=drop_masks, dtype=dtype)
    loss, dlog, correct = criterion(c["logits"], labels)
    g = backward(arch, p, c, dlog)
    for k, v in c["new_buffers"].items():
        p[k] = v
    for bn in arch.bn:
        p[bn + ".num_batches_tracked"] = p[bn + ".num_batches_tracked"] + 1
    adam_step(arch, p, g, state, lr, weight_decay=weight_decay, dtype=dtype)
    return loss, correct, c, g


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_state(arch, input_dim, num_classes, seed):
    """mlp_ref.make_state for this architecture (the same draws in the same order, so the default architecture gets the same state):
    the biases in front of a BatchNorm keep |b| >= 0.02, so that their weight-decay gradient stays far above the rounding noise of
    their (analytically zero) loss gradient and Adam's normalisation does not amplify that noise."""
    rng = np.random.default_rng(seed)

    def lin(o, i, prebn):
        s = 1.0 / math.sqrt(i)
        w = rng.uniform(-s, s, (o, i))
        b = rng.choice([-1.0, 1.0], o) * rng.uniform(0.02, 0.1, o) if prebn else rng.uniform(-s, s, o)
        return w.astype(np.float32), b.astype(np.float32)

    p, k = {}, input_dim
    for l, w in enumerate(arch.hidden):
        p[arch.lin[l] + ".weight"], p[arch.lin[l] + ".bias"] = lin(w, k, True)
        k = w
    p[arch.last + ".weight"], p[arch.last + ".bias"] = lin(num_classes, k, False)
    for name, c in zip(arch.bn, arch.hidden):
        p[name + ".weight"] = (1.0 + 0.2 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".running_mean"] = (0.3 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".running_var"] = rng.uniform(0.5, 2.0, c).astype(np.float32)
        p[name + ".num_batches_tracked"] = np.array(3, dtype=np.int64)
    return p


# ------------------------------------------------------------------------------------------------------------------ yardstick
def _quantities(arch, loss, correct, c, g, p, state):
    q = {"logits": c["logits"], "loss": np.asarray(loss), "correct": correct, "o": c["o"]}
    for k in arch.params:
        q["grad/" + k] = g[k]
        q["param/" + k] = p[k].copy()
        q["m/" + k] = state["m"][k].copy()
        q["v/" + k] = state["v"][k].copy()
    for k in arch.buffers:
        q["buf/" + k] = np.asarray(p[k]).copy()
    q["dx"] = g["dx"]
    return q


def run_reference(arch, p0, batches, lr, weight_decay=1e-4, dtype=np.float64, criterion=M.cross_entropy, step0=0):
    """Consecutive fused steps from state p0 over batches [(x, labels, keep masks)], Adam starting after step count step0 with zero
    moments: one dict of named quantities per step, with ``cancel/<bias>`` = max_j sum_b |dh[b, j]|, the magnitude that cancels in
    the column sums that are the pre-BN bias gradients, and ``nbt``: num_batches_tracked per layer."""
    p, state, out = M.cast(p0, dtype), {"step": step0, "m": {}, "v": {}}, []
    for x, y, masks in batches:
        loss, correct, c, g = train_step(arch, p, state, x, y, lr, weight_decay, masks, dtype=dtype, criterion=criterion)
        q = _quantities(arch, np.dtype(dtype).type(loss), correct, c, g, p, state)
        for l, name in enumerate(arch.prebn_bias):
            q["cancel/" + name] = float(np.abs(g["dh"][l]).sum(axis=0).max())
        q["nbt"] = [int(p[bn + ".num_batches_tracked"]) for bn in arch.bn]
        out.append(q)
    return out


def relu_ties(ref_q, yard_q, masks=None):
    """Number of the reference's BN outputs within TIE_FACTOR x yardstick of zero, over all hidden layers.  masks: the keep masks; a
    dropped unit is 0 whatever its sign, so it cannot tie."""
    n = 0
    for l, (r, y) in enumerate(zip(ref_q["o"], yard_q["o"])):
        t = np.abs(r) <= M.TIE_FACTOR * M.deviation(y, r)
        if masks is not None and masks[l] is not None:
            t &= np.asarray(masks[l]) > 0
        n += int(t.sum())
    return n
