"""Plain NumPy restatement of the external MLP (Linear-BN1d-ReLU-Dropout(0.3)-Linear-BN1d-ReLU-Linear), its CrossEntropy,
backward (with dx), running-statistics update and one coupled-L2 Adam step, for arbitrary (B, IN, C), plus the Philox4x32-10
keep mask of the kernel's dropout.

Everything is computed in ``dtype`` (float64 by default: the reference the GPU tests compare with; float32: the yardstick for
pieces the fp32 oracle lacks).  Parameters are a dict with the module's state_dict names (net.0.weight ... net.7.bias,
net.1/net.5 running_mean / running_var / num_batches_tracked)."""
import math

import numpy as np

H1, H2 = 128, 64
BN_EPS, BN_MOM, P_DROP = 1e-5, 0.1, 0.3
PARAMS = ("net.0.weight", "net.0.bias", "net.1.weight", "net.1.bias", "net.4.weight", "net.4.bias", "net.5.weight", "net.5.bias",
          "net.7.weight", "net.7.bias")
BUFFERS = ("net.1.running_mean", "net.1.running_var", "net.5.running_mean", "net.5.running_var")
PREBN_BIAS = ("net.0.bias", "net.4.bias")       # analytically zero gradient: BatchNorm removes the column mean


# ------------------------------------------------------------------------------------------------------------------ Philox
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter: 4 uint32 arrays (or scalars) of one shape, key: 2 uint32 scalars.
    Returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        h0, l0 = p0 >> np.uint64(32), p0 & _MASK
        h1, l1 = p1 >> np.uint64(32), p1 & _MASK
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def philox_uniform(seed, step, n):
    """u[i] for element index i < n: counter (i, step lo, step hi, 0x9E3779B9), key (seed lo, seed hi), u = (word0 >> 8) * 2^-24.
    float32, exact."""
    seed, step = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF
    idx = np.arange(n, dtype=np.uint64)
    w = philox4x32_10((idx, step & 0xFFFFFFFF, step >> 32, _W0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_keep_mask(seed, step, B):
    """Keep mask [B,128] (float32 0/1) of the kernel's dropout: element b*128+j is kept iff u >= float32(0.3)."""
    return (philox_uniform(seed, step, B * H1) >= np.float32(P_DROP)).astype(np.float32).reshape(B, H1)


# ------------------------------------------------------------------------------------------------------------------ model
def cast(p, dtype):
    return {k: (np.asarray(v).astype(dtype) if np.asarray(v).dtype.kind == "f" else np.asarray(v).copy()) for k, v in p.items()}


def _bn(h, gamma, beta, rm, rv, train, dtype):
    if train:
        n = h.shape[0]
        mean = h.mean(axis=0)
        var = ((h - mean) ** 2).mean(axis=0)                    # biased: normalises
        unb = var * (dtype(n) / dtype(max(n - 1, 1)))           # unbiased: running statistics
        new_rm = dtype(1 - BN_MOM) * rm + dtype(BN_MOM) * mean
        new_rv = dtype(1 - BN_MOM) * rv + dtype(BN_MOM) * unb
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    inv = dtype(1) / np.sqrt(var + dtype(BN_EPS))
    xhat = (h - mean) * inv
    return gamma * xhat + beta, xhat, inv, new_rm, new_rv


def forward(p, x, train, drop_mask=None, dtype=np.float64):
    """Returns a dict: logits, the intermediates (h1 o1 a1 h2 o2 a2, xhat / inv of both BatchNorms) and, in train mode, the
    updated running statistics under their state_dict names in ``new_buffers``.  drop_mask [B,128] is the keep mask (train)."""
    dtype = np.dtype(dtype).type
    p = cast(p, dtype)
    x = np.asarray(x).astype(dtype)
    c = {"x": x, "train": train, "dtype": dtype}
    c["h1"] = x @ p["net.0.weight"].T + p["net.0.bias"]
    c["o1"], c["xh1"], c["inv1"], rm1, rv1 = _bn(c["h1"], p["net.1.weight"], p["net.1.bias"], p["net.1.running_mean"],
                                                 p["net.1.running_var"], train, dtype)
    a1 = np.maximum(c["o1"], dtype(0))
    if train:
        if drop_mask is None:
            raise ValueError("train mode needs the keep mask")
        c["keep"] = np.asarray(drop_mask).astype(dtype) / dtype(1 - P_DROP)
        a1 = a1 * c["keep"]
    c["a1"] = a1
    c["h2"] = a1 @ p["net.4.weight"].T + p["net.4.bias"]
    c["o2"], c["xh2"], c["inv2"], rm2, rv2 = _bn(c["h2"], p["net.5.weight"], p["net.5.bias"], p["net.5.running_mean"],
                                                 p["net.5.running_var"], train, dtype)
    c["a2"] = np.maximum(c["o2"], dtype(0))
    c["logits"] = c["a2"] @ p["net.7.weight"].T + p["net.7.bias"]
    c["new_buffers"] = {"net.1.running_mean": rm1, "net.1.running_var": rv1, "net.5.running_mean": rm2,
                        "net.5.running_var": rv2} if train else {}
    return c


def cross_entropy(logits, labels):
    """CrossEntropyLoss, mean reduction: (loss, dL/dlogits, number of rows whose first maximum is the label)."""
    m = logits.max(axis=1, keepdims=True)
    ls = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    b = logits.shape[0]
    rows = np.arange(b)
    loss = -ls[rows, labels].mean()
    d = np.exp(ls)
    d[rows, labels] -= 1
    return loss, d / logits.dtype.type(b), int((logits.argmax(axis=1) == labels).sum())


def _bn_bwd(do, gamma, xhat, inv):
    n = do.shape[0]
    dgamma = (do * xhat).sum(axis=0)
    dbeta = do.sum(axis=0)
    dh = gamma * inv / n * (n * do - dbeta - xhat * dgamma)
    return dh, dgamma, dbeta


def backward(p, c, dlogits):
    """Gradients of sum(dlogits * logits) for a train-mode forward ``c``: the ten parameters under their names, plus dx and the
    per-row gradients in front of both BatchNorms (dh1, dh2: their column sums are the analytically zero bias gradients)."""
    dtype = c["dtype"]
    p = cast(p, dtype)
    dlog = np.asarray(dlogits).astype(dtype)
    g = {}
    g["net.7.weight"], g["net.7.bias"] = dlog.T @ c["a2"], dlog.sum(axis=0)
    do2 = (dlog @ p["net.7.weight"]) * (c["o2"] > 0)
    dh2, g["net.5.weight"], g["net.5.bias"] = _bn_bwd(do2, p["net.5.weight"], c["xh2"], c["inv2"])
    g["net.4.weight"], g["net.4.bias"] = dh2.T @ c["a1"], dh2.sum(axis=0)
    da1 = dh2 @ p["net.4.weight"]
    if c["train"]:
        da1 = da1 * c["keep"]
    do1 = da1 * (c["o1"] > 0)
    dh1, g["net.1.weight"], g["net.1.bias"] = _bn_bwd(do1, p["net.1.weight"], c["xh1"], c["inv1"])
    g["net.0.weight"], g["net.0.bias"] = dh1.T @ c["x"], dh1.sum(axis=0)
    g["dx"] = dh1 @ p["net.0.weight"]
    g["dh1"], g["dh2"] = dh1, dh2
    return g


def new_adam_state():
    return {"step": 0, "m": {}, "v": {}}


def adam_step(p, g, state, lr, weight_decay=1e-4, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float64):
    """torch.optim.Adam with coupled L2: g += wd * p; p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps).  Mutates p and state."""
    dtype = np.dtype(dtype).type
    state["step"] += 1
    t = state["step"]
    step_size = dtype(lr / (1.0 - b1 ** t))
    bc2_sqrt = dtype(math.sqrt(1.0 - b2 ** t))
    for k in PARAMS:
        pk = p[k].astype(dtype)
        gk = g[k].astype(dtype) + dtype(weight_decay) * pk
        m = state["m"].get(k, np.zeros_like(pk))
        v = state["v"].get(k, np.zeros_like(pk))
        m = dtype(b1) * m + dtype(1 - b1) * gk
        v = dtype(b2) * v + dtype(1 - b2) * gk * gk
        p[k] = pk - step_size * (m / (np.sqrt(v) / bc2_sqrt + dtype(eps)))
        state["m"][k], state["v"][k] = m, v


def train_step(p, state, x, labels, lr, weight_decay=1e-4, drop_mask=None, dtype=np.float64):
    """One fused iteration (forward, CE, backward, running statistics, num_batches_tracked, Adam).  Mutates p and state;
    returns (loss, number correct, forward dict, gradients)."""
    c = forward(p, x, True, drop_mask=drop_mask, dtype=dtype)
    loss, dlog, correct = cross_entropy(c["logits"], labels)
    g = backward(p, c, dlog)
    for k, v in c["new_buffers"].items():
        p[k] = v
    for k in ("net.1.num_batches_tracked", "net.5.num_batches_tracked"):
        p[k] = p[k] + 1
    adam_step(p, g, state, lr, weight_decay=weight_decay, dtype=dtype)
    return loss, correct, c, g


# ------------------------------------------------------------------------------------------------------------------ inputs
def make_state(input_dim, num_classes, seed):
    """Float32 state: fan-in scaled weights, BatchNorm affine parameters away from (1, 0), non-trivial running statistics.
    The biases in front of a BatchNorm keep |b| >= 0.02, so that their weight-decay gradient stays far above the rounding
    noise of their (analytically zero) loss gradient and Adam's normalisation does not amplify that noise."""
    rng = np.random.default_rng(seed)

    def lin(o, i, prebn):
        s = 1.0 / math.sqrt(i)
        w = rng.uniform(-s, s, (o, i))
        b = rng.choice([-1.0, 1.0], o) * rng.uniform(0.02, 0.1, o) if prebn else rng.uniform(-s, s, o)
        return w.astype(np.float32), b.astype(np.float32)

    p = {}
    p["net.0.weight"], p["net.0.bias"] = lin(H1, input_dim, True)
    p["net.4.weight"], p["net.4.bias"] = lin(H2, H1, True)
    p["net.7.weight"], p["net.7.bias"] = lin(num_classes, H2, False)
    for name, c in (("net.1", H1), ("net.5", H2)):
        p[name + ".weight"] = (1.0 + 0.2 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".bias"] = (0.1 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".running_mean"] = (0.3 * rng.standard_normal(c)).astype(np.float32)
        p[name + ".running_var"] = rng.uniform(0.5, 2.0, c).astype(np.float32)
        p[name + ".num_batches_tracked"] = np.array(3, dtype=np.int64)
    return p


def make_batch(B, input_dim, num_classes, seed):
    """x [B,IN] float32 and int64 labels with a non-uniform class histogram (class c has weight c + 1; C = 1: all zeros)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, input_dim)).astype(np.float32)
    w = np.arange(1, num_classes + 1, dtype=np.float64)
    y = rng.choice(num_classes, size=B, p=w / w.sum()).astype(np.int64)
    return x, y


# ------------------------------------------------------------------------------------------------------------------ yardstick
def _quantities(loss, correct, c, g, p, state):
    q = {"logits": c["logits"], "loss": np.asarray(loss), "correct": correct, "o1": c["o1"], "o2": c["o2"]}
    for k in PARAMS:
        q["grad/" + k] = g[k]
        q["param/" + k] = p[k].copy()
        q["m/" + k] = state["m"][k].copy()
        q["v/" + k] = state["v"][k].copy()
    for k in BUFFERS:
        q["buf/" + k] = np.asarray(p[k]).copy()
    q["dx"] = g["dx"]
    return q


def run_reference(p0, batches, lr, weight_decay=1e-4, dtype=np.float64):
    """Consecutive fused steps from state p0 over batches [(x, labels, keep mask)]: one dict of named quantities per step, plus
    the gradient bookkeeping of the last backward (``g``: dh1 / dh2 for the cancellation scale of the pre-BN bias gradients)."""
    p, state, out = cast(p0, dtype), new_adam_state(), []
    for x, y, mask in batches:
        loss, correct, c, g = train_step(p, state, x, y, lr, weight_decay, mask, dtype=dtype)
        q = _quantities(loss, correct, c, g, p, state)
        # sum_b |terms of dh[b, j]|: the magnitude that cancels in the column sums that are the pre-BN bias gradients
        q["cancel/net.0.bias"] = float(np.abs(g["dh1"]).sum(axis=0).max())
        q["cancel/net.4.bias"] = float(np.abs(g["dh2"]).sum(axis=0).max())
        q["nbt"] = int(p["net.1.num_batches_tracked"])
        out.append(q)
    return out


def run_oracle(p0, batches, lr, weight_decay=1e-4):
    """The same steps on the fp32 NumPy oracle (oracle.ae_numpy.mlp_train_step): the fp32 yardstick."""
    from oracle import ae_numpy as O
    p = {k: np.asarray(v).copy() for k, v in p0.items()}
    state, out = O.new_adam_state(), []
    for x, y, mask in batches:
        loss, fw, g = O.mlp_train_step(p, state, x, y, lr, drop_mask=mask, weight_decay=weight_decay)
        c = {"logits": fw["logits"], "o1": fw["cache"]["o1"], "o2": fw["cache"]["o2"]}
        out.append(_quantities(loss, int((fw["logits"].argmax(1) == y).sum()), c, g, p, state))
    return out


def deviation(a, b):
    """max |a - b| in float64 (0 for empty tensors)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


EPS32 = float(np.finfo(np.float32).eps)
MARGIN = 8.0          # bound = MARGIN * fp32 yardstick + floor
FLOOR_ULPS = 4.0      # floor = FLOOR_ULPS * eps32 * scale: keeps a bound above zero where the yardstick happens to be exact
TIE_FACTOR = 16.0     # ReLU ties: no pre-activation of the reference within TIE_FACTOR * yardstick of zero


def bound(yard, scale):
    return MARGIN * yard + FLOOR_ULPS * EPS32 * scale


def relu_ties(ref_q, yard_q, kept=None):
    """Boolean masks (o1 [B,128], o2 [B,64]) of the reference's pre-activations within TIE_FACTOR * yardstick of zero.
    kept: the keep mask; a dropped layer-1 unit has a1 = 0 whatever its sign, so it cannot tie."""
    t1 = np.abs(ref_q["o1"]) <= TIE_FACTOR * deviation(yard_q["o1"], ref_q["o1"])
    t2 = np.abs(ref_q["o2"]) <= TIE_FACTOR * deviation(yard_q["o2"], ref_q["o2"])
    if kept is not None:
        t1 &= np.asarray(kept) > 0
    return t1, t2
