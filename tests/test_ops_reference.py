"""tests/ops_ref.py against torch on the CPU in float64: the proof that the GPU op tests (test_gpu_bn_ops.py,
test_gpu_bn_statistics.py, test_gpu_head_shapes.py) compare the kernels with the right thing."""
import numpy as np
import pytest
import torch

import ops_ref as R

EPS, MOM = 1e-5, 0.1


def _bn_case(seed, n, c, h, w):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c, h, w)) * rng.uniform(0.5, 2.0, (1, c, 1, 1)) + rng.uniform(-1.0, 1.0, (1, c, 1, 1))
    gamma, beta = rng.uniform(0.5, 1.5, c), rng.standard_normal(c) * 0.2
    rm, rv = rng.standard_normal(c) * 0.3, rng.uniform(0.5, 2.0, c)
    g = rng.standard_normal((n, c, h, w))
    return x, gamma, beta, rm, rv, g


def _module(c, gamma, beta, rm, rv):
    bn = torch.nn.BatchNorm2d(c, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm)); bn.running_var.copy_(torch.from_numpy(rv))
        bn.num_batches_tracked.fill_(41)
    return bn


def _rows(a):      # NCHW -> [N*H*W][C]
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, a.shape[1])


@pytest.mark.parametrize("n,c,h,w", [(2, 3, 1, 1), (3, 5, 4, 2), (7, 32, 3, 3)])
def test_bn_train_and_backward_vs_torch(n, c, h, w):
    x, gamma, beta, rm, rv, g = _bn_case(n * 100 + c, n, c, h, w)
    bn = _module(c, gamma, beta, rm, rv).train()
    xt = torch.from_numpy(x).requires_grad_(True)
    out = bn(xt)
    out.backward(torch.from_numpy(g))
    y2, g2 = _rows(x), _rows(g)
    r = R.bn_train_ref(y2, gamma, beta, rm, rv, MOM, EPS)
    # s*y + t is the module's output
    assert np.abs(r["s"] * y2 + r["t"] - _rows(out.detach().numpy())).max() < 1e-10
    assert np.abs(r["running_mean"] - bn.running_mean.numpy()).max() < 1e-10
    assert np.abs(r["running_var"] - bn.running_var.numpy()).max() < 1e-10
    assert int(bn.num_batches_tracked) == 42
    b = R.bn_bwd_ref(g2, y2, gamma, r["mean"], r["invstd"])
    assert np.abs(b["dgamma"] - bn.weight.grad.numpy()).max() < 1e-10
    assert np.abs(b["dbeta"] - bn.bias.grad.numpy()).max() < 1e-10
    dx = _rows(xt.grad.numpy())
    assert np.abs(b["dy"] - dx).max() < 1e-10
    # A*g + B*y + C from the two sums is autograd's input gradient
    A, B, Cc = R.bn_bwd_coef_ref(b["dbeta"], b["dgamma"], y2.shape[0], gamma, r["mean"], r["invstd"])
    assert np.abs(A * g2 + B * y2 + Cc - dx).max() < 1e-10


def test_bn_partials_carry_the_moments():
    """Unequal chunks: the partial sums give back mean and biased variance (to the fp32 rounding of each partial)."""
    rng = np.random.default_rng(3)
    y = rng.standard_normal((500, 6)) + 0.5
    for nt in (1, 5, 499, 500):
        sp = R.splits_for(500, nt, rng)
        assert len(sp) == nt and len(set(sp.tolist())) == nt and sp[0] == 0
        p = R.partials(y, sp)
        assert p.shape == (2, 6, nt) and p.dtype == np.float32
        mean, var = R.moments_from_partials(p, 500)
        assert np.abs(mean - y.mean(0)).max() < 2e-7 * np.abs(y).mean() * 2
        assert np.abs(var - y.var(0)).max() < 1e-6
    # a single element: biased variance 0 goes into the running variance
    r = R.bn_from_moments(np.array([2.0]), np.array([0.0]), 1, [1.0], [0.0], [0.5], [3.0], MOM, EPS)
    assert abs(r["running_var"][0] - 2.7) < 1e-12 and abs(r["invstd"][0] - 1.0 / np.sqrt(EPS)) < 1e-9


def test_bn_eval_vs_torch():
    x, gamma, beta, rm, rv, g = _bn_case(9, 3, 7, 2, 2)
    bn = _module(7, gamma, beta, rm, rv).eval()
    out = bn(torch.from_numpy(x)).detach().numpy()
    r = R.bn_eval_ref(gamma, beta, rm, rv, EPS)
    assert np.abs(r["s"] * _rows(x) + r["t"] - _rows(out)).max() < 1e-10
    assert np.array_equal(bn.running_mean.numpy(), rm) and int(bn.num_batches_tracked) == 41


@pytest.mark.parametrize("b,l,c,scale", [(1, 4, 1, 1.0), (9, 132, 3, 1.0), (17, 64, 10, 1.0), (8, 256, 64, 1.0), (8, 64, 10, 50.0)])
def test_head_vs_torch(b, l, c, scale):
    rng = np.random.default_rng(b * 1000 + l + c)
    z = rng.standard_normal((b, l)) * scale
    w1, b1 = rng.standard_normal((128, l)) * 0.2, rng.standard_normal(128) * 0.1
    w2, b2 = rng.standard_normal((c, 128)) * 0.2, rng.standard_normal(c) * 0.1
    labels = rng.integers(0, c, b)
    zt = torch.from_numpy(z).requires_grad_(True)
    l1, l2 = torch.nn.Linear(l, 128).double(), torch.nn.Linear(128, c).double()
    with torch.no_grad():
        l1.weight.copy_(torch.from_numpy(w1)); l1.bias.copy_(torch.from_numpy(b1))
        l2.weight.copy_(torch.from_numpy(w2)); l2.bias.copy_(torch.from_numpy(b2))
    logits = l2(torch.relu(l1(zt)))
    loss = torch.nn.CrossEntropyLoss()(logits, torch.from_numpy(labels))
    loss.backward()
    r = R.head_ref(z, w1, b1, w2, b2, labels)
    sc = max(1.0, float(np.abs(r["logits"]).max()))
    assert np.abs(r["logits"] - logits.detach().numpy()).max() < 1e-10 * sc
    assert abs(r["loss"] - float(loss.detach())) < 1e-10 * sc
    assert r["correct"] == int((logits.argmax(1) == torch.from_numpy(labels)).sum())
    for name, t in (("dz", zt.grad), ("dw1", l1.weight.grad), ("db1", l1.bias.grad), ("dw2", l2.weight.grad), ("db2", l2.bias.grad)):
        assert np.abs(r[name] - t.numpy()).max() < 1e-10 * sc * scale, name
    assert set(R.head_ref(z, w1, b1, w2, b2)) == {"logits", "argmax"}


def test_head_tie_goes_to_the_first_class():
    rng = np.random.default_rng(5)
    z = rng.standard_normal((6, 8))
    w1, b1 = rng.standard_normal((128, 8)), rng.standard_normal(128)
    w2, b2 = rng.standard_normal((4, 128)), rng.standard_normal(4)
    w2[:] = np.abs(w2); w2[1] = w2[3] = w2[0] + 1.0; b2[3] = b2[1] = b2.max() + 1.0     # classes 1 and 3 tie, above the rest
    r = R.head_ref(z, w1, b1, w2, b2, np.array([1, 3, 1, 3, 0, 2]))
    assert np.array_equal(r["logits"][:, 1], r["logits"][:, 3])
    assert (r["argmax"] == 1).all() and r["correct"] == 2
