"""CPU checks of the float64 MLP reference and the NumPy Philox of tests/mlp_ref.py: the conditions that are on the reference
alone, so that the GPU tests of test_gpu_mlp_shapes.py compare the kernel with something that is itself pinned down."""
import numpy as np
import pytest

import golden_util as gu
import mlp_ref as R
from helpers import mlp_state_np
from oracle import ae_numpy as O


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox_known_answer_vectors():
    """Philox4x32-10 known-answer vectors of the Random123 distribution (kat_vectors)."""
    z, ones = 0, 0xFFFFFFFF
    assert _hex(v[()] for v in R.philox4x32_10((z, z, z, z), (z, z))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(v[()] for v in R.philox4x32_10((ones, ones, ones, ones), (ones, ones))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    # the third published vector (digits of pi) and the vectorised form agreeing with the scalar one
    pi = R.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    assert _hex(v[()] for v in pi) == "d16cfe09 94fdcceb 5001e420 24126ea1"
    vec = R.philox4x32_10((np.array([0, ones], dtype=np.uint64), np.array([0, ones]), np.array([0, ones]), np.array([0, ones])), (z, z))
    assert _hex(v[0] for v in vec) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"


def test_philox_uniform_layout():
    """counter = (element index, step lo, step hi, 0x9E3779B9), key = (seed lo, seed hi); u = (word0 >> 8) * 2^-24, exact in fp32."""
    seed, step = 0x0123456789ABCDEF, 0x00000002_00000005
    u = R.philox_uniform(seed, step, 300)
    for i in (0, 1, 129, 299):
        w0 = int(R.philox4x32_10((i, 5, 2, 0x9E3779B9), (0x89ABCDEF, 0x01234567))[0])
        assert u[i] == np.float32((w0 >> 8) / 16777216.0)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    m = R.philox_keep_mask(seed, step, 2)
    assert m.shape == (2, 128) and np.array_equal(m.ravel(), (u[:256] >= np.float32(0.3)).astype(np.float32))


def test_keep_fraction_of_every_mask_the_gpu_tests_use():
    from test_gpu_mlp_shapes import PHILOX_TRIPLES
    assert (3, 1, 64) in PHILOX_TRIPLES and any(s >> 32 for s, _, _ in PHILOX_TRIPLES) and any(b == 1500 for _, _, b in PHILOX_TRIPLES)
    for seed, step, B in PHILOX_TRIPLES:
        keep = float(R.philox_keep_mask(seed, step, B).mean())
        sigma = np.sqrt(0.21 / (128 * B))
        assert abs(keep - 0.7) <= 4 * sigma, (hex(seed), step, B, keep, abs(keep - 0.7) / sigma)
    assert abs(float(R.philox_keep_mask(3, 1, 64).mean()) - 0.687) < 5e-4
    # consecutive steps and neighbouring seeds (low and high word) give different masks
    m = R.philox_keep_mask(3, 1, 64)
    for other in (R.philox_keep_mask(3, 2, 64), R.philox_keep_mask(4, 1, 64), R.philox_keep_mask(3 | 1 << 32, 1, 64),
                  R.philox_keep_mask(3, 1 | 1 << 32, 64)):
        assert 0.3 < float((m != other).mean()) < 0.55          # independent masks differ in 2 * 0.7 * 0.3 = 42 % of the bits


def test_reference_agrees_with_oracle_and_golden(golden):
    """IN = 64, C = 10, B = 64: the float64 reference against oracle.mlp_train_step and the reference project's recorded
    forward / backward, to fp32 level."""
    g = golden("mlp_fwd_bwd_b64.npz")
    p0 = mlp_state_np()
    x, y, mask = g["x"], g["labels"], g["drop_mask"]
    ev = R.forward(p0, x, False)["logits"]
    assert np.abs(ev - g["eval_logits"]).max() < 2e-5
    assert np.abs(ev - O.mlp_forward(p0, x, train=False)["logits"]).max() < 2e-5
    ref = R.run_reference(p0, [(x, y, mask)], lr=1e-3)[0]
    orc = R.run_oracle(p0, [(x, y, mask)], lr=1e-3)[0]
    assert np.abs(ref["logits"] - g["logits"]).max() < 2e-5 and np.abs(ref["logits"] - orc["logits"]).max() < 2e-5
    assert abs(float(ref["loss"]) - float(g["loss"])) < 1e-5 and abs(float(ref["loss"]) - float(orc["loss"])) < 1e-5
    assert ref["correct"] == orc["correct"]
    for name in R.PARAMS:
        r = ref["grad/" + name]
        for other in (g["grad/" + name], orc["grad/" + name]):
            if name in R.PREBN_BIAS:
                assert np.abs(r).max() < 1e-12 and np.abs(other).max() < 1e-6      # analytically zero; fp32 leaves rounding noise
            else:
                assert np.abs(r - other).max() <= 1e-4 * np.abs(r).max(), name
        for q in ("param/", "m/", "v/"):
            a, b = ref[q + name], orc[q + name]
            np.testing.assert_allclose(a, b, rtol=3e-3, atol=3e-4 if name in R.PREBN_BIAS else 3e-5, err_msg=q + name)
    for k in g.files:
        if k.startswith("buf/") and not k.endswith("num_batches_tracked"):
            np.testing.assert_allclose(ref[k], g[k], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(ref[k], orc[k], rtol=1e-5, atol=1e-6)
    assert ref["nbt"] == int(g["buf/net.1.num_batches_tracked"])
    dx = O.mlp_backward(p0, O.mlp_forward(p0, x, True, drop_mask=mask), y)[1]["dx"]
    assert np.abs(ref["dx"] - dx).max() <= 1e-4 * np.abs(ref["dx"]).max()


def test_reference_gradients_by_finite_differences():
    """Central differences in float64 through forward + CE, at an odd shape: the backward (dx included) is the derivative."""
    IN, Cn, B = 5, 3, 6
    p = R.cast(R.make_state(IN, Cn, 4), np.float64)
    x, y = R.make_batch(B, IN, Cn, 5)
    x = x.astype(np.float64)
    mask = R.philox_keep_mask(9, 2, B)

    def loss_of(pp, xx):
        return R.cross_entropy(R.forward(pp, xx, True, drop_mask=mask)["logits"], y)[0]

    c = R.forward(p, x, True, drop_mask=mask)
    g = R.backward(p, c, R.cross_entropy(c["logits"], y)[1])
    rng = np.random.default_rng(0)
    h = 1e-6
    for name in R.PARAMS + ("dx",):
        base = x if name == "dx" else p[name]
        for _ in range(4):
            idx = tuple(rng.integers(0, s) for s in base.shape)
            d = np.zeros_like(base)
            d[idx] = h
            if name == "dx":
                fd = (loss_of(p, x + d) - loss_of(p, x - d)) / (2 * h)
            else:
                fd = (loss_of({**p, name: base + d}, x) - loss_of({**p, name: base - d}, x)) / (2 * h)
            assert abs(fd - g[name][idx]) <= 1e-7 + 1e-5 * abs(fd), (name, idx, fd, g[name][idx])


def test_running_statistics_and_adam_restatement():
    """Biased variance normalises, the unbiased one (n / (n - 1)) goes to the running statistics with momentum 0.1; Adam is
    torch.optim.Adam(weight_decay=...) (coupled L2), checked against torch on the CPU over three steps."""
    import torch
    B = 5
    p0 = R.make_state(3, 2, 8)
    x, _ = R.make_batch(B, 3, 2, 9)
    c = R.forward(p0, x, True, drop_mask=np.ones((B, 128), np.float32))
    h1 = c["h1"]
    np.testing.assert_allclose(c["new_buffers"]["net.1.running_var"],
                               0.9 * p0["net.1.running_var"].astype(np.float64) + 0.1 * h1.var(axis=0, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(c["new_buffers"]["net.1.running_mean"],
                               0.9 * p0["net.1.running_mean"].astype(np.float64) + 0.1 * h1.mean(axis=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(c["o1"], p0["net.1.weight"] * (h1 - h1.mean(0)) / np.sqrt(h1.var(axis=0) + 1e-5) + p0["net.1.bias"], rtol=1e-10, atol=1e-12)
    rng = np.random.default_rng(1)
    p = {k: rng.standard_normal(np.asarray(p0[k]).shape) for k in R.PARAMS}
    tp = {k: torch.tensor(v.copy(), dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    opt = torch.optim.Adam(list(tp.values()), lr=1e-2, weight_decay=1e-4)
    state = R.new_adam_state()
    for _ in range(3):
        g = {k: rng.standard_normal(v.shape) for k, v in p.items()}
        for k in tp:
            tp[k].grad = torch.tensor(g[k])
        opt.step()
        R.adam_step(p, g, state, 1e-2, weight_decay=1e-4)
    for k in p:
        np.testing.assert_allclose(p[k], tp[k].detach().numpy(), rtol=1e-10, atol=1e-12)


def test_case_matrix_covers_the_issue():
    from test_gpu_mlp_shapes import CASES
    assert {c[0] for c in CASES} == {1, 37, 48, 64, 128, 256, 1024} and {c[1] for c in CASES} == {1, 2, 10, 16}
    assert {c[2] for c in CASES} == {2, 3, 7, 33, 64, 200, 1024, 1025, 1500}
    shapes = {c[:3] for c in CASES}
    assert {(1024, 16, 1500), (1, 1, 2), (37, 16, 3), (48, 10, 1025)} <= shapes and 20 <= len(CASES) <= 25
    assert sum(c[3] > 1 for c in CASES) >= 3
    x, y = R.make_batch(200, 4, 10, 0)
    hist = np.bincount(y, minlength=10)
    assert hist.max() >= 3 * max(1, hist.min())                      # non-uniform class histogram
    assert (R.make_batch(9, 4, 1, 0)[1] == 0).all()


@pytest.mark.parametrize("case", range(22))
def test_cases_have_no_relu_ties(case):
    """The condition the GPU gradient comparison rests on, checked where no GPU is needed: with the hard-coded seeds no
    pre-activation of the reference lies within 16 x its fp32 yardstick of zero."""
    from test_gpu_mlp_shapes import CASES, prepare
    assert len(CASES) == 22
    assert prepare(*CASES[case])[4] == 0
