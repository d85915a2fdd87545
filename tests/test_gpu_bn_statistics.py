"""BatchNorm statistics of the default (folded) train step, layer by layer, and the stand-alone finalize kernels inside a whole step.

Part 1.  The default step takes the batch statistics inside the conv kernels (bn_fold_fwd_finish) and the suite saw them only
behind whole-network goldens at b = 8 / 32.  Here one training-mode forward runs at B = 2, 3, 8, 33 (the images-per-tile tails of
every layer: 1, 2 and 8 images per tile), the seven raw pre-BatchNorm tensors are read back and the running statistics the step
left behind are compared with the moments of those very tensors in fp64.

The engine sums the fp32 accumulator values and stores the tensor as bf16 (round to nearest: |stored - value| <= 2^-9 |value|), so
   |mean(stored) - mean(values)|    <= 2^-9 * mean|y|
   |E[stored^2] - E[values^2]|      <= 2^-8 * E[y^2]        (2 * 2^-9, plus the square of it)
hold exactly; they are propagated to the unbiased variance and multiplied by the momentum 0.1.  The sums themselves are kept in
64-bit fixed point with a quantum of 2^-24 per workgroup contribution: beside 2^-9 that is nothing (a few thousand contributions of
half a quantum each move a mean over >= 32 elements by less than 1e-5 of these bounds).  The momentum update adds a few fp32
roundings (4 ulp of the two terms, as derived in test_gpu_bn_ops.py).  A dropped tile or image moves the mean by a fraction of
order 1/B of its size, far above the bound.  Observed on an MI355X: at most 0.004 of the bound on a running mean and 0.032 on a
running variance (the roundings of a channel average out; the bound is the worst case).

Part 2.  The same step with EAE_NO_FOLD_FWD=1 EAE_NO_FOLD_BWD=1 (stand-alone bn_finalize / bn_bwd_finalize kernels) in ONE child
process: all 38 gradients and the running statistics against the folded run's, under the limits test_gradients_vs_golden_and_oracle
uses against the bf16 oracle (two bf16 pipelines with different summation orders: bitwise equality is not expected)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_util as gu
from helpers import ae_state_np, load_state_np

pytestmark = pytest.mark.gpu

CH = (32, 64, 128, 256, 128, 64, 32)          # channels of BN layer l: enc.encoder.{1,4,7,10}, dec.decoder.{2,5,8}
HW = (32, 16, 8, 4, 8, 16, 32)                # map size of its input at 64 x 64 images
U = 2.0 ** -23
RECORD_ENV = "EAE_TEST_BN_RECORD_DIR"


def _engine(max_batch=64):
    import eae_amd
    from eae_amd.engine import engine_for
    torch.manual_seed(gu.AE_SEED)
    m = eae_amd.SupervisedAutoencoder(latent_dim=64, num_classes=10)
    load_state_np(m, ae_state_np(64))
    m = m.to("cuda")
    eng = engine_for(m, max_batch=max_batch)
    # known, non-trivial running statistics and step counters in the bound arenas
    rng = np.random.default_rng(99)
    run0 = np.zeros(eng.boff[14], np.float32)
    for l, c in enumerate(CH):
        run0[eng.boff[2 * l]: eng.boff[2 * l] + c] = rng.standard_normal(c) * 0.3
        run0[eng.boff[2 * l + 1]: eng.boff[2 * l + 1] + c] = rng.uniform(0.5, 2.0, c)
    nbt0 = np.arange(7, dtype=np.int64) * 3 + 5
    eng.bn_running.copy_(torch.from_numpy(run0).cuda())
    eng.bn_nbt.copy_(torch.from_numpy(nbt0).cuda())
    torch.cuda.synchronize()
    return m, eng, run0, nbt0


def _read_bf16(eng, kind, idx, n):
    b = np.empty(n, np.uint16)
    assert eng.lib.eae_debug_read(eng.ctx, kind, idx, b.ctypes.data_as(C.c_void_p), b.nbytes) == b.nbytes
    return (b.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("B", [2, 3, 8, 33])
def test_running_statistics_are_the_moments_of_the_stored_tensors(B):
    m, eng, run0, nbt0 = _engine()
    x, y = gu.make_images(B, 500 + B)
    eng.forward(torch.from_numpy(x).cuda(), labels=torch.from_numpy(y).cuda(), train=True, alpha=35.0)
    torch.cuda.synchronize()
    run1 = eng.bn_running.cpu().numpy().astype(np.float64)
    assert eng.bn_nbt.cpu().numpy().tolist() == (nbt0 + 1).tolist()
    assert np.isfinite(run1).all()
    worst = [0.0, 0.0]
    for l, (c, hw) in enumerate(zip(CH, HW)):
        n = B * hw * hw
        t = _read_bf16(eng, 0 if l < 4 else 2, l if l < 4 else l - 4, n * c).reshape(n, c).astype(np.float64)
        assert np.isfinite(t).all()
        mean, e2, mabs = t.mean(0), (t * t).mean(0), np.abs(t).mean(0)
        unb = (e2 - mean * mean) * (n / (n - 1.0))
        d_mean = 2.0 ** -9 * mabs * (1 + 2.0 ** -8)                 # (the bound is on the VALUES' magnitudes: at most (1 + 2^-9) of the stored ones)
        d_e2 = (2.0 ** -8 + 2.0 ** -18) * e2 * (1 + 2.0 ** -7)
        d_unb = (d_e2 + 2 * np.abs(mean) * d_mean + d_mean ** 2) * (n / (n - 1.0))
        rm0 = run0[eng.boff[2 * l]: eng.boff[2 * l] + c].astype(np.float64)
        rv0 = run0[eng.boff[2 * l + 1]: eng.boff[2 * l + 1] + c].astype(np.float64)
        rm1 = run1[eng.boff[2 * l]: eng.boff[2 * l] + c]
        rv1 = run1[eng.boff[2 * l + 1]: eng.boff[2 * l + 1] + c]
        tol_m = 0.1 * d_mean + 4 * U * (np.abs(0.9 * rm0) + np.abs(0.1 * mean))
        tol_v = 0.1 * d_unb + 4 * U * (np.abs(0.9 * rv0) + np.abs(0.1 * unb))
        em, ev = np.abs(rm1 - (0.9 * rm0 + 0.1 * mean)), np.abs(rv1 - (0.9 * rv0 + 0.1 * unb))
        worst = [max(worst[0], float((em / tol_m).max())), max(worst[1], float((ev / tol_v).max()))]
        print(f"B {B} layer {l}: running_mean err/bound {float((em / tol_m).max()):.3f}  running_var err/bound {float((ev / tol_v).max()):.3f}")
        assert (em <= tol_m).all(), (l, float((em / tol_m).max()))
        assert (ev <= tol_v).all(), (l, float((ev / tol_v).max()))


# ---------------------------------------------------------------------------------------------------- part 2
def _grad_step_record(b):
    """one eae_ae_grad_step from the fixed state -> {parameter name: gradient}, running statistics, step counters"""
    m, eng, run0, nbt0 = _engine()
    x, y = gu.make_images(b, 700 + b)
    eng.grad_step(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 35.0)
    torch.cuda.synchronize()
    eng.expose_grads()
    rec = {"grad/" + name: p.grad.cpu().numpy().copy() for name, p in m.named_parameters()}
    assert len(rec) == 38
    rec["running"] = eng.bn_running.cpu().numpy().copy()
    rec["nbt"] = eng.bn_nbt.cpu().numpy().copy()
    assert rec["nbt"].tolist() == (nbt0 + 1).tolist()
    return rec


def _rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(1e-30, np.linalg.norm(b)))


def _compare_with_record(rec, ref):
    import gpu_util as G
    bad = []
    for k in sorted(ref.files):
        got, want = rec[k], ref[k]
        if k == "nbt":
            assert np.array_equal(got, want)
            continue
        assert np.isfinite(got).all(), k
        if np.abs(want).max() == 0.0:          # bias in front of a BatchNorm: exact zeros in either form
            assert np.abs(got).max() == 0.0, k
            continue
        r, c, l2 = G.relmax(got, want), G.cosine(got, want), _rel_l2(got, want)
        nr = float(np.linalg.norm(got.astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
        print(f"{k:40s} relmax {r:.3e} relL2 {l2:.3e} norm {nr:.4f} cos {c:.6f}")
        if not (c > 0.995 and r <= 0.25 and l2 <= 0.12 and 0.97 <= nr <= 1.03):
            bad.append(k)
    assert not bad, bad
    # the running statistics: also the element-wise bound test_forward_train_and_eval_vs_golden puts on them
    np.testing.assert_allclose(rec["running"], ref["running"], rtol=2e-2, atol=2e-3)


@pytest.mark.parametrize("b", [3, 8])
def test_grad_step_is_repeatable_and_matches_a_record(b):
    """One gradient step from a fixed state, twice: finite, bitwise repeatable.  When the environment names a directory of
    records (the test below does, for its child process), the step is compared with the record of the same batch size."""
    rec = _grad_step_record(b)
    again = _grad_step_record(b)
    for k, v in rec.items():
        assert np.isfinite(v).all(), k
        assert np.array_equal(v, again[k]), k
    d = os.environ.get(RECORD_ENV)
    if d:
        _compare_with_record(rec, np.load(os.path.join(d, f"b{b}.npz")))


def test_stand_alone_finalize_kernels_in_a_whole_step_match_the_folded_step(tmp_path):
    for b in (3, 8):
        np.savez(os.path.join(str(tmp_path), f"b{b}.npz"), **_grad_step_record(b))
    env = dict(os.environ, EAE_NO_FOLD_FWD="1", EAE_NO_FOLD_BWD="1")
    env[RECORD_ENV] = str(tmp_path)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "matches_a_record",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-2000:]
