"""The fixed-point BatchNorm statistics of the default (folded) train step over their whole range: right, or loud.

Every producer workgroup adds its per-channel sums to the layer's accumulators as 64-bit fixed point (csrc/eae_bn_acc.h: scale 2^24
forward, 2^42 backward); a contribution at or above 2^62 / (workgroups per channel) after scaling sets the channel's flag instead, and
a flagged channel reads NaN.  test_gpu_bn_statistics.py sees this arithmetic at magnitudes of order 1 only.  Here the tensor in front
of ONE BatchNorm layer is scaled (its conv's weight and bias times 2^(j/2), through the model state) so that the channels land in

  (a) the quantum regime: rms about 2^-20 and 2^-12, where a workgroup's sums round to a few quanta or to none,
  (b) comfortably inside: rms about 2^8,
  (c) just under the limit: the largest contribution between 1/32 and 1/2 of it,
  (d) the window in which the commits before eae_bn_acc.h were silently wrong: sum y^2 >= 2^40 over the channel with every single
      contribution below the old per-contribution guard 9.0e18 / 2^24 (the total wrapped modulo 2^64),
  (e) past the limit, and rms 2^62, where the fp32 squares themselves are infinite,

with the exponent taken from the unscaled tensor's own sums.  One training-mode forward runs, the layer's stored tensor is read back
and every channel is held to: EITHER the running statistics are the fp64 moments of the stored tensor, within the bound of
test_gpu_bn_statistics.py widened by the quantum (workgroups * 2^-25 / count on the mean and on E[y^2]), OR the channel's running
statistics are NaN, the step's three losses are NaN and a following train_step leaves every parameter as it was.  Which of the two
is not free: the per-workgroup sums are recomputed in fp64 over the tiles of the plan (conv_ref.expected_geo, the edge kernel's
4 x 32 tiles; the tile COUNT is asserted against what the library reports), and a channel whose contributions are all below half
the limit must be right, one with a contribution above it must be loud.  Every regime must hold a channel of every layer; a layer of
at most two workgroups, whose window (d) is empty, must show that it is.  After the loud step the repaired model's next forward is
bitwise the fresh engine's.

Batch sizes 3 and 33 at 64 x 64: the images-per-tile tails of test_gpu_bn_statistics.py; 33 gives conv4's 4 x 4 map nine workgroups.

The backward accumulators (sum g, sum g * xhat at 2^42) are driven through the stand-alone Encoder / Decoder in train mode:
z.backward(2^k dz) and x_hat.backward(2^k g).  Every floating-point operation of the backward is equivariant under a power of two,
so the reference is ONE run of the bf16 oracle (oracle.ae_numpy.ae_backward, dout given) times 2^k; what remains is the fixed point.
Per channel: dgamma / dbeta within the limits test_gradients_vs_golden_and_oracle puts on them against the oracle (0.25 of the
tensor's largest entry) plus workgroups * 2^-43, OR both are NaN and so is the layer's weight gradient for that channel.  (dgamma of
a flagged channel used to be finite garbage -- the partial integer total -- and reached .grad of a stand-alone module: fixed in
bn_acc_bwd_finish.)  The exponents k are clamped to the range in which the oracle's bf16 tensors neither under- nor overflow, which
test_oracle_backward_is_equivariant_under_the_powers_of_two_used_here checks on the CPU.

The oracle serves as the reference wherever its premise holds: for the layer the backward meets first at every k, and for the layers
behind it while no layer in front of them is near its quantum or loud (dy of a BatchNorm is built from its ROUNDED sums, so there the
gradient that travels on is no longer 2^k times the unscaled one).  Every layer at every k is also held to the fp64 sums over the g
and y the engine stored in that very backward, within workgroups * 2^-43 plus 2^-14 of the sums of magnitudes.  A loud layer hands
NaN gradients on, so the window (d) of a layer behind another is reachable only if an integer k puts it there while the layers in
front are inside their limits: the test looks for that k in the unscaled sums and asserts that a layer it calls shadowed has none.

The last test runs regime (d) in ONE child process with EAE_NO_FOLD_FWD=1 EAE_NO_FOLD_BWD=1: the stand-alone finalize kernels sum
float partials in fp64, have no fixed point and no window, and must be right there.

Observed on an MI355X, worst err / bound per regime over all layers and both batch sizes.  Forward (running mean or variance):
(a) 0.244, (b) 6e-5, (c) 6e-5; (d) and (e) every channel loud; (d) held channels of every layer at both batch sizes (3 to 264
workgroups per channel) except conv4 and deconv1 at batch 3, which run one workgroup per channel and have no window.  Backward
against the stored sums: (a) 0.993 (one workgroup, a rounding of nearly half a quantum), (b) 8e-4, (c) 8e-4; against the oracle:
(a) 0.206, (b) 0.122, (c) 0.122.  The window was populated for enc.encoder.10 (k = 23 at batch 3, 21 at 33) and dec.decoder.8
(k = 19); for every other layer the layer in front of it is past its limit at every k that would reach the window.  With the
library of the commit before, the forward test fails in (d) (finite, wrong variances: err / bound 31 and more) and the backward test
at "a channel past the limit is not loud".  Stand-alone finalize kernels in the window: right everywhere."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_acc_ref as A
import conv_ref as R
import edge_ref as E
import golden_util as gu
from helpers import ae_state_np, load_state_np
from test_gpu_bn_statistics import CH, HW, U, _engine, _read_bf16

pytestmark = pytest.mark.gpu

OLD_GUARD = 9.0e18 / 2.0 ** 24 / (1 + 2.0 ** -6)     # per contribution, on sum y^2 (bf16 storage moves a sum of squares by < 2^-7 of it)
CONV_OF_BN = ("enc.encoder.0", "enc.encoder.3", "enc.encoder.6", "enc.encoder.9", "dec.decoder.1", "dec.decoder.4", "dec.decoder.7")
CHILD_ENV = "EAE_TEST_BN_RANGE_UNFOLDED"
FOLDED = not (os.environ.get("EAE_NO_FOLD_FWD") or os.environ.get("EAE_NO_FOLD_BWD"))


def _lib():
    from eae_amd import _lib as L
    return L.load()


def _tile_ids(l, B, forward=True):
    """[B, hw, hw] workgroup of every position of BN layer l's tensor in the launch that takes its statistics, and their number as
    the library's plan reports it.  Forward: the layer's own conv.  Backward: the backward-data kernel behind it, whose epilogue
    applies the layer's ReLU mask (l = 3: the latent projection, 128 images x one position per workgroup)."""
    hw = HW[l]
    b, h, w = np.meshgrid(np.arange(B), np.arange(hw), np.arange(hw), indexing="ij")
    lib = _lib()
    # (kind, cin of the launch, position grid of the plan, 1: the tensor is the grid / 2: the tensor is twice the grid)
    if forward:
        launch = {0: "edge", 1: (0, 32, 16, 1), 2: (0, 64, 8, 1), 3: (0, 128, 4, 1), 4: (1, 256, 4, 2), 5: (1, 128, 8, 2), 6: (1, 64, 16, 2)}[l]
    else:
        launch = {6: "edge", 5: (0, 32, 16, 1), 4: (0, 64, 8, 1), 3: "fc", 2: (1, 256, 4, 2), 1: (1, 128, 8, 2), 0: (1, 64, 16, 2)}[l]
    if launch == "edge":
        ids = (b * (hw // E.E_TH) + h // E.E_TH) * (hw // E.E_TW) + w // E.E_TW
        n = E.edge_tiles(2 * hw, 2 * hw, B)
    elif launch == "fc":
        ids = (b // 128 * hw + h) * hw + w
        n = -(-B // 128) * hw * hw                      # eae_launch_fc_nt: M tiles x (N / 256)
    else:
        kind, cin, grid, up = launch
        cout = 2 * cin if kind == 0 else cin // 2
        assert grid * up == hw and CH[l] == cout
        tw, th, ni = R.expected_geo(kind, cin, cout, grid, grid, B, R.ig_small_setting())
        ids = (b // ni * (grid // th) + h // up // th) * (grid // tw) + w // up // tw
        n = lib.eae_op_conv_s2_ntiles(kind, cin, B, 2 * grid if kind == 0 else grid, 2 * grid if kind == 0 else grid)
    assert len(np.unique(ids)) == n == ids.max() + 1, (l, B, n)
    return ids.reshape(-1), int(n)


def _tile_sums(values, ids, n):
    """values [positions, C] fp64 -> [n, C] sums per workgroup"""
    out = np.zeros((n, values.shape[1]))
    np.add.at(out, ids, values)
    return out


def _scale_conv(m, eng, sd0, l, factor, run0, nbt0):
    """the original state with the conv in front of BN layer l times `factor`; running statistics and counters as at the start"""
    load_state_np(m, sd0)
    mod = m.get_submodule(CONV_OF_BN[l])
    with torch.no_grad():
        mod.weight.mul_(factor)
        mod.bias.mul_(factor)
    eng.params_changed()
    eng.bn_running.copy_(torch.from_numpy(run0).cuda())
    eng.bn_nbt.copy_(torch.from_numpy(nbt0).cuda())
    torch.cuda.synchronize()


def _forward_and_judge(eng, l, B, xd, yd, run0, ids, n):
    """one training-mode forward; per channel of layer l: the sums of the stored tensor, err / bound of the two running statistics,
    whether they are NaN, and what the channel owes (must be right / must be loud)"""
    out = eng.forward(xd, labels=yd, train=True, alpha=35.0)
    torch.cuda.synchronize()
    c, N = CH[l], B * HW[l] * HW[l]
    t = _read_bf16(eng, 0 if l < 4 else 2, l if l < 4 else l - 4, N * c).reshape(N, c).astype(np.float64)
    with np.errstate(all="ignore"):
        mean, e2, mabs = t.mean(0), (t * t).mean(0), np.abs(t).mean(0)
        unb = (e2 - mean * mean) * (N / (N - 1.0))
        q = n * 2.0 ** -25 / N                                      # half a quantum per workgroup contribution
        d_mean = 2.0 ** -9 * mabs * (1 + 2.0 ** -8) + q
        d_e2 = (2.0 ** -8 + 2.0 ** -18) * e2 * (1 + 2.0 ** -7) + q
        d_unb = (d_e2 + 2 * np.abs(mean) * d_mean + d_mean ** 2) * (N / (N - 1.0))
        run1 = eng.bn_running.cpu().numpy().astype(np.float64)
        sl_m, sl_v = slice(eng.boff[2 * l], eng.boff[2 * l] + c), slice(eng.boff[2 * l + 1], eng.boff[2 * l + 1] + c)
        rm0, rv0, rm1, rv1 = run0[sl_m].astype(np.float64), run0[sl_v].astype(np.float64), run1[sl_m], run1[sl_v]
        tol_m = 0.1 * d_mean + 4 * U * (np.abs(0.9 * rm0) + np.abs(0.1 * mean))
        tol_v = 0.1 * d_unb + 4 * U * (np.abs(0.9 * rv0) + np.abs(0.1 * unb))
        em, ev = np.abs(rm1 - (0.9 * rm0 + 0.1 * mean)) / tol_m, np.abs(rv1 - (0.9 * rv0 + 0.1 * unb)) / tol_v
        m1, m2 = np.abs(_tile_sums(t, ids, n)).max(0), _tile_sums(t * t, ids, n).max(0)
    lim = float(A.value_limit(A.SCALE_FWD, n, 1))
    j = dict(rms=np.sqrt(e2), s2=e2 * N, m2=m2, top=np.maximum(m1, m2), lim=lim,
             loud=np.isnan(rm1) & np.isnan(rv1), right=(em <= 1.0) & (ev <= 1.0), em=em, ev=ev,
             must_right=np.maximum(m1, m2) < lim / 2, must_loud=m2 >= lim * (1 + 2.0 ** -6),
             losses=eng.loss_last.cpu().numpy()[:3].copy(), out=[o.clone() for o in out], run1=eng.bn_running.clone())
    j["window"] = (j["s2"] >= 2.0 ** 40) & (m2 < OLD_GUARD)
    return j


@pytest.mark.skipif(not FOLDED, reason="the stand-alone finalize kernels have no fixed point: the last test holds them to regime (d)")
@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("l", range(7))
def test_forward_statistics_are_right_or_loud_in_every_regime(l, B):
    m, eng, run0, nbt0 = _engine()
    sd0 = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    x, y = gu.make_images(B, 500 + B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ids, n = _tile_ids(l, B)
    assert n > 1 or (l, B) in ((3, 3), (4, 3))       # conv4 and deconv1 at batch 3: one workgroup per channel, 4 x 4 maps
    base = _forward_and_judge(eng, l, B, xd, yd, run0, ids, n)
    assert base["right"].all() and not base["loud"].any() and np.isfinite(base["losses"]).all()
    lim, med = base["lim"], int(np.argsort(base["m2"])[CH[l] // 2])

    def half_steps(target, value):                  # j with value * 2^j ~ target, for a quantity that scales with the SQUARE
        return int(np.round(np.log2(target / value)))      # of the factor 2^(j/2)

    ratio = base["s2"] / base["m2"]                  # how many times its largest contribution a channel's sum y^2 is
    best = int(np.argmax(ratio))
    admits = ratio[best] > 2.0 ** 40 / OLD_GUARD * 2.0 ** 0.2     # (the window is [2^40, ratio * guard): 0.1 bits of room on either side)
    plan = [("a", half_steps(2.0 ** -40, base["rms"][med] ** 2)), ("a", half_steps(2.0 ** -24, base["rms"][med] ** 2)),
            ("b", half_steps(2.0 ** 16, base["rms"][med] ** 2)), ("c", half_steps(lim / 8, base["top"][med])),
            ("e", half_steps(lim * 4, base["m2"][med])), ("e", half_steps(2.0 ** 124, base["rms"][med] ** 2))]
    if admits:
        # (the middle of that channel's window, not rounded to a half step: with three workgroups the window is half a bit wide)
        plan.insert(4, ("d", float(np.log2(np.sqrt(2.0 ** 40 * OLD_GUARD * ratio[best]) / base["s2"][best]))))
    else:
        assert n <= 2, (n, float(ratio[best]))      # no window: at most two workgroups (one of them the tail)
    hit = dict.fromkeys(["a: rms < 2^-17", "a: rms 2^-15..2^-9", "b", "c", "e: past the limit", "e: rms > 2^58"] + ["d"] * bool(admits), 0)
    worst = {}
    for regime, j in plan:
        _scale_conv(m, eng, sd0, l, 2.0 ** (j / 2.0), run0, nbt0)
        r = _forward_and_judge(eng, l, B, xd, yd, run0, ids, n)
        ok = r["right"] | r["loud"]
        e = np.where(r["loud"], 0.0, np.maximum(r["em"], r["ev"]))
        worst[regime] = max(worst.get(regime, 0.0), float(e[ok].max()) if ok.any() else 0.0)
        print(f"layer {l} B {B} n {n} regime {regime} scale 2^{j / 2:.1f}: right {int((r['right'] & ~r['loud']).sum())} loud {int(r['loud'].sum())} "
              f"of {CH[l]}; window {int(r['window'].sum())}; worst err/bound mean {float(np.nanmax(np.where(r['loud'], 0, r['em']))):.3f} "
              f"var {float(np.nanmax(np.where(r['loud'], 0, r['ev']))):.3f}")
        assert ok.all(), (regime, j, np.flatnonzero(~ok)[:8], r["em"][~ok][:8], r["ev"][~ok][:8])
        assert (r["right"] & ~r["loud"])[r["must_right"]].all(), (regime, j, "a channel inside half the limit is not right")
        assert r["loud"][r["must_loud"]].all(), (regime, j, "a channel past the limit is not loud")
        assert not (r["window"] & ~r["loud"]).any()           # (what is in the window is past the limit of its launch)
        if r["loud"].any():
            assert np.isnan(r["losses"]).all(), r["losses"]
        if r["must_right"].all():
            assert np.isfinite(r["losses"]).all(), r["losses"]
        hit["a: rms < 2^-17"] += int((r["must_right"] & (r["rms"] < 2.0 ** -17)).sum())
        hit["a: rms 2^-15..2^-9"] += int((r["must_right"] & (r["rms"] >= 2.0 ** -15) & (r["rms"] < 2.0 ** -9)).sum())
        hit["b"] += int((r["must_right"] & (r["rms"] >= 2.0 ** 6) & (r["rms"] < 2.0 ** 10)).sum())
        hit["c"] += int((r["must_right"] & (r["top"] >= lim / 32)).sum())
        hit["e: past the limit"] += int((r["must_loud"] & (r["rms"] < 2.0 ** 58)).sum())
        hit["e: rms > 2^58"] += int((r["must_loud"] & (r["rms"] > 2.0 ** 58)).sum())
        if admits:
            hit["d"] += int(r["window"].sum())
    print(f"layer {l} B {B}: channels per regime {hit}; worst err/bound per regime {worst}")
    assert all(hit.values()), hit
    # the last step was loud: a train step on that state changes no parameter ...
    assert r["loud"].any()
    before = eng.params.clone()
    eng.train_step(xd, yd, 35.0, 1e-3)
    torch.cuda.synchronize()
    assert np.isnan(eng.loss_last.cpu().numpy()[:3]).all()
    assert bool(((eng.params == before) | (torch.isnan(eng.params) & torch.isnan(before))).all())
    # ... and the repaired model's next forward is bitwise the fresh engine's
    _scale_conv(m, eng, sd0, l, 1.0, run0, nbt0)
    again = _forward_and_judge(eng, l, B, xd, yd, run0, ids, n)
    assert all(torch.equal(a, b) for a, b in zip(again["out"], base["out"])) and torch.equal(again["run1"], base["run1"])
    assert np.array_equal(again["losses"], base["losses"])


# ---------------------------------------------------------------------------------------------------- backward
K_RANGE = (-60, 60)                                  # exponents of the scale on dout the oracle is checked at, on the CPU, below
OLD_GUARD_B = 9.0e18 / 2.0 ** 42 / 1.01              # per contribution, on |sum g| and |sum g * xhat|
BN_NAMES = ("enc.encoder.1", "enc.encoder.4", "enc.encoder.7", "enc.encoder.10", "dec.decoder.2", "dec.decoder.5", "dec.decoder.8")
_ORACLE = {}


def _oracle(B):
    """inputs and ONE bf16-oracle backward per half at batch B: (x, z, dz, g, encoder gradients for dout = dz, decoder's for g)"""
    if B not in _ORACLE:
        from oracle import ae_numpy as O
        p = ae_state_np()
        x, _ = gu.make_images(B, 900 + B)
        out = O.ae_forward(p, x, train=True, quant="bf16", head=False)
        rng = np.random.default_rng(7)
        dz = rng.standard_normal((B, 64)).astype(np.float32)
        g = rng.standard_normal(x.shape).astype(np.float32)
        ge = O.ae_backward(p, out, x, None, 1.0, quant="bf16", head=False, dout=(np.zeros_like(x), None, dz))
        gd = O.ae_backward(p, out, x, None, 1.0, quant="bf16", head=False, dout=(g, None, None))
        _ORACLE[B] = dict(p=p, out=out, x=x, z=out["z"].astype(np.float32), dz=dz, g=g, enc=ge, dec=gd)
    return _ORACLE[B]


def _half(half, B):
    import eae_amd
    from eae_amd.engine import engine_for
    sd = ae_state_np()
    mod = eae_amd.Encoder(latent_dim=64) if half == "enc" else eae_amd.Decoder(latent_dim=64)
    load_state_np(mod, {k[4:]: v for k, v in sd.items() if k.startswith(half + ".")})
    mod = mod.cuda().train()
    return mod, engine_for(mod)


def _backward(mod, half, o, k):
    """forward + backward with dout * 2^k -> {parameter name: gradient}"""
    for p in mod.parameters():
        p.grad = None
    inp = torch.from_numpy(o["x"] if half == "enc" else o["z"]).cuda()
    dout = torch.from_numpy((o["dz"] if half == "enc" else o["g"]) * np.float32(2.0 ** k)).cuda()
    mod(inp).backward(dout)
    torch.cuda.synchronize()
    return {half + "." + n: p.grad.cpu().numpy().astype(np.float64) for n, p in mod.named_parameters()}


def _backward_sums(eng, l, B, strict=True):
    """per-workgroup sums of BN layer l's backward, in fp64 from the g and y the engine stored in the backward that just ran:
    [n, C] sum g, sum g * xhat, n, and the channel totals of |g| and |g * xhat|"""
    c, N = CH[l], B * HW[l] * HW[l]
    enc = l < 4
    y = _read_bf16(eng, 0 if enc else 2, l if enc else l - 4, N * c).reshape(N, c).astype(np.float64)
    g = _read_bf16(eng, 1 if enc else 3, l if enc else l - 4, N * c).reshape(N, c).astype(np.float64)
    if strict:
        assert np.isfinite(g).all() and np.abs(g).max() > 0
    xhat = (y - y.mean(0)) / np.sqrt(y.var(0) + 1e-5)
    ids, n = _tile_ids(l, B, forward=False)
    with np.errstate(all="ignore"):
        return _tile_sums(g, ids, n), _tile_sums(g * xhat, ids, n), n, np.abs(g).sum(0) + np.abs(g * xhat).sum(0)


@pytest.mark.skipif(not FOLDED, reason="the stand-alone finalize kernels have no fixed point: the last test holds them to regime (d)")
@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("half", ["enc", "dec"])
def test_backward_sums_are_right_or_loud_in_every_regime(half, B):
    """Two references.  (1) The oracle times 2^k under the limits named above, wherever its premise holds: always for the layer the
    backward meets first, and for a later layer while no layer before it is within 2^12 quanta of its own quantum -- dy of a
    BatchNorm is built from ITS rounded sums (B = -A invstd dgamma / count), so near the quantum the gradient that reaches the
    layers behind is no longer 2^k times the unscaled one, and the oracle times 2^k is not what they should give.  (2) For every
    layer at every k, the fp64 sums over the g and y the engine stored in that very backward: dbeta = sum g, dgamma = sum g * xhat
    within workgroups * 2^-43 plus 2^-14 of sum |g| + sum |g * xhat| (fp32 summation inside a workgroup, xhat from the engine's
    fp32 coefficients) -- far tighter than (1), and valid whatever arrived from the layers before."""
    o = _oracle(B)
    mod, eng = _half(half, B)
    layers = [3, 2, 1, 0] if half == "enc" else [6, 5, 4]            # in the order the backward meets them
    ref = o[half]
    base = _backward(mod, half, o, 0)
    info = {}
    for l in layers:
        s1, s2, n, _ = _backward_sums(eng, l, B)
        info[l] = dict(n=n, lim=float(A.value_limit(A.SCALE_BWD, n, 1)), top=np.maximum(np.abs(s1).max(0), np.abs(s2).max(0)),
                       tot=np.stack([np.abs(s1.sum(0)), np.abs(s2.sum(0))]), tops=np.stack([np.abs(s1).max(0), np.abs(s2).max(0)]))

    def window_at(tot, tops):                           # the parent wrapped the total while every contribution passed its guard
        return ((tot >= 2.0 ** 21 * 1.01) & (tops < OLD_GUARD_B)).any(0)

    def clamp(k):
        return int(min(max(k, K_RANGE[0]), K_RANGE[1]))

    ks, window_k, shadowed = set(), {}, []
    for pos, l in enumerate(layers):
        i = info[l]
        med = float(np.median(i["top"]))
        for target in (2.0 ** -44, 2.0 ** -36, 1.0, i["lim"] / 8, i["lim"] * 4, 2.0 ** 50):
            ks.add(clamp(np.round(np.log2(target / med))))
        # an integer k that puts channels of this layer into the window while every layer BEFORE it is still inside its limit (a loud
        # layer hands NaN gradients on: what lies behind it is loud whatever its own sums would have been)
        counts = {k: int(window_at(i["tot"] * 2.0 ** k, i["tops"] * 2.0 ** k).sum()) for k in range(K_RANGE[0], K_RANGE[1] + 1)}
        clear = {k: c for k, c in counts.items() if all((info[u]["top"] * 2.0 ** k < info[u]["lim"] * 0.75).all() for u in layers[:pos])}
        if clear and max(clear.values()):
            window_k[l] = max(clear, key=clear.get)
            ks.add(window_k[l])
        elif max(counts.values()):
            shadowed.append(l)
    hit = {l: dict.fromkeys(["a: below the quantum", "a: a few quanta", "b", "c", "d", "e", "oracle"], 0) for l in layers}
    worst = {"sums": {}, "oracle": {}}
    for k in sorted(ks):
        got = _backward(mod, half, o, k)
        s = 2.0 ** k
        premise = True                                  # of reference (1): no layer before this one is near its quantum, or loud
        for l in layers:
            i, h, name = info[l], hit[l], BN_NAMES[l]
            s1, s2, n, mag = _backward_sums(eng, l, B, strict=False)
            assert n == i["n"]
            dg, db = got[name + ".weight"], got[name + ".bias"]
            wname = CONV_OF_BN[l] + ".weight"
            wgrad = got[wname] if l < 4 else np.moveaxis(got[wname], 1, 0)          # [channel of this BatchNorm, ...]
            loud = np.isnan(dg) & np.isnan(db) & ~np.isfinite(wgrad.reshape(CH[l], -1)).all(1)
            assert not (np.isnan(dg) ^ np.isnan(db)).any(), (l, k, "dgamma and dbeta of a flagged channel are both NaN")
            with np.errstate(all="ignore"):
                finite = np.isfinite(s1).all(0) & np.isfinite(s2).all(0)
                tops = np.stack([np.abs(s1).max(0), np.abs(s2).max(0)])
                top = tops.max(0)
                tol = n * 2.0 ** -43 + 2.0 ** -14 * mag
                err = np.maximum(np.abs(db - s1.sum(0)), np.abs(dg - s2.sum(0))) / tol
                right = finite & (err <= 1.0)
                must_right = finite & (top < i["lim"] / 2)
                must_loud = ~finite | (top >= i["lim"] * 1.25)
                window = finite & window_at(np.stack([np.abs(s1.sum(0)), np.abs(s2.sum(0))]), tops)
            assert (right | loud).all(), (l, k, np.flatnonzero(~(right | loud))[:8], err[~(right | loud)][:8])
            assert right[must_right].all() and not loud[must_right].any(), (l, k, "a channel inside half the limit is not right")
            assert loud[must_loud].all(), (l, k, "a channel past the limit, or with a non-finite gradient, is not loud")
            assert loud[window].all(), (l, k)
            e = float(err[right & ~loud].max()) if (right & ~loud).any() else 0.0
            regime = "a" if (top[finite] < 2.0 ** -32).all() else "c" if (top[finite] >= i["lim"] / 32).any() else "b"
            worst["sums"][regime] = max(worst["sums"].get(regime, 0.0), e)
            h["a: below the quantum"] += int((must_right & (top < 2.0 ** -43)).sum())
            h["a: a few quanta"] += int((must_right & (top >= 2.0 ** -42) & (top < 2.0 ** -32)).sum())
            h["b"] += int((must_right & (top >= 2.0 ** -4) & (top < 2.0 ** 4)).sum())
            h["c"] += int((must_right & (top >= i["lim"] / 32)).sum())
            h["d"] += int(window.sum())
            h["e"] += int((loud & must_loud).sum())
            eo = float("nan")
            if premise and not loud.any():
                rg, rb = ref[name + ".weight"].astype(np.float64) * s, ref[name + ".bias"].astype(np.float64) * s
                eg = np.abs(dg - rg) / (0.25 * np.abs(rg).max() + n * 2.0 ** -43)
                eb = np.abs(db - rb) / (0.25 * np.abs(rb).max() + n * 2.0 ** -43)
                eo = float(np.maximum(eg, eb).max())
                assert eo <= 1.0, (l, k, "against the oracle", eo)
                worst["oracle"][regime] = max(worst["oracle"].get(regime, 0.0), eo)
                h["oracle"] += 1
            print(f"{half} B {B} k {k} layer {l} n {n}: right {int((right & ~loud).sum())} loud {int(loud.sum())} of {CH[l]}; window "
                  f"{int(window.sum())}; worst err/bound vs the stored sums {e:.3f}, vs the oracle {eo:.3f}")
            premise = premise and not loud.any() and n * 2.0 ** -43 <= 2.0 ** -12 * float(np.median(top))
    print(f"{half} B {B}: channels per regime {hit}; worst err/bound {worst}; window exponents {window_k}; window shadowed {shadowed}")
    for l in layers:
        h = hit[l]
        assert h["a: below the quantum"] and h["a: a few quanta"] and h["b"] and h["e"] and h["oracle"], (l, h)
        # every layer with more than two workgroups has channels and an integer k in the parent's window, and was seen there -- or
        # a layer before it is past its own limit at every such k
        assert (h["d"] if l in window_k else l in shadowed or info[l]["n"] <= 2), (l, h, window_k, shadowed)
    assert layers[0] in window_k and hit[layers[0]]["c"]
    # the layer the backward meets first is held to the oracle at every k at which it is not loud
    assert hit[layers[0]]["oracle"] >= 4


# ---------------------------------------------------------------------------------------------------- the two paths side by side
def test_regime_d_is_loud_folded_and_right_with_the_stand_alone_finalize_kernels():
    """Regime (d) of conv2 forward (batch 3: six workgroups) and of the encoder's backward (the latent projection's sixteen), in
    whichever path this process runs: the folded finalize must be loud for every channel in the window, the stand-alone finalize
    kernels (EAE_NO_FOLD_FWD=1 EAE_NO_FOLD_BWD=1: float partials, fp64 sums, no fixed point) must be right for every channel."""
    l, B = 1, 3
    m, eng, run0, nbt0 = _engine()
    sd0 = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}
    x, y = gu.make_images(B, 500 + B)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    ids, n = _tile_ids(l, B)
    base = _forward_and_judge(eng, l, B, xd, yd, run0, ids, n)
    ratio = base["s2"] / base["m2"]
    best = int(np.argmax(ratio))
    assert n == 6 and ratio[best] > 2.0 ** 40 / OLD_GUARD * 2.0 ** 0.2
    _scale_conv(m, eng, sd0, l, float(np.sqrt(np.sqrt(2.0 ** 40 * OLD_GUARD * ratio[best]) / base["s2"][best])), run0, nbt0)
    r = _forward_and_judge(eng, l, B, xd, yd, run0, ids, n)
    assert r["window"].any()
    print(f"forward, folded {FOLDED}: window {int(r['window'].sum())} right {int(r['right'].sum())} loud {int(r['loud'].sum())} of {CH[l]}; "
          f"worst err/bound mean {float(np.nan_to_num(r['em']).max()):.3f} var {float(np.nan_to_num(r['ev']).max()):.3f}")
    if FOLDED:
        assert r["loud"][r["window"]].all() and np.isnan(r["losses"]).all()
    else:
        assert r["right"].all() and not r["loud"].any() and np.isfinite(r["losses"]).all()
    # backward: the exponent that puts most channels of the first layer the backward meets into the window
    o = _oracle(B)
    mod, henc = _half("enc", B)
    _backward(mod, "enc", o, 0)
    s1, s2, nb, _ = _backward_sums(henc, 3, B)
    tot, tops = np.stack([np.abs(s1.sum(0)), np.abs(s2.sum(0))]), np.stack([np.abs(s1).max(0), np.abs(s2).max(0)])
    counts = {k: int(((tot * 2.0 ** k >= 2.0 ** 21 * 1.01) & (tops * 2.0 ** k < OLD_GUARD_B)).any(0).sum()) for k in range(0, K_RANGE[1] + 1)}
    k = max(counts, key=counts.get)
    assert nb == 16 and counts[k] > 0
    window = ((tot * 2.0 ** k >= 2.0 ** 21 * 1.01) & (tops * 2.0 ** k < OLD_GUARD_B)).any(0)
    got = _backward(mod, "enc", o, k)
    for lb in (3, 2, 1, 0):
        name = BN_NAMES[lb]
        for kind in (".weight", ".bias"):
            ref = o["enc"][name + kind].astype(np.float64) * 2.0 ** k
            err = np.abs(got[name + kind] - ref) / (0.25 * np.abs(ref).max())
            if FOLDED and lb == 3:
                assert np.isnan(got[name + kind][window]).all()
            elif not FOLDED:
                assert (err <= 1.0).all(), (lb, kind, float(np.nanmax(err)))
        print(f"backward, folded {FOLDED}, k {k}, layer {lb}: window {int(window.sum()) if lb == 3 else '-'}; "
              f"dbeta worst err/bound {float(np.nan_to_num(np.abs(got[name + '.bias'] - o['enc'][name + '.bias'] * 2.0 ** k)).max() / (0.25 * np.abs(o['enc'][name + '.bias']).max() * 2.0 ** k)):.3f}")


@pytest.mark.skipif(not FOLDED or bool(os.environ.get(CHILD_ENV)), reason="this is the child process of the test")
def test_stand_alone_finalize_kernels_are_right_in_the_window():
    env = dict(os.environ, EAE_NO_FOLD_FWD="1", EAE_NO_FOLD_BWD="1")
    env[CHILD_ENV] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "regime_d_is_loud_folded_and_right",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "1 passed" in r.stdout and "folded False" in r.stdout, r.stdout[-2000:]
