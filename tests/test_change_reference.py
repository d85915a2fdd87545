"""Change detection without a device: the chi-square closed forms against scipy, the host solve (`mad_from_moments`) against the
NumPy restatement (tests/change_ref.py), the algorithm itself (reference IR-MAD + median calibration on the planted-change scenes),
`report.transition_table`, and every host-side argument error of eae_amd.change."""
import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import change as CH
import change_ref as R


# ---------------------------------------------------------------------------------------------------- chi-square survival function
@pytest.mark.parametrize("dof", range(1, 17))
def test_chi2_sf_matches_scipy(dof):
    from scipy.special import chdtrc
    z = np.concatenate([np.linspace(0.0, 200.0, 4001), [1e-12, 1e-6, 0.5, 255.9]])
    want = chdtrc(dof, z)
    assert np.abs(R.chi2_sf(dof, z) - want).max() <= 5e-15
    assert max(abs(CH.chi2_sf(dof, float(v)) - w) for v, w in zip(z[::40], want[::40])) <= 5e-15
    assert R.chi2_sf(dof, 0.0) == 1.0 and CH.chi2_sf(dof, 0.0) == 1.0
    for p in (0.5, 0.01):
        assert abs(chdtrc(dof, CH.chi2_isf(dof, p)) - p) <= 1e-12 and abs(CH.chi2_isf(dof, p) - R.chi2_isf(dof, p)) <= 1e-9


# ---------------------------------------------------------------------------------------------------- the solve
def _population(c, rho, seed):
    """Mean and covariance of [x G_x + o_x, y G_y + o_y] for unit-variance pairs (x_i, y_i) correlated by rho_i: the canonical
    correlations are rho exactly."""
    rng = np.random.default_rng(seed)
    gx, gy = np.eye(c) + 0.4 * rng.standard_normal((c, c)), np.eye(c) + 0.4 * rng.standard_normal((c, c))
    cov = np.block([[gx.T @ gx, gx.T @ np.diag(rho) @ gy], [gy.T @ np.diag(rho) @ gx, gy.T @ gy]])
    return rng.standard_normal(2 * c) * 10, cov


@pytest.mark.parametrize("c,seed", [(1, 0), (2, 1), (4, 2), (7, 3), (16, 4)])
def test_mad_from_moments_recovers_known_correlations(c, seed):
    rho = np.sort(np.random.default_rng(seed).uniform(0.05, 0.98, c))[::-1]
    mean, cov = _population(c, rho, seed)
    m = CH.mad_from_moments(CH.JointMoments(1.0, mean, cov, 1))
    assert np.abs(m.rho - rho).max() <= 1e-10 and (np.diff(m.rho) <= 0).all()
    r_rho, r_a, r_b, r_sigma = R.mad_ref(mean, cov)
    assert np.abs(m.rho - r_rho).max() <= 1e-10 and np.abs(m.sigma - r_sigma).max() <= 1e-8
    scale = max(np.abs(r_a).max(), np.abs(r_b).max())
    assert np.abs(m.a - r_a).max() <= 1e-6 * scale and np.abs(m.b - r_b).max() <= 1e-6 * scale
    # unit variance of both sides, correlation rho, mean passed through
    assert np.abs(m.a.T @ cov[:c, :c] @ m.a - np.eye(c)).max() <= 1e-9
    assert np.abs(m.b.T @ cov[c:, c:] @ m.b - np.eye(c)).max() <= 1e-9
    assert np.abs(m.a.T @ cov[:c, c:] @ m.b - np.diag(rho)).max() <= 1e-9
    assert np.array_equal(m.mean_a, mean[:c]) and np.array_equal(m.mean_b, mean[c:])
    assert m.iterations == 0 and m.history == ()


def _sample(c, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, c)) @ (np.eye(c) + 0.3 * rng.standard_normal((c, c)))
    y = x @ (np.eye(c) + 0.3 * rng.standard_normal((c, c))) + 0.5 * rng.standard_normal((n, c))
    return x, y


def _moments_of(x, y):
    v = np.concatenate([x, y], 1)
    mean = v.mean(0)
    return CH.JointMoments(float(len(v)), mean, (v - mean).T @ (v - mean) / len(v), len(v))


def _chi2(x, y, m):
    mean, t = CH.variate_matrix(m)
    return (((np.concatenate([x, y], 1) - mean) @ t) ** 2).sum(1)


def test_chi2_is_invariant_to_affine_changes_of_either_scene():
    c = 4
    x, y = _sample(c, 3000, 5)
    rng = np.random.default_rng(6)
    g, o = np.eye(c) + 0.5 * rng.standard_normal((c, c)), 100 * rng.standard_normal(c)
    base = _chi2(x, y, CH.mad_from_moments(_moments_of(x, y)))
    for x2, y2 in ((x, y @ g + o), (x @ g + o, y), (3.0 * x - 7.0, y @ g)):
        m2 = CH.mad_from_moments(_moments_of(x2, y2))
        assert np.abs(_chi2(x2, y2, m2) - base).max() <= 1e-8 * base.max()
    assert abs(base.mean() - c) <= 1e-9 * c                              # unit-variance variates: the mean of chi2 is C


def test_sign_rule():
    c = 5
    x, y = _sample(c, 2000, 7)
    for xs, ys in ((x, y), (-x, -y), (x[:, ::-1], y)):
        mom = _moments_of(xs, ys)
        m = CH.mad_from_moments(mom)
        t = mom.cov[:c, :c] @ m.a
        assert (t[np.abs(t).argmax(0), np.arange(c)] > 0).all()
        assert (np.diag(m.a.T @ mom.cov[:c, c:] @ m.b) > 0).all()        # a pair is negated together: rho stays positive
    # the rule fixes a by Sxx alone: negating scene b leaves a as it is and negates b
    m1, m2 = CH.mad_from_moments(_moments_of(x, y)), CH.mad_from_moments(_moments_of(x, -y))
    assert np.abs(m1.a - m2.a).max() <= 1e-9 * np.abs(m1.a).max() and np.abs(m1.b + m2.b).max() <= 1e-9 * np.abs(m1.b).max()


def test_collinear_and_constant_bands_raise():
    x, y = _sample(3, 500, 8)
    for bad in (np.concatenate([x, x[:, :1] + x[:, 1:2]], 1), np.concatenate([x, np.full((500, 1), 3.0)], 1)):
        mom = _moments_of(bad, np.concatenate([y, y[:, :1] ** 2], 1))
        with pytest.raises(RuntimeError, match=r"constant or collinear bands.*reg"):
            CH.mad_from_moments(mom)
        assert np.isfinite(CH.mad_from_moments(mom, reg=1e-3).rho).all()          # the shrinkage the message names repairs it
    with pytest.raises(RuntimeError, match="not finite"):
        CH.mad_from_moments(CH.JointMoments(0.0, np.full(4, np.nan), np.full((4, 4), np.nan), 0))
    with pytest.raises(RuntimeError, match="reg must be"):
        CH.mad_from_moments(_moments_of(x, y), reg=-0.1)
    with pytest.raises(RuntimeError, match="mean \\[2C\\]"):
        CH.mad_from_moments(CH.JointMoments(1.0, np.zeros(3), np.eye(3), 1))


# ---------------------------------------------------------------------------------------------------- the algorithm on planted change
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["uint8", "uint16"])
@pytest.mark.parametrize("seed", range(5))
def test_reference_irmad_finds_the_planted_block(seed, dtype):
    """10 iterations, alpha = 0.01, median calibration: recall on the block >= 0.99, false alarms outside <= 0.02.  Uncalibrated, the
    raw prob < 0.01 flags a third of the unchanged pixels (0.33 - 0.42 on these ten scenes): the reason the calibration exists."""
    a, b, changed = R.planted(seed, dtype)
    history, chi2, prob, _ = R.irmad_ref(a, b, 10)
    changed = changed.reshape(-1)
    _, change = R.median_calibration(chi2, np.ones(changed.shape, dtype=bool), 4, 0.01)
    assert change[changed].mean() >= 0.99
    assert change[~changed].mean() <= 0.02
    assert (prob < 0.01)[~changed].mean() > 0.2
    assert len(history) == 10 and all((np.diff(h) <= 0).all() for h in history)


def test_planted_scene_is_what_the_issue_describes():
    for dtype, lo, top in ((np.uint16, 500, 3500), (np.uint8, 20, 220)):
        a, b, changed = R.planted(0, dtype)
        assert a.dtype == dtype and b.dtype == dtype and a.shape == b.shape == (4, 96, 96)
        assert a.min() == lo and a.max() == top and changed.sum() == 24 * 24 and changed[30:54, 40:64].all()
        a2, b2, _ = R.planted(0, dtype)
        assert np.array_equal(a, a2) and np.array_equal(b, b2)


# ---------------------------------------------------------------------------------------------------- transition table
def test_transition_table_text():
    t = np.array([[5, 2, 0, 1], [0, 7, 3, 0], [4, 0, 0, 0], [1, 0, 2, 9]])
    text = eae_amd.transition_table(torch.from_numpy(t), class_names=["water", "forest", "urban"])
    lines = text.splitlines()
    assert lines[0].split() == ["class", "date", "A", "date", "B", "kept", "lost", "to", "gained", "from"]
    assert lines[2].split() == ["water", "8", "10", "5", "forest", "2", "urban", "4"]
    assert lines[3].split() == ["forest", "10", "9", "7", "urban", "3", "water", "2"]
    assert lines[4].split() == ["urban", "4", "5", "0", "water", "4", "forest", "3"]
    assert len(lines) == 5
    assert eae_amd.transition_table(np.diag([3, 4, 0])).splitlines()[2].split() == ["0", "3", "3", "3", "-", "-", "-", "-"]
    with pytest.raises(ValueError):
        eae_amd.transition_table(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        eae_amd.transition_table(t, class_names=["a"])


# ---------------------------------------------------------------------------------------------------- host-side argument errors
def _pair(c=3, h=8, w=9, dtype=torch.uint8):
    return torch.zeros((c, h, w), dtype=dtype), torch.ones((c, h, w), dtype=dtype)


_MODEL = CH.MadModel(np.ones(3), np.eye(3), np.eye(3), np.zeros(3), np.zeros(3), np.ones(3), 1, ())


def _calls(a, b, **kw):
    """Every public function that takes the scene pair, as thunks."""
    prob = torch.zeros((8, 9), dtype=torch.float32)
    return [lambda: CH.joint_moments(a, b, **kw), lambda: CH.mad_fit(a, b, **kw), lambda: CH.mad_transform(a, b, _MODEL, **kw),
            lambda: CH.detect_change(a, b, **kw), lambda: CH.invariant_regression(a, b, prob, **kw)]


def _all_raise(match, a, b, **kw):
    for call in _calls(a, b, **kw):
        with pytest.raises(RuntimeError, match=match):
            call()


def test_scene_pair_errors():
    a, b = _pair()
    _all_raise("planar tensor", a[0], b)
    _all_raise("planar tensor", a, None)
    _all_raise("dtype must be uint8, uint16 or float32", a.to(torch.int32), b)
    _all_raise("must have one shape", a, b[:, :, :-1])
    _all_raise("scene a is on cpu, scene b on meta", a, b.to("meta"))
    _all_raise("bands must be in 1..16", *_pair(c=17))
    _all_raise("scene is empty", *_pair(h=0))
    _all_raise("divisor_a must have one value per band \\(3\\), got 2", a, b, divisor_a=[1.0, 2.0])
    _all_raise("divisor_b must have one value per band \\(3\\), got 4", a, b, divisor_b=torch.ones(4))
    _all_raise("mask must be a \\[H, W\\]", a, b, mask=torch.zeros((8, 8), dtype=torch.bool))
    _all_raise("mask dtype", a, b, mask=torch.zeros((8, 9), dtype=torch.float32))
    _all_raise("nodata of a uint8 scene must be an integer in 0..255", a, b, nodata_a=256)
    _all_raise("nodata of a uint8 scene", a, b, nodata_b=1.5)
    _all_raise("rule must be 'all' or 'any'", a, b, rule_a="some")
    _all_raise("rule must be 'all' or 'any'", a, b, rule_b=None)
    # valid arguments on the CPU get as far as the device check: there is no CPU path
    _all_raise("HIP device only", a, b, divisor_a=255.0, divisor_b=[1.0, 2.0, 3.0], nodata_a=0, mask=torch.zeros((8, 9), dtype=torch.bool))
    _all_raise("HIP device only", a.to(torch.float32), b.to(torch.uint16), nodata_a=float("nan"), nodata_b=65535, rule_b="any")


def test_weights_errors():
    a, b = _pair()
    for fn in (lambda w: CH.joint_moments(a, b, weights=w), lambda w: CH.invariant_regression(a, b, w)):
        for bad, match in ((torch.zeros((9, 8)), "must be a \\[H, W\\] = \\[8, 9\\]"), (torch.zeros((1, 8, 9)), "must be a \\[H, W\\]"),
                           (np.zeros((8, 9), dtype=np.float32), "must be a \\[H, W\\]"),
                           (torch.zeros((8, 9), dtype=torch.float64), "dtype must be float32"),
                           (torch.zeros((8, 9), device="meta"), "on meta, the scenes on cpu")):
            with pytest.raises(RuntimeError, match=match):
                fn(bad)
    with pytest.raises(RuntimeError, match="must be a \\[H, W\\]"):
        CH.invariant_regression(a, b, None)


def test_scalar_argument_errors():
    a, b = _pair()
    with pytest.raises(RuntimeError, match="pivot must hold 2C = 6 finite numbers"):
        CH.joint_moments(a, b, pivot=np.zeros(5))
    with pytest.raises(RuntimeError, match="pivot must hold"):
        CH.joint_moments(a, b, pivot=[0, 0, 0, 0, 0, float("nan")])
    for fn in (CH.mad_fit, CH.detect_change):
        for kw, match in ((dict(max_iter=0), "max_iter must be an integer"), (dict(max_iter=2.5), "max_iter must be an integer"),
                          (dict(tol=-1e-3), "tol must be a number >= 0"), (dict(tol="x"), "tol must be"),
                          (dict(reg=1.5), "reg must be a number in \\[0, 1\\]"), (dict(reg=True), "reg must be")):
            with pytest.raises(RuntimeError, match=match):
                fn(a, b, **kw)
    for kw, match in ((dict(alpha=0.0), "alpha must be a number in \\(0, 1\\)"), (dict(alpha=1.0), "alpha must be"),
                      (dict(calibrate=1), "calibrate must be True or False")):
        with pytest.raises(RuntimeError, match=match):
            CH.detect_change(a, b, **kw)
    prob = torch.zeros((8, 9))
    for t in (1.0, -0.1, "high"):
        with pytest.raises(RuntimeError, match="threshold must be a number in \\[0, 1\\)"):
            CH.invariant_regression(a, b, prob, threshold=t)
    with pytest.raises(RuntimeError, match="model must be a MadModel"):
        CH.mad_transform(a, b, (np.ones(3),))
    with pytest.raises(RuntimeError, match="fitted to 3 bands, the scenes have 4"):
        CH.mad_transform(*_pair(c=4), _MODEL)
    with pytest.raises(RuntimeError, match="variates must be True or False"):
        CH.mad_transform(a, b, _MODEL, variates=1)


def test_class_transitions_errors():
    m = torch.zeros((4, 5), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="must have one shape"):
        CH.class_transitions(m, m[:, :-1], 3)
    with pytest.raises(RuntimeError, match="num_classes must be in 1..64"):
        CH.class_transitions(m, m, 0)
    with pytest.raises(RuntimeError, match="2-D int64 map"):
        CH.class_transitions(m, m.to(torch.int32), 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        CH.class_transitions(m.to(torch.int32), m, 3)
