"""The fixed-point arithmetic of the folded BatchNorm finalize (csrc/eae_bn_acc.h) against its exact restatement, without a GPU.

bn_acc_check.cpp includes only that header.  Built with -Wall -Werror under the address and undefined-behaviour sanitisers (and
-ffp-contract=off: one rounding per operation, like the restatement), it sweeps contributions of magnitude 2^-60 .. 2^70 with 23
random mantissa bits, all positive, all negative and mixed, over launches of 1, 2, 3, 16, 1000, 4096 and 2^15 workgroups per
channel on 1, 2 and 8 SyncBN replicas, at both scales (2^24 forward, 2^42 backward), and prints the two accumulator words, the flag
and the finished values (s, t, mean, invstd, running mean / variance; A, B, C, dgamma, dbeta).  Every line must be bit for bit what
tests/bn_acc_ref.py gives with Python integers and NumPy scalars.

The property the range rests on -- contributions that all pass the limit of their launch cannot take the signed total out of
(-2^63, 2^63) -- is asserted here on the restatement for every launch size, and by the program on every case; the rule of the
commits before (one constant, 9.0e18, whatever the launch) is shown to fail it at two contributions, on the restatement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bn_acc_ref as R
import eae_amd

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(eae_amd.__file__), "csrc")
COUNTS = (1, 2, 3, 16, 1000, 4096, 32768)
WORLDS = (1, 2, 8)
EXPONENTS = range(-60, 71)
F32 = np.float32


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """the program's output: the case lines and the worst-case lines; built and run once"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("bn_acc") / "bn_acc_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "bn_acc_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].endswith(" cases, 0 violations") and "VIOLATION" not in r.stdout, lines[-1]
    out = {"case": [l for l in lines[:-1] if not l.startswith("worst ")], "worst": [l[6:] for l in lines[:-1] if l.startswith("worst ")]}
    assert int(lines[-1].split()[0]) > len(out["case"]) + len(out["worst"])       # + the launch sizes that are not printed
    return out


def _hash(seed, n):
    i = np.arange(n, dtype=np.uint32)
    h = (i * np.uint32(2654435761)) ^ np.uint32((seed * 40503 + 0x9e3779b9) & 0xffffffff)
    h ^= h >> np.uint32(15)
    h *= np.uint32(2246822519)
    h ^= h >> np.uint32(13)
    return h


def _mantissas(g, ni, wi, which):
    """the program's contributions of accumulator `which` before the power of two: float32 in +-[1, 2)"""
    h = _hash(((g * 7 + ni) * 3 + wi) * 2 + which, COUNTS[ni] * WORLDS[wi])
    m = F32(1.0) + (h >> np.uint32(9)).astype(F32) * F32(2.0 ** -23)
    neg = np.full(h.shape, g == 1) | ((g == 2) & (((h >> np.uint32(8)) & np.uint32(1)) == 1))
    return np.where(neg, -m, m).astype(F32)


def test_sweep_is_the_restatement_bit_for_bit(sweep):
    mant, bad, seen = {}, [], set()
    hit = dict.fromkeys(["inside", "flagged", "some pass and some do not", "variance clamped", "rounds to zero", "half a quantum"], 0)
    for line in sweep["case"]:
        args, _, res = line.partition(" : ")
        s, e, g, n, w = map(int, args.split())
        ni, wi = COUNTS.index(n), WORLDS.index(w)
        scale = R.SCALE_BWD if s else R.SCALE_FWD
        lim = R.limit(n, w)
        words, flag, passed = [], False, 0
        for which in (0, 1):
            key = (g, ni, wi, which)
            if key not in mant:
                mant[key] = _mantissas(*key)
            v = np.ldexp(mant[key], e).astype(F32)
            word, fl = R.accumulate(v, scale, lim)
            words.append(word)
            flag |= fl
            passed += int((np.abs(v * scale) < lim).sum())
        count = n * w * 128
        want = [f"{R.bits(lim):08x}", str(words[0]), str(words[1]), str(int(flag))]
        if s == 0:
            o = R.fwd_finish(words[0], words[1], flag, scale, count, 1e-5, 1.25, -0.5)
            rm, rv = R.running(o, count, 0.1, 0.25, 1.5)
            want += [f"{R.bits(x):08x}" for x in (o["s"], o["t"], o["mean"], o["invstd"], rm, rv)]
            hit["variance clamped"] += (not flag) and o["var"] == 0.0 and words[1] != 0
        else:
            o = R.bwd_finish(words[0], words[1], flag, scale, count, 1.25, 0.375, 0.8125)
            want += [f"{R.bits(o[k]):08x}" for k in ("A", "Bc", "Cc", "dgamma", "dbeta")]
        if res.split() != want:
            bad.append((line, " ".join(want)))
        seen.add((s, e, g, n, w))
        hit["inside"] += not flag
        hit["flagged"] += flag
        hit["some pass and some do not"] += 0 < passed < 2 * n * w
        hit["rounds to zero"] += (not flag) and words == [0, 0]
        hit["half a quantum"] += float(scale) * 2.0 ** e == 0.5
    assert not bad, (len(bad), bad[:3])
    assert seen == {(s, e, g, n, w) for s in (0, 1) for e in EXPONENTS for g in (0, 1, 2) for n in COUNTS for w in WORLDS
                    if not (g == 2 and n > 1000)}
    assert all(hit.values()), hit


def test_vectorised_and_integer_restatements_agree():
    """accumulate() (NumPy int64, which wraps by itself) against accumulate_ints() (Python integers, wrap written out), on
    contributions around the limit, around the quantum and far beyond, under the new rule and the parent's"""
    rng = np.random.default_rng(5)
    for scale in (R.SCALE_FWD, R.SCALE_BWD):
        for n, w in ((1, 1), (2, 1), (3, 2), (16, 8), (33, 1)):
            for lim in (R.limit(n, w), R.PARENT_LIMIT):
                top = float(lim) / float(scale)
                for mag in (top, top / 2, top * 4, 2.0 ** -26, 1.0, np.inf):
                    v = (rng.uniform(0.5, 1.25, n * w) * rng.choice([-1.0, 1.0], n * w)).astype(F32) * F32(mag)
                    word, flag = R.accumulate(v, scale, lim)
                    word_i, flag_i, _ = R.accumulate_ints(v, scale, lim)
                    assert (word, flag) == (word_i, flag_i), (scale, n, w, lim, mag)
    assert R.accumulate(np.array([np.nan, 1.0], F32), R.SCALE_FWD, R.limit(2))[1]
    assert R.signed((1 << 64) - 1) == -1 and R.signed(1 << 63) == -(1 << 63) and R.signed((1 << 63) - 1) == (1 << 63) - 1


def _worst_total(lim, contributions):
    """`contributions` times the largest value that passes `lim`, all of one sign: (fixed-point value, exact total)"""
    top = np.nextafter(F32(lim), F32(0.0))
    assert abs(top) < lim and not (abs(F32(lim)) < lim)
    q = int(np.rint(np.float64(top)))
    return q, q * contributions


def test_contributions_inside_the_limit_cannot_leave_the_signed_range(sweep):
    sizes = {(n, w) for n in list(range(1, 4200)) + [1 << k for k in range(13, 37)] + [(1 << k) - 1 for k in range(13, 37)]
             for w in (1, 2, 3, 8, 64)} | {(n, w) for n in COUNTS for w in WORLDS}
    for n, w in sizes:
        q, total = _worst_total(R.limit(n, w), n * w)
        assert total < 2 ** 63 and q > 0, (n, w)
        assert R.signed(total) == total and R.signed(-total) == -total
        # ... and the limit is not needlessly small: the total it admits is at least 2^61.9
        assert total > 2 ** 61.9, (n, w)
    # the C++ header's limit is the restatement's on the sweep's launch sizes (the program checked the property itself)
    got = {tuple(map(int, l.partition(" : ")[0].split())): l.partition(" : ")[2].split() for l in sweep["worst"]}
    assert set(got) == {(n, w) for n in COUNTS for w in WORLDS}
    for (n, w), (lim_bits, q) in got.items():
        assert (int(lim_bits, 16), int(q)) == (R.bits(R.limit(n, w)), _worst_total(R.limit(n, w), 1)[0]), (n, w)


def test_the_parents_constant_limit_wraps_at_two_contributions():
    """One constant per contribution, 9.0e18 ~ 2^62.96: one contribution cannot wrap, two can, and nothing is flagged."""
    q, total = _worst_total(R.PARENT_LIMIT, 1)
    assert total < 2 ** 63 and 2 * q >= 2 ** 63 and R.signed(2 * q) < 0
    # in the forward setting of the smallest launch that has a window: 2 workgroups of 128 values of y with rms 2^15.8
    sq = np.full(2, 128 * (2.0 ** 15.8) ** 2, F32)                     # the two workgroups' sums of y^2
    assert (np.abs(sq * R.SCALE_FWD) < R.PARENT_LIMIT).all()
    word, flag, true_sum = R.accumulate_ints(sq, R.SCALE_FWD, R.parent_limit(2))
    assert not flag and true_sum >= 2 ** 63 and R.signed(word) == true_sum - 2 ** 64 < 0
    o = R.fwd_finish(0, word, flag, R.SCALE_FWD, 256, 1e-5, 1.0, 0.0)
    assert o["var"] == 0.0 and np.isclose(o["invstd"], 1 / np.sqrt(1e-5))           # the silent answer: a finite invstd of 316
    # the same contributions under the launch's own limit: flagged, and the consumers read NaN
    word, flag, _ = R.accumulate_ints(sq, R.SCALE_FWD, R.limit(2))
    assert flag and word == 0
    mean_word, mean_flag = R.accumulate(np.zeros(2, F32), R.SCALE_FWD, R.limit(2))
    o = R.fwd_finish(mean_word, word, flag or mean_flag, R.SCALE_FWD, 256, 1e-5, 1.0, 0.0)
    assert np.isnan(o["mean"]) and np.isnan(o["s"]) and np.isnan(o["t"])
    # the issue's table: 2048 values per channel in 16 contributions of 128, the variance the parent's rule returns
    for log_rms, silent in ((13.9, False), (15, True)):
        sq = np.full(16, 128 * 4.0 ** log_rms, F32)
        word, flag, true_sum = R.accumulate_ints(sq, R.SCALE_FWD, R.parent_limit(16))
        var = R.fwd_finish(0, word, flag, R.SCALE_FWD, 2048, 1e-5, 1.0, 0.0)["var"]
        assert not flag and (R.signed(word) != true_sum) == silent and var == (0.0 if silent else float(sq[0]) / 128)
        assert R.accumulate(sq, R.SCALE_FWD, R.limit(16))[1]                # now: loud in both
    assert not R.accumulate(np.full(16, 128 * 4.0 ** 13.4, F32), R.SCALE_FWD, R.limit(16))[1]
    # and the backward scale: sums of g near 2^20.5
    g = np.full(2, 2.0 ** 20.5, F32)
    word, flag, true_sum = R.accumulate_ints(g, R.SCALE_BWD, R.parent_limit(2))
    assert not flag and true_sum >= 2 ** 63 and R.signed(word) < 0
    assert R.accumulate(g, R.SCALE_BWD, R.limit(2))[1]


@pytest.mark.parametrize("B", [3, 33])
def test_oracle_backward_is_equivariant_under_the_powers_of_two_the_gpu_tests_use(B):
    """test_gpu_bn_range.py scales the gradient that enters the stand-alone Encoder / Decoder by 2^k and compares with ONE run of
    the bf16 oracle times 2^k.  That is sound while the oracle's own bf16 tensors neither under- nor overflow: dout times 2^k must
    give every BatchNorm gradient times 2^k bit for bit, finite and not zero, at both ends of the range of k and in between.  It
    does over the whole range, so no k had to be dropped."""
    from oracle import ae_numpy as O
    from test_gpu_bn_range import BN_NAMES, K_RANGE, _oracle
    o = _oracle(B)
    for k in (K_RANGE[0], -44, 21, K_RANGE[1]):
        s = np.float32(2.0 ** k)
        ge = O.ae_backward(o["p"], o["out"], o["x"], None, 1.0, quant="bf16", head=False, dout=(np.zeros_like(o["x"]), None, o["dz"] * s))
        gd = O.ae_backward(o["p"], o["out"], o["x"], None, 1.0, quant="bf16", head=False, dout=(o["g"] * s, None, None))
        for name in BN_NAMES:
            for kind in (".weight", ".bias"):
                ref, got = (o["enc"], ge) if name.startswith("enc.") else (o["dec"], gd)
                assert np.isfinite(got[name + kind]).all() and np.abs(got[name + kind]).max() > 0
                assert np.array_equal(got[name + kind], ref[name + kind] * s), (k, name + kind)
