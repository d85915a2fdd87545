"""Object-based classification (eae_amd.zonal; include/eae.h, "zonal statistics"): the two entry points in the header, the library
and the ctypes table; the argument errors of the C calls and of the wrappers, all raised before a device is touched; and the parts
that are plain torch -- `compact_zones`, `zone_labels`, `zone_confusion`, `report.zone_table` -- against the NumPy restatement
(tests/zonal_ref.py) on CPU tensors.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import eae_amd
from eae_amd import _lib
from eae_amd import zonal as Z
from zonal_ref import compact_ref, q_ref, zonal_ref, zone_labels_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("eae_zonal_accumulate", "eae_zonal_paint")
PUBLIC = ("compact_zones", "zonal_stats", "zone_labels", "paint_zones", "classify_zones", "zone_confusion", "zone_table")


def test_symbols_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "eae.h")).read()
    assert "zonal statistics" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/eae.h"
        assert hasattr(raw, name), f"{name} is not exported by the library"
        assert name in _lib.EXPORTS
    for name in PUBLIC:
        assert name in eae_amd.__all__ and callable(getattr(eae_amd, name))
    assert "ZonalStats" in eae_amd.__all__ and eae_amd.ZonalStats is Z.ZonalStats
    from eae_amd import build as B
    assert "eae_zonal.hip" in B.SOURCES


# ---------------------------------------------------------------------------------------------------- the C entry points
def _accumulate(lib, a):
    return lib.eae_zonal_accumulate(None, a["zones"], a["eb"], a["h"], a["w"], a["labels"], a["probs"], a["ch"], a["cw"], a["cell"],
                                    a["oy"], a["ox"], None, a["k"], a["z"], a["acc"], a["votes"], a["sums"])


def test_accumulate_rejects_bad_arguments():
    """The checks of the C call come before any launch, so they run without a device (the pointers are never dereferenced)."""
    lib = _lib.load()
    buf = (C.c_longlong * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(zones=p, eb=4, h=4, w=4, labels=p, probs=None, ch=1, cw=1, cell=4, oy=0, ox=0, k=3, z=2, acc=0, votes=p, sums=None)
    bad = [dict(zones=None), dict(labels=None), dict(votes=None), dict(eb=2), dict(eb=1), dict(k=0), dict(k=65), dict(z=0), dict(z=-1),
           dict(z=2 ** 31 // 4), dict(z=2 ** 31 - 1, k=1), dict(cell=0), dict(oy=-1), dict(ox=-1), dict(h=0), dict(w=0), dict(ch=0),
           dict(cw=0), dict(h=2 ** 16, w=2 ** 15), dict(acc=2), dict(acc=-1), dict(probs=p), dict(sums=p)]
    for change in bad:
        rc = _accumulate(lib, dict(ok, **change))
        assert rc == -2 and b"zonal_accumulate" in lib.eae_last_error(), change
    # the largest table that is allowed passes the size check (and fails on the next one: a NULL labels)
    rc = _accumulate(lib, dict(ok, z=(2 ** 31 - 1) // 4, labels=None))
    assert rc == -2 and b"NULL labels" in lib.eae_last_error()


def test_paint_rejects_bad_arguments():
    lib = _lib.load()
    buf = (C.c_longlong * 16)()
    p = C.cast(buf, C.c_void_p)
    ok = dict(zones=p, eb=8, h=4, w=4, values=p, z=3, out=p)
    bad = [dict(zones=None), dict(values=None), dict(out=None), dict(eb=2), dict(eb=0), dict(z=0), dict(h=0), dict(w=0),
           dict(h=2 ** 16, w=2 ** 15)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.eae_zonal_paint(None, a["zones"], a["eb"], a["h"], a["w"], a["values"], a["z"], -1, a["out"])
        assert rc == -2 and b"zonal_paint" in lib.eae_last_error(), change


# ---------------------------------------------------------------------------------------------------- the wrappers' host errors
def test_zonal_stats_host_errors():
    zones = torch.zeros((40, 50), dtype=torch.int32)
    labels = torch.zeros((5, 7), dtype=torch.int64)
    probs = torch.zeros((3, 5, 7), dtype=torch.float32)
    f = eae_amd.zonal_stats
    for k in (0, 65, 2.0, True):
        with pytest.raises(RuntimeError, match="num_classes must be an integer in 1..64"):
            f(zones, 4, labels, k)
    with pytest.raises(RuntimeError, match=r"zones must be a \[H, W\]"):
        f(zones[0], 4, labels, 3)
    for bad in (zones.to(torch.float32), zones.to(torch.bool)):
        with pytest.raises(RuntimeError, match="zones must have an integer dtype"):
            f(bad, 4, labels, 3)
    with pytest.raises(RuntimeError, match="zones is empty"):
        f(zones[:0], 4, labels, 3)
    with pytest.raises(RuntimeError, match="below 2\\^31"):
        f(torch.zeros((1, 1), dtype=torch.int8).expand(2 ** 16, 2 ** 15), 4, labels, 3)
    for z in (0, -1, 2.5, 2 ** 31):
        with pytest.raises(RuntimeError, match="num_zones must be an integer"):
            f(zones, z, labels, 3)
    with pytest.raises(RuntimeError, match=r"num_zones \* \(num_classes \+ 1\)"):
        f(zones, 2 ** 31 // 4, labels, 3)
    for bad in (labels.to(torch.float32), labels[0], labels.to(torch.bool)):
        with pytest.raises(RuntimeError, match="labels must be a 2-D integer map"):
            f(zones, 4, bad, 3)
    with pytest.raises(RuntimeError, match="labels is empty"):
        f(zones, 4, labels[:0], 3)
    for bad in (probs.to(torch.float64), probs[:2], probs[:, :4], "probs"):
        with pytest.raises(RuntimeError, match=r"probs must be a float32 \[K, cH, cW\]"):
            f(zones, 4, labels, 3, probs=bad)
    for cell in (0, -2, 1.5):
        with pytest.raises(RuntimeError, match="cell must be a positive integer"):
            f(zones, 4, labels, 3, cell=cell)
    for origin in ((-1, 0), (0, -3)):
        with pytest.raises(RuntimeError, match="origin must not be negative"):
            f(zones, 4, labels, 3, cell=8, origin=origin)
    with pytest.raises(RuntimeError, match="origin must be a pair"):
        f(zones, 4, labels, 3, cell=8, origin=4)
    with pytest.raises(RuntimeError, match=r"mask must be a \[H, W\]"):
        f(zones, 4, labels, 3, cell=8, mask=torch.zeros((40, 49), dtype=torch.bool))
    with pytest.raises(RuntimeError, match="mask dtype"):
        f(zones, 4, labels, 3, cell=8, mask=torch.zeros((40, 50), dtype=torch.int32))
    votes, sums = torch.zeros((4, 4), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="out must be a ZonalStats"):
        f(zones, 4, labels, 3, cell=8, out=votes)
    for out in (Z.ZonalStats(votes[:3], None), Z.ZonalStats(votes, sums), Z.ZonalStats(torch.zeros((4, 5), dtype=torch.int64), None)):
        with pytest.raises(RuntimeError, match="out must hold"):
            f(zones, 4, labels, 3, cell=8, out=out)
    with pytest.raises(RuntimeError, match="out must hold"):                  # probs given, out without prob_sums
        f(zones, 4, labels, 3, probs=probs, cell=8, out=Z.ZonalStats(votes, None))
    with pytest.raises(RuntimeError, match="out.votes must be an int64"):
        f(zones, 4, labels, 3, cell=8, out=Z.ZonalStats(votes.to(torch.int32), None))
    with pytest.raises(RuntimeError, match="out.prob_sums must be None or an int64"):
        f(zones, 4, labels, 3, probs=probs, cell=8, out=Z.ZonalStats(votes, sums[:, :2]))
    with pytest.raises(RuntimeError, match="out must be contiguous"):
        f(zones, 4, labels, 3, cell=8, out=Z.ZonalStats(torch.zeros((4, 8), dtype=torch.int64)[:, ::2], None))
    with pytest.raises(RuntimeError, match="HIP device"):               # everything is in order but the tensors are on the host
        f(zones, 4, labels, 3, probs=probs, cell=8, out=Z.ZonalStats(votes, sums))


def test_paint_zones_host_errors():
    zones = torch.zeros((4, 5), dtype=torch.int64)
    values = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match=r"zones must be a \[H, W\]"):
        eae_amd.paint_zones(zones[0], values)
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.paint_zones(zones.to(torch.float32), values)
    for bad in (values.to(torch.int32), values[:0], values.reshape(1, 3)):
        with pytest.raises(RuntimeError, match="values must be a non-empty 1-D int64"):
            eae_amd.paint_zones(zones, bad)
    for fill in (1.5, True, 2 ** 63):
        with pytest.raises(RuntimeError, match="fill must be an integer"):
            eae_amd.paint_zones(zones, values, fill=fill)
    with pytest.raises(RuntimeError, match="HIP device"):
        eae_amd.paint_zones(zones, values)


def test_classify_zones_host_errors():
    torch.manual_seed(0)
    ae = eae_amd.SupervisedAutoencoder(64, 10, image_size=64, in_channels=3).eval()
    mlp = eae_amd.MLP(64, 10).eval()
    scene = torch.zeros((3, 150, 200), dtype=torch.uint8)
    zones = torch.zeros((150, 200), dtype=torch.int32)
    f = eae_amd.classify_zones
    with pytest.raises(RuntimeError, match="blend=False needs stride == patch"):
        f(scene, ae, mlp, zones, divisor=255.0, stride=32)
    with pytest.raises(RuntimeError, match="stride that divides"):
        f(scene, ae, mlp, zones, divisor=255.0, stride=48, blend=True)
    with pytest.raises(RuntimeError, match="mlp must be an MLP"):
        f(scene, ae, ae, zones, divisor=255.0)
    for bad in (zones[:, :199], zones.T.contiguous(), "zones"):
        with pytest.raises(RuntimeError, match="zone raster of the scene's size"):
            f(scene, ae, mlp, bad, divisor=255.0)
    with pytest.raises(RuntimeError, match="zones must have an integer dtype"):
        f(scene, ae, mlp, zones.to(torch.float32), divisor=255.0)
    with pytest.raises(RuntimeError, match="rule must be 'probs' or 'votes'"):
        f(scene, ae, mlp, zones, rule="all", divisor=255.0)
    with pytest.raises(RuntimeError, match="rule must be 'all' or 'any'"):
        f(scene, ae, mlp, zones, invalid_rule="votes", divisor=255.0)
    for c in (-0.1, 1.5, "x", float("nan")):
        with pytest.raises(RuntimeError, match="min_coverage must be a number in"):
            f(scene, ae, mlp, zones, min_coverage=c, divisor=255.0)
    with pytest.raises(RuntimeError, match="num_zones must be an integer"):
        f(scene, ae, mlp, zones, num_zones=0, divisor=255.0)
    with pytest.raises(RuntimeError):                                   # everything is in order but the scene is a host tensor
        f(scene, ae, mlp, zones, num_zones=4, divisor=255.0)


# ---------------------------------------------------------------------------------------------------- compact_zones
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16, torch.uint8])
def test_compact_zones_against_the_reference(dtype):
    rng = np.random.default_rng(3)
    lo, hi = (0, 200) if dtype == torch.uint8 else (-4, 3000)
    ids = np.repeat(rng.integers(lo, hi, (9, 11)), 3, 1)                       # runs, gaps between the values, negatives
    zones, table = eae_amd.compact_zones(torch.from_numpy(ids).to(dtype))
    rz, rt = compact_ref(ids)
    assert zones.dtype == torch.int32 and table.dtype == torch.int64 and zones.device.type == "cpu"
    assert np.array_equal(zones.numpy(), rz) and np.array_equal(table.numpy(), rt)
    back = np.where(rz >= 0, rt[np.maximum(rz, 0)], -1)
    assert np.array_equal(back, np.where(ids >= 0, ids, -1))


def test_compact_zones_edge_cases():
    zones, table = eae_amd.compact_zones(torch.full((3, 4), -1, dtype=torch.int64))       # no zone at all
    assert table.numel() == 0 and bool((zones == -1).all())
    zones, table = eae_amd.compact_zones(torch.tensor([[2 ** 40, 7], [7, -2 ** 40]]))     # ids that do not fit 32 bits
    assert zones.tolist() == [[1, 0], [0, -1]] and table.tolist() == [7, 2 ** 40]
    with pytest.raises(RuntimeError, match="integer dtype"):
        eae_amd.compact_zones(torch.zeros((2, 2)))


# ---------------------------------------------------------------------------------------------------- zone_labels
def _stats(votes, sums=None):
    return Z.ZonalStats(torch.tensor(votes, dtype=torch.int64), None if sums is None else torch.tensor(sums, dtype=torch.int64))


def _same(got, ref):
    label, conf, cov = got
    assert label.dtype == torch.int64 and conf.dtype == torch.float32 and cov.dtype == torch.float32
    assert np.array_equal(label.numpy(), ref[0])
    assert np.array_equal(conf.numpy(), ref[1], equal_nan=True) and np.array_equal(cov.numpy(), ref[2], equal_nan=True)


def test_zone_labels_hand_worked():
    one = 2 ** 32
    votes = [[3, 3, 0, 2],        # a tie in the votes: class 0, the lowest, wins
             [1, 4, 0, 0],        # a tie in prob_sums (classes 0 and 2) that the votes would break in favour of class 1
             [0, 0, 0, 9],        # nothing classified
             [0, 0, 0, 0],        # an empty zone
             [0, 2, 2, 4],        # coverage exactly 0.5
             [0, 0, 5, 0]]
    sums = [[3 * one, 3 * one, 0], [2 * one + 5, 2 * one, 2 * one + 5], [0, 0, 0], [0, 0, 0], [7, one, one + 1], [0, 0, 5 * one]]
    st = _stats(votes, sums)
    label, conf, cov = eae_amd.zone_labels(st, "votes")
    assert label.tolist() == [0, 1, -1, -1, 1, 2]
    assert np.allclose(conf[:2].numpy(), [0.5, 0.8], rtol=0, atol=1e-7)
    assert np.isnan(float(conf[2])) and np.isnan(float(conf[3])) and float(conf[5]) == 1.0
    assert cov.tolist()[:3] == [0.75, 1.0, 0.0] and np.isnan(float(cov[3])) and float(cov[4]) == 0.5
    label, conf, cov = eae_amd.zone_labels(st, "probs")
    assert label.tolist() == [0, 0, -1, -1, 2, 2]                 # zone 1: class 0 (tie with 2, lowest wins) although class 1 has the votes
    assert float(conf[0]) == 0.5 and float(conf[5]) == 1.0 and np.isnan(float(conf[2]))
    # min_coverage at exact equality keeps the zone (classified < min_coverage * total is false), just above it drops it
    assert eae_amd.zone_labels(st, "votes", min_coverage=0.5)[0].tolist() == [0, 1, -1, -1, 1, 2]
    assert eae_amd.zone_labels(st, "votes", min_coverage=0.5000001)[0].tolist() == [0, 1, -1, -1, -1, 2]
    assert eae_amd.zone_labels(st, "votes", min_coverage=0.75)[0].tolist() == [0, 1, -1, -1, -1, 2]
    assert eae_amd.zone_labels(st, "votes", min_coverage=1.0)[0].tolist() == [-1, 1, -1, -1, -1, 2]
    dropped = eae_amd.zone_labels(st, "probs", min_coverage=0.75)
    assert np.isnan(float(dropped[1][4])) and float(dropped[2][4]) == 0.5    # the coverage is reported for a dropped zone too
    for rule in ("votes", "probs"):
        for c in (0.0, 0.5, 0.75, 1.0):
            _same(eae_amd.zone_labels(st, rule, c), zone_labels_ref(np.array(votes), np.array(sums), rule, c))


@pytest.mark.parametrize("k,seed", [(1, 0), (3, 1), (10, 2), (64, 3)])
def test_zone_labels_against_the_reference(k, seed):
    """Tables from the reference accumulation of a random map: sums that differ only below float64's 53 bits must still be told
    apart (the comparison is on the integers)."""
    rng = np.random.default_rng(seed)
    zones = rng.integers(-1, 12, (30, 40))
    labels = rng.integers(-1, k + 1, (8, 10))
    probs = rng.random((k, 8, 10)).astype(np.float32)
    votes, sums = zonal_ref(zones, 12, labels, k, probs, cell=4)
    votes[5] = 0
    sums[5] = 0                                                   # an empty zone
    if k >= 3:
        sums[0, :3] = [2 ** 60 + 1, 2 ** 60 + 2, 2 ** 60]         # equal as float64
        sums[1, :3] = [2 ** 60 + 1, 2 ** 60 + 1, 2 ** 60]         # a tie: the lowest
    st = Z.ZonalStats(torch.from_numpy(votes), torch.from_numpy(sums))
    for rule in ("probs", "votes"):
        for c in (0.0, 0.3, 0.9):
            _same(eae_amd.zone_labels(st, rule, c), zone_labels_ref(votes, sums, rule, c))
    if k >= 3:
        assert eae_amd.zone_labels(st, "probs")[0][:2].tolist() == [1, 0]
    _same(eae_amd.zone_labels(Z.ZonalStats(st.votes, None), "votes"), zone_labels_ref(votes, None, "votes"))


def test_zone_labels_errors():
    st = _stats([[1, 2, 3]])
    with pytest.raises(RuntimeError, match="needs prob_sums"):
        eae_amd.zone_labels(st)
    with pytest.raises(RuntimeError, match="rule must be"):
        eae_amd.zone_labels(st, "mean")
    with pytest.raises(RuntimeError, match="min_coverage"):
        eae_amd.zone_labels(st, "votes", min_coverage=2)
    with pytest.raises(RuntimeError, match="stats must be a ZonalStats"):
        eae_amd.zone_labels((st.votes, None), "votes")
    with pytest.raises(RuntimeError, match="votes must be an int64"):
        eae_amd.zone_labels(Z.ZonalStats(st.votes.to(torch.float32), None), "votes")
    with pytest.raises(RuntimeError, match="prob_sums must be None or an int64"):
        eae_amd.zone_labels(Z.ZonalStats(st.votes, torch.zeros((1, 3), dtype=torch.int64)))


def test_q_ref_edge_values():
    p = np.array([0.0, 1.0, 2.0 ** -33, 1.5 * 2.0 ** -32, 2.0 ** -32, np.nan, 1.5, -0.25, 0.5, np.inf, -np.inf], dtype=np.float32)
    assert q_ref(p).tolist() == [0, 2 ** 32, 0, 2, 1, 0, 2 ** 32, 0, 2 ** 31, 2 ** 32, 0]


# ---------------------------------------------------------------------------------------------------- zone_confusion, zone_table
def test_zone_confusion_counts_zones():
    pred = torch.tensor([0, 1, 1, -1, 2, 7, 0], dtype=torch.int64)
    truth = torch.tensor([0, 1, 0, 1, -1, 2, 0], dtype=torch.int32)
    cm = eae_amd.zone_confusion(pred, truth, 3)
    ref = np.zeros((4, 4), dtype=np.int64)
    for p, t in zip(pred.tolist(), truth.tolist()):
        ref[t if 0 <= t < 3 else 3, p if 0 <= p < 3 else 3] += 1
    assert cm.dtype == torch.int64 and np.array_equal(cm.numpy(), ref) and int(cm.sum()) == 7
    m = eae_amd.confusion_metrics(cm)
    assert m["total"] == 6 and abs(m["accuracy"] - 3 / 6) < 1e-15
    with pytest.raises(RuntimeError, match="1-D integer"):
        eae_amd.zone_confusion(pred.to(torch.float32), truth, 3)
    with pytest.raises(RuntimeError, match="zones"):
        eae_amd.zone_confusion(pred[:3], truth, 3)
    with pytest.raises(RuntimeError, match="num_classes"):
        eae_amd.zone_confusion(pred, truth, 0)


def test_zone_table_text():
    st = _stats([[3, 1, 0], [0, 0, 0], [2, 2, 4]], [[2 ** 33, 2 ** 33], [0, 0], [5, 2 ** 32]])
    text = eae_amd.zone_table(st, eae_amd.zone_labels(st, "probs", 0.5), ["water", "wood"])
    lines = text.splitlines()
    assert lines[0].split() == ["zone", "pixels", "coverage", "class", "confidence"] and len(lines) == 5
    assert lines[2].split() == ["0", "4", "1.0000", "water", "0.5000"]
    assert lines[3].split() == ["1", "0", "-", "-", "-"]
    assert lines[4].split() == ["2", "8", "0.5000", "wood", "0.2500"]
    assert eae_amd.zone_table(st, eae_amd.zone_labels(st, "votes")).splitlines()[2].split()[3] == "0"
    with pytest.raises(ValueError, match="class_names"):
        eae_amd.zone_table(st, eae_amd.zone_labels(st, "votes"), ["a"])
    with pytest.raises(ValueError, match="triple"):
        eae_amd.zone_table(st, 5)
