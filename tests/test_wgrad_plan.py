"""The slice plan of the weight-gradient launches (csrc/eae_wgrad_plan.h) against its Python restatements, without a GPU.

wgrad_plan_check.cpp includes only the plan header.  Built with -Wall -Werror under the address and undefined-behaviour sanitisers, it
prints one line per case of its sweep: every conv_ref.WGRAD_INSTANCES row on nine small maps (and two that have no geometry), the
edge kernel at every edge_ref.EDGE_BANDS value on seven image sizes, batches 1..600, scratch at the engine's default, at three
slices, at one slice and one float short of a slice, 1 / 2 / 8 / 64 members of a grouped step, workgroup budgets 64 (the default), 16,
256 and a mixed triple, edge caps 512 / 256 (the default) and 64 / 32; the fp8 variant; eae_fc_klen at 1024 map sizes and five
settings.  Every line must be what conv_ref.expected_wgrad_launch / edge_ref.expected_edge_wgrad_launch -- the functions the GPU
tests take their expected launches from -- say under the same settings, and every branch of the plan must occur in the sweep.  The
program itself checks on every case, and on extreme arguments, that every tile is covered once and the partials fit the scratch."""
import os
import shutil
import subprocess

import pytest

import conv_ref as R
import edge_ref as E
import eae_amd

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(eae_amd.__file__), "csrc")
SIDE_SCRATCH = 6 * 1024 * 1024                       # eae_ctx::wscratch_floats
MAPS = [(4, 4), (8, 8), (16, 16), (8, 16), (16, 32), (8, 32), (24, 16), (32, 32), (64, 64)]
NO_GEOMETRY_MAPS = [(16, 8), (6, 6)]
IMAGES = [(8, 64), (16, 64), (24, 64), (64, 64), (16, 128), (24, 192), (256, 256)]
REFUSED = {1: R.WGRAD_NO_GEOMETRY, 2: R.WGRAD_SCRATCH, 3: R.WGRAD_FP8_NARROW}      # WG_* of the header


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    """the program's output, split into the lines of the three plans; built and run once"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++, g++ or clang++) on PATH")
    exe = str(tmp_path_factory.mktemp("wgrad_plan") / "wgrad_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(HERE, "wgrad_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stderr == "", r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert lines[-1].endswith(" cases, 0 violations") and "VIOLATION" not in r.stdout, lines[-1]
    out = {"s2": [], "edge": [], "edge_row": [], "fc": []}
    for line in lines[:-1]:
        head, _, rest = line.partition(" ")
        out[head].append(rest)
    assert int(lines[-1].split()[0]) > sum(len(v) for v in out.values())      # + the extreme arguments, which are not printed
    return out


def test_s2_plan_is_the_restatement(sweep):
    bad, seen, maps, scratch_kinds = [], set(), set(), set()
    hit = dict.fromkeys(["halved", "recount drops slices", "one slice", "several slices", "group floor", "group share",
                         R.WGRAD_NO_GEOMETRY, R.WGRAD_SCRATCH, R.WGRAD_FP8_NARROW], 0)
    configs, per_batch = set(), [0] * 601
    for line in sweep["s2"]:
        args, _, res = line.partition(" : ")
        cs, cb, sm, bm, hs, ws, B, scratch, one, wide, last, mult, fp8 = map(int, args.split())
        refused, tw, th, ni, tiles, slices, per, nblk, grid, used, writes_dw = map(int, res.split())
        want = R.expected_wgrad_launch(cs, cb, sm, hs, ws, B, scratch, mult, (one, wide, last), bool(fp8))
        got = REFUSED[refused] if refused else ((tw, th, ni), tiles, slices, per)
        if got != want:
            bad.append((line, want))
            continue
        seen.add((cs, cb, sm, bm))
        maps.add((hs, ws))
        per_batch[B] += 1
        sz = cs * cb * 9
        kind = "default" if scratch == SIDE_SCRATCH else {3 * sz: "three", sz: "one", sz - 1: "short"}[scratch]
        scratch_kinds.add(kind)
        configs.add((kind, one, wide, last, mult, fp8))
        if refused:
            hit[want] += 1
            if refused != 3:
                continue
        # every tile is covered once, and the partials fit (the fp8 refusal comes last: the plan is complete)
        # (slices * nblk workgroups, each with a partial of its 64 x 32 x 9 block)
        assert slices * nblk * 64 * 32 * 9 <= scratch and grid == slices * nblk and nblk == (cs // 64) * (cb // 32), line
        assert (slices - 1) * per < tiles <= slices * per, line
        assert writes_dw == (slices == 1) and used == (0 if slices == 1 else slices * sz), line
        budget = R.wgrad_workgroups_setting(cs, sm, (one, wide, last))
        if mult > 1:
            hit["group floor" if budget // mult < 8 else "group share"] += 1
            budget = max(budget // mult, 8)
        first = min(max(budget // nblk, 1), tiles)                  # before the scratch and the recount have their say
        halved = first * sz > scratch
        hit["halved"] += halved
        hit["recount drops slices"] += (not halved) and slices < first
        hit["one slice" if slices == 1 else "several slices"] += 1
    assert not bad, (len(bad), bad[:5])
    assert seen == set(R.WGRAD_INSTANCES) and len(seen) == 13
    assert maps == set(MAPS + NO_GEOMETRY_MAPS) and scratch_kinds == {"default", "three", "one", "short"}
    # batches 1..600 of every row on every map, under each of the settings: 4 scratch sizes and the fp8 variant under the defaults,
    # the other eleven (budget, members) pairs and a triple that tells the three budgets apart on the maps that have a geometry
    assert per_batch[0] == 0 and set(per_batch[1:]) == {13 * (11 * 5 + 9 * 12)}
    uniform = {(64, 64, 64), (16, 16, 16), (256, 256, 256)}
    assert configs == ({(k, 64, 64, 64, 1, 0) for k in scratch_kinds} | {("default", 64, 64, 64, 1, 1), ("default", 48, 96, 24, 1, 0)}
                       | {("default",) + b + (m, 0) for b in uniform for m in (1, 2, 8, 64)})
    assert all(hit.values()), hit


def test_edge_plan_is_the_restatement(sweep):
    bad, seen, scratch_kinds, configs, per_batch = [], set(), set(), set(), [0] * 601
    hit = dict.fromkeys(["halved", "recount drops workgroups", "one workgroup", "group floor", "group share", "refused"], 0)
    for line in sweep["edge"]:
        args, _, res = line.partition(" : ")
        kind, C, H, W, B, scratch, cap_main, cap_side, mult = map(int, args.split())
        ok, tiles, blocks, per, used = map(int, res.split())
        want = E.expected_edge_wgrad_launch(kind, C, H, W, B, scratch, mult, (cap_main, cap_side))
        if ((tiles, blocks, per) if ok else None) != want:
            bad.append((line, want))
            continue
        seen.add((kind, C, H, W))
        per_batch[B] += 1
        sl = 288 * C
        default = SIDE_SCRATCH if kind == 1 else 2048 * sl
        sk = "default" if scratch == default else {3 * sl: "three", sl: "one", sl - 1: "short"}[scratch]
        scratch_kinds.add(sk)
        configs.add((sk, cap_main, cap_side, mult))
        assert tiles == E.edge_tiles(H, W, B) and (blocks - 1) * per < tiles <= blocks * per and used == blocks * sl, line
        assert ok == (used <= scratch), line
        cap = (cap_main, cap_side)[kind]
        if mult > 1:
            hit["group floor" if cap // mult < 32 else "group share"] += 1
            cap = max(cap // mult, 32)
        first = min(tiles, cap)
        halved = first * sl > scratch and first > 1
        hit["halved"] += halved
        hit["recount drops workgroups"] += (not halved) and blocks < first
        hit["one workgroup"] += blocks == 1
        hit["refused"] += not ok
    assert not bad, (len(bad), bad[:5])
    assert seen == {(k, c, h, w) for k in (0, 1) for c in E.EDGE_BANDS for h, w in IMAGES}
    assert {i[0] for i in E.EDGE_WGRAD_INSTANCES} == {0, 1}          # the plan sees the source kind of an instantiation, nothing else
    assert scratch_kinds == {"default", "three", "one", "short"}
    # batches 1..600 of both source kinds at every band count on every image, under each of the settings
    assert per_batch[0] == 0 and set(per_batch[1:]) == {2 * 7 * 7 * len(configs)}
    assert configs == ({(k, 512, 256, 1) for k in scratch_kinds}
                       | {("default",) + c + (m,) for c in ((512, 256), (64, 32)) for m in (1, 2, 8, 64)})
    assert all(hit.values()), hit


def test_fc_klen_closed_form(sweep):
    """klen = 128 * 2^j with the smallest j that brings K / klen down to the setting, but no further than K stays divisible"""
    settings = set()
    for line in sweep["fc"]:
        args, _, res = line.partition(" : ")
        (K, setting), klen = map(int, args.split()), int(res)
        need = next(j for j in range(64) if (128 << j) * (setting + 1) > K)
        divisible = ((K // 128) & -(K // 128)).bit_length() - 1
        assert klen == 128 << min(need, divisible), line
        settings.add(setting)
    assert len(sweep["fc"]) == 5 * 1024 and settings == {1, 16, 64, 512, 1 << 20}
    assert "fc 4096 64 : 128" in ("fc " + s for s in sweep["fc"])      # the reference's 64x64 inputs: 32 slices of 128


def test_multi_tile_rows_come_out_of_the_c_plan(sweep):
    """The rows the GPU tests name for their multi-tile launches, looked up in the C plan's own output under the default settings"""
    s2 = {}
    for line in sweep["s2"]:
        args, _, res = line.partition(" : ")
        if args.endswith(f" {SIDE_SCRATCH} 64 64 64 1 0"):
            s2[tuple(map(int, args.split()[:7]))] = tuple(map(int, res.split()))
    for geo, (case, tiles, slices, per) in R.WGRAD_MULTI_TILE.items():
        got = s2[case]
        assert got[0] == 0 and got[1:4] == geo and got[4:7] == (tiles, slices, per), (case, got)
    edge = {}
    for line in sweep["edge_row"]:                                   # these rows bring their own scratch: the program lists them apart
        args, _, res = line.partition(" : ")
        edge[tuple(map(int, args.split()))] = tuple(map(int, res.split()))
    assert len(edge) == len(E.EDGE_WGRAD_MULTI_TILE) == 5
    for case, want in E.EDGE_WGRAD_MULTI_TILE.items():
        kind, smode, c, h, w, b, slices = case
        got = edge[(kind, c, h, w, b, E.edge_wgrad_scratch_floats(case), 512, 256, 1)]
        assert got[0] == 1 and got[1:4] == want and got[4] == want[1] * 288 * c, (case, got)
