"""Batch invariance of the inference forward's plans, checked on the CPU.

An executor planned for inference BN sets gemm_plan_images() = B for its forward ("Batch
size"): every choice that fixes the order of a sum is then made per image, so an image's result cannot depend on
the batch it shares a launch with.  tests/kernels/batch_invariance --plan makes no HIP call; for every case of
its table and every batch size of the case it prints the order-relevant plan twice, under gemm_plan_images() = B
("img") and = 0 ("launch"):
  GEMM   plan_gemm2(B * Mi, N, K): wsk (k_gemm2k: K split over a workgroup's waves) and splits (K split over
         workgroups); res / nper (k_gemm2r and the N tiles of one run) and the tile are printed too, they follow
         the launch and do not reorder a sum (tests/test_gpu_batch_invariance.py holds that on the device)
  SE     se_plan_info(B, C, Cse, chunks): s1, cs1 (the slices whose shares of the squeeze product are added), s2,
         cs2, kg, jg (the lane groups the excite and the fold sum over)
  pools  red_plan_info(HW, C, B): rpc, chunks (the rows of one fp32 partial sum)
The tests hold the "img" fields equal across a case's batch sizes, and hold the table to the classes the device
test is meant to cover: for each of the three, at least one case whose "launch" fields do move with B (invariance
is not trivial there), the backbones' SE shapes at the batch sizes where se_plan moved, a deep-K GEMM the launch
alone would run unsplit, a few-tile K < 256 GEMM, an A-resident GEMM whose run length changes, and a fused
depthwise conv on both sides of its few-workgroups switch.

Before se_plan consulted gemm_plan_images(), test_img_plans_do_not_follow_the_batch failed on every SE case, e.g.
se_d0_c1152_n48_hw17_view: B=8 plans (32, 36, 36, 32, 2, 8, 16, 2) against B=1's (36, 32, 36, 32, 2, 8, 16, 2).
"""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

SE_FIELDS = ("s1", "cs1", "s2", "cs2", "kg", "jg")
POOL_FIELDS = ("rpc", "chunks")
GEMM_FIELDS = ("wsk", "splits")


@pytest.fixture(scope="module")
def plans():
    path = os.path.join(KERN, "batch_invariance")
    if not os.path.isfile(path):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/batch_invariance is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "batch_invariance"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("PHX_")}
    r = subprocess.run([path, "--plan"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert lines[-1].get("done") is True
    return {d["case"]: d for d in lines[:-1]}


def _order_fields(d, mode):
    """One tuple of order-relevant fields per batch size of the case."""
    out = []
    for p in d["plans"][mode]:
        if d["op"] == "se":
            out.append(tuple(p[k] for k in SE_FIELDS + POOL_FIELDS))
        elif d["op"] == "gemm":
            out.append(tuple(p["g"][k] for k in GEMM_FIELDS))
        elif d["op"] == "group":
            out.append(tuple(m[k] for m in p["members"] for k in GEMM_FIELDS))
        else:
            out.append(())  # K and tap orders are fixed in the kernels: nothing planned
    return out


def test_table_matches_the_source(plans):
    src = open(os.path.join(KERN, "batch_invariance.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    names = re.findall(r'^\s*bc\("([a-z0-9_]+)"', body, re.M)
    assert len(names) == len(set(names)) and set(names) == set(plans)
    for d in plans.values():
        assert d["Bs"] == sorted(set(d["Bs"])) and d["Bs"][0] == 1 and len(d["Bs"]) >= 3
        assert [p["B"] for p in d["plans"]["img"]] == d["Bs"] == [p["B"] for p in d["plans"]["launch"]]


def test_img_plans_do_not_follow_the_batch(plans):
    bad = []
    for name, d in plans.items():
        f = _order_fields(d, "img")
        for B, x in zip(d["Bs"], f):
            if x != f[0]:
                bad.append(f"{name}: B={B} plans {x} against B=1's {f[0]}")
    assert not bad, "\n".join(bad)


def test_no_cross_workgroup_split_in_a_batch_invariant_forward(plans):
    """splits > 1 is planned from the launch's tiles: it may not occur where k_gemm2k was not chosen."""
    for name, d in plans.items():
        for p in d["plans"]["img"]:
            for g in ([p["g"]] if d["op"] == "gemm" else p.get("members", [])):
                assert g["impl"] == 2, (name, g)
                assert g["wsk"] or g["splits"] == 1, (name, g)


def _moves(d, fields_of):
    f = [fields_of(p) for p in d["plans"]["launch"]]
    return any(x != f[0] for x in f)


def test_table_has_teeth(plans):
    """For GEMM, SE and pools at least one case's launch-planned fields differ across its batch sizes."""
    se = [d for d in plans.values() if d["op"] == "se"]
    gemm = [d for d in plans.values() if d["op"] == "gemm"]
    assert any(_moves(d, lambda p: tuple(p[k] for k in SE_FIELDS if k != "kg")) for d in se)
    assert any(_moves(d, lambda p: tuple(p[k] for k in POOL_FIELDS)) for d in se)
    assert any(_moves(d, lambda p: tuple(p["g"][k] for k in GEMM_FIELDS)) for d in gemm)


def test_table_has_the_backbone_se_shapes(plans):
    want = {(1152, 48): [1, 4, 8, 16], (672, 28): [1, 4, 8, 16], (2688, 112): [1, 3, 4, 8]}
    for (C, N), Bs in want.items():
        cases = [d for d in plans.values() if d["op"] == "se" and (d["a"], d["b"]) == (C, N)]
        assert cases, (C, N)
        assert all(d["Bs"] == Bs for d in cases), (C, N)
        # the launch-planned slicing moves within those batch sizes
        assert all(_moves(d, lambda p: (p["s1"], p["cs1"], p["s2"], p["cs2"])) for d in cases), (C, N)
        # HW = 1 and the smallest HW with more than one pool chunk; raw and BN-view input
        assert {d["c"] for d in cases} >= {1} and {d["d"] for d in cases} == {0, 1}
        many = [d for d in cases if d["c"] > 1]
        assert many and all(p["chunks"] > 1 for d in many for p in d["plans"]["img"])
        assert all(d["c"] - 1 <= p["rpc"] for d in many for p in d["plans"]["img"])  # one row less: one chunk


def test_table_has_the_gemm_classes(plans):
    gemm = [d for d in plans.values() if d["op"] == "gemm"]
    img = lambda d: [p["g"] for p in d["plans"]["img"]]
    launch = lambda d: [p["g"] for p in d["plans"]["launch"]]
    # deep K: k_gemm2k per image at every B, and the launch alone runs the largest batch unsplit
    deep = [d for d in gemm if d["d"] >= 256 and all(g["wsk"] for g in img(d))]
    assert any(not launch(d)[-1]["wsk"] and launch(d)[-1]["splits"] == 1 and launch(d)[0]["wsk"] for d in deep)
    # K < 256 over few tiles: k_gemm2k for the launch alone, never in a batch-invariant forward
    few = [d for d in gemm if d["d"] < 256 and all(g["wsk"] for g in launch(d))]
    assert few and all(not g["wsk"] for d in few for g in img(d))
    # A-resident with two K chunks, and a run length that changes with the M tiles
    res = [d for d in gemm if any(g["res"] for g in img(d))]
    assert any(len({g["nper"] for g in img(d)}) >= 3 for d in res)
    # modes 1 and 2 in every class; Mi no multiple of 32 rows (the smallest tile)
    for cls in (deep, few):
        assert {d["a"] for d in cls} == {1, 2}
    assert {d["a"] for d in res} & {2}
    assert all(d["b"] % 32 for d in gemm)
    assert any(d["b"] == 9 for d in gemm) and any(d["b"] == 49 for d in gemm)


def test_table_has_the_group_and_conv_cases(plans):
    grp = [d for d in plans.values() if d["op"] == "group"]
    assert any([m["M"] for m in d["plans"]["img"][0]["members"]] == [64, 16, 4] and (d["a"], d["b"]) == (64, 64) and
               d["Bs"] == [1, 4, 16] for d in grp)
    sep = [d for d in plans.values() if d["op"] == "sep"]
    assert {len(d["plans"]["img"][0]["ntiles"]) for d in sep} >= {1, 5}
    assert any(d["op"] == "dw" for d in plans.values())
    fused = [d for d in plans.values() if d["op"] == "dwf"]
    # both sides of launch_dw_fwd_fused's few-workgroups switch within one case, and one case wholly below it
    assert any({p["small"] for p in d["plans"]["img"]} == {0, 1} for d in fused)
    assert any({p["small"] for p in d["plans"]["img"]} == {1} for d in fused)
    assert {d["c"] for d in fused} == {2, 3}
