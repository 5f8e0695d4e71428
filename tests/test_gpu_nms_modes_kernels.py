"""Kernel-level parity of the segmented NonMaxSuppressionV5 (kernels_nms_seg.hip: hard NMS, any sigma / IoU threshold,
per-class NMS with its merge) against the host reference of tests/kernels_nms_seg, case by case.

tests/kernels_nms_seg/nms_seg_parity runs its table once, in one child process on one stream, and prints a JSON line
per case; each test below asserts one case's verdict.  Selected indices, scores, boxes, classes and counts are
compared exactly (a bad_* field counts the elements that differ bit for bit); the reference takes expf, the decay's
one library function, from the device (nms_seg_parity.cpp), so every other operation is held to the bit.  A soft case
at IoU threshold 1 must also be bit-equal to k_soft_nms on the same inputs (the yardstick).  If the child dies, times
out or never prints `done`, every test fails with the last line it printed and nothing more is started."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels_nms_seg")
BIN = os.path.join(KERN, "nms_seg_parity")

pytestmark = pytest.mark.gpu

TIMEOUT_S = 60  # the run takes about a second


def _binary():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels_nms_seg/nms_seg_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return BIN


def _case_names():
    src = open(os.path.join(KERN, "nms_seg_check.hpp")).read()
    body = src[src.index("// ---- the table"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*add\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def plan():
    """The case table's geometry and launch plans from --plan (host code only)."""
    r = subprocess.run([_binary(), "--plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(x) for x in r.stdout.splitlines() if x.strip()]


@pytest.fixture(scope="module")
def verdicts():
    state = {"cases": {}, "error": None}
    try:
        r = subprocess.run([_binary()], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
        out, rc = r.stdout, r.returncode
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        rc = "timeout"
    lines = [x for x in out.splitlines() if x.strip()]
    done = False
    for x in lines:
        d = json.loads(x)
        if "done" in d:
            done = True
        elif "case" in d and "fatal" not in d:
            state["cases"][d["case"]] = d
    if rc != 0 or not done:
        state["error"] = f"nms_seg_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_covers_what_it_must(verdicts, plan):
    """The table's geometry, from --plan: the N values, both plan boundaries the kernel has (keys past the
    LDS-resident positions; chunk factor 2), every setting, the per-class shapes, and a yardstick on every soft case
    at IoU threshold 1."""
    assert verdicts["error"] is None, verdicts["error"]
    PLAN = plan
    assert len(CASES) >= 40 and len(CASES) == len(set(CASES)) and set(verdicts["cases"]) == set(CASES)
    assert [p["case"] for p in PLAN] == CASES
    glob = [p for p in PLAN if p["kind"] == 1]
    assert {1, 63, 64, 65, 257, 3069, 49104} <= {p["N"] for p in glob}
    assert any(p["N"] > p["plan_lds_positions"] and p["thresh"] == "-inf" for p in glob)   # keys spill to global memory
    assert any(p["plan_m"] == 2 for p in glob)                                             # chunk factor 2
    assert {0, 0.5, 1} <= {p["iou"] for p in glob if p["sigma"] == 0}
    assert {"-inf", 0.5} <= {p["thresh"] for p in glob} and any(abs(p["thresh"] - 0.001) < 1e-9 for p in glob if p["thresh"] != "-inf")
    assert {1, 7, 100} <= {p["max_out"] for p in glob}
    assert {0, 0.25} <= {p["sigma"] for p in glob} and any(abs(p["sigma"] - 0.15) < 1e-6 for p in glob)
    for p in glob:
        if p["sigma"] > 0 and p["iou"] == 1:
            assert p["yardstick"], p
    assert any(p["ref_requeues"] > 0 for p in glob) and any(p["ref_hard_drops"] > 0 for p in glob)
    pc = [p for p in PLAN if p["kind"] == 2]
    assert len(pc) >= 6 and any(p["B"] == 3 for p in pc) and all(p["C"] == 90 for p in pc)
    assert any(p["kind"] == 0 for p in PLAN) and sum(p["kind"] == 3 for p in PLAN) >= 2


@pytest.mark.parametrize("case", CASES)
def test_nms_seg_case(verdicts, plan, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    print(d)
    assert "exception" not in d, d
    if case.startswith("refuse_"):
        assert d["threw_global"] and d["threw_per_class"] and d["ok"], d
        return
    assert d["bad_count"] == 0 and d["bad_index"] == 0 and d["bad_scores"] == 0 and d["bad_boxes"] == 0, d
    assert d["bad_classes"] == 0 and d["inputs_ok"], d
    geom = next(p for p in plan if p["case"] == case)
    assert d["yardstick_run"] == geom["yardstick"] and d["bad_yardstick"] == 0, d
    assert d["ok"], d
