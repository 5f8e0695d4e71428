"""Kernel-level parity of the squeeze-excite backward whose input gradient is formed on load by the
depthwise dgrad (launch_se_bwd_sums, launch_dw_bwd_se, launch_se_da) against an fp64 host reference and,
bit for bit, against the launchers they stand in for, case by case.

tests/kernels_sefold/sefold_parity runs its table once, in one child process on one stream, and prints a
JSON line per case; each test below asserts one case's verdict.  The bounds are the derived ones of
DESIGN.md ("Norm kernel parity", "Conv kernel parity"): a ratio is max(err / bound) over every element
and must be <= 1; a field that ends in _bits is 0 where two buffers are byte-identical.  If the child dies,
times out or never prints `done`, every test fails with the last line it printed and nothing more is
started."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels_sefold")
BIN = os.path.join(KERN, "sefold_parity")

pytestmark = pytest.mark.gpu

TIMEOUT_S = 30  # the run takes about a second


def _case_names():
    src = open(os.path.join(KERN, "sefold_parity.cpp")).read()
    body = src[src.index("// ---- the table"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*run_(?:sums|dw|chain|refuse)\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels_sefold/sefold_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    state = {"cases": {}, "error": None, "head": None}
    env = {k: v for k, v in os.environ.items() if not k.startswith("PHX_RED_")}  # the table is for the defaults
    try:
        r = subprocess.run([BIN], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT, env=env)
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
        elif "knobs_unset" in d:
            state["head"] = d
        elif "case" in d and "fatal" not in d:
            state["cases"][d["case"]] = d
    if rc != 0 or not done:
        state["error"] = f"sefold_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    assert len(CASES) == len(set(CASES)) and len(CASES) >= 13
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)
    assert verdicts["head"] == {"knobs_unset": True, "red_depth": 8}


@pytest.mark.parametrize("case", CASES)
def test_sefold_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    print(d)
    if d["refuse"]:
        assert d["threw"] and d["untouched"], d
        assert d["pass"], d
        return
    assert not d["threw"], d
    assert d["nonfinite"] == 0, d
    assert d["fields"] and all(v <= 1.0 for v in d["fields"].values()), d
    assert d["ratio"] <= 1.0, d
    assert d["guards_ok"] and d["slot_ok"], d
    if d["has_sink"]:
        assert d["rows_written"] and d["sum_ratio"] <= 1.0 and d["m2_ratio"] <= 1.0, d
    assert d["pass"], d
