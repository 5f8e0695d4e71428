"""Kernel-level parity of the 1x1-conv GEMM family (k_gemm2, k_gemm2r, k_gemm2k, split-K and its reduce,
the grouped launch, the 16x16x4 kernel) against an fp64 host reference, case by case.

tests/kernels/gemm_parity runs its whole table once, in one child process on one stream, and prints a
JSON line per case; each test below asserts one case's verdict fields.  The bounds are derived (DESIGN.md,
"GEMM kernel parity"): a ratio is max(err / bound) and must be <= 1.  If the child dies, times out or
never prints `done`, every test fails with the last line it printed and nothing more is started."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "gemm_parity")

pytestmark = pytest.mark.gpu

# the run takes about 6 s on an MI355X box (fp64 host reference included); the limit leaves room for a slow host
TIMEOUT_S = 120


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    import re
    src = open(os.path.join(KERN, "gemm_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- the planner's choice")]
    return re.findall(r'(?:add|grp)\("([a-z0-9_]+)"|Case(?: c)?\{"([a-z0-9_]+)"', body)


CASES = [a or b for a, b in _case_names()]


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/gemm_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "gemm_parity"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    state = {"cases": {}, "error": None}
    try:
        r = subprocess.run([BIN], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
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
        state["error"] = f"gemm_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran."""
    assert len(CASES) == len(set(CASES)) and len(CASES) > 60
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_gemm_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    if d["path"] == "refuse":
        assert d["threw"] and d["untouched"], d
        return
    assert not d["threw"], d
    assert d["c_nonfinite"] == 0, d
    assert d["c_ratio"] <= 1.0, d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    if d["sink"]:
        assert d["P_ok"] and d["P"] == d["P_expected"], d
        assert d["rows_written"], d
        assert d["sum_ratio"] <= 1.0 and d["m2_ratio"] <= 1.0, d
        if d["sink"] == 1:
            assert d["cnt_ok"] and d["cnt_sum_ok"], d
    assert d["pass"], d
