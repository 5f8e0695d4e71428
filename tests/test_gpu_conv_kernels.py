"""Kernel-level parity of the depthwise convs (k_dw_fwd, k_dw_bwd: 3x3 / 5x5, stride 1 / 2, grouped, with
the BiFPN fuse view) and the fused separable conv (k_sep_fwd, k_sep_bwd) against an fp64 host reference,
case by case.

tests/kernels/conv_parity runs its whole table once, in one child process on one stream, and prints a
JSON line per case; each test below asserts one case's verdict fields.  The bounds are derived (DESIGN.md,
"Conv kernel parity"): a ratio is max(err / bound) over every element and must be <= 1.  If the child
dies, times out or never prints `done`, every test fails with the last line it printed and nothing more
is started."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "conv_parity")

pytestmark = pytest.mark.gpu

# the run takes about 1.2 s on an MI355X box (0.6 s for the 182 cases, fp64 host reference included, after the
# runtime's start); the limit leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "conv_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'\b(?:fwd|bwd|fus|grp|sepf|sepb|ref)\("([a-z0-9_]+)"', body)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/conv_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "conv_parity"], capture_output=True, text=True)
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
        state["error"] = f"conv_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran."""
    assert len(CASES) == len(set(CASES)) and len(CASES) > 150
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_conv_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    if d["refuse"]:
        assert d["threw"] and d["untouched"], d
        return
    assert not d["threw"], d
    assert d["c_nonfinite"] == 0, d
    assert d["c_ratio"] <= 1.0, d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["kink_share"] <= 0.01, d
    if d["sink"]:
        assert d["P_ok"] and d["P"] == d["P_expected"], d
        assert d["rows_written"], d
        assert d["sum_ratio"] <= 1.0 and d["m2_ratio"] <= 1.0, d
        if d["sink"] == 1:
            assert d["cnt_ok"] and d["cnt_sum_ok"], d
    assert d["pass"], d
