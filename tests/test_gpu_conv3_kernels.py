"""Kernel-level parity of the dense 3x3 convolutions — the stem (k_stem_fwd, k_stem_bwd, k_stem_bwd_gx), the GEMM
over an implicitly gathered column matrix (launch_gemm_gather) and the U-Net's un_im2col, un_wprep, un_conv3_small
and un_wgrad — against an fp64 host reference, case by case.

tests/kernels/conv3_parity runs its whole table once, in one child process on one stream, and prints a JSON
line per case; each test below asserts one case's verdict fields.  The bounds are derived ("Dense 3x3
conv kernel parity"): a ratio is max(err / bound) over every element and must be <= 1; `exact_ok` covers what
must match bit for bit (the column matrix, the prepared weight matrices, the dead tiles of the stem's data
gradient, the gather GEMM against the explicit one).  The stem data gradient's contract is per 32 x 32-pixel
tile: a tile without an owned element is +0.0 everywhere, a tile with one holds the full gradient.  If the
child dies, times out or never prints `done`, every test fails with the last line it printed and nothing more
is started.  Run time measured on the first full run: 0.53 s for the child (0.48 s in the table)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "conv3_parity")

pytestmark = pytest.mark.gpu

# the first full run took 0.53 s on an MI355X box (0.48 s for the 146 cases, fp64 host reference included, after
# the runtime's start); the limit, the siblings' 30 s, leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "conv3_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*(?:sf|sb|gx|ic|wp|cv|gg|wg|ref)\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/conv3_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "conv3_parity"], capture_output=True, text=True)
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
        state["error"] = f"conv3_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran."""
    assert len(CASES) == len(set(CASES)) and 120 <= len(CASES) <= 160
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_conv3_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    if d["refuse"]:
        # threw, or returned false (un_conv3_small), with nothing launched
        assert d["refused"] and d["untouched"] and d["inputs_ok"] and d["agree_ok"], d
        assert d["threw"] == (d["op"] != "conv3"), d
        assert d["pass"], d
        return
    assert not d["threw"] and not d["refused"], d
    assert d["nonfinite"] == 0, d
    assert d["ratio"] <= 1.0, d
    assert all(v <= 1.0 for k, v in d["fields"].items() if not k.endswith("_bad")), d
    assert all(v == 0 for k, v in d["fields"].items() if k.endswith("_bad")), d
    assert d["exact_ok"], d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["inputs_ok"], d
    assert d["agree_ok"], d
    assert d["kink_share"] <= 0.01, d
    if d["op"] == "stem_fwd":
        assert d["P_ok"] and d["P_got"] == d["P_expected"], d
    if d["has_sink"]:
        assert d["rows_written"] and d["cnt_ok"] and d["cnt_sum_ok"], d
        assert d["sum_ratio"] <= 1.0 and d["m2_ratio"] <= 1.0, d
    assert d["pass"], d
