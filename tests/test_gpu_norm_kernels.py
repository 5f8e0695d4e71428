"""Kernel-level parity of kernels_norm.hip (BN statistics, finalizes and backward reductions, the bn=sync sum
halves, squeeze-excite, residual add / gradient copy with their GradSink, max-pool, nearest upsample, the BiFPN
fuse and the small elementwise launchers) against an fp64 host reference, case by case.

tests/kernels/norm_parity runs its whole table once, in one child process on one stream, and prints a
JSON line per case; each test below asserts one case's verdict fields.  The bounds are derived (DESIGN.md,
"Norm kernel parity"): a ratio is max(err / bound) over every element and must be <= 1; `exact_ok` covers
what must match bit for bit (selected or moved values, recorded taps, replayed gathers).  If the child
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
BIN = os.path.join(KERN, "norm_parity")

pytestmark = pytest.mark.gpu

# the run takes about 1.2 s on an MI355X box (0.7 - 0.8 s for the 251 cases, fp64 host reference included, after
# the runtime's start); the limit leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "norm_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*(?:red|fin|se|pool|ups|ew|misc|fuse|ref)\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/norm_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "norm_parity"], capture_output=True, text=True)
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
        state["error"] = f"norm_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran, with the reduction knobs unset."""
    assert len(CASES) == len(set(CASES)) and len(CASES) > 200
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)
    assert verdicts["head"] == {"knobs_unset": True, "red_depth": 8}


@pytest.mark.parametrize("case", CASES)
def test_norm_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    if d["refuse"]:
        assert d["threw"] and d["untouched"], d
        assert d["pass"], d
        return
    assert not d["threw"], d
    assert d["nonfinite"] == 0, d
    assert d["ratio"] <= 1.0, d
    assert all(v <= 1.0 for k, v in d["fields"].items() if not k.endswith(("_exact", "_bad"))), d
    assert d["exact_ok"], d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["inputs_ok"], d
    assert d["kink_share"] <= 0.01, d
    if d["has_sink"]:
        assert d["P_ok"] and d["P_got"] == d["P_expected"], d
        assert d["rows_written"], d
        assert d["sum_ratio"] <= 1.0 and d["m2_ratio"] <= 1.0, d
    assert d["pass"], d
