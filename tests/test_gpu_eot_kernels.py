"""Kernel-level parity of the EOT patch pipeline (kernels_eot.hip) — placement and its compact lists, the
brightness matcher, the banded antialiased resize, the rotate-and-paste compositor with its owner map and mask,
the rotation gradient, the two-stage resize adjoint, the patch gradient and TV — against an fp64 host reference,
stage by stage and case by case.

tests/kernels/eot_parity runs its whole table once, in one child process on one stream, and prints a JSON line
per case; each test below asserts one case's verdict fields.  Every stage after the placement takes its BoxPlace,
lists, spans and tensors from what the device wrote before it, so a stage is judged on its own.  The bounds are
derived ("EOT kernel parity"): a ratio is max(err / bound) over every element and must be <= 1; the
`*_bad` fields count what must match exactly (the placement's integers and lists, the spans' ends, the owner map
outside the decision allowance, the resize against its fp32 restatement bit for bit, buffer tails no kernel
writes); `exact_ok` adds the v1 kernels (PHX_EOT_V1=1) and the owner-null / mask-null launches, bit-equal.  If the
child dies, times out or never prints `done`, every test fails with the last line it printed and nothing more
is started.  Run time measured on the first full run: 2.3 s for the child (1.7 s in the table, fp64 reference
included)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "eot_parity")

pytestmark = pytest.mark.gpu

# the first full run took 2.3 s on an MI355X box (1.7 s for the 26 cases after the runtime's start); the limit,
# the siblings' 30 s, leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "eot_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*ec\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/eot_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "eot_parity"], capture_output=True, text=True)
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
        state["error"] = f"eot_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran."""
    assert len(CASES) == len(set(CASES)) and 20 <= len(CASES) <= 40
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)


@pytest.mark.parametrize("case", CASES)
def test_eot_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    if d["refuse"]:
        # the launcher threw before any launch: canary-filled outputs untouched, inputs as uploaded
        assert d["threw"] and d["untouched"] and d["inputs_ok"], d
        assert d["pass"], d
        return
    assert not d["threw"], d
    assert d["place_ok"] and not d["stopped"], d
    assert d["nonfinite"] == 0, d
    assert d["ratio"] <= 1.0, d
    assert all(v <= 1.0 for k, v in d["fields"].items() if not k.endswith("_bad")), d
    assert all(v == 0 for k, v in d["fields"].items() if k.endswith("_bad")), d
    want = {"img_w", "img_b", "fwd", "inv", "span_ulp", "place_int_bad", "angle_delta_bad", "lists_bad", "span_int_bad"}
    if not d["place_only"]:
        want |= {"ymean", "matched", "resize", "resize_exact_bad", "img_out", "mask", "owner_bad", "drot", "drot_tail_bad",
                 "urows", "dmatched", "urows_tail_bad", "adjoint", "grad", "tv", "loss", "metrics_other_bad"}
    assert set(d["fields"]) == want, d
    assert d["exact_ok"] and d["v1_ok"] and d["variants_ok"], d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["inputs_ok"], d
    assert d["allow_share"] <= 0.01, d
    assert d["pass"], d
