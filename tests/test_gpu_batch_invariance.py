"""Kernel-level batch invariance of the inference forward's launchers: launch_se_fwd (pool, hidden, scale),
launch_gemm forward (BN view, and the SE row scale whose rows_per_img makes an image's position index an
operand), gemm_group_run, launch_sep_fwd (single and grouped), launch_dw_fwd and launch_dw_fwd_fused.

tests/kernels/batch_invariance runs its whole table once, in one child process on one stream, and prints a JSON
line per case; each test below asserts one case's verdict.  A case draws Bmax seeded images and one set of
weights, runs the product's launcher under gemm_plan_images() = B (as a batch-invariant forward does) on the
first B images for every B of its list, once on the largest batch in reversed image order, and on every image
alone; image p's slice of every output must be the same bytes in all of them.  There is no reference and no
tolerance: diff_words counts 32-bit words that differ and must be 0; first_diff names output, batch size, image
and index.  canary_ok: guard regions, the rows past the launch's images and the scratch guards untouched;
inputs_ok: inputs and weights as uploaded afterwards; repeat_ok: the largest batch run twice gives the same bytes.
tests/test_batch_invariance_host.py holds the table to the classes it is meant to cover (host only).  If the
child dies, times out or never prints `done`, every test fails with the last line it printed and nothing more is
started.

Before se_plan was planned per image every launch_se_fwd case failed here, from the first batch size at which its
slicing moved (hidden and scale: 2,780 to 17,302 differing words per case, first_diff e.g. hidden:B8:0:0 for D0's
1152 channels and hidden:B4:0:3 for D4's 2688; pool always equal); every other case passed then as now (DESIGN.md
section 15, "Batch size").
Run time measured on an MI355X: 0.62 s for the 22 cases (1.0 s for this module with the child's start); the largest
are gemm_deepk_flip (101 ms: 17 MB of C) and gemm_res (92 ms: 35 MB of C), then the two fused depthwise cases past
the switch (24 and 34 ms)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "batch_invariance")

pytestmark = pytest.mark.gpu

# the siblings' limit; it leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "batch_invariance.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*bc\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/batch_invariance is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "batch_invariance"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    state = {"cases": {}, "error": None, "done": None}
    try:
        r = subprocess.run([BIN], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
        out, rc = r.stdout, r.returncode
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        rc = "timeout"
    lines = [x for x in out.splitlines() if x.strip()]
    for x in lines:
        d = json.loads(x)
        if "done" in d:
            state["done"] = d
        elif "case" in d and "fatal" not in d:
            state["cases"][d["case"]] = d
    if rc != 0 or state["done"] is None:
        state["error"] = f"batch_invariance ended with {rc}, done={state['done'] is not None}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran."""
    assert len(CASES) == len(set(CASES)) and 15 <= len(CASES) <= 30
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)
    done = verdicts["done"]
    slow = sorted(verdicts["cases"].values(), key=lambda d: -d["ms"])[:3]
    print(f"batch_invariance: {done['seconds']} s for {done['cases']} cases; slowest: " +
          ", ".join(f"{d['case']} {d['ms']:.0f} ms" for d in slow))
    assert done["cases"] == len(CASES)


@pytest.mark.parametrize("case", CASES)
def test_batch_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    print({k: v for k, v in d.items() if k != "plans"})
    assert not d["threw"], d["what"]
    # every batch size, the repeat, the reversed order and every image alone
    assert d["runs"] == len(d["Bs"]) + d["Bs"][-1] + 2, d["runs"]
    assert d["diff_words"] == 0, (d["diff_words"], d["first_diff"])
    assert d["canary_ok"], d
    assert d["inputs_ok"], d
    assert d["repeat_ok"], d
    assert d["pass"], d
