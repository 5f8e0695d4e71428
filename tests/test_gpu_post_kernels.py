"""Kernel-level parity of the post-processing and attack-loss kernels (kernels_post.hip and k_adam) — pre_nms with
its validity filter and candidate lists, soft-NMS, count_ge, the per-image max, the loss, zero_segs, the sparse
class-head backward and Adam — against an exact or fp64 host reference, stage by stage and case by case.

tests/kernels/post_parity runs its whole table once, in one child process on one stream, and prints a JSON line
per case; each test below asserts one case's verdict fields.  A chain case runs every stage on what the device
wrote in the stages before, so a stage is judged on its own.  The bounds are derived ("Post-processing
kernel parity"): a ratio is max(err / bound) over every element and must be <= 1; the `*_bad` fields count what
must match exactly (classes, keep bits outside the decision allowance, the candidate lists as sets, soft-NMS's
selected indices, counts and clipped boxes, the per-image max, the loss, count_ge and zero_segs against their fp32
restatement bit for bit, rows no kernel writes, soft-NMS with out_index null, with PHX_NMS_FAST=0 and over a
shuffled list).  `dx_exact_bad` and `adam_exact_bad` were 0 on the first GPU run and are asserted.  If the child
dies, times out or never prints `done`, every test fails with the last line it printed and nothing more is started.
Run time measured on the first full run: 0.4 s for the 35 cases, fp64 references included (0.8 s for this module
with the child's start); the largest cases are Adam over the patch (79 ms) and soft-NMS at N = 262,208 (39 ms)."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "post_parity")

pytestmark = pytest.mark.gpu

# the siblings' limit; it leaves room for a slow host
TIMEOUT_S = 30


def _case_names():
    """The table's case names, read from the source so collection needs no binary."""
    src = open(os.path.join(KERN, "post_parity.cpp")).read()
    body = src[src.index("static std::vector<Case> table()"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*pc\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()

PRE = {"cls_bad", "score", "box", "keep_bad", "list_bad"}
NMS = {"nms_index_bad", "nms_count_bad", "nms_box_bad", "nms_score", "nms_tail_bad", "nms_reset_bad", "nms_variant_bad"}
LOSS = {"loss", "loss_exact_bad", "metrics_other_bad"}
FIELDS = {
    "chain": PRE | NMS | LOSS | {"count_ge_exact_bad", "imax_exact_bad", "zero_bad", "dx", "dx_exact_bad", "dx_untouched_bad"},
    "nms": NMS,
    "imax": {"imax_exact_bad"} | LOSS,
    "loss": LOSS,
    "zero": {"zero_bad"},
    "count": {"count_ge_exact_bad"},
    "adam": {"adam", "adam_exact_bad"},
}


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/post_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "post_parity"], capture_output=True, text=True)
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
        state["error"] = f"post_parity ended with {rc}, done={state['done'] is not None}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_source(verdicts):
    """The parametrisation below names exactly the cases the binary ran; the expf figure is a sane one."""
    assert len(CASES) == len(set(CASES)) and 25 <= len(CASES) <= 35
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)
    done = verdicts["done"]
    print(f"post_parity: {done['seconds']} s, expf measured {done['exp_ulp_measured']} ulp, used {done['exp_ulp_used']}")
    # twice the measured error of the device's expf, at least 1 ulp; a library off by more than 2 ulp is a finding
    assert done["exp_ulp_used"] == pytest.approx(max(1.0, 2 * done["exp_ulp_measured"]), rel=1e-4) and done["exp_ulp_measured"] <= 2.0, done


@pytest.mark.parametrize("case", CASES)
def test_post_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    print(d)
    if d["refuse"]:
        # the launcher threw before any launch: canary-filled outputs untouched, inputs as uploaded
        assert d["threw"] and d["untouched"] and d["inputs_ok"], d
        assert d["pass"], d
        return
    assert not d["threw"], d
    assert not d["stopped"], d
    assert all(v <= 1.0 for k, v in d["fields"].items() if not k.endswith("_bad")), d
    assert all(v == 0 for k, v in d["fields"].items() if k.endswith("_bad")), d
    assert set(d["fields"]) == FIELDS[d["kind"]], d
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["inputs_ok"], d
    assert d["allow_share"] <= 0.01, d
    assert d["pass"], d
