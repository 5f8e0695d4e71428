"""Kernel-level parity of kernels_unet.hip below k_wgrad_fold (the fp64 column reductions with the BN statistics,
BN backward and column-sum finals, k_un_bnact / k_un_bnb_apply, pool + Dropout and its backward, the attention
gate, the output layer with its loss and un_out, k_un_small_dgrad, k_un_add, and the Masker's permutation, crops
and box filter) against an fp64 host reference, case by case.

tests/kernels/unet_parity runs its whole table once, in one child process on one stream, and prints a JSON line
per case; each test below asserts one case's verdict fields.  The bounds are derived ("U-Net kernel
parity"): a ratio is max(err / bound) over every element and must be <= 1; a flag covers what must match bit for
bit (moved or selected values, recorded taps, replayed stores, un_out against un_out_loss).  If the child dies,
times out or never prints `done`, every test fails with the last line it printed and nothing more is started.

Measured on an MI355X: the child runs its 173 cases in 2.4 s (fp64 references included; about 3 s with the runtime's
start).  Device expf 0.761 ulp, tanhf 0.929 ulp (allowances 1.52 and 1.86).  Worst max(err / bound) per family:
BN statistics 0.99, BN backward 1.00 (dbeta 0.9996), column sums 0.99, bnact 0.97, att_s 0.82, att_s_bwd 0.87,
att_t 0.99, att_cat 0.57, output layer 0.82, small_dgrad 0.97; every exact flag true, kink share 0."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
BIN = os.path.join(KERN, "unet_parity")

pytestmark = pytest.mark.gpu

TIMEOUT_S = 30

# the table's case names (tests/golden/unet/cases.txt, held equal to `unet_parity --plan` by
# tests/test_unet_parity_host.py), so collection needs no binary
CASES = open(os.path.join(ROOT, "tests", "golden", "unet", "cases.txt")).read().split()


@pytest.fixture(scope="module")
def verdicts():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/unet_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "unet_parity"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    state = {"cases": {}, "error": None, "head": None}
    try:
        r = subprocess.run([BIN], capture_output=True, text=True, timeout=TIMEOUT_S, cwd=ROOT)
        out, rc = r.stdout, r.returncode
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        rc = "timeout"
    lines = [x for x in out.splitlines() if x.strip()]
    done = False
    for x in lines:
        try:
            d = json.loads(x)
        except ValueError:
            continue
        if "done" in d:
            done = True
        elif "head" in d:
            state["head"] = d
        elif "case" in d and "fatal" not in d:
            state["cases"][d["case"]] = d
    if rc != 0 or not done:
        state["error"] = f"unet_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_matches_the_list(verdicts):
    """The parametrisation below names exactly the cases the binary ran; the library-function allowances are twice
    the measured maxima, at least 1 ulp."""
    assert len(CASES) == len(set(CASES)) and len(CASES) > 150
    assert verdicts["error"] is None, verdicts["error"]
    assert set(verdicts["cases"]) == set(CASES)
    h = verdicts["head"]
    assert h["golden_read"] is True
    assert h["exp_ulp_used"] == pytest.approx(max(1.0, 2 * h["exp_ulp_measured"]), rel=1e-4)
    assert h["tanh_ulp_used"] == pytest.approx(max(1.0, 2 * h["tanh_ulp_measured"]), rel=1e-4)


@pytest.mark.parametrize("case", CASES)
def test_unet_case(verdicts, case):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(case)
    assert d is not None, f"{case}: no verdict line"
    assert d["canary_ok"], d
    assert d["repeat_ok"], d
    assert d["inputs_ok"], d
    assert d["scratch_ok"], d
    if d["refuse"]:
        assert d["threw"] and d["untouched"], d
        assert d["pass"], d
        return
    assert not d["threw"], d
    assert d["nonfinite"] == 0, d
    assert d["ratio"] <= 1.0, d
    assert all(v <= 1.0 for v in d["fields"].values()), d
    assert d["exact_ok"] and all(d["flags"].values()), d
    assert d["kink_share"] <= 0.01, d
    assert d["pass"], d
