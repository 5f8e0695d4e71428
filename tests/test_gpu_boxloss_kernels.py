"""Kernel-level parity of the box-regression term (kernels_boxloss.hip: k_idiou_part / k_idiou_merge / k_idiou_batch
and k_box_scatter) against the fp64 host reference of tests/kernels_boxloss, case by case.

tests/kernels_boxloss/boxloss_parity runs its table once, in one child process on one stream, and prints a JSON line
per case; each test below asserts one case's verdict.  The reference carries a bound with every value, derived from
the operations that produced it (boxloss_check.hpp): every (image, gt) maximum must lie within
its bound, the anchor must be the reference's lowest exact winner and the tie count the reference's, with the margin
that makes this well defined asserted for every (image, gt); the scatter must match the fp64 dense dx = dY W^T of the
reference's sparse dY within the bound its contributions carry, and give identical bytes when launched twice.  If the
child dies, times out or never prints `done`, every test fails with the last line it printed and nothing more is
started."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels_boxloss")
BIN = os.path.join(KERN, "boxloss_parity")

pytestmark = pytest.mark.gpu

TIMEOUT_S = 60  # the run takes about a second


def _binary():
    if not os.path.isfile(BIN):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels_boxloss/boxloss_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return BIN


def _case_names():
    src = open(os.path.join(KERN, "boxloss_check.hpp")).read()
    body = src[src.index("// ---- the table"):src.index("// ---- end of the table")]
    return re.findall(r'^\s*add\("([a-z0-9_]+)"', body, re.M)


CASES = _case_names()


@pytest.fixture(scope="module")
def plan():
    """The case table's geometry from --plan (host code only)."""
    r = subprocess.run([_binary(), "--plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return {d["case"]: d for d in (json.loads(x) for x in r.stdout.splitlines() if x.strip())}


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
        state["error"] = f"boxloss_parity ended with {rc}, done={done}; last line: {lines[-1] if lines else '(none)'}"
    return state


def test_table_covers_what_it_must(plan):
    """A = 3069 (D0 at 128^2: no multiple of the 1024-anchor chunk), 49 104 and 76 725; G = 0, 1, 7 and 100; an image
    without a kept anchor; one kept anchor in the last chunk only; exact ties by the hundred; zero-area and flipped
    gts; B = 1 and 3."""
    assert set(plan) == set(CASES)
    P = list(plan.values())
    assert {3069, 49104, 76725} <= {d["A"] for d in P}
    assert all(d["A"] % d["chunk"] for d in P if d["A"] in (3069, 76725))
    assert {0, 1, 7, 100} <= {g for d in P for g in d["G"]}
    assert {1, 3} <= {d["B"] for d in P}
    assert any(d["images_without_kept"] > 0 and d["kept"] > 0 for d in P)
    last = [d for d in P if d["kept"] == 1 and d["kept_in_last_chunk"] == 1]
    assert {d["A"] for d in last} >= {3069, 76725} and all(d["chunks"] > 1 for d in last)
    assert any(d["max_ties"] >= 100 for d in P)
    assert any(d["degenerate_gts"] > 0 for d in P)
    assert len({d["K"] for d in P}) > 1


@pytest.mark.parametrize("name", CASES)
def test_case(verdicts, name):
    assert verdicts["error"] is None, verdicts["error"]
    d = verdicts["cases"].get(name)
    assert d is not None, f"no verdict for {name}"
    print(json.dumps(d))
    assert "exception" not in d, d
    assert d["margin_fail"] == 0, d          # the generator's margin, asserted for every (image, gt)
    assert d["bad_max"] == 0 and d["bad_anchor"] == 0 and d["bad_nties"] == 0 and d["bad_pad"] == 0, d
    assert d["bad_image"] == 0 and not d["bad_batch"] and not d["bad_loss"], d
    assert d["scatter_same_bytes"] is True, d
    assert d["bad_dx"] == 0 and d["stray_dx"] == 0, d
    assert d["ok"] is True, d


def test_scatter_checks_are_not_vacuous(verdicts, plan):
    """Every case with a kept anchor and a gt scatters into some rows, with a gradient of some size."""
    assert verdicts["error"] is None, verdicts["error"]
    for name, d in verdicts["cases"].items():
        if plan[name]["kept"] and max(plan[name]["G"]):
            assert d["dx_rows"] > 0 and d["dx_ref_norm"] > 0, d
