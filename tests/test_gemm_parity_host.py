"""The GEMM kernel parity checker (tests/kernels), host side: what its case table covers, read from
`gemm_parity --plan` (plan_gemm2 / plan_gemm are host code: no GPU needed), and the teeth of its compare
functions, driven by a CPU stand-in GEMM with seeded faults (gemm_teeth)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

# Paths the issue lists that no shape within the caps reaches, with the reason (kernels_gemm.hip):
UNREACHABLE = {
    # g2_pick returns the 128x96 tile above N = 96 only when N % 96 == 0, and the 128x160 tile above
    # N = 160 only when N % 160 == 0; below, one N tile spans N and the resident sweep (gy >= 2) is not
    # taken.  So k_gemm2r on these two tiles never sees a ragged last N tile; 222 and 212 carry that edge.
    "res:413 ragged N": "N % 96 == 0 whenever the 413 tile has two or more N tiles",
    "res:415 ragged N": "N % 160 == 0 whenever the 415 tile has two or more N tiles",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if name == "gemm_parity" and not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/gemm_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", name], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return path


def _lines(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert out and out[-1].get("done") is True, r.stdout[-500:]
    return out[:-1]


@pytest.fixture(scope="module")
def plan():
    return _lines([_binary("gemm_parity"), "--plan"])


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("gemm_teeth")])}


def test_every_case_takes_the_path_it_was_chosen_for(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names)
    wrong = {c["case"]: (c["expect"], c["path"]) for c in plan if c["path"] != c["expect"]}
    assert not wrong, wrong


def test_table_covers_every_planner_path(plan):
    f32 = {c["path"] for c in plan if not c["bf16"]}
    want = {f"g2:{k}" for k in (411, 412, 413, 415, 222, 212, 211, 111)}
    want |= {f"res:{k}" for k in (222, 413, 415, 212)}
    # every tile wsk_pick can return, by the few route (K = 64) and the deep-K route, none forced
    want |= {f"wsk:{t}:{r}" for t in (11, 12, 13, 21, 22) for r in ("few", "deep")}
    want |= {"split", "group", "group_res", "g1", "refuse"}
    assert want <= f32, sorted(want - f32)
    assert not any(c["forced"] for c in plan)
    # both compute types; bf16 on a reduced set of the same families
    bf = {c["path"].split(":")[0] for c in plan if c["bf16"]}
    assert {"g2", "res", "wsk", "split"} <= bf, bf
    by = lambda pred: [c for c in plan if pred(c)]
    assert by(lambda c: c["path"] == "split" and c["sink"] == 1) and by(lambda c: c["path"] == "split" and not c["sink"])
    assert by(lambda c: c["path"] == "split" and c["acc"] and c["bias"])
    assert by(lambda c: c["path"] == "split" and c["bf16"])
    # split-K slices that round up and leave a short last slice
    for c in by(lambda c: c["path"] == "split"):
        assert c["splits"] >= 2 and c["K"] % c["kslice"] != 0 and c["splits"] * c["kslice"] > c["K"], c
    # deep-K wave splits whose K is no multiple of four 16-deep (fp32) / 32-deep (bf16) wave slices
    for c in by(lambda c: c["path"].endswith(":deep")):
        assert c["K"] >= 256 and c["K"] % (128 if c["bf16"] else 64) != 0, c
    for c in by(lambda c: c["path"].endswith(":few")):
        assert c["K"] <= 64, c
    # sinks on every kernel family; the three view modes and activations
    for fam in ("g2", "res", "wsk", "group", "group_res", "g1"):
        sinks = {c["sink"] for c in plan if c["path"].split(":")[0] == fam}
        assert {1, 2} <= sinks, (fam, sinks)
    assert {c["mode"] for c in plan} == {0, 1, 2, 3}
    assert {c["act"] for c in plan} == {0, 1, 2}
    # grouped: three and five (kMaxSeg) members
    assert {c["nseg"] for c in plan if c["path"] in ("group", "group_res")} == {3, 5}
    # N <= 16 at both widths
    assert {c["N"] for c in plan if c["path"] == "g1"} == {8, 16}
    # the SE row scale over images that do not align with any tile, and one row per image
    assert {c["rpi"] for c in plan if c["mode"] == 2} >= {1, 100}
    assert UNREACHABLE  # recorded above, not dropped


def test_table_edges(plan):
    run = [c for c in plan if c["path"] != "refuse"]
    g2 = [c for c in run if c["path"].startswith("g2:")]
    rows = {411: 128, 412: 128, 413: 128, 415: 128, 222: 128, 212: 64, 211: 64, 111: 32}
    tails = {c["M"] % rows[c["key"]] for c in g2}
    assert 0 not in tails and 1 in tails and any(1 < t < 32 for t in tails), tails
    # (the few-row wide-N extras need N % 96 == 0 / N % 160 == 0 to stay on the 413 / 415 tiles)
    assert all(c["N"] % 32 for c in g2 if "_wide_" not in c["case"])
    # few rows under every sink: M <= 2000, where (M + 8) 2^-24 < 1 / (2 M), so a column sum with one row
    # too many or too few fails its bound
    for fam in ("g2", "res", "wsk", "group", "group_res", "g1"):
        small = [c for c in run if c["path"].split(":")[0] == fam and c["sink"] and
                 (c["M"] <= 2000 or c["nseg"])]
        assert small, fam
    assert any(c["N"] % 4 == 2 and not c["sink"] for c in g2)
    assert all(c["N"] % 8 == 4 for c in g2 if c["sink"] == 1)
    for bf, chunk in ((0, 16), (1, 32)):
        ks = {c["K"] for c in g2 if c["bf16"] == bf}
        assert 4 in ks and chunk + 4 in ks and any(k > 2 * chunk and k % chunk for k in ks), (bf, ks)
    assert {(c["bias"], c["acc"]) for c in g2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # resident sweeps: at least two N tiles per run; a ragged last N tile and a short last run where reachable
    cols = {222: 128, 413: 96, 415: 160, 212: 128}
    res = [c for c in run if c["path"].startswith("res:")]
    for c in res:
        assert c["kslice"] >= 2, c  # N tiles per run
    for key in (222, 212):
        assert any(c["N"] % cols[key] for c in res if c["key"] == key), key
    assert any(-(-c["N"] // cols[c["key"]]) % c["kslice"] for c in res)  # the last run is shorter than nper
    # grouped: unequal members, the smallest under one tile
    for c in run:
        if c["nseg"]:
            assert c["path"] in ("group", "group_res")


def test_table_respects_the_caps(plan):
    for c in plan:
        assert c["macs"] <= 1.5e9, c["case"]
        assert c["device_bytes"] < 256e6, c["case"]
    assert sum(c["macs"] for c in plan) < 2e10  # seconds of fp64 host reference on 16 threads


CLEAN = ("clean_se_stat", "clean_bn_relu6_acc", "clean_dgrad_gs", "clean_dgrad_relu6_gs", "clean_bf16",
         "clean_bf16_bn_swish_acc")


def _ok(d, *, but=()):
    bad = []
    for k in ("c_ratio", "sum_ratio", "m2_ratio"):
        if (d[k] <= 1.0) == (k in but):
            bad.append(k)
    for k in ("rows_written", "cnt_ok", "cnt_sum_ok"):
        if d[k] == (k in but):
            bad.append(k)
    if d["c_nonfinite"]:
        bad.append("c_nonfinite")
    return bad


@pytest.mark.parametrize("run", CLEAN)
def test_clean_standin_passes(teeth, run):
    assert not _ok(teeth[run]), teeth[run]


# fault -> the fields that must report it (every other field must stay clean)
FAULTS = {
    "drop_last_quad": ("c_ratio",),
    "no_bias_last_ntile": ("c_ratio",),
    "se_next_image": ("c_ratio",),
    "slice_twice": ("c_ratio",),
    "bf16_quantum": ("c_ratio",),
    "clamped_row": ("sum_ratio", "m2_ratio"),
    "clamped_row_gs": ("sum_ratio", "m2_ratio"),
    # (the fold divides the last partial's sum by the wrong count, so its M2 is off too)
    "cnt_full_tile": ("cnt_sum_ok", "m2_ratio"),
    "part_row_shifted": ("rows_written", "sum_ratio", "m2_ratio"),
    "part_row_shifted_gs": ("rows_written", "sum_ratio", "m2_ratio"),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_reported_in_its_field(teeth, fault):
    assert not _ok(teeth[fault], but=FAULTS[fault]), teeth[fault]
