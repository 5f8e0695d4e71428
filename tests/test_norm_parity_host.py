"""The norm kernel parity checker (tests/kernels/norm_parity), host side: what its case table covers, read
from `norm_parity --plan` (the column reductions' geometry, the SE plan and the partial counts come from the
library's own planners through red_plan_info / se_plan_info: no GPU needed), the golden keep flags against
oracle/philox.py, and the teeth of its reference and compare functions, driven by a CPU stand-in with
seeded faults (norm_teeth)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

# tensors of a case stay within a few MB ...
CAP_BYTES = 4 << 20
# ... except where the edge needs more to exist at all (each below 8 MiB):
OVER_CAP = {
    # k_se_squeeze's one-lane-per-channel fold (slices above 128 channels) needs B >= 64 at C = 1152, and its
    # 4-deep body 4 chunks of 16 rows on top: 64 x 49 x 1152 elements, bf16 to halve them
    "sef_c1152_n48_b64_hw49_bf",
    # the 8-deep body of the lane-group fold needs more than 7 * 8 chunks of 80 rows at tpr 24; the backward
    # holds dy and dx beside x
    "seb_c96_n4_b1_hw9121",
    # the one D4-wide pair at B = 4 with GradSink and accumulation: x, dy, dx, prev of 4 x 49 x 2688
    "seb_c2688_n112_b4_hw49_gs_acc",
}

# Edges the issue lists that the default PHX_RED_* knobs do not reach, with the reason (kernels_norm.hip: red_plan):
UNREACHABLE = {
    # A whole-tensor reduction (nseg = 1) aims for 1024 chunks and never gives a chunk fewer than 8 rows per
    # lane, so a lane sees more than 8 rows only once M > 8 * 1024 * rpi / cgroups: at least 8 * 1024 * 129 * 4
    # / 3 elements (rpi * tpr >= 129 for every C) = 1.4 M elements for three channel groups and 4.2 M (17 MB)
    # for one.  Below that a lane's rows are the 8-deep body exactly once, or the scalar tail alone.  The row
    # past the body is reached through the per-image reductions instead (16 rows per lane at least: the SE
    # pools, sef_c32_n8_b16_hw288 with 9 rows per lane), and k_ew_gstats's 4-deep body + tail by the gradient
    # copies with 5 and 6 rows per lane.
    "BN reductions: one row past the 8-deep body": "needs M > 8192 * rpi / cgroups rows, > 17 MB at one channel group",
    # 64 rows per lane need rpc = 64 * rpi, i.e. M >= 64 * rpi * 1024 / cgroups rows: >= 33.8 M elements (135 MB).
    # Per-image reductions reach it no sooner (B * HW * C >= 17 M elements).  The fp32 run therefore always
    # holds fewer than 64 rows with the default knobs; PHX_RED_BLOCKS=1 would reach it, and the harness runs
    # with the knobs unset.
    "exactly 64 and 65 rows per lane (the fp32 run's boundary)": "needs >= 135 MB of input with the default knobs",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if name == "norm_parity" and not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/norm_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", name], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return path


def _lines(cmd):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PHX_RED_")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert out and out[-1].get("done") is True, r.stdout[-500:]
    return out[:-1]


@pytest.fixture(scope="module")
def plan():
    out = _lines([_binary("norm_parity"), "--plan"])
    assert out[0] == {"knobs_unset": True, "red_depth": 8}
    return out[1:]


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("norm_teeth")])}


def _op(plan, *ops):
    return [c for c in plan if c["op"] in ops]


def test_names_are_unique_and_the_table_is_the_source(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names) and 200 < len(names) < 300
    from test_gpu_norm_kernels import CASES
    assert CASES == names


def test_column_reduction_coverage(plan):
    widths = {4: 1, 8: 2, 40: 10, 144: 36, 240: 60, 672: 168, 1152: 256, 2688: 256}
    for op in ("bn_stats", "bn_bwd_reduce"):
        cs = _op(plan, op)
        assert {c["C"]: c["red"]["tpr"] for c in cs} == widths, op
        assert {(c["red"]["cgroups"], c["red"]["tpr_last"]) for c in cs if c["C"] >= 1152} == {(2, 32), (3, 160)}
        # lanes beyond rpi * tpr idle: 4 of them at tpr 36, 16 at 60, 88 at 168
        assert {c["red"]["tpr"]: c["red"]["idle"] for c in cs if c["red"]["idle"]} == {10: 6, 36: 4, 60: 16, 168: 88}
        assert {c["red"]["tpr"]: c["red"]["rpi"] for c in cs} == {1: 256, 2: 128, 10: 25, 36: 7, 60: 4, 168: 1, 256: 1}
        reds = [c["red"] for c in cs]
        assert any(r["rows"] == 1 for r in reds)
        assert any(1 < r["rows"] < r["rpi"] for r in reds)                      # fewer rows than lanes per pass
        assert any(r["rpi"] > 2 and r["rows"] % r["rpi"] == 1 for r in reds)    # rpi k + 1
        assert any(r["rpi"] > 2 and r["rows"] % r["rpi"] == r["rpi"] - 1 for r in reds)  # rpi k - 1
        assert any(r["chunks"] > 1 and r["last_chunk_rows"] < r["rpc"] for r in reds)    # a short last chunk
        assert any(r["chunks"] > 1 and r["last_chunk_rows"] == r["rpc"] for r in reds)   # and a full one
        assert {1, 16, 17, 49} <= {r["chunks"] for r in reds} and max(r["chunks"] for r in reds) >= 65, op
        assert any(r["lane_rows"] == 8 for r in reds) and any(r["lane_rows"] == 7 for r in reds)
        assert {c["bf"] for c in cs} == {0, 1}
        # UNREACHABLE: no whole-tensor case gets past the 8-deep body, none near a 64-row run
        assert max(r["lane_rows"] for r in reds) == 8
    assert {c["flav"] for c in _op(plan, "bn_stats")} == {0, 1, 2}      # no moving stats, moving, side pairs
    assert {c["act"] for c in _op(plan, "bn_bwd_reduce")} == {0, 1, 2}
    for op in ("bn_stats_sums", "bn_bwd_reduce_sums", "bn_bwd"):
        cs = _op(plan, op)
        assert {c["red"]["cgroups"] for c in cs} >= {1, 2} and len({c["red"]["tpr"] for c in cs}) >= 4, op
    bb = _op(plan, "bn_bwd")
    assert {c["flav"] for c in bb} == {0, 1} and {c["acc"] for c in bb} == {0, 1} and {c["act"] for c in bb} == {0, 1, 2}
    # the row past a D-deep body: D = 8 through the SE pools, D = 4 through the gradient copies' GradSink
    assert any(c["red"]["lane_rows"] == 9 for c in _op(plan, "se_fwd", "se_bwd"))
    assert {5, 6} <= {c["red"]["lane_rows"] for c in _op(plan, "copy_grad", "grad_sums") if c["sink"]}
    assert all(c["red"]["lane_rows"] < 64 for c in plan if "red" in c)
    # the scratch holds the chunk partials and the tail exactly
    for c in plan:
        if "red" in c:
            r = c["red"]
            assert r["scratch_doubles"] == 2 * r["nseg"] * c["C"] * (r["chunks"] + 1), c["case"]
    assert len(UNREACHABLE) == 2


def test_finalize_coverage(plan):
    for op in ("bn_finalize", "bn_bwd_finalize"):
        cs = _op(plan, op)
        one = {c["members"][0]["P"] for c in cs if c["B"] == 1}
        assert {1, 2, 255, 256, 257, 768, 769, 1024, 1025} <= one and any(1700 <= p <= 1900 for p in one), op
        assert {c["B"] for c in cs} == {1, 2, 5}
        for c in cs:
            if c["B"] > 1:
                assert len({m["P"] for m in c["members"]}) == c["B"] and len({m["M"] for m in c["members"]}) == c["B"]
    fw = _op(plan, "bn_finalize")
    assert any(m["zero_cnt"] > 0 for c in fw for m in c["members"]) and any(c["flav"] & 2 for c in fw)
    assert any(c["members"][0]["zero_cnt"] > 0 and c["members"][0]["P"] > 1024 for c in fw)
    fold = _op(plan, "bn_fold_from_sums")
    assert {c["members"][0]["P"] for c in fold} >= {1, 257, 1025} and any(c["flav"] & 1 for c in fold)
    assert {c["flav"] for c in _op(plan, "bn_moving_apply")} == {0, 1}  # one and two passes
    assert len(_op(plan, "bn_frozen_stats")) >= 2


def test_squeeze_excite_coverage(plan):
    d0 = {(32, 8), (96, 4), (144, 6), (240, 10), (480, 20), (672, 28), (1152, 48)}
    for op in ("se_fwd", "se_bwd"):
        cs = _op(plan, op)
        assert {(c["C"], c["N"]) for c in cs} >= d0 | {(2688, 112)}, op
        assert any((c["C"], c["N"], c["B"]) == (2688, 112, 4) for c in cs)
        assert {1, 2, 3, 16} <= {c["B"] for c in cs}
        assert any(c["B"] >= 256 and c["se"]["s1"] == 1 for c in cs)
        assert {1, 4, 49} <= {c["M"] for c in cs}
        # both fold branches, each with its unrolled body (fold_deep) and without
        assert {(c["se"]["fold_small"], c["se"]["fold_deep"]) for c in cs} >= {(1, 0), (1, 1), (0, 0)}, op
        assert {c["se"]["kg"] for c in cs} >= {1, 2, 4, 7, 8}
        assert {c["se"]["jg"] for c in cs} >= {1, 7, 8}
        assert any(c["se"]["cs2"] >= 256 for c in cs) and any(128 < c["se"]["cs2"] < 256 for c in cs)
        assert {c["view"] for c in cs} == {0, 1, 2} and {c["bf"] for c in cs} == {0, 1}
        # the shares fit the scratch tail that colred_scratch_doubles reserves (s1 * Cse <= 4 C)
        assert all(c["se"]["shares_floats"] <= c["se"]["tail_floats"] for c in cs)
        assert any(c["red"]["cgroups"] == 3 for c in cs) and any(c["red"]["idle"] == 88 for c in cs)
    assert (0, 1) in {(c["se"]["fold_small"], c["se"]["fold_deep"]) for c in _op(plan, "se_fwd")}
    bw = _op(plan, "se_bwd")
    assert {(c["acc"], c["sink"]) for c in bw} == {(0, 0), (0, 2), (1, 0), (1, 2)}
    for c in bw:
        if c["sink"]:
            assert c["P_expected"] == c["B"] * c["red"]["chunks"], c["case"]


def test_resampling_and_fuse_coverage(plan):
    mp = _op(plan, "maxpool")
    assert {c["C"] for c in mp} == {3, 4, 6, 64} and {c["pool"]["quad"] for c in mp} == {0, 1}
    for quad in (0, 1):
        cs = [c for c in mp if c["pool"]["quad"] == quad]
        assert {(1, 1), (2, 2), (8, 8), (9, 7)} <= {(c["H"], c["W"]) for c in cs}
        assert {c["flav"] for c in cs} == {0, 1, 2, 3} and {c["k"] for c in cs} == {2, 3}
        assert {c["bf"] for c in cs} == {0, 1} and {c["acc"] for c in cs} == {0, 1}
    for c in mp:  # TF SAME
        for n, o, p in ((c["H"], c["pool"]["Ho"], c["pool"]["pt"]), (c["W"], c["pool"]["Wo"], c["pool"]["pl"])):
            assert o == -(-n // c["s"]) and p == max((o - 1) * c["s"] + c["k"] - n, 0) // 2, c["case"]
    up = _op(plan, "upsample")
    for quad in (0, 1):
        cs = [c for c in up if c["ups"]["quad"] == quad]
        assert {(c["H"], c["Ho"]) for c in cs} >= {(1, 2), (5, 10), (3, 5), (2, 3), (7, 10), (8, 8)}
        assert {c["bf"] for c in cs} == {0, 1} and {c["acc"] for c in cs} == {0, 1}
        assert {c["ups"]["max_fan"] for c in cs} >= {1, 2}
    assert {c["view"] for c in up} == {0, 1, 2}
    for op in ("fuse_fwd", "fuse_bwd"):
        cs = _op(plan, op)
        assert {(c["N"], c["k"]) for c in cs} == {(2, 0), (2, 1), (3, 0), (3, 1)}, op
        assert {c["flav"] for c in cs} == {0, 1, 2, 3}   # positive, one negative, one zero, all zero
        assert {c["C"] % 4 == 0 for c in cs} == {False, True} and {c["bf"] for c in cs} == {0, 1}
        assert {c["act"] for c in cs} == {1, 2}
    fb = _op(plan, "fuse_bwd")
    assert any(c["P"] != (1 << c["N"]) - 1 for c in fb)                       # an input that takes no gradient
    assert any(0 < c["s"] < (1 << c["N"]) - 1 for c in fb)                   # mixed accumulation


def test_elementwise_coverage(plan):
    for op in ("add", "copy_grad"):
        cs = _op(plan, op)
        assert {c["drop"] for c in cs} == {0, 1, 2, 3}, op   # off, p = 1, 0.8, small
        assert {c["C"] for c in cs} >= {4, 40, 144, 672}
    assert {c["bf"] for c in _op(plan, "add")} == {0, 1} and {c["view"] for c in _op(plan, "add")} == {0, 1, 2}
    cg = _op(plan, "copy_grad")
    assert {(c["acc"], bool(c["sink"])) for c in cg} == {(0, False), (0, True), (1, False), (1, True)}
    # drop connect on the GradSink path: images that do not divide a chunk, a kept / dropped boundary inside
    # one lane's run of rows
    assert any(c["sink"] and c["drop"] and c["M"] % c["red"]["rpi"] and c["red"]["lane_rows"] > 1 and
               c["M"] < c["red"]["last_chunk_rows"] for c in cg)
    assert {c["red"]["cgroups"] for c in cg if c["sink"]} == {1, 2, 3}
    assert any(c["red"]["chunks"] > 1 for c in _op(plan, "grad_sums"))
    a2 = _op(plan, "bn_bwd_apply2")
    assert {c["bf"] for c in a2} == {0, 1} and any(c["flav"] == 1 for c in a2)  # fp32 / bf16 y, pass-through
    ck = _op(plan, "cksum")
    assert min(c["M"] for c in ck) < 256 and max(c["M"] for c in ck) > 2048 * 256  # one workgroup .. the capped grid
    assert _op(plan, "bn_apply") and _op(plan, "bf16_to_f32") and _op(plan, "drop_keep")


def test_refusals_and_caps(plan):
    assert {c["refuse"] for c in plan if c["refuse"]} == set(range(1, 18))
    for c in plan:
        if c["case"] in OVER_CAP:
            assert CAP_BYTES < c["bytes"] <= 2 * CAP_BYTES, c["case"]
        else:
            assert c["bytes"] <= CAP_BYTES, c["case"]
        # no more than 1 % of the elements under a kink or tie allowance, by the fp64 reference alone
        assert c["kink_share"] <= 0.01, c["case"]
    assert sum(c["bytes"] for c in plan) < 120e6


def test_golden_keep_flags_are_the_oracles():
    """tests/golden/norm/drop_keep.txt holds floor(p + U) with U drawn by oracle/philox.py."""
    import sys
    sys.path.insert(0, ROOT)
    from oracle import philox
    tok = open(os.path.join(ROOT, "tests", "golden", "norm", "drop_keep.txt")).read().split()
    seed, step, gimg0, pas, nd, B = int(tok[0], 16), int(tok[1]), int(tok[2]), int(tok[3]), int(tok[4]), int(tok[5])
    blocks = [int(x) for x in tok[6:6 + nd]]
    ps = np.array([int(x, 16) for x in tok[6 + nd:6 + 2 * nd]], np.uint32).view(np.float32)
    keep = np.array([int(x) for x in tok[6 + 2 * nd:]], np.float32).reshape(nd, B)
    assert ps[0] == 1.0 and np.float32(0.8) in ps and ps.min() < 0.02   # p = 1, 0.8 and a small one
    for d in range(nd):
        r = philox.draw(seed, np.full(B, blocks[d], np.uint32), np.full(B, pas, np.uint32),
                        (gimg0 + np.arange(B)).astype(np.uint32), step, philox.RNG_DROP)
        want = np.floor(ps[d] + philox.u01(r[0])).astype(np.float32)
        assert np.array_equal(want, keep[d]), d
    assert keep[0].all() and 0 < keep[1].mean() < 1 and keep[-1].sum() <= 3


CLEAN = ("clean_stats", "clean_stats_sums", "clean_finalize", "clean_moving", "clean_se_fwd", "clean_se_bwd",
         "clean_maxpool", "clean_upsample", "clean_fuse_bwd", "clean_copy_grad")

# fault -> the fields / flags that must report it (every other one of the run must stay clean)
FAULTS = {
    # a wrong sum moves every statistic derived from it
    "chunk_last_row_dropped": ("mean", "rstd", "sc", "moving"),
    "idle_lane_rows_twice": ("mean", "rstd", "sc", "moving"),
    "group2_reads_group1": ("mean", "rstd", "sc", "moving"),
    "finalize_partial_1030_dropped": ("mean", "rstd", "sc", "moving"),
    "finalize_zero_cnt_folded": ("mean", "rstd", "sc", "moving"),
    "sums_not_unshifted": ("sums",),
    "bessel_missing": ("moving",),
    "moving_two_pass_order": ("exact",),
    "se_gate_derivative_missing": ("gsum", "dx"),   # dx carries dpool
    "se_dpool_not_divided": ("dx",),
    "se_shares_one_slice_short": ("hidden", "scale"),  # the scale is computed from the hidden units
    "maxpool_last_maximum": ("amax_ok",),
    "upsample_bwd_candidate_short": ("dx_exact",),
    "fuse_eps_missing": ("dx0", "dx1"),
    "dropview_chunk_row": ("dst_exact",),
}


def _bad(d, *, but=()):
    bad = [k for k, v in d["fields"].items() if (v <= 1.0) == (k in but)]
    bad += [k for k, v in d["flags"].items() if v == (k in but)]
    return bad


@pytest.mark.parametrize("run", CLEAN)
def test_clean_standin_passes(teeth, run):
    assert not _bad(teeth[run]), teeth[run]


def test_every_teeth_run_is_asserted(teeth):
    assert set(teeth) == set(CLEAN) | set(FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_reported_in_its_field(teeth, fault):
    d = teeth[fault]
    assert set(FAULTS[fault]) <= set(d["fields"]) | set(d["flags"]), d
    assert not _bad(d, but=FAULTS[fault]), d
