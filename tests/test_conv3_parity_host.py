"""The dense 3x3 conv kernel parity checker (tests/kernels), host side: what its case table covers, read from
`conv3_parity --plan` (the geometry, the stem's blocks and tiles, k_conv3_small's grid and XCD ranges, the weight
gradient's slices and the gather GEMM's plans are host code: no GPU needed), and the teeth of its references and
compare functions, driven by a CPU fp32 stand-in with seeded faults (conv3_teeth)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

# no tensor of a case above about 1.5 M elements ...
CAP_ELEMS = 1_500_000
# ... except the one that needs more to exist at all: un_im2col's grid is capped at 8192 blocks of 256 lanes, so
# the grid-stride loop runs twice only from 8192 * 256 + 1 = 2.1 M column elements (B 2 x 48 x 48 x Kp 576 = 2.65 M).
# (The 4608-row weight gradient the issue allows over the cap stays under it: its widest tensor, the 72 slices
# of partials, holds 83 k elements.)
OVER_CAP = {"ic_s1_c64_2x48x48_gridstride"}

# Edges the issue lists that no shape reaches, with the reason read from the kernel or its launcher:
UNREACHABLE = {
    # launch_gemm_gather refuses every C that is no power of two >= 4 (gemm_gather_ok) and the table's N stay
    # <= 128, so g2_pick's column tile (64 for N <= 64, 128 for N <= 128) always spans N: gy = 1.  plan_gemm2
    # rounds gx down to a multiple of 8 only for gy > 1, so "gridDim.x % 8 == 0" comes from the M tiles alone
    # (8, 16, 32 tiles on, 4 off), never from the rounding.
    "gather GEMM with gx rounded down to a multiple of 8": "needs gy > 1, i.e. N > 128: outside the issue's N",
    # k_gemm2r (the A-resident sweep) and k_gemm2k (wave-split K) are never planned for MODE 4
    # (plan_gemm2(allow_res = false)), and the explicit route passes allow_wsk = false and has gy = 1 (the resident
    # sweep needs gy >= 2): both routes get the same plan at every table shape, which --plan shows.
    "gather and explicit GEMM on different kernels": "plan_gemm2 returns the same plan for both at gy = 1",
    # un_wgrad's src 0 reads x[m * ldx + k] for k < Kp: with Kp > ldx the last row's tail would lie outside x, so
    # the 1x1 cases keep Kp = ldx = the channels (the defender's own call does, defender.cpp).
    "src 0 with Kp padded beyond ldx": "would read past the last row of x",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if name == "conv3_parity" and not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/conv3_parity is missing and there is no hipcc to build it")
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
    return _lines([_binary("conv3_parity"), "--plan"])


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("conv3_teeth")])}


def _run(plan, op):
    return [c for c in plan if not c["refuse"] and c["op"] == op]


def test_names_are_unique_and_the_table_is_the_source(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names) and 120 <= len(names) <= 160
    from test_gpu_conv3_kernels import CASES
    assert CASES == names


def test_stem_forward_coverage(plan):
    cs = _run(plan, "stem_fwd")
    shapes = {(1, 2, 2), (1, 2, 514), (3, 6, 10), (2, 34, 30)}
    for co in (32, 40, 48, 56, 64):
        mine = [c for c in cs if c["N"] == co]
        assert {(c["B"], c["H"], c["W"]) for c in mine} == shapes, co
        assert {c["sink"] for c in mine} == {0, 1} and {c["ybf"] for c in mine} == {0, 1}, co
        assert any(c["sink"] and c["ybf"] for c in mine) and any(c["sink"] and not c["ybf"] for c in mine), co
        # the last block holds one valid pixel, with the statistics on: every row group but one is empty
        assert any(c["sink"] and c["blocks"] == 2 and c["last_valid"] == 1 for c in mine), co
    by = {(c["B"], c["H"], c["W"]): c for c in cs}
    assert (by[(1, 2, 2)]["blocks"], by[(1, 2, 2)]["last_valid"]) == (1, 1)
    assert (by[(3, 6, 10)]["blocks"], by[(3, 6, 10)]["last_valid"]) == (1, 45)
    assert (by[(2, 34, 30)]["blocks"], by[(2, 34, 30)]["last_valid"]) == (2, 254)
    for c in cs:  # TF SAME on even sides: out = in / 2, pads 0 in front
        assert c["H"] % 2 == 0 and c["W"] % 2 == 0 and (c["Ho"], c["Wo"]) == (c["H"] // 2, c["W"] // 2)


def test_stem_backward_coverage(plan):
    cs = _run(plan, "stem_bwd")
    for co in (32, 40, 48, 56, 64):
        mine = [c for c in cs if c["N"] == co]
        assert {(c["B"], c["H"], c["W"]) for c in mine} == {(1, 2, 2), (2, 34, 30), (3, 6, 10)}, co
        assert {c["acc"] for c in mine} == {0, 1}, co
    gx = _run(plan, "stem_gx")
    assert {c["N"] for c in gx} == {32, 40, 48} and all(c["gx_supported"] for c in gx)
    for co in (32, 40, 48):
        mine = [c for c in gx if c["N"] == co]
        assert {c["own"] for c in mine} == {0, 1, 2, 3, 4}, co
        assert {c["act"] for c in mine} == {0, 1, 2}, co  # raw (no y), swish, relu6
        assert {c["ybf"] for c in mine} == {0, 1}, co
        assert {(c["H"], c["W"]) for c in mine} == {(34, 34), (66, 34)}, co
    for c in gx:
        # 34 x 34: 2 x 2 tiles, the last of one quad row / column; 66 x 34: 3 x 2 tiles
        want = (2, 2) if c["H"] == 34 else (3, 2)
        assert (c["tiles_y"], c["tiles_x"]) == want and (c["last_qy"], c["last_qx"]) == (1, 1), c["case"]
        n = c["tiles"]
        assert n == c["B"] * want[0] * want[1]
        # the owner maps give the live tiles the per-tile contract expects
        assert c["live_tiles"] == {0: n, 1: 0, 2: 1, 3: 1, 4: n}[c["own"]], c["case"]
        # dy / y are NaN wherever no live tile reads them: everywhere with no owner, most of the image with one
        if c["own"] in (1, 2, 3):
            assert c["poisoned_px"] > 0.9 * c["B"] * c["Ho"] * c["Wo"], c["case"]
        if c["own"] == 1:
            assert c["poisoned_px"] == c["B"] * c["Ho"] * c["Wo"], c["case"]
    refused = {c["refuse"]: c for c in plan if c["op"] == "stem_gx" and c["refuse"]}
    assert len(refused) == 2  # Co 56 and 64: stem_bwd_gx_supported agrees (asserted on the device run too)


def test_im2col_and_wprep_coverage(plan):
    cs = _run(plan, "im2col")
    small = [c for c in cs if c["case"] not in OVER_CAP]
    assert {(c["mode"], c["s"], c["pt"]) for c in small} == {(0, 1, 1), (0, 2, 0), (1, 2, 0)}
    for gk in (0, 1, 2):
        mine = [c for c in small if c["gk"] == gk]
        assert {c["C"] for c in mine} == {1, 3, 6, 8} and {c["Kp"] for c in mine} == {12, 28, 56, 72}, gk
        assert all(c["H"] != c["W"] for c in mine) and any(c["H"] % 2 or c["W"] % 2 for c in mine), gk
        assert all(c["grid_strides"] == 1 for c in mine)
    big = [c for c in cs if c["case"] in OVER_CAP]
    assert len(big) == 1 and big[0]["grid_strides"] == 2 and big[0]["elems"] > 8192 * 256
    wp = _run(plan, "wprep")
    assert {c["kind"] for c in wp} == {0, 1, 2, 3, 4, 5}
    assert all(c["C"] != c["N"] and c["Kp"] > c["taps"] * c["Kin"] and c["Kp"] % 4 == 0 for c in wp)


def test_conv3_small_coverage(plan):
    cs = _run(plan, "conv3")
    assert {c["N"] for c in cs} == {3, 16, 17, 32} and {c["C"] for c in cs} == {3, 4, 6, 8, 32}
    assert {c["Kp_f"] for c in cs} == {28, 36, 56, 72, 288}
    assert all(c["KpR_f"] > c["Kp_f"] and c["KpR_d"] > c["Kp_d"] for c in cs)
    assert {c["bias"] for c in cs} == {0, 1} and {c["tconv"] for c in cs} == {0, 1}
    # all three gathers: conv (forward and its data gradient), the transposed conv, and its stride-2 data
    # gradient, whose last tap row reads iy == H of the gradient it gathers
    gath = {(c["mode_f"], c["s_f"]) for c in cs} | {(c["mode_d"], c["s_d"]) for c in cs}
    assert gath == {(0, 1), (1, 2), (0, 2)}
    for c in cs:
        if c["tconv"]:
            assert (c["mode_d"], c["s_d"], c["pt_d"]) == (0, 2, 0) and 2 * (c["Ho_d"] - 1) + 2 == c["H_d"], c["case"]
    # both instantiations of each launch; the scalar one also by pointer alignment alone
    assert {c["vec_f"] for c in cs} == {0, 1} and {c["vec_d"] for c in cs} == {0, 1}
    mis = [c for c in cs if c["mis"]]
    assert len(mis) == 2 and all(c["C"] % 4 == 0 and not c["vec_f"] for c in mis)
    assert {c["tconv"] for c in mis} == {0, 1}
    plans = [c[k] for c in cs for k in ("fwd", "dgrad")]
    # one workgroup with an idle wave: fewer tiles than waves
    assert any(p["G"] == 1 and p["tiles"] < 4 for p in plans)
    # fewer than 8 workgroups: one range over all tiles
    assert any(1 < p["G"] < 8 and not p["xr"] and p["xcd_tiles"][0] == p["tiles"] for p in plans)
    assert any(p["G"] == 7 for p in plans)
    # XCD ranges with an empty last range
    assert any(p["xr"] and p["xcd_tiles"][7] == 0 and p["xcd_tiles"][6] > 0 for p in plans)
    # XCD ranges, a ragged last tile, and waves that sweep a second tile
    assert any(p["xr"] and p["M"] % 16 and p["sweeps"] >= 2 and all(p["xcd_tiles"]) for p in plans)
    for p in plans:
        assert sum(p["xcd_tiles"]) == p["tiles"] == -(-p["M"] // 16), p
        assert p["xr"] == int(p["G"] >= 8)
    for tc in (0, 1):  # every row-count situation under both forwards
        ps = [c["fwd"] for c in cs if c["tconv"] == tc]
        assert {48, 448, 520} <= {p["M"] for p in ps}
    assert 675 in {c["fwd"]["M"] for c in cs}
    assert {c["refuse"] for c in plan if c["op"] == "conv3" and c["refuse"]} == {7, 8, 9, 10}


def test_gather_coverage(plan):
    cs = _run(plan, "gather")
    assert {c["C"] for c in cs} == {4, 64, 128} and {c["N"] for c in cs} == {40, 64, 128}
    assert {(c["mode"], c["s"]) for c in cs} == {(0, 1), (0, 2), (1, 2)}
    assert {(c["Ho"], c["Wo"]) for c in cs} >= {(16, 16), (8, 32), (32, 8)}
    for c in cs:
        assert c["gather_ok"] and c["impl"] == 2 and c["K"] == 9 * c["C"], c["case"]
        # both routes multiply under the same plan (the claim defender.cpp makes for its two forms)
        assert c["plan_gather"] == c["plan_explicit"], c["case"]
        assert not c["plan_gather"]["res"] and not c["plan_gather"]["wsk"]
        assert c["partial_floats"] >= (c["plan_gather"]["splits"] > 1) * c["plan_gather"]["splits"] * c["M"] * c["N"]
    assert any(c["plan_gather"]["splits"] > 1 for c in cs) and any(c["plan_gather"]["splits"] == 1 for c in cs)
    assert any(c["xcd_ranges"] and c["plan_gather"]["gx"] % 8 == 0 for c in cs)
    assert any(not c["xcd_ranges"] for c in cs)
    assert any(c["xcd_ranges"] and c["plan_gather"]["splits"] > 1 for c in cs)
    assert {c["refuse"] for c in plan if c["op"] == "gather" and c["refuse"]} == {11, 12, 13, 14}


def test_weight_gradient_coverage(plan):
    cs = _run(plan, "wgrad")
    s0, s1, s2 = ([c for c in cs if c["src"] == s] for s in (0, 1, 2))
    assert any(c["N"] == 1 and c["ldy"] == 1 for c in s0) and {3, 16} <= {c["N"] for c in s0}
    assert any(c["C"] == 6 and c["Kp"] == 6 and not c["vec"] for c in s0)  # the scalar path by ldx = Kp = 6
    assert any(c["mis"] and c["C"] % 4 == 0 and not c["vec"] for c in s0)
    assert any(c["ldy"] > c["N"] for c in s0)
    assert {c["C"] for c in s1} == {3, 8, 16, 64} and {c["N"] for c in s1} == {3, 16, 17, 40}
    assert any(c["C"] == 3 and c["Kp"] == 28 for c in s1)
    assert {c["C"] for c in s2} == {6, 16} and all(c["H"] % 2 == 0 and c["W"] % 2 == 0 for c in s2)
    assert all(c["kind"] == {0: 4, 1: 0, 2: 2}[c["src"]] for c in cs)
    assert all(c["C"] != c["N"] for c in cs)  # ci != co: a transposed layout cannot pass
    # the slice edges, from the launcher's own planner
    assert any(c["M"] == 9 and c["slices"] == 1 and c["rps"] > c["M"] for c in cs)
    assert any(c["M"] == 675 and c["slices"] == 11 and c["last_rows"] == 35 for c in cs)
    assert any(c["slices"] == 17 for c in cs)
    big = [c for c in cs if c["M"] == 4608]
    assert len(big) == 1 and big[0]["slices"] >= 65  # k_wgrad_fold's four-deep loop runs (z + 48 < slices)
    for c in cs:
        assert c["slices"] == -(-c["M"] // c["rps"]) and c["rps"] % 16 == 0, c["case"]
        # the bound's constant is the depth of the summation tree, never the row count
        assert c["depth"] == c["rps"] // 4 + 3 + -(-c["slices"] // 16) + 15, c["case"]
    assert max(c["depth"] for c in cs) < 64 and big[0]["depth"] + 16 < big[0]["M"] / 50
    # every case but the >= 65-slice one at M <= 1100
    assert all(c["M"] <= 1100 for c in cs if c["M"] != 4608)
    assert {c["refuse"] for c in plan if c["op"] == "wgrad" and c["refuse"]} == {15, 16}


def test_refusals_and_caps(plan):
    assert {c["refuse"] for c in plan if c["refuse"]} == set(range(1, 17))
    for c in plan:
        if c["case"] in OVER_CAP:
            assert c["op"] == "im2col" and c["elems"] < 2 * CAP_ELEMS
        else:
            assert c["elems"] <= CAP_ELEMS, c["case"]
        # no more than 1 % of the elements under the relu6 kink allowance, by the fp64 reference alone
        assert c["kink_share"] <= 0.01, c["case"]
    assert UNREACHABLE  # recorded above, not dropped


CLEAN = ("clean_conv_c8_n17_bias", "clean_conv_c3_n3", "clean_tconv_c6_n16_bias", "clean_stem_fwd_c40",
         "clean_stem_fwd_c32_one_lane_block", "clean_stem_gx_c32", "clean_wgrad_src1_m4608", "clean_wgrad_src2_c6_co5")

RATIOS = ("y", "dx", "g", "sum_ratio", "m2_ratio")
COUNTS = ("nonfinite", "dead_bad", "bt_bad")
FLAGS = ("rows_written", "cnt_ok", "cnt_sum_ok")


def _ok(d, *, but=()):
    """The fields that are not as they should be: every field clean, except those in `but`, which must be tripped."""
    bad = [k for k in RATIOS if (d[k] <= 1.0) == (k in but)]
    bad += [k for k in COUNTS if (d[k] == 0) == (k in but)]
    bad += [k for k in FLAGS if d[k] == (k in but)]
    return bad


@pytest.mark.parametrize("run", CLEAN)
def test_clean_standin_passes(teeth, run):
    assert not _ok(teeth[run]), teeth[run]


# fault -> the fields that must report it (every other field must stay clean)
FAULTS = {
    # (the exact image of un_wprep's output differs too: both the product and the moved values report it)
    "dgrad_unflipped": ("dx", "bt_bad"),
    "kind2_as_kind0": ("g",),
    "top_pad_zero": ("y",),
    "tconv_odd_tap": ("y",),
    "stem_bottom_right_tap": ("y",),
    # (the dropped tile keeps its NaN fill)
    "ragged_tile_dropped": ("nonfinite",),
    "last_k_quad_dropped": ("y",),
    "bias_dropped": ("y",),
    "row_twice_m4608": ("g",),
    # (a dead tile's bound is zero, so the value comparison reports the stray element as well)
    "dead_tile_nonzero": ("dead_bad", "dx"),
    "sink_row_sentinel": ("rows_written", "sum_ratio", "m2_ratio"),
}


def test_every_teeth_run_is_asserted(teeth):
    assert set(teeth) == set(CLEAN) | set(FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_reported_in_its_field(teeth, fault):
    assert not _ok(teeth[fault], but=FAULTS[fault]), teeth[fault]


def test_depth_bound_sees_a_row_counted_twice_where_m_would_not(teeth):
    """With M for the constant the 4608-row weight gradient's bound is 80 x wider: the doubled row, far outside
    the derived bound, would sit within a few multiples of it ("Dense 3x3 conv kernel parity")."""
    d = teeth["row_twice_m4608"]
    assert d["g"] > 100.0 and d["g_if_M"] < d["g"] / 50.0
