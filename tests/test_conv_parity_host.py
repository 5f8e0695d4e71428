"""The depthwise / separable conv kernel parity checker (tests/kernels), host side: what its case table
covers, read from `conv_parity --plan` (the TF-SAME geometry, the launchers' tile plans and partial counts
are host code: no GPU needed), and the teeth of its reference and compare functions, driven by a CPU
stand-in conv with seeded faults (conv_teeth)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

# no case above 48 x 48 x B 2 x C 144 input elements ...
CAP_ELEMS = 48 * 48 * 2 * 144
# ... except the one that needs more to exist at all (see UNREACHABLE)
OVER_CAP = {"fused_125x33_n3_m0_swish_large", "fused_124x33_n2_m0_relu6_below"}

# Edges the issue lists that no shape within its limits reaches, with the reason (kernels_dw.hip, kernels_sep.hip):
UNREACHABLE = {
    # launch_dw_fwd_fused keeps the four-rows-per-lane plan from 512 workgroups up.  A workgroup of that
    # plan covers at least 33 columns x 4 rows x 4 << lcg channels (a narrower image packs several row
    # groups into the block), i.e. >= 2064 elements whatever lcg, so 512 of them need >= 1.06 M input
    # elements: 1.6 x the cap.  The table carries the smallest such shape (B 4 x 125 x 33 x C 64, exactly
    # 512 workgroups) and its neighbour one tile row shorter (496, the other side), both over the cap.
    "fused view, >= 512 workgroups, within the size cap": "512 workgroups x >= 2064 elements each > 663552",
    # sep_supported admits every N in 1..64, so none of N = 64, 36, 8, 1 is a refusal case.
    "k_sep_fwd N refused": "sep_supported(64, N) holds for 1 <= N <= 64",
    # dw_lcg caps lcg at 2 for stride-1 forwards and for 5x5 data gradients: lcg 3 exists forward only
    # at stride 2 and backward only for 3x3 (C = 96 and 672 run at lcg 2 elsewhere, as the issue notes).
    "lcg 3, stride-1 forward / 5x5 backward": "dw_lcg's cap",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if name == "conv_parity" and not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/conv_parity is missing and there is no hipcc to build it")
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
    return _lines([_binary("conv_parity"), "--plan"])


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("conv_teeth")])}


def _run(plan, op=None):
    return [c for c in plan if not c["refuse"] and (op is None or c["op"] == op)]


def test_names_are_unique_and_the_table_is_the_source(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names) and len(names) > 150
    from test_gpu_conv_kernels import CASES
    assert CASES == names


def test_same_padding_rule(plan):
    """The table's pt / pl / Ho / Wo, recomputed here from H, W, k, s by the TF SAME rule."""
    for c in plan:
        for m in c["members"]:
            for n, o, p in ((m["H"], m["Ho"], m["pt"]), (m["W"], m["Wo"], m["pl"])):
                assert o == -(-n // c["s"]), c["case"]
                assert p == max((o - 1) * c["s"] + c["k"] - n, 0) // 2, c["case"]


def test_depthwise_coverage(plan):
    for op in ("dw_fwd", "dw_bwd"):
        cs = _run(plan, op)
        assert {(c["k"], c["s"]) for c in cs} == {(3, 1), (3, 2), (5, 1), (5, 2)}
        assert {c["members"][0]["lcg"] for c in cs} == {0, 1, 2, 3}, op
        for k, odd, even in ((3, 1, 0), (5, 2, 1)):
            s2 = [c for c in cs if c["k"] == k and c["s"] == 2]
            # (H parity, k) -> pt: both parities of pt, each reached through the input parity that gives it
            assert {(c["members"][0]["H"] % 2, c["members"][0]["pt"]) for c in s2
                    if c["members"][0]["H"] >= k} == {(1, odd), (0, even)}, (op, k)
        for k in (3, 5):
            for s in (1, 2):
                ks = [c for c in cs if (c["k"], c["s"]) == (k, s)]
                sizes = {(c["members"][0]["H"], c["members"][0]["W"]) for c in ks}
                assert {(1, 1), (2, 2), (3, 3), (4, 4), (5, 7), (15, 15), (16, 16), (30, 30), (33, 17)} <= sizes, (op, k, s)
                assert {c["C"] for c in ks} >= {20, 24, 48, 96, 672} and {16, 48} & {c["C"] for c in ks}
                assert all(c["members"][0]["H"] * c["members"][0]["W"] <= 64 for c in ks if c["C"] == 672)
                assert {c["act"] for c in ks if c["view"]} == {0, 1, 2}, (op, k, s)
                assert 0 in {c["view"] for c in ks}
                assert {bool(c["sink"]) for c in ks} == {False, True}
                # several tiles per image: in x (W beyond the block's columns), in y with a partial last tile
                tiled = lambda m, n_out, t: m["ntiles"] // m["tiles_x"] > 1 and n_out % t
                out = (lambda m: (m["Ho"], m["Wo"])) if op == "dw_fwd" else (lambda m: (m["H"], m["W"]))
                assert any(c["members"][0]["tiles_x"] > 1 and out(c["members"][0])[1] % c["members"][0]["otw"]
                           for c in ks), (op, k, s)
                assert any(tiled(c["members"][0], out(c["members"][0])[0], c["members"][0]["oth"]) for c in ks), (op, k, s)
                # tiles in both directions at once (the tile index splits into a row and a column)
                assert any(c["members"][0]["tiles_x"] > 1 and c["members"][0]["ntiles"] > c["members"][0]["tiles_x"]
                           for c in ks), (op, k, s)
                # a partial last row group: rows that are no multiple of the rows per lane
                assert any(out(c["members"][0])[0] % c["members"][0]["rpt"] for c in ks)
                # levels so small that whole waves hold no output (fewer than 64 lanes' worth with a sink)
                assert any(c["sink"] and out(c["members"][0])[0] * out(c["members"][0])[1] * (1 << c["members"][0]["lcg"]) < 64
                           for c in ks), (op, k, s)
                # bf16 storage at two shapes, with and without the sink
                bf = [c for c in ks if c["st"]]
                assert len({(c["members"][0]["H"], c["members"][0]["W"]) for c in bf}) == 2
                assert {bool(c["sink"]) for c in bf} == {False, True}
    bw = _run(plan, "dw_bwd")
    assert {(c["members"][0]["acc"], c["sink"]) for c in bw} == {(0, 0), (0, 2), (1, 0), (1, 2)}
    # lcg differs between the directions for the same C (the cap)
    f96 = {c["members"][0]["lcg"] for c in _run(plan, "dw_fwd") if c["C"] == 96 and (c["k"], c["s"]) == (3, 1)}
    b96 = {c["members"][0]["lcg"] for c in bw if c["C"] == 96 and (c["k"], c["s"]) == (3, 1)}
    b96k5 = {c["members"][0]["lcg"] for c in bw if c["C"] == 96 and c["k"] == 5}
    assert f96 == {2} and b96 == {3} and b96k5 == {2}
    # the partial counts the planners return are the tiles: P = B * ntiles
    for c in _run(plan):
        for m in c["members"]:
            if c["op"] != "dw_fused":
                assert m["P"] == c["B"] * m["ntiles"], c["case"]


def test_fused_view_coverage(plan):
    cs = _run(plan, "dw_fused")
    # each case lies on the side of the few-workgroups switch it was chosen for
    for c in cs:
        m = c["members"][0]
        assert m["small"] == c["expect_small"] and (m["wgs"] < 512) == bool(m["small"]), c["case"]
        if m["small"]:
            assert (m["rpt"], m["lcg"]) == (1, 0), c["case"]
    assert {c["members"][0]["small"] for c in cs} == {0, 1}
    large = [c for c in cs if not c["members"][0]["small"]]
    assert min(c["members"][0]["wgs"] for c in large) == 512  # the smallest shape that crosses
    assert {(c["nin"], c["method"]) for c in cs} == {(2, 0), (2, 1), (3, 0), (3, 1)}
    assert {c["act"] for c in cs} == {1, 2}
    assert any(c["neg"] >= 0 for c in cs if c["method"] == 0)
    sizes = {(c["members"][0]["H"], c["members"][0]["W"]) for c in cs}
    assert {(4, 4), (8, 8)} <= sizes


def test_grouped_coverage(plan):
    heads = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    three = [(20, 12), (5, 3), (1, 1)]
    for op, sink in (("dw_fwd_group", 1), ("dw_bwd_group", 2), ("sep_fwd", 1), ("sep_bwd", 2)):
        cs = [c for c in _run(plan, op) if c["n"] > 1]
        shapes = {tuple((m["H"], m["W"]) for m in c["members"]) for c in cs}
        assert shapes >= {tuple(heads), tuple(three)}, op
        assert any(c["sink"] == sink for c in cs), op
        assert all(c["C"] == 64 and c["k"] == 3 and c["s"] == 1 for c in cs)
        # members get different partial counts, the 1x1 and 2x2 members included
        assert any(len({m["P"] for m in c["members"]}) > 1 for c in cs)
        if op.endswith("bwd_group") or op == "sep_bwd":
            assert any(len({m["acc"] for m in c["members"]}) == 2 for c in cs), op


def test_separable_coverage(plan):
    fw, bw = _run(plan, "sep_fwd"), _run(plan, "sep_bwd")
    sizes = {(1, 1), (4, 4), (5, 8), (8, 8), (9, 9), (16, 8), (17, 33)}
    for cs in (fw, bw):
        one = [c for c in cs if c["n"] == 1]
        assert sizes <= {(c["members"][0]["H"], c["members"][0]["W"]) for c in one}
        assert {(m["tw"], m["th"]) for c in cs for m in c["members"]} == {(16, 8), (8, 16), (4, 16)}
        for tw, th in ((16, 8), (8, 16), (4, 16)):  # a partial tile of each shape, and a full or multiple one
            ms = [m for c in cs for m in c["members"] if (m["tw"], m["th"]) == (tw, th)]
            assert any(m["H"] % th or m["W"] % tw for m in ms), (tw, th)
            assert any(m["ntiles"] > 1 for m in ms), (tw, th)
        assert all(c["C"] == 64 for c in cs)
    assert {c["N"] for c in fw} == {64, 36, 8, 1}
    assert {c["bias"] for c in fw} == {0, 1} and {bool(c["sink"]) for c in fw} == {False, True}
    assert {c["act"] for c in fw if c["view"] == 1} == {0, 1, 2}
    assert {(c["nin"], c["method"]) for c in fw if c["view"] == 2} >= {(2, 0), (3, 0), (2, 1)}
    assert all(c["n"] == 1 for c in fw if c["view"] == 2)
    assert {c["N"] for c in bw} == {64}
    assert {c["view"] for c in bw} == {0, 3}
    assert {(c["members"][0]["acc"], bool(c["sink"])) for c in bw if c["n"] == 1} == {(0, False), (0, True), (1, False), (1, True)}
    # the flat (member, image, tile) list does not divide into its 8 ranges evenly
    assert any(sum(m["P"] for m in c["members"]) % 8 for c in fw + bw if c["n"] > 1)


def test_refusals_and_caps(plan):
    assert {c["refuse"] for c in plan if c["refuse"]} == set(range(1, 12))
    for c in plan:
        if c["case"] in OVER_CAP:
            assert c["op"] == "dw_fused" and c["elems"] < 1.7 * CAP_ELEMS
        else:
            assert c["elems"] <= CAP_ELEMS, c["case"]
        # no more than 1 % of the elements under the relu6 kink allowance, by the fp64 reference alone
        assert c["kink_share"] <= 0.01, c["case"]
    assert sum(c["elems"] * c["k"] ** 2 for c in plan) < 3e8  # a second or two of fp64 host reference
    assert UNREACHABLE  # recorded above, not dropped


CLEAN = ("clean_fwd_k3s2_odd_stat", "clean_fwd_k3s2_even_stat", "clean_fwd_k5s1_relu6_stat", "clean_fwd_k5s2_raw",
         "clean_fwd_fuse_swish", "clean_fwd_bf16_stat", "clean_bwd_k3s1_gx_swish_gs_acc",
         "clean_bwd_k3s2_gx_relu6_gs_acc", "clean_bwd_k5s2_gx_swish", "clean_bwd_k5s1_raw_gs", "clean_sep_fwd_stat",
         "clean_sep_bwd_gs_acc", "clean_pad_fault_even_input", "clean_bwd_1x1_gx_swish_gs_acc")


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
    "pad_off_odd_s2": ("c_ratio",),
    "halo_col_zero": ("c_ratio",),
    "bwd_halo_col_zero": ("c_ratio",),
    "tap_transposed_k5": ("c_ratio",),
    "bwd_unflipped": ("c_ratio",),
    # (the fold divides the last partial's sum by the wrong count, so its M2 is off too)
    "cnt_full_tile": ("cnt_sum_ok", "m2_ratio"),
    "part_row_shifted": ("rows_written", "sum_ratio", "m2_ratio"),
    "part_row_shifted_gs": ("rows_written", "sum_ratio", "m2_ratio"),
    "acc_ignored": ("c_ratio",),
    "fuse_no_eps": ("c_ratio",),
    "view_on_pad": ("c_ratio",),
    "sep_no_bias_last_col": ("c_ratio",),
    "sep_bwd_halo_col_zero": ("c_ratio",),
    "bf16_two_quanta": ("c_ratio",),
}


def test_every_teeth_run_is_asserted(teeth):
    assert set(teeth) == set(CLEAN) | set(FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_seeded_fault_is_reported_in_its_field(teeth, fault):
    assert not _ok(teeth[fault], but=FAULTS[fault]), teeth[fault]
