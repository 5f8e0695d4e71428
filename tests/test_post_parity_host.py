"""The post-processing kernel parity checker (tests/kernels), host side: what its case table covers, read from
`post_parity --plan` (tiles per staging branch, planted argmax ties and validity edges, candidate lists, soft-NMS
pops, ties and decision margins, nms_plan's numbers, tie chunks of the per-image max, the decision-allowance share:
host code by the reference alone, no GPU needed), and the teeth of its references, bounds and compare functions,
driven by a CPU fp32 stand-in with seeded faults (post_teeth)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")

# all the device buffers of a case together stay under about 1.5 M elements ...
CAP_ELEMS = 1_500_000
# ... except two cases that cannot exist below it: soft-NMS picks the chunk factor m = 2 only from N > 64^3 =
# 262,144 positions per image (boxes, scores, keep and 7 N work floats), and launch_adam_clip's scale slot lies
# behind the 640 x 640 x 3 patch (params, grad, m, v)
OVER_CAP = {"nms_m2_n262208", "adam_clip_npatch_plus_1"}
OVER_CAP_ELEMS = 5_000_000

# Edges the issue lists that no case reaches or proves, with the reason read from the kernel or its launcher:
UNREACHABLE = {
    # k_soft_nms's fast path keeps at most kNmsFl = 24 decay factors per row candidate and falls back to a full
    # visit at the pop (`dirty`).  nms_mask_n4096_b2_ties_dups pops a candidate over 30 earlier selections
    # (nms_max_first_overlaps), which needs that fallback when the candidate sits in a row while they are selected;
    # whether it did is not observable from outside (PHX_NMS_STATS is a device printf, left off).  The result is
    # bit-equal to PHX_NMS_FAST=0 either way, which is what the case asserts.
    "kNmsFl overflow taken": "a counter only PHX_NMS_STATS prints; the case asserts the outcome on both paths",
    # the fast path's other fallbacks (a batch over lp entries, no free re-queue row) end in the general queue and
    # cannot be told from outside either; N = 262,208 leaves qrows = 2, the smallest re-queue set of the table
    "fast path's overflow to the general queue": "not observable without PHX_NMS_STATS; both paths are run and compared",
    # launch_adam_clip clips every index >= PHX_NPATCH_DEV to [0, 1]; with n = PHX_NPATCH_DEV + 1 there is one
    # such slot, so one launch crosses one of its two limits (0, which tells [0, 1] from [-1, 1]); 1 is crossed
    # in the patch part
    "the scale slot crossing 0 and 1 in one launch": "one slot at n = PHX_NPATCH_DEV + 1: it crosses 0",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail(f"tests/kernels/{name} is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", name], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return path


def _lines(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert out and out[-1].get("done") is True, r.stdout[-500:]
    return out


@pytest.fixture(scope="module")
def plan_all():
    return _lines([_binary("post_parity"), "--plan"])


@pytest.fixture(scope="module")
def plan(plan_all):
    return plan_all[:-1]


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("post_teeth")])[:-1]}


def _kind(plan, kind):
    return [c for c in plan if c["kind"] == kind]


def _plants(c):
    return {p[0] for p in c["plants"]}


def test_names_are_unique_and_the_table_is_the_source(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names) and 25 <= len(names) <= 35
    from test_gpu_post_kernels import CASES
    assert CASES == names


def test_harness_constants_are_the_librarys(plan_all):
    d = plan_all[-1]
    assert d["pre_tile"] == d["check_pre_tile"] == 128
    assert d["imax_chunks"] == d["check_imax_chunks"] == 48
    assert d["nms_fl"] == d["check_nms_fl"] == 24
    # the host's expf, measured as the device's is: a correctly rounded or 1-ulp library
    assert d["host_exp_ulp"] <= 1.0


def test_pre_nms_geometry(plan):
    ch = _kind(plan, "chain")
    nine = [c for c in ch if c["na"] == 9]
    assert nine and all(c["A"] == 846 for c in nine)
    # ragged last tiles (8x8x9 = 576 anchors: 4.5 tiles; 4x4x9 = 144: 1.125) and three levels of one short tile
    assert all(c["ragged_tiles"] == 2 * c["B"] and c["short_tiles"] == 3 * c["B"] for c in nine)
    # the scalar-staging branch: runs off a 16-byte boundary, fp32 and bf16; both bf16 branches in one case
    assert any(c["unaligned_tiles"] and not c["bf"] for c in ch)
    assert any(c["unaligned_tiles"] and c["aligned_tiles"] and c["bf"] and c["nclass"] == 90 for c in ch)
    # nclass 1, 2, 3, 90, 91, 100 (51 KB of LDS); na 1, 9, 17; fp32 and bf16 storage of the same logits
    assert {c["nclass"] for c in ch} == {1, 2, 3, 90, 91, 100}
    assert max(c["lds_bytes"] for c in ch) == 51200
    assert {c["na"] for c in ch} == {1, 9, 17}
    same = [c for c in ch if c["case"] in ("chain_f32_b3_c90", "chain_bf16_b3_c90")]
    assert [c["bf"] for c in same] == [0, 1] and same[0]["plants"] == same[1]["plants"]
    assert {c["B"] for c in ch} == {1, 2, 3}


def test_pre_nms_argmax_ties(plan):
    big = [c for c in _kind(plan, "chain") if c["nclass"] >= 3]
    for c in big:
        # two equal maxima inside the first half; one in each half; the second half strictly greater; all classes
        # equal; the maximum at the last class
        for k in ("tie_first_half", "tie_both_halves", "second_greater", "all_equal", "max_last"):
            assert c[k] > 0, (c["case"], k)
    two = [c for c in _kind(plan, "chain") if c["nclass"] == 2]
    assert two and all(c["tie_both_halves"] > 0 and c["second_greater"] > 0 for c in two)
    assert all({"tie_first_half", "tie_both_halves", "second_half_greater", "all_equal", "max_last_class"} <= _plants(c) for c in big)


def test_pre_nms_validity_edges_and_keep_bits(plan):
    for c in _kind(plan, "chain"):
        # bw / img_w == 1 (valid), area == 100 (invalid), area just above 100 (valid): exact in fp64, no allowance
        assert c["bw_eq_1"] >= 1 and c["area_eq_100"] >= 1 and c["area_just_above"] >= 1, c["case"]
        assert {"bw_over_w_eq_1", "area_eq_100", "area_just_above_100", "score_eq_half"} <= _plants(c)
        # a score exactly on thresh, scores on both sides
        assert c["sc_eq_thresh"] >= 1 and c["sc_ge"] > 1 and c["sc_lt"] > 0
        kh = c["keep_hist"]
        # class 0 with an invalid box (4 only), valid below thresh (5), valid at or above (7), and no other value
        assert kh[4] >= 1 and kh[7] > 0 and kh[1] == kh[2] == kh[3] == kh[6] == 0
        if c["nclass"] > 1:
            assert c["cls_nonzero"] > 0 and kh[0] > 0
    assert any(c["keep_hist"][5] > 0 for c in _kind(plan, "chain"))


def test_candidate_list_coverage(plan):
    ch = _kind(plan, "chain")
    assert {c["cand_mask"] for c in ch if c["cand_list"]} == {2, 1, 4, -1}
    assert any(not c["cand_list"] for c in ch)
    assert {round(c["cand_thresh"], 3) for c in ch} == {0.5, 0.001}
    # an image whose list is empty, next to images with lists
    assert any(0 in c["cand"] and max(c["cand"]) > 0 for c in ch if c["cand_list"])
    # an image where every anchor is a candidate
    assert any(c["A"] in c["cand"] for c in ch if c["cand_list"])


def test_soft_nms_coverage(plan):
    ch = [c for c in _kind(plan, "chain")]
    nm = _kind(plan, "nms")
    # the list path from pre_nms's own lists, and the keep-mask path without one in the chain
    assert sum(c["cand_list"] for c in ch) >= 8 and any(not c["cand_list"] for c in ch)
    # N 1, 77, 1000 (no multiples of 64) and 4096; max_out 1, 7, 100
    assert {1, 77, 1000, 4096} <= {c["N"] for c in nm}
    assert {c["max_out"] for c in nm + ch} == {1, 7, 100}
    # keep mask with count null; a count prefix clamped and 0
    assert any(c["nms_mode"] == 0 for c in nm) and any(c["nms_mode"] == 1 for c in nm)
    # the chunk factor: 1 everywhere but the one case with N > 64^3, whose candidate count keeps the reference cheap
    m2 = [c for c in nm if c["nms_m"] == 2]
    assert [c["case"] for c in m2] == ["nms_m2_n262208"] and m2[0]["N"] == 262208 and 2000 <= m2[0]["nms_candidates"] <= 4000
    assert all(c["nms_m"] == 1 for c in nm + ch if c not in m2)
    # more candidates than one batch (kNmsTopWant) and than the LDS-resident positions
    assert any(c["nms_candidates"] > c["B"] * c["nms_top_want"] for c in nm)
    # score ties broken by candidate order, duplicate boxes, a candidate over more than kNmsFl earlier selections at
    # its first pop (see UNREACHABLE for what that does not prove)
    t = next(c for c in nm if c["case"] == "nms_mask_n4096_b2_ties_dups")
    assert t["nms_tie_pops"] >= 32 and t["nms_dup_visits"] >= 1 and t["nms_max_first_overlaps"] > 24
    assert any(c["nms_tie_pops"] > 0 for c in ch)
    # re-queued candidates and runs that end at max_out and below it
    assert any(c["nms_requeues"] > 50 for c in nm + ch)
    assert any(c["nms_selected"] == c["B"] * c["max_out"] for c in nm) and any(c["nms_selected"] < c["B"] * c["max_out"] for c in nm + ch)


def test_soft_nms_margins(plan):
    """No allowance in soft-NMS: over every pop of the reference run, the relative margin to a flipped decision
    (the order of two queue keys of which one is a decayed score; a decayed score against the threshold) is at least
    8 times the products' bound, and every overlapping pair's decay argument is far enough from 0 that expf of it
    is not 1 (the selection test sc == orig)."""
    for c in _kind(plan, "chain") + _kind(plan, "nms"):
        assert c["nms_min_margin"] >= 8.0, (c["case"], c["nms_min_margin"])
        assert c["nms_min_arg"] >= 2.0 ** -22, (c["case"], c["nms_min_arg"])


def test_image_max_and_scatter_coverage(plan):
    im = {c["N"]: c for c in _kind(plan, "imax")}
    assert set(im) == {47, 48, 846, 12301} and {c["B"] for c in im.values()} == {1, 3, 4, 65}
    assert im[47]["imax_empty_chunks"] >= 1 and im[48]["imax_empty_chunks"] == 0
    assert im[12301]["N"] > 48 * 256 and im[12301]["B"] > 64
    for c in (im[846], im[12301]):
        # the maximum tied inside a chunk, across two chunks, across three; no kept anchor; a maximum of exactly 0
        # (0.0 and -0.0 tied) and a negative one; higher scores under bits 2 / 4 alone
        for k in ("imax_ties_in_chunk", "imax_ties_2_chunks", "imax_ties_3_chunks", "imax_empty_images", "imax_max_zero", "imax_max_neg",
                  "imax_bits_without_1"):
            assert c[k] >= 1, (c["case"], k)
    ch = _kind(plan, "chain")
    assert {c["K"] for c in ch} == {1, 63, 64, 65, 160}
    for c in ch:
        # the image maximum shared by anchors of one pixel and of another level; an image with dm == 0 where B = 3
        assert c["sc_win_anchors"] >= 3 and c["sc_levels_hit"] >= 2, c["case"]
        assert c["imax_ties_in_chunk"] >= 1 and c["imax_ties_2_chunks"] >= 1
        if c["na"] >= 6:
            assert c["sc_pixels_2_winners"] >= 1, c["case"]
        if c["nclass"] >= 3:
            assert c["sc_max_class_ties"] >= 3, c["case"]
        if c["B"] == 3:
            assert c["sc_images_dm0"] == 1 and c["imax_empty_images"] == 1
        assert {"win_ties_3", "win_same_pixel", "win_other_level"} <= _plants(c)
    # both fallback paths of k_cls_scatter, bf16 logits
    assert any(c["nclass"] > 96 for c in ch) and any(c["na"] > 16 for c in ch) and any(c["bf"] and c["nclass"] > 64 for c in ch)


def test_direct_cases_and_refusals(plan):
    assert sorted(c["nseg"] for c in _kind(plan, "zero")) == [1, 8]
    assert any(c["nseg"] == 8 for c in _kind(plan, "chain"))
    assert sorted(c["max_out"] for c in _kind(plan, "count")) == [7, 100]
    ad = _kind(plan, "adam")
    assert {(c["n"], c["t"]) for c in ad if not c["clip"]} == {(1, 1), (257, 2), (1000, 1000)}
    assert [(c["n"], c["clip"]) for c in ad if c["clip"]] == [(640 * 640 * 3 + 1, 1)]
    assert len(_kind(plan, "loss")) == 2
    rf = {c["refuse"]: c for c in _kind(plan, "refuse")}
    assert sorted(rf) == [1, 2, 3, 4, 5]
    assert rf[1]["max_out"] == 101 and rf[2]["nseg"] == 9 and rf[4]["na"] == 33


def test_element_cap(plan):
    for c in plan:
        if c["refuse"]:
            continue
        cap = OVER_CAP_ELEMS if c["case"] in OVER_CAP else CAP_ELEMS
        assert c["elems"] <= cap, (c["case"], c["elems"])
    assert {c["case"] for c in plan if not c["refuse"] and c["elems"] > CAP_ELEMS} == OVER_CAP
    assert UNREACHABLE  # recorded above, not dropped


def test_allowance_share_and_standin(plan):
    for c in plan:
        if c["refuse"]:
            continue
        assert c["allow_share"] <= 0.01, (c["case"], c["allow_share"])
        assert c["standin_pass"] and not c["stopped"], c["case"]
        assert all(v <= 1.0 for k, v in c["fields"].items() if not k.endswith("_bad")), c
        assert all(v == 0 for k, v in c["fields"].items() if k.endswith("_bad")), c


# every seeded fault trips its own fields: `must` are tripped, nothing outside `must | may` is
FAULTS = {
    "second_half_wins_ties": ({"cls_bad", "keep_bad"}, {"list_bad"}),
    "ragged_last_anchor_dropped": ({"cls_bad", "score", "box", "keep_bad"}, {"list_bad"}),
    "level_lookup_off_by_one": ({"cls_bad", "score", "box", "keep_bad"}, {"list_bad"}),
    "area_ge_100": ({"keep_bad"}, set()),
    "person_bit_after_filter": ({"keep_bad"}, set()),
    "candidate_gate_ge": ({"list_bad"}, set()),
    "candidate_appended_twice": ({"list_bad"}, set()),
    "imax_tie_counts_not_added": ({"imax_exact_bad"}, set()),
    "imax_first_index_not_smallest": ({"imax_exact_bad"}, set()),
    "loss_grad_zero_at_raw_zero": ({"loss", "loss_exact_bad"}, set()),
    "tied_classes_not_divided": ({"dx", "dx_exact_bad"}, set()),
    "only_first_tied_class": ({"dx", "dx_exact_bad"}, set()),
    "dx_overwritten": ({"dx", "dx_exact_bad"}, set()),
    "nms_ties_higher_index": ({"nms_index_bad"}, {"nms_box_bad", "nms_score"}),
    "nms_clip_omitted": ({"nms_box_bad"}, set()),
    "cand_count_not_reset": ({"nms_reset_bad"}, set()),
    "adam_scale_clipped_pm1": ({"adam", "adam_exact_bad"}, set()),
}


def _tripped(d):
    return {k for k, v in d["fields"].items() if (v != 0 if k.endswith("_bad") else v > 1.0)}


def test_teeth_clean_runs_pass(teeth):
    clean = [d for n, d in teeth.items() if n.startswith("clean_")]
    assert len(clean) >= 4
    for d in clean:
        assert d["pass"] and not d["stopped"] and not _tripped(d), d
    assert set(teeth) == {d["run"] for d in clean} | set(FAULTS)


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_teeth_fault_trips_its_own_fields(teeth, fault):
    d = teeth[fault]
    must, may = FAULTS[fault]
    got = _tripped(d)
    assert not d["pass"], d
    assert must <= got <= must | may, (fault, got)
    # a wrong pre_nms stops the chain: nothing downstream ran on it
    pre = {"cls_bad", "score", "box", "keep_bad", "list_bad"}
    assert d["stopped"] == bool(got & pre), d
    if d["stopped"]:
        assert set(d["fields"]) == pre, d
