"""The U-Net kernel parity checker (tests/kernels/unet_parity), host side: what its case table covers, read from
`unet_parity --plan` (the column reductions' row blocks come from the library's own un_colred_plan_info: no GPU
needed), the kink share by the reference alone, the golden Dropout / shuffle / flip draws against
oracle/defender.py, and the teeth of its references and bounds, driven by a CPU stand-in with seeded faults
(unet_teeth).

`python tests/test_unet_parity_host.py --write` rewrites tests/golden/unet from the oracle and the plan."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
GOLD = os.path.join(ROOT, "tests", "golden", "unet")

# the keys of the harness's draws (unet_check.hpp) and the size up to which a case's keep flags are committed
SEED_POOL, SEED_CAT, SEED_PERM = 0x5eed0000beef, 0x5eed0000cafe, 0x5eed0000d00d
GOLDEN_MAX_FLAGS = 40000

# What the issue puts out of scope, with the arithmetic (every listed edge is reached with the default PHX_UN_RED_* values):
UNPINNED = {
    # counter word 3 is (uint32)(step << 8) | stream: steps >= 2^24 alias earlier ones
    "Philox counter: step << 8 truncates at steps >= 2^24": "out of scope (a 16.7 M-step run)",
    # counter word 0 is (uint32) of the element index within the image
    "Dropout element indices >= 2^32": "out of scope (an image of 4.3 G elements)",
}


def _binary(name):
    path = os.path.join(KERN, name)
    if not os.path.isfile(path):
        if name == "unet_parity" and not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/unet_parity is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", name], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return path


def _lines(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert out and out[-1].get("done") is True, r.stdout[-500:]
    return out[:-1]


def _plan():
    out = _lines([_binary("unet_parity"), "--plan"])
    assert out[0]["head"] is True
    return out[0], out[1:]


@pytest.fixture(scope="module")
def plan_all():
    return _plan()


@pytest.fixture(scope="module")
def plan(plan_all):
    return plan_all[1]


@pytest.fixture(scope="module")
def teeth():
    return {d["run"]: d for d in _lines([_binary("unet_teeth")])}


def _op(plan, *ops):
    return [c for c in plan if c["op"] in ops]


def test_names_are_unique_and_the_list_is_the_table(plan):
    names = [c["case"] for c in plan]
    assert len(set(names)) == len(names) and 150 < len(names) < 260
    from test_gpu_unet_kernels import CASES
    assert CASES == names


def test_head(plan_all):
    head = plan_all[0]
    assert head["red_elems"] == 8192 and head["red_maxblk"] == 1024   # the default PHX_UN_RED_* values
    assert head["golden_read"] is True
    # the attention backward's reference against central differences of the fp64 forward (M 3, C 4, step 1e-6)
    assert head["fd_gap"] <= 1e-6


def test_column_reduction_coverage(plan):
    for op in ("bn_stats", "bn_bwd", "colsum"):
        cs = _op(plan, op)
        assert {c["C"] for c in cs} == {1, 3, 8, 24, 64, 100, 128, 129, 256}, op
        for c in cs:
            r = c["red"]
            assert r["check_same"], c["case"]                  # the harness's geometry is the library's
            assert r["lane_rows"] == 256 // c["C"] and r["idle"] == 256 - (256 // c["C"]) * c["C"], c["case"]
        idle = {c["C"]: c["red"]["idle"] for c in cs}
        assert idle[24] == 16 and idle[100] == 56 and idle[129] == 127 and idle[3] == 1
        assert any(c["M"] == 1 for c in cs)
        assert any(1 < c["M"] < c["red"]["lane_rows"] for c in cs)            # fewer rows than lane groups
        assert {1, 2, 65} <= {c["red"]["blocks"] for c in cs}, op
        assert any(c["red"]["blocks"] > 1 and 0 < c["red"]["last_rows"] < c["red"]["rpb"] for c in cs)   # a short last block
        # C = 1 and C = 3 with many blocks; finals whose workgroup has waves past C
        assert any(c["C"] == 1 and c["red"]["blocks"] >= 65 for c in cs) and any(c["C"] == 3 and c["red"]["blocks"] >= 65 for c in cs)
        assert any(c["C"] % 4 for c in cs)
    st = _op(plan, "bn_stats")
    # the 8-deep body bracketed for every C
    for C in (1, 3, 8, 24, 64, 100, 128, 129, 256):
        ms = {c["M"] for c in st if c["C"] == C}
        lr = 256 // C
        assert {8 * lr - 1, 8 * lr, 8 * lr + 1} <= ms, C
    assert {1, 2, 64, 65, 193, 257, 1024} <= {c["red"]["blocks"] for c in st}
    capped = [c for c in st if c["red"]["blocks"] == 1024]
    assert all(c["M"] * c["C"] > 8192 * 1024 for c in capped)
    assert any(c["red"]["last_rows"] <= 0 for c in capped)                     # blocks that start past M
    # and below the cap: (nb - 1) ceil(M / nb) reaches M where 8192 / C is no whole number (129 x 4096: 65 blocks of 64)
    for op in ("bn_stats", "bn_bwd", "colsum"):
        assert any(c["red"]["last_rows"] <= 0 and c["red"]["blocks"] < 1024 for c in _op(plan, op)), op
    assert {c["flav"] for c in st} == {0, 1}                                   # moving statistics null and present
    assert any(c["data"] == 1 and c["C"] > 1 for c in st) and any(c["data"] == 2 for c in st)   # 1e3 x spread, constant
    assert any(c["M"] == 1 and c["flav"] == 1 for c in st)                     # variance 0, no Bessel
    bw = _op(plan, "bn_bwd")
    assert {c["act"] for c in bw} == {0, 1}
    assert {193, 257} <= {c["red"]["blocks"] for c in bw}
    assert {1, 255, 256, 257} <= {c["n"] for c in bw} and any(c["sweeps"] == 2 for c in bw)   # k_un_bnb_apply
    assert any(c["red"]["blocks"] == 193 for c in _op(plan, "colsum"))
    assert len(UNPINNED) == 2


def test_elementwise_coverage(plan):
    for op in ("bnact", "att_s", "att_s_bwd", "small_dgrad"):
        cs = _op(plan, op)
        assert {1, 255, 256, 257} <= {c["n"] for c in cs}, op
        assert {c["sweeps"] for c in cs} == {1, 2}, op
        assert {1, 3, 8, 64} <= {c["C"] for c in cs}, op
    assert {c["act"] for c in _op(plan, "bnact")} == {0, 1}
    sd = _op(plan, "small_dgrad")
    assert {(c["O"], c["acc"]) for c in sd} == {(1, 0), (1, 1), (3, 0), (3, 1)}
    ad = _op(plan, "add")
    assert {1, 255, 256, 257} <= {c["n"] for c in ad} and any(c["sweeps"] == 2 for c in ad)
    at = _op(plan, "att_t")
    assert {(c["M"], c["C"]) for c in at} >= {(m, k) for m in (1, 257) for k in (1, 8, 64)}
    assert any(c["sweeps"] == 2 for c in at)


def test_pool_coverage(plan):
    ps = _op(plan, "pool_drop")
    shapes = {(c["B"], c["H"], c["W"], c["C"]) for c in ps}
    assert {(1, 2, 2, 1), (2, 4, 6, 3), (1, 5, 7, 8), (3, 16, 16, 16)} <= shapes
    assert {c["layer"] for c in ps} == {-1, 0, 1, 2, 3}
    assert any(c["sweeps"] == 2 and c["layer"] >= 0 for c in ps)
    assert any(c["gimg0"] and c["B"] >= 2 for c in ps)
    assert len({c["step"] for c in ps if (c["B"], c["H"], c["W"], c["C"], c["layer"]) == (2, 4, 6, 3, 0)}) == 2
    for c in ps:
        assert c["flags"]["has_ties"], c["case"]
        if c["layer"] >= 0:
            odd = (c["H"] | c["W"]) & 1
            want = {"dx_exact_fwd_acc", "dx_exact_map_acc"} | (set() if odd else {"dx_exact_fwd", "dx_exact_map", "dropped_taps_zero"})
            assert want <= set(c["flags"]), c["case"]
            assert c["golden_used"] == (c["n"] <= GOLDEN_MAX_FLAGS), c["case"]
    rf = {c["refuse"] for c in plan if c["refuse"]}
    assert rf == {1, 2, 3, 4, 5}     # pool backward odd H / odd W without acc; att_cat_bwd C 0, 3, 128


def test_attention_and_output_coverage(plan):
    cs = _op(plan, "att_cat")
    assert {c["C"] for c in cs} == {1, 2, 4, 8, 16, 32, 64}
    assert {c["layer"] for c in cs} == {-1, 4, 5, 6, 7}
    assert {(c["B"] * c["HW"], c["C"]) for c in cs} >= {(5, 8), (33, 8)}       # clamped lanes beside live ones
    assert all((c["B"] * c["HW"] * c["C"]) % 256 for c in cs)
    assert any(c["B"] == 2 and (c["HW"] * c["C"]) % 256 and c["HW"] * c["C"] < 256 for c in cs)   # an image boundary in a workgroup
    assert any(c["flav"] == 1 and c["layer"] >= 0 for c in cs) and any(c["flav"] == 1 and c["layer"] < 0 for c in cs)
    assert all(c["golden_used"] for c in cs if c["layer"] >= 0)
    os_ = _op(plan, "out_loss")
    assert {c["C"] for c in os_} == {1, 5, 8}
    assert {(c["B"], c["HW"]) for c in os_} == {(1, 1), (1, 255), (3, 257), (1, 262145)}
    assert any(c["sweeps"] == 2 for c in os_) and all(c["loss_blocks"] == c["check_loss_blocks"] for c in os_)
    assert any(c["flav"] == 1 and c["flags"]["loss_zero"] for c in os_)
    assert all(c["flags"]["z_reaches_8"] for c in os_)


def test_masker_coverage(plan):
    pm = _op(plan, "def_perm_crops")
    assert {c["B"] for c in pm} == {1, 2, 5, 257}
    assert any(c["H"] != c["W"] for c in pm)
    assert any(c["P"] == 1 for c in pm) and any(1 < c["P"] < min(c["H"], c["W"]) for c in pm) and any(c["P"] == c["H"] == c["W"] for c in pm)
    # a non-identity permutation and all four flip combinations, by the oracle
    from oracle import defender
    combos, non_identity = set(), False
    for c in pm:
        perm = defender.shuffle_perm(c["B"], SEED_PERM, c["step"], c["gimg0"])
        non_identity |= c["B"] <= 5 and list(perm) != list(range(c["B"]))
        combos |= {defender.flips(SEED_PERM, c["step"], c["gimg0"] + b) for b in range(c["B"])}
    assert non_identity and len(combos) == 4
    fl = _op(plan, "def_filter")
    assert {c["B"] for c in fl} == {1, 5, 64, 65}
    assert {c["nc_mode"] for c in fl} == {0, 1, 2, 3}          # mixed, nc 0, nc = maxo, all rejected
    assert {0, 1, 15} <= {c["sets"] for c in fl} and any(c["sets"] & 1 == 0 for c in fl)
    assert any(c["flav"] == 1 and c["flags"]["edges_planted"] for c in fl)


def test_kink_share_and_standin(plan):
    for c in plan:
        assert c["kink_share"] <= 0.01, c["case"]     # by the fp64 reference alone
        assert c["standin_pass"], c
        if not c["refuse"]:
            assert c["nonfinite"] == 0 and c["ratio"] <= 1.0 and c["exact_ok"], c


# ---- the golden draws -------------------------------------------------------------------------------
def _golden_text(plan):
    sys.path.insert(0, ROOT)
    from oracle import defender
    drops, perms = {}, {}
    for c in plan:
        if c["op"] == "pool_drop" and c["layer"] >= 0:
            key, shape = (SEED_POOL, c["step"], c["gimg0"], c["layer"], c["B"]), (c["H"] // 2, c["W"] // 2, c["C"])
        elif c["op"] == "att_cat" and c["layer"] >= 0:
            key, shape = (SEED_CAT, c["step"], c["gimg0"], c["layer"], c["B"]), (1, c["HW"], 2 * c["C"])
        elif c["op"] == "def_perm_crops":
            perms[(SEED_PERM, c["step"], c["gimg0"], c["B"])] = None
            continue
        else:
            continue
        n = shape[0] * shape[1] * shape[2]
        if c["B"] * n <= GOLDEN_MAX_FLAGS:
            drops[key + (n,)] = shape
    dtxt = []
    for (seed, step, g0, layer, B, n), shape in sorted(drops.items()):
        keep = defender.dropout_mask((B,) + shape, layer, seed, step, g0).reshape(B, n)
        dtxt.append(f"{seed:x} {step} {g0} {layer} {B} {n}")
        dtxt += ["".join("1" if k else "0" for k in row) for row in keep]
    ptxt = []
    for seed, step, g0, B in sorted(perms):
        perm = defender.shuffle_perm(B, seed, step, g0)
        fl = [defender.flips(seed, step, g0 + b) for b in range(B)]
        ptxt.append(f"{seed:x} {step} {g0} {B}")
        ptxt.append(" ".join(str(int(p)) for p in perm))
        ptxt.append(" ".join(f"{int(lr)} {int(ud)}" for lr, ud in fl))
    return "\n".join(dtxt) + "\n", "\n".join(ptxt) + "\n"


def test_golden_files_are_the_oracles_draw(plan):
    """tests/golden/unet holds dropout_mask, shuffle_perm and the flip draw of oracle/defender.py (through
    oracle/philox.py) for every case that draws; the harness holds its restated Philox equal to them."""
    dtxt, ptxt = _golden_text(plan)
    assert open(os.path.join(GOLD, "drop_keep.txt")).read() == dtxt
    assert open(os.path.join(GOLD, "perm_flip.txt")).read() == ptxt
    keep = [x for x in dtxt.split("\n") if x and " " not in x]
    share = sum(x.count("1") for x in keep) / sum(len(x) for x in keep)
    assert 0.75 < share < 0.85                       # Dropout(0.2)
    for c in plan:
        if c["golden_used"]:
            assert c["flags"]["golden_found"] and c["flags"]["golden_is_philox"], c["case"]
    names = open(os.path.join(GOLD, "cases.txt")).read().split()
    assert names == [c["case"] for c in plan]


CLEAN = ("clean_colsum", "clean_colsum_blk65", "clean_stats", "clean_stats_moving", "clean_bn_bwd", "clean_bnact", "clean_att_s",
         "clean_att_s_bwd", "clean_att_t", "clean_small_dgrad", "clean_add", "clean_pool", "clean_att_cat",
         "clean_att_cat_saturated", "clean_out", "clean_out_target_is_output", "clean_perm", "clean_filter")

# fault -> the fields / flags that must report it (every other one of the run must stay clean)
FAULTS = {
    "block_last_row_dropped": ("sum",),
    "idle_threads_rows_added": ("sum",),
    "block_64_skipped": ("sum",),
    "shift_not_added_back": ("mean",),
    "bessel_missing": ("moving",),
    "last_maximum": ("arg_exact",),
    "pool_bwd_scale_missing": ("dx_exact_fwd", "dx_exact_fwd_acc", "dx_exact_map", "dx_exact_map_acc"),
    "element_index_not_restarted": ("out_exact",),
    "xor_tree_one_step_short": ("dz3",),
    "clamped_lane_stores": ("dup_exact",),
    "sigmoid_derivative_missing": ("dz3",),
    "loss_divided_by_m": ("loss",),
    "un_out_other_order": ("upd_bit_equal",),
    "filter_area_ge": ("boxes_exact", "count_exact"),
    "filter_tail_rows_unzeroed": ("boxes_exact",),
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


if __name__ == "__main__" and "--write" in sys.argv:
    # the plan's geometry does not depend on the golden files; its golden_* flags do, so write first, then test
    r = subprocess.run([_binary("unet_parity"), "--plan"], capture_output=True, text=True)
    cases = [json.loads(x) for x in r.stdout.splitlines() if '"case"' in x]
    os.makedirs(GOLD, exist_ok=True)
    d, p = _golden_text(cases)
    open(os.path.join(GOLD, "drop_keep.txt"), "w").write(d)
    open(os.path.join(GOLD, "perm_flip.txt"), "w").write(p)
    open(os.path.join(GOLD, "cases.txt"), "w").write("\n".join(c["case"] for c in cases) + "\n")
    print(len(cases), "cases,", len(d), "+", len(p), "bytes")
