"""The executor's plan (csrc/exec_plan.hpp), checked on the CPU: tests/kernels/exec_plan prints the plan of a
configuration as one JSON line (plan_exec makes no HIP call), and every line must equal the recording in
tests/golden/exec_plan/plans.json, which was taken from the executor before the planner was split from
its allocator (DESIGN.md says from which commit and how to regenerate it).  A planner change that is
meant to change a plan regenerates the golden; anything else that moves a field fails here."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERN = os.path.join(ROOT, "tests", "kernels")
GOLDEN = os.path.join(ROOT, "tests", "golden", "exec_plan", "plans.json")

MODELS = ["efficientdet-d%d" % i for i in range(8)] + ["efficientdet-lite%d" % i for i in range(5)]


def _specs():
    out = []
    # the flagship: tag 0 the step's executor, tag 1 the concurrent first pass's, tag 2 the serving
    # executor, which only a batch-statistics context creates (a bn=frozen context serves from tag 0)
    for B in (1, 2, 16):
        for bn in ("local", "frozen", "sync"):
            for dt in ("f32", "bf16"):
                for tag in (0, 1, 2):
                    if tag == 2 and bn == "frozen":
                        continue
                    out.append("efficientdet-d0:512:%d:%d:%s:%s" % (B, tag, bn, dt))
    # the small size of the GPU tests (tests/test_gpu_exec_plan.py reads these lines' bytes; nothing
    # builds a bn=frozen context's tag 1 executor: its steps run on one stream)
    for B in (1, 2):
        for bn in ("local", "frozen"):
            for dt in ("f32", "bf16"):
                for tag in (0, 1) if bn == "local" else (0,):
                    out.append("efficientdet-d0:128:%d:%d:%s:%s" % (B, tag, bn, dt))
    # every other model at its default size: drop connect, the other fuse methods and head widths
    out += ["%s:0:2:0:local:f32" % m for m in MODELS if m != "efficientdet-d0"]
    return out


KNOB_SPEC = "efficientdet-d0:512:16:0:local:f32"
# variant -> (environment, specs); PHX_FOLD / PHX_GROUP are read once per process, so each variant is
# a process of its own
VARIANTS = {"default": ({}, _specs())}
for _k in ("PHX_SEP", "PHX_SEP_MINROWS", "PHX_SEPB", "PHX_GROUP", "PHX_FOLD"):
    VARIANTS[_k + "=0"] = ({_k: "0"}, [KNOB_SPEC])

KNOBS = ("PHX_SEP", "PHX_SEP_MINROWS", "PHX_SEPB", "PHX_GROUP", "PHX_FOLD")


def _binary():
    path = os.path.join(KERN, "exec_plan")
    if not os.path.isfile(path):
        if not (shutil.which("hipcc") or os.path.isfile("/opt/rocm/bin/hipcc")):
            pytest.fail("tests/kernels/exec_plan is missing and there is no hipcc to build it")
        r = subprocess.run(["make", "-C", KERN, "-j8", "exec_plan"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return path


def _dump(variant, full=False):
    env_add, specs = VARIANTS[variant]
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_add)
    cmd = [_binary()] + (["--full"] if full else []) + specs
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    out = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert out and out[-1].get("done") is True, r.stdout[-500:]
    assert [d["config"] for d in out[:-1]] == specs
    return {d["config"]: d for d in out[:-1]}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dumps():
    return {v: _dump(v) for v in VARIANTS}


def test_golden_covers_the_configurations(golden):
    assert set(golden["plans"]) == set(VARIANTS)
    for v, (_, specs) in VARIANTS.items():
        assert set(golden["plans"][v]) == set(specs), v


def _pack(golden, d):
    """A dump line in the golden's form: the scalars in scalar_keys order, (length, set entries) per
    vector in vector_keys order, and one hash over the vectors' content hashes."""
    sk, vk = golden["scalar_keys"], golden["vector_keys"]
    assert set(d) == set(sk) | set(vk) | {"config"}, sorted(set(d) ^ (set(sk) | set(vk) | {"config"}))
    h = hashlib.sha256("".join(d[k]["hash"] for k in vk).encode()).hexdigest()[:16]
    return {"s": [d[k] for k in sk], "v": [[d[k]["n"], d[k]["set"]] for k in vk], "h": h}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_plan_equals_the_recording(golden, dumps, variant):
    sk, vk = golden["scalar_keys"], golden["vector_keys"]
    for spec, want in golden["plans"][variant].items():
        got = _pack(golden, dumps[variant][spec])
        diff = [(k, w, g) for k, w, g in zip(sk, want["s"], got["s"]) if w != g]
        diff += [(k, w, g) for k, w, g in zip(vk, want["v"], got["v"]) if w != g]
        assert not diff, (variant, spec, diff[:6])
        # (the vectors' contents; `exec_plan --full` of two builds shows which entries moved)
        assert got["h"] == want["h"], (variant, spec)
        # "bytes" is the allocator's: tests/test_gpu_exec_plan.py


def test_the_knobs_change_what_they_name(dumps):
    """Each variant differs from the default plan in the fields its knob governs (the variants are not
    vacuous), and a recording exists for the plan it leaves."""
    base = dumps["default"][KNOB_SPEC]
    assert base["sep"]["set"] > 0 and base["sepb"]["set"] > 0 and base["n_groups"] > 0 and base["fuse_folded"]["set"] > 0
    assert dumps["PHX_SEP=0"][KNOB_SPEC]["sep"]["set"] == 0
    assert dumps["PHX_SEP_MINROWS=0"][KNOB_SPEC]["sep"]["set"] > base["sep"]["set"]
    sb = dumps["PHX_SEPB=0"][KNOB_SPEC]
    assert sb["sepb"]["set"] == 0 and sb["sep"] == base["sep"]
    assert dumps["PHX_GROUP=0"][KNOB_SPEC]["n_groups"] == 0
    assert dumps["PHX_FOLD=0"][KNOB_SPEC]["fuse_folded"]["set"] == 0


def test_no_plan_fuses_a_grouped_depthwise_with_ungrouped_pointwise(dumps):
    """The planner no longer has the branch: no configuration here would have taken it."""
    for v in dumps:
        for spec, d in dumps[v].items():
            assert d["sep_grouped_dw_ungrouped_pw"] == 0, (v, spec)


SWEEP = ["%s:%d:%d:0:%s:%s" % (m, size, B, bn, dt) for m in MODELS for size in (0, 128, 320)
         for B in (1, 2, 3, 4, 8, 16) for bn in ("local", "sync") for dt in ("f32", "bf16")]


@pytest.mark.parametrize("minrows", [None, "0"])
def test_no_plan_of_a_wider_sweep_does_either(minrows):
    """Every model x {default, 128, 320} x six batch sizes x {local, sync} x {f32, bf16}, at the default
    row threshold and with every level fused (PHX_SEP_MINROWS=0): 1872 plans, none with a fused sepconv
    whose depthwise ops are grouped and whose pointwise ops are not (a few seconds of host planning)."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    if minrows is not None:
        env["PHX_SEP_MINROWS"] = minrows
    r = subprocess.run([_binary()] + SWEEP, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == len(SWEEP) + 1 and lines[-1].get("done") is True
    assert [d["config"] for d in lines[:-1] if d["sep_grouped_dw_ungrouped_pw"]] == []
    assert any(d["sep"]["set"] for d in lines[:-1])


def test_only_a_same_padded_depthwise_is_folded_or_fused():
    """The planner's eligibility test on hand-built programs (exec_plan --guard): a 3x3 stride-1 depthwise
    op after a BiFPN fuse and before a 1x1 conv is folded / fused when it pads SAME, and not when it pads
    VALID, keeps the size without a top / left pad, or has depth multiplier 2."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([_binary(), "--guard"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {d["case"]: (d["fuse_folded"], d["sep"]) for d in map(json.loads, r.stdout.splitlines()) if "case" in d}
    assert got == {"same": (1, 1), "valid": (0, 0), "same_size_no_pad": (0, 0), "multiplier_2": (0, 0)}


def test_full_dump_carries_the_vectors():
    d = _dump("PHX_SEP=0", full=True)[KNOB_SPEC]
    assert len(d["grp_of"]["v"]) == d["grp_of"]["n"] == d["n_ops"]
    assert sum(1 for x in d["fused_bn"]["v"] if x > 0) == d["fused_bn"]["set"]
