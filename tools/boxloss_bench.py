"""What the box-regression term (phx_set_box_loss: the reference's InverseDIOULoss) costs a C2 step: EfficientDet-D0
at 512^2, 16 images, injected boxes, f32 (bench.py's flagship configuration, its images and boxes), as two arms:

  off   PatchAttacker(victim)                         the step as bench.py times it
  on    PatchAttacker(victim, box_loss="inv_diou")    + the idiou kernels, the box scatter and the box head's backward

and the term's own kernels alone (launch groups "idiou": k_idiou_part / _merge / _batch, and "box_scatter":
k_box_scatter) from a profiled run of the `on` arm, with the whole backward's groups beside them.  Prints one JSON
line; --out writes it to a file as well.

    python tools/boxloss_bench.py [--steps 100] [--warmup 10] [--rounds 5] [--out profiles/boxloss_bench.json]

Timing (tools/nms_bench.py's method): a window is `steps` back-to-back train_step calls between two HIP events on the
stream after `warmup` untimed ones; the arms are interleaved round by round in one process, each on its own victim
context (a change of the setting makes a context plan its executors again), and the best window of each is reported
with all the rounds.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, B, MODEL = 512, 16, "efficientdet-d0"
WEIGHT = 0.0625


def window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 50:
        sys.exit("boxloss_bench: at least 50 timed steps per window")
    import numpy as np
    import torch

    import bench
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim, PatchAttacker, _pad_boxes
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    gidx = np.arange(B)
    images = torch.as_tensor(bench.synth_images(gidx, S), device=dev)
    boxes = _pad_boxes(bench.synth_boxes(gidx, S), B, dev)
    arms, atts = {}, {}
    for name, kind in (("off", None), ("on", "inv_diou")):
        victim = EfficientDetVictim(MODEL, "synthetic", seed=0, image_size=S, max_batch=B, rng_seed=0, device=0)
        att = PatchAttacker(victim, seed=7, device=dev, box_loss=kind, box_loss_weight=WEIGHT)
        atts[name] = att
        arms[name] = (lambda t=att: t.train_step(images, boxes=boxes))
    for k in arms:
        for _ in range(a.warmup):
            arms[k]()
    torch.cuda.synchronize()
    rounds = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k in arms:
            rounds[k].append(window(torch, arms[k], a.steps))
    out = {"metric": "one C2 attack step with and without the box-regression term", "unit": "ms",
           "higher_is_better": False, "model": MODEL, "image_size": S, "batch": B}
    for k in arms:
        out[k] = {"ms_per_step": round(min(rounds[k]), 4), "rounds_ms": [round(v, 4) for v in rounds[k]],
                  "workspace_bytes": atts[k].model.ctx.workspace_bytes(B)}
    out["on_minus_off_ms"] = round(min(rounds["on"]) - min(rounds["off"]), 4)
    out["on_over_off"] = round(min(rounds["on"]) / min(rounds["off"]), 4)
    m = atts["on"].step_metrics()
    out["box_loss_last_step"] = m["box_loss"]
    # the term's own launch groups, and the step's others for scale, from profiled steps (one stream, an event
    # pair around every launch group)
    ctx = atts["on"].model.ctx
    ctx.profile(True)
    for _ in range(a.profile_steps):
        arms["on"]()
    torch.cuda.synchronize()
    rep = ctx.profile_report()
    ctx.profile(False)
    out["kernels_alone_ms_per_step"] = {k: round(v["ms"] / a.profile_steps, 5) for k, v in rep.items()
                                        if k in ("idiou", "box_scatter")}
    out["profiled_groups_ms_per_step"] = {k: round(v["ms"] / a.profile_steps, 4) for k, v in sorted(rep.items())}
    out["config"] = {"dtype": "f32", "weights": "synthetic", "placement": "injected", "box_loss_weight": WEIGHT,
                     "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "profile_steps": a.profile_steps,
                     "timing": "HIP events around a window of back-to-back train_step calls on one stream, arms "
                               "interleaved round by round in one process, best window; kernels alone: the "
                               "library's per-launch-group events over profiled steps"}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
