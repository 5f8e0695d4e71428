"""The attack step with each patch-to-scene matcher on one build (BASELINE config C2: D0 512x512, 16
images, injected placement): ms/step with the mean matcher (BrightnessMatcher, the default) and with
the histogram matcher, and the kernel times of the matcher launches of both from a rocprofv3 kernel
trace.  Prints one JSON line.

    python tools/matcher_bench.py [--batch 16] [--steps 50] [--rounds 3] [--no-trace]

The tool itself opens no GPU: the step times come from one child process (the two matchers timed in
alternating rounds on one victim, a device synchronise around each window), the kernel times from a
second one run under `rocprofv3 --kernel-trace` (tracing slows the host, so it is a run of its own).
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MATCHERS = ("brightness", "histogram")
# the matcher's launches per step: forward (statistics, table, remap) and backward
KERNELS = {"brightness": ("k_eot_ysum", "k_eot_ymean", "k_eot_match", "k_eot_dyc_sum", "k_eot_patch_grad"),
           "histogram": ("k_eot_hist", "k_eot_lut", "k_eot_hmatch", "k_eot_hpatch_grad")}


def setup(a):
    import torch
    from bench import synth_boxes, synth_images
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim, PatchAttacker, _pad_boxes
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.image_size
    victim = EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=B, rng_seed=0,
                                device=0)
    atts = {m: PatchAttacker(victim, seed=7, device=dev, matcher=m) for m in MATCHERS}
    gidx = list(range(B))
    if a.scene == "photo":
        # the two photographs of the reference's own matcher test, enlarged by pixel repetition: most
        # pixels of a wave fall into a few histogram bins (the case the per-wave LDS histograms are for)
        import numpy as np
        d = np.load(os.path.join(ROOT, "tests", "golden", "burj_khalifa_96.npz"))
        f = -(-S // 96)
        ph = [((np.repeat(np.repeat(d[k], f, 0), f, 1)[:S, :S].astype(np.float32) - 127.0) / 127.0)
              for k in ("burj_khalifa_day", "burj_khalifa_sunset")]
        images = torch.as_tensor(np.stack([ph[g % 2] for g in gidx]).astype(np.float32), device=dev)
    else:
        images = torch.as_tensor(synth_images(gidx, S), device=dev)
    boxes = _pad_boxes(synth_boxes(gidx, S), B, dev)
    return torch, atts, images, boxes


def role_time(a):
    torch, atts, images, boxes = setup(a)
    rounds = {m: [] for m in MATCHERS}
    for _ in range(a.rounds):
        for m in MATCHERS:
            for _ in range(a.warmup):
                atts[m].train_step(images, boxes=boxes)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                atts[m].train_step(images, boxes=boxes)
            torch.cuda.synchronize()
            rounds[m].append(round(1e3 * (time.perf_counter() - t0) / a.steps, 4))
    print(json.dumps({"rounds_ms_per_step": rounds,
                      "loss": {m: atts[m].step_metrics()["loss"] for m in MATCHERS}}))


def role_trace(a):
    torch, atts, images, boxes = setup(a)
    for m in MATCHERS:
        for _ in range(a.warmup + a.trace_steps):
            atts[m].train_step(images, boxes=boxes)
    torch.cuda.synchronize()


def kernel_times(path, skip):
    """Mean duration (us) per matcher kernel over its dispatches after the first `skip`."""
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0]
        for k in KERNELS["brightness"] + KERNELS["histogram"]:
            if re.search(rf"\b{k}\b", name):
                d[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    return {k: {"us": round(sum(v[skip:]) / len(v[skip:]), 2), "calls": len(v[skip:])}
            for k, v in d.items() if len(v) > skip}


def child(cmd, limit):
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit(f"matcher_bench: {' '.join(cmd[:3])} ... exited {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace-steps", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--scene", choices=("uniform", "photo"), default="uniform",
                    help="the images: the bench's U(-1,1) noise, or photographs (few occupied histogram bins)")
    ap.add_argument("--role", choices=("time", "trace"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.role == "time":
        return role_time(a)
    if a.role == "trace":
        return role_trace(a)
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(a.batch), "--image-size", str(a.image_size),
          "--steps", str(a.steps), "--warmup", str(a.warmup), "--rounds", str(a.rounds),
          "--trace-steps", str(a.trace_steps), "--scene", a.scene]
    timed = json.loads(child(me + ["--role", "time"], 900).strip().splitlines()[-1])
    kernels = ratio = None
    if not a.no_trace:
        with tempfile.TemporaryDirectory() as tmp:
            child(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "run", "--"]
                  + me + ["--role", "trace"], 900)
            traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
            if not traces:
                sys.exit("matcher_bench: rocprofv3 wrote no kernel trace")
            kernels = kernel_times(traces[0], a.warmup)
        if "k_eot_hist" in kernels and "k_eot_ysum" in kernels:
            ratio = round(kernels["k_eot_hist"]["us"] / kernels["k_eot_ysum"]["us"], 3)
    rounds = timed["rounds_ms_per_step"]
    print(json.dumps({
        "metric": "attack step ms/step by patch-to-scene matcher",
        "unit": "ms/step", "higher_is_better": False,
        "ms_per_step": {m: min(rounds[m]) for m in MATCHERS}, "rounds_ms_per_step": rounds,
        "loss_last_step": timed["loss"],
        "matcher_kernels_us": None if kernels is None else
        {m: {k: kernels.get(k) for k in KERNELS[m]} for m in MATCHERS},
        "k_eot_hist_over_k_eot_ysum": ratio,
        "config": {"workload": f"C2: efficientdet-d0 {a.image_size}x{a.image_size}, {a.batch} images, injected "
                               "placement, train_step (step + Adam)", "scene": a.scene, "steps": a.steps, "warmup": a.warmup,
                   "rounds": a.rounds, "dtype": "f32",
                   "timing": "host clock around a synchronised window, matchers alternating per round, best round; "
                             "kernel times: rocprofv3 --kernel-trace in a run of its own, mean per dispatch"}}))


if __name__ == "__main__":
    main()
