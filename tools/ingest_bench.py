"""Stream-ingest throughput: phx_ingest (streaming.Stream.change_frame_size on the device) on 16
device-resident frames per case, against a torch device-to-device copy that moves the same number of
bytes in the same run.

  1080x1920 -> 640   sparse bilinear taps (every third source row and column is touched)
  720x1280  -> 640   the 2x box: every source byte is read
  360x640   -> 1280  upscale: write-bound

Algorithmic bytes of a frame: min(source bytes, 12 x output pixels) read + 3 x output pixels written.
The yardstick copy moves half of that from one buffer to another, so it reads and writes the same total.
Each case runs with 4-byte aligned output offsets (the dword stores) and with the output one byte off
(the byte stores): that is the A/B of the two store paths, in one process.

Timing: device events around one call, the kernel legs and the copy alternating; a 64 MiB device copy is
enqueued in front of every timed call so that the host has finished enqueueing before the device gets
there (the call is a 512-byte table copy plus one kernel, and an idle device would time the enqueue).
The median over --iters is reported.  The upload of the raw frames from pageable host memory
(detector.pack_frames) is timed separately with a host clock and is not part of the kernel's figure.
Prints one JSON line; --out also writes it to a file.

    python tools/ingest_bench.py [--frames 16] [--iters 30] [--out profiles/ingest_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mladversarialobjectdetection_amd import _lib  # noqa: E402
from mladversarialobjectdetection_amd.detector import pack_frames  # noqa: E402
from mladversarialobjectdetection_amd.streaming import ingest_dims  # noqa: E402

CASES = [("1080p_to_640_linear", 1080, 1920, 640), ("720p_to_640_box", 720, 1280, 640),
         ("360p_to_1280_upscale", 360, 640, 1280)]


def algorithmic_bytes(h, w, dh, dw, n):
    return n * (min(h * w * 3, 12 * dh * dw) + 3 * dh * dw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench: no GPU (nothing is measured without one)")
    B = a.frames
    dev = torch.device("cuda", 0)
    ctx = _lib.Context("efficientdet-d0", 0, B)
    stream = torch.cuda.current_stream().cuda_stream
    filler_a = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    filler_b = torch.empty_like(filler_a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        filler_b.copy_(filler_a)
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    results = []
    rng = np.random.default_rng(0)
    for name, h, w, sw in CASES:
        frames = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
        pack_frames(frames, dev)  # untimed: the first upload of a size pays for its host and device buffers
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = pack_frames(frames, dev)
        torch.cuda.synchronize()
        upload_s = time.perf_counter() - t0
        dh, dw = (int(v) for v in ingest_dims(sw, [(h, w)])[0])
        fsz = dh * dw * 3
        ooff = np.arange(B, dtype=np.int64) * fsz
        out = torch.empty(B * fsz + 16, dtype=torch.uint8, device=dev)
        nbytes = algorithmic_bytes(h, w, dh, dw, B)
        ca = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        cb = torch.empty_like(ca)

        def ingest(shift):
            ctx.call("phx_ingest", p.src.data_ptr(), p.offsets.ctypes.data, p.dims.ctypes.data, B, sw, 0,
                     out.data_ptr() + shift, ooff.ctypes.data, stream)

        legs = {"dword_stores": lambda: ingest(0), "byte_stores": lambda: ingest(1), "copy": lambda: cb.copy_(ca)}
        for fn in legs.values():  # warm up every leg
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.iters):
            for k, fn in legs.items():
                ms[k].append(timed(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        gbs = {k: nbytes / (med[k] * 1e-3) / 1e9 for k in med}
        results.append({
            "case": name, "frames": B, "src": [h, w], "set_width": sw, "out": [dh, dw],
            "algorithmic_bytes": nbytes,
            "ms_per_batch": {k: round(v, 4) for k, v in med.items()},
            "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
            "gb_per_s": {k: round(v, 1) for k, v in gbs.items()},
            "fraction_of_copy_rate": {k: round(gbs[k] / gbs["copy"], 3) for k in ("dword_stores", "byte_stores")},
            "upload": {"bytes": int(frames.nbytes), "seconds": round(upload_s, 4),
                       "gb_per_s": round(frames.nbytes / upload_s / 1e9, 2),
                       "what": "pack_frames: np.concatenate on the host + one pageable host-to-device copy, host clock"},
        })
    line = json.dumps({
        "metric": "phx_ingest ms per batch and GB/s of algorithmic bytes, against a device copy of the same bytes",
        "unit": "GB/s", "higher_is_better": True, "results": results,
        "config": {"iters": a.iters, "timing": "device events around one call behind a 64 MiB filler copy; median",
                   "copy": "torch uint8 copy_ of algorithmic_bytes / 2 (reads + writes = algorithmic_bytes)"}})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
