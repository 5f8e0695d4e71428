"""Training summaries: where the results of PatchAttacker.vis_images / PatchAttackDefender.vis_images
go every visualize_freq steps (the reference hands them to TensorBoard, attacker.py:257-305,
attack_detection.py:239-288).

A writer is any object with

    images(tag, u8, step, split)      u8: uint8 [N,H,W,3] (or [H,W,3]), split: "train" / "val"
    series(tag, x, y, step, split)    x, y: 1-D arrays (the ASR curve over its thresholds, the two score
                                      sets of the defender: x the original, y the recovered scores)

passed as ``summary_writer=`` to either class.  Summaries are rank-local, as the reference's are (it
visualises on one GPU): under data parallelism every rank with a writer writes what its own shard
shows, and no collective is issued.  DirWriter writes plain files; TensorBoard event files and the
matplotlib / seaborn plots of the reference are not mirrored (the numbers behind them are).
"""
from __future__ import annotations

import os

import numpy as np


class DirWriter:
    """PNG images and .npz series under ``logdir/train`` and ``logdir/val``:
    ``<split>/<tag>_<step:08d>_<i>.png`` per image of a batch and ``<split>/<tag>_<step:08d>.npz`` with
    arrays ``x`` and ``y`` per series."""

    def __init__(self, logdir):
        self.logdir = str(logdir)

    def _dir(self, split):
        if split not in ("train", "val"):
            raise ValueError("split must be 'train' or 'val'")
        d = os.path.join(self.logdir, split)
        os.makedirs(d, exist_ok=True)
        return d

    def images(self, tag, u8, step, split="train"):
        from PIL import Image
        u8 = np.asarray(u8)
        if u8.dtype != np.uint8 or u8.ndim not in (3, 4) or u8.shape[-1] != 3:
            raise ValueError(f"images: uint8 [N,H,W,3] or [H,W,3] expected, got {u8.dtype} {u8.shape}")
        if u8.ndim == 3:
            u8 = u8[None]
        d = self._dir(split)
        for i, im in enumerate(u8):
            Image.fromarray(np.ascontiguousarray(im)).save(os.path.join(d, f"{tag}_{int(step):08d}_{i}.png"))

    def series(self, tag, x, y, step, split="train"):
        np.savez(os.path.join(self._dir(split), f"{tag}_{int(step):08d}.npz"), x=np.asarray(x), y=np.asarray(y))


def due(writer, step: int, visualize_freq) -> bool:
    """tf.cond(step % visualize_freq == 0, ...) with a writer attached; a visualize_freq of 0 or less
    (or None) means never."""
    return writer is not None and bool(visualize_freq) and visualize_freq > 0 and step % visualize_freq == 0


def write(writer, results: dict, step: int, split: str):
    """Hands a vis_images dict to a writer: uint8 arrays as images, (x, y) pairs as series."""
    for tag, v in results.items():
        if isinstance(v, tuple):
            writer.series(tag, v[0], v[1], step, split)
        else:
            writer.images(tag, v, step, split)
