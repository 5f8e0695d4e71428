"""Host-side mirror of the reference's attack interface (attacker.py, brightness_matcher.py,
util.get_victim_model) over the libphx C ABI.

Same names, argument meaning and error behaviour as the reference where they exist:

  EfficientDetVictim       util.get_victim_model (util.py:177-189) + KerasDriver (infer_lib.py:383)
  BrightnessMatcher.call   brightness_matcher.py:43-73
  HistogramMatcher.call    brightness_matcher.py:82-115
  Patcher.call             attacker.py:490-498
  PatchAttacker            attacker.py:24-341: first_pass :91, second-pass loss and gradient in
                           call :172-219, calc_asr :238, train_step :307, save_weights :328

Every computation runs in the HIP kernels of libphx.so on PyTorch-ROCm device memory; PyTorch
provides only allocation, streams and torch.distributed (RCCL).  Data parallelism: one process per
GPU, each holding B/world images; the [patch | scale] gradient is SUM-all-reduced once per step
(bn=local: statistics per rank).
"""
from __future__ import annotations

import ctypes
import math
import os
from collections.abc import Mapping
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from . import distributed as ddp
from . import summaries
from . import tiff
from . import weights as wmod

MEAN_RGB = {"efficientdet": [0.485 * 255, 0.456 * 255, 0.406 * 255], "lite": [127.0] * 3}
STDDEV_RGB = {"efficientdet": [0.229 * 255, 0.224 * 255, 0.225 * 255], "lite": [128.0] * 3}


def _stream():
    return torch.cuda.current_stream().cuda_stream


@dataclass
class NmsConfig:
    """hparams_config.py:258-266 (+ attacker_train.py:31 override); mirrors the library context once
    honour_nms_configs forwards it (VictimConfig.override)"""
    method: str | None = "gaussian"
    iou_thresh: float | None = None
    score_thresh: float = 0.0
    sigma: float | None = None
    max_output_size: int = 100


@dataclass
class VictimConfig:
    name: str
    image_size: int
    mean_rgb: list
    stddev_rgb: list
    nms_configs: NmsConfig = field(default_factory=NmsConfig)
    # the library context this config describes (set by EfficientDetVictim): overrides that change
    # the computation are forwarded to it, as the reference's model.config.override reaches the model
    ctx: object = field(default=None, repr=False, compare=False)
    # False: nms_configs other than the reference's defaults (method 'gaussian', sigma 0.5, max_output_size
    # 100) are refused and iou_thresh is ignored, as before the library honoured them.  True: method, iou_thresh,
    # sigma and max_output_size reach the library context as postprocess.nms reads them.
    honour_nms_configs: bool = False

    def override(self, d: dict, ctx=None):
        """Config.override (hparams_config.py:91-109) for the keys the attack uses.  The values that
        change the computation are forwarded to the library context (score_thresh; with honour_nms_configs
        also method, iou_thresh, sigma, max_output_size); overrides the library does not implement raise
        instead of diverging silently from the reference."""
        ctx = ctx if ctx is not None else self.ctx
        for k, v in d.items():
            if k != "nms_configs":
                raise ValueError(f"config_override: unsupported key {k!r} (only nms_configs)")
            for kk, vv in v.items():
                if kk == "score_thresh":
                    if ctx is None:
                        raise ValueError("config_override: score_thresh needs the victim's library context "
                                         "(a VictimConfig not owned by an EfficientDetVictim)")
                    ctx.set_score_thresh(float(vv))
                elif kk in ("pyfunc", "max_nms_inputs"):
                    if vv:
                        raise ValueError(f"config_override: nms_configs.{kk} = {vv!r} is not built")
                elif kk == "max_output_size" and vv is not None and vv > 100:
                    raise ValueError("config_override: max_output_size is fixed at 100")
                elif kk in ("method", "iou_thresh", "sigma", "max_output_size") and self.honour_nms_configs:
                    self._forward_nms(ctx, kk, vv)
                elif kk == "iou_thresh":
                    pass  # unused by the gaussian method: iou_thresh = 1.0 (postprocess.py:184-188)
                elif kk == "method" and vv != "gaussian":
                    raise ValueError("config_override: only nms method 'gaussian' (the reference's) is built")
                elif kk == "sigma" and vv not in (None, 0.5):
                    raise ValueError("config_override: soft-NMS sigma is fixed at the default 0.5")
                elif kk == "max_output_size" and vv != 100:
                    raise ValueError("config_override: max_output_size is fixed at 100")
                elif kk not in ("method", "sigma", "max_output_size"):
                    raise ValueError(f"config_override: unsupported nms_configs key {kk!r}")
                setattr(self.nms_configs, kk, vv)

    @staticmethod
    def _forward_nms(ctx, key, value):
        """One of method / iou_thresh / sigma / max_output_size as postprocess.nms reads it (postprocess.py:
        175-188): method 'hard', '' or None is hard NMS; "iou_thresh or 0.5"; "sigma or 0.5"."""
        if ctx is None:
            raise ValueError(f"config_override: {key} needs the victim's library context "
                             "(a VictimConfig not owned by an EfficientDetVictim)")
        if key == "method":
            if value not in ("hard", "", None, "gaussian"):
                raise ValueError(f"config_override: Inference has invalid nms method {value}")
            ctx.set_nms_config(method="gaussian" if value == "gaussian" else "hard")
        elif key == "iou_thresh":
            ctx.set_nms_config(iou_thresh=float(value or 0.0))  # 0 = unset: the library applies "or 0.5"
        elif key == "sigma":
            ctx.set_nms_config(sigma=float(value or 0.5))
        else:
            if value is None or int(value) != value or value < 1:
                raise ValueError(f"config_override: max_output_size = {value!r}: an integer in [1, 100]")
            ctx.set_nms_config(max_output_size=int(value))


class EfficientDetVictim:
    """The victim detector held by a libphx context (one device)."""

    def __init__(self, model_name="efficientdet-d0", weights="synthetic", *, seed=0, image_size=0,
                 max_batch=16, bn_mode="local", score_thresh=0.5, rng_seed=0, device=None,
                 person_bias=0.0, dtype="f32", honour_nms_configs=False):
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.device = device
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' (the reference's precision) or 'bf16'")
        modes = {"local": _lib.BN_LOCAL, "frozen": _lib.BN_FROZEN, "sync": _lib.BN_SYNC}
        if bn_mode not in modes:
            raise ValueError("bn_mode must be 'local', 'frozen' or 'sync'")
        self.ctx = _lib.Context(model_name, image_size, max_batch, modes[bn_mode], score_thresh, rng_seed, device,
                                _lib.DTYPE_BF16 if dtype == "bf16" else _lib.DTYPE_F32)
        self.bn_mode = bn_mode
        if bn_mode == "sync":
            # SyncBN: the library hands every BN's per-channel sums to this collective
            from .distributed import bn_sync_callback
            self._ar = bn_sync_callback()
            self.ctx.call("phx_set_allreduce", ctypes.cast(self._ar, ctypes.c_void_p), None)
        self.dtype = dtype
        self.manifest = self.ctx.manifest()
        if isinstance(weights, str) and weights == "synthetic":
            blob = wmod.synthetic_blob(self.manifest, seed=seed, person_bias=person_bias)
        elif isinstance(weights, (str, os.PathLike)):
            # a TensorFlow checkpoint (directory or prefix), restored as KerasDriver does
            # (util_keras.restore_ckpt with ema_decay 0.9998, skip_mismatch=False)
            from .ckpt import checkpoint_to_blob
            blob = np.ascontiguousarray(checkpoint_to_blob(os.fspath(weights), self.manifest, ema_decay=0.9998))
        else:
            blob = np.ascontiguousarray(np.asarray(weights, dtype=np.float32))
        self.load_weights(blob)
        fam = "lite" if "lite" in model_name else "efficientdet"
        self.config = VictimConfig(model_name, self.ctx.image_size, MEAN_RGB[fam], STDDEV_RGB[fam],
                                   NmsConfig(score_thresh=score_thresh), ctx=self.ctx,
                                   honour_nms_configs=bool(honour_nms_configs))
        self.num_anchors = self.ctx.num_anchors
        self.max_batch = max_batch

    def load_weights(self, blob: np.ndarray):
        blob = np.ascontiguousarray(blob, dtype=np.float32)
        if blob.size != self.ctx.weight_count():
            raise ValueError(f"weight blob has {blob.size} floats, manifest needs {self.ctx.weight_count()}")
        self.ctx.call("phx_load_weights", blob.ctypes.data, blob.size)
        self.blob = blob

    def read_weights(self) -> np.ndarray:
        out = np.empty(self.ctx.weight_count(), np.float32)
        self.ctx.call("phx_read_weights", out.ctypes.data, out.size)
        return out

    def _check_images(self, images):
        S = self.ctx.image_size
        if images.dim() != 4 or tuple(images.shape[1:]) != (S, S, 3) or images.dtype != torch.float32:
            raise ValueError(f"images must be float32 [B,{S},{S},3], got {tuple(images.shape)} {images.dtype}")
        if not images.is_cuda:
            raise ValueError("images must be a device tensor")
        if images.shape[0] > self.max_batch:
            raise ValueError("batch exceeds max_batch")
        return images.contiguous()

    def detect(self, images):
        """EfficientDetModel.call(pre_mode=None, post_mode=None) + postprocess.pre_nms."""
        images = self._check_images(images)
        B, A = images.shape[0], self.num_anchors
        scores = torch.empty(B, A, device=images.device)
        classes = torch.empty(B, A, dtype=torch.int32, device=images.device)
        boxes = torch.empty(B, A, 4, device=images.device)
        self.ctx.call("phx_detect", images.data_ptr(), B, scores.data_ptr(), classes.data_ptr(),
                      boxes.data_ptr(), _stream())
        return boxes, scores, classes

    def first_pass(self, images):
        images = self._check_images(images)
        B = images.shape[0]
        ob = torch.empty(B, _lib.MAX_OUT, 4, device=images.device)
        os_ = torch.empty(B, _lib.MAX_OUT, device=images.device)
        oc = torch.empty(B, dtype=torch.int32, device=images.device)
        self.ctx.call("phx_first_pass", images.data_ptr(), B, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(),
                      _stream())
        return ob, os_, oc

    def soft_nms(self, boxes, scores, count=None):
        """postprocess.nms(padded=True) over [B,N,4] / [B,N] candidates, under the context's nms_configs."""
        boxes = boxes.contiguous().float()
        scores = scores.contiguous().float()
        B, N = scores.shape
        if count is None:
            count = torch.full((B,), N, dtype=torch.int32, device=scores.device)
        count = count.to(torch.int32).contiguous()
        ob = torch.empty(B, _lib.MAX_OUT, 4, device=scores.device)
        os_ = torch.empty(B, _lib.MAX_OUT, device=scores.device)
        oc = torch.empty(B, dtype=torch.int32, device=scores.device)
        self.ctx.call("phx_soft_nms", boxes.data_ptr(), scores.data_ptr(), count.data_ptr(), B, N,
                      ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), _stream())
        return ob, os_, oc


class BrightnessMatcher:
    """brightness_matcher.BrightnessMatcher: Y-channel mean transfer patch -> scene."""

    _entry = "phx_brightness_match"

    def __init__(self, victim: EfficientDetVictim):
        self.victim = victim

    def __call__(self, inputs):
        src, tgt = inputs
        squeeze = src.dim() == 3
        if squeeze:
            src, tgt = src[None], tgt[None]
        src = src.contiguous().float()
        tgt = tgt.contiguous().float()
        B, Pp = src.shape[0], src.shape[1]
        out = torch.empty_like(src)
        self.victim.ctx.call(self._entry, src.data_ptr(), Pp, tgt.data_ptr(), tgt.shape[1],
                             tgt.shape[2], B, out.data_ptr(), _stream())
        return out[0] if squeeze else out

    call = __call__


class HistogramMatcher(BrightnessMatcher):
    """brightness_matcher.HistogramMatcher: histogram specification of the patch's Y channel onto the
    scene's (256-bin CDFs, a lookup table, a per-pixel piecewise-linear remap)."""

    _entry = "phx_histogram_match"

    def lut(self, inputs):
        """The intermediates of the match: (hist [B,2,256] int32 — source and target Y histograms —,
        lut [B,256] float32)."""
        src, tgt = inputs
        if src.dim() == 3:
            src, tgt = src[None], tgt[None]
        src = src.contiguous().float()
        tgt = tgt.contiguous().float()
        B = src.shape[0]
        hist = torch.empty(B, 2, 256, dtype=torch.int32, device=src.device)
        lut = torch.empty(B, 256, device=src.device)
        self.victim.ctx.call("phx_histogram_lut", src.data_ptr(), src.shape[1], tgt.data_ptr(), tgt.shape[1],
                             tgt.shape[2], B, hist.data_ptr(), lut.data_ptr(), _stream())
        return hist, lut


MATCHERS = {"brightness": (_lib.MATCH_MEAN, BrightnessMatcher), "histogram": (_lib.MATCH_HISTOGRAM, HistogramMatcher)}


def _withdraw_if_refilled(obj, withdraw):
    """The first pass prefetched for the next step (phx_set_next / phx_def_set_next) read that batch's
    buffer as it was then.  If the buffer has been written in place since — the tensor's version
    counter (shared with every view of it) moved, as a pinned-ring loader refilling one device buffer
    does — the prefetched detections are stale: withdraw them (set_next(NULL)), so the step runs its
    own first pass (attacker.py:172-184 computes it from the images the step gets)."""
    rec = getattr(obj, "_next_rec", None)
    if rec is not None and rec[0]._version != rec[1]:
        withdraw()


def _pad_boxes(boxes, B, device):
    """list of [n_b,4] (or a padded [B,maxb,4] + count) -> ([B,maxb,4], count[B])"""
    if isinstance(boxes, (tuple, list)) and len(boxes) == 2 and torch.is_tensor(boxes[0]) and boxes[0].dim() == 3:
        bx, cnt = boxes
        return bx.contiguous().float(), cnt.to(torch.int32).contiguous()
    maxb = max(1, max(len(b) for b in boxes))
    if maxb > _lib.MAX_OUT:
        raise ValueError("at most 100 boxes per image")
    # padded on the host, then one transfer: [B*maxb*4 boxes | B counts] as raw 32-bit words
    out = np.zeros((B, maxb, 4), np.float32)
    cnt = np.zeros(B, np.int32)
    for i, b in enumerate(boxes):
        b = np.asarray(b, dtype=np.float32).reshape(-1, 4)
        out[i, :len(b)] = b
        cnt[i] = len(b)
    flat = torch.as_tensor(np.concatenate([out.reshape(-1).view(np.int32), cnt])).to(device)
    return flat[:out.size].view(torch.float32).view(B, maxb, 4), flat[out.size:]


class Patcher:
    """attacker.Patcher: EOT paste of the current patch onto every box of every image."""

    def __init__(self, attacker: "PatchAttacker"):
        self.attacker = attacker

    def __call__(self, inputs, step=None):
        boxes, images = inputs
        a = self.attacker
        images = a.model._check_images(images)
        B = images.shape[0]
        bx, cnt = _pad_boxes(boxes, B, images.device)
        out = torch.empty_like(images)
        a._select_matcher()
        self.last_placements = torch.zeros(B, bx.shape[1], 8, device=images.device)
        a.model.ctx.call("phx_patch_images", images.data_ptr(), B, bx.data_ptr(), cnt.data_ptr(), bx.shape[1],
                         a.params.data_ptr(), int(a.cur_step if step is None else step), a.global_offset(B),
                         out.data_ptr(), self.last_placements.data_ptr(), _stream())
        return out

    call = __call__


class _Mean:
    """keras.metrics.Mean (what add_metric aggregates per epoch)."""

    def __init__(self):
        self.total, self.count = 0.0, 0

    def update(self, v):
        self.total += float(v)
        self.count += 1

    def result(self):
        return self.total / max(self.count, 1)


class _StepMetrics(Mapping):
    """The {name: running mean} dict train_step returns, evaluated on first access."""

    def __init__(self, attacker, sid):
        self._a, self._sid, self._d = attacker, sid, None

    def _get(self):
        if self._d is None:
            self._a._flush_metrics()
            snap = self._a._snapshots.get(self._sid)
            # a reset_metrics() after this step dropped its snapshot: report the current means
            self._d = dict(snap) if snap is not None else {k: m.result() for k, m in self._a.metrics.items()}
        return self._d

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._get())


class PatchAttacker:
    """attacker.PatchAttacker: trainable [patch | scale] optimised against the victim."""

    METRICS = ("loss", "scale", "scale_loss", "tv_loss", "mean_max_score", "std_max_score", "asr",
               "asr_to_scale")

    def __init__(self, model: EfficientDetVictim, initial_patch=None, config_override=None,
                 visualize_freq=200, *, seed=0, learning_rate=1e-2, device=None, matcher="brightness",
                 summary_writer=None, box_loss=None, box_loss_weight=1.0):
        """box_loss: None (the reference's objective) or "inv_diou": loss += box_loss_weight *
        InverseDIOULoss()(second-pass person boxes, placement boxes) (regression_loss.py, which the reference
        kept but never wired in; phx.h phx_set_box_loss), in train_step and test_step alike; their metric
        dicts then carry "box_loss", the unweighted batch value.  fp32 victims only.
        summary_writer (summaries.py; None = no summaries, and no launch beyond the step's own): when
        set, train_step hands vis_images() to it at every step with cur_step % visualize_freq == 0 and
        test_step at every such val step, as the reference's call does (attacker.py:209-213); a
        visualize_freq of 0 or less means never."""
        if matcher not in MATCHERS:
            raise ValueError("matcher must be 'brightness' (the reference's Patcher) or 'histogram'")
        self.matcher = matcher
        if box_loss not in _lib.BOX_LOSSES:
            raise ValueError("box_loss must be None or 'inv_diou' (the reference's InverseDIOULoss)")
        self.box_loss = box_loss
        self.box_loss_weight = float(box_loss_weight)
        if box_loss is not None:
            self.METRICS = self.METRICS + ("box_loss",)
        self.model = model
        self.config = model.config
        if config_override:
            self.config.override(config_override, model.ctx)
        dev = torch.device("cuda", model.device) if device is None else torch.device(device)
        if initial_patch is None:
            # np.random.uniform(-1, 1, (640, 640, 3)), scale .4 (attacker.py:42-44)
            patch_img = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(640, 640, 3))
            scale = 0.4
        else:
            patch_img, scale = load_patch(initial_patch)
        params = np.concatenate([np.asarray(patch_img, np.float32).reshape(-1), [np.float32(scale)]])
        self.params = torch.as_tensor(params, dtype=torch.float32, device=dev).contiguous()
        # [d patch | d scale | metric row]: one SUM all-reduce per step carries the gradient and the
        # per-rank metric sums (loss, counts, #images; TV only on the rank that adds it), so every
        # rank issues exactly the same collective at the same point of train_step
        # (with a box-regression term its unweighted batch value rides behind the metric row, whose length
        # the ABI pins)
        self._red = torch.zeros(_lib.NPARAM + _lib.NMETRIC + (box_loss is not None), device=dev)
        self.grad = self._red[:_lib.NPARAM]
        self.metrics_buf = self._red[_lib.NPARAM:_lib.NPARAM + _lib.NMETRIC]
        self._box_val = self._red[_lib.NPARAM + _lib.NMETRIC:]  # empty without the term
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.learning_rate = learning_rate
        self.iterations = 0
        self.cur_step = 0
        self.visualize_freq = visualize_freq
        self.summary_writer = summary_writer
        self._val_step = 0  # attacker.py:69, counted by test_step
        self._last_B = None  # batch size of the last call (vis_images)
        self._patcher = Patcher(self)
        self._matcher = MATCHERS[matcher][1](model)
        self.metrics = {k: _Mean() for k in self.METRICS}
        self._pending = []      # (step id, device metric row) not yet folded into self.metrics
        self._snapshots = {}    # step id -> running-mean dict after that step
        self._step_id = 0
        self.bins = np.arange(self.config.nms_configs.score_thresh, .805, .01, dtype="float32")

    # ---- variables -----------------------------------------------------------------------------
    @property
    def patch(self):
        return self.params[:_lib.NPATCH].view(640, 640, 3)

    @property
    def scale(self):
        return self.params[_lib.NPATCH]

    @property
    def _trainable_variables(self):
        return [self.params[_lib.NPATCH:], self.patch]

    def global_offset(self, B):
        return ddp.global_offset(B)

    def _select_matcher(self):
        """The matcher is a setting of the victim's library context, which attackers may share:
        every call that pastes patches selects this attacker's first (a host-side assignment)."""
        self.model.ctx.call("phx_set_matcher", MATCHERS[self.matcher][0])

    def _select_box_loss(self):
        """The box-regression term is a setting of the shared context too; a change of kind makes the
        library plan its executors again, so it is set only where it differs."""
        ctx = self.model.ctx
        if ctx.get_box_loss() != (self.box_loss, float(np.float32(self.box_loss_weight))):
            ctx.set_box_loss(self.box_loss, self.box_loss_weight)

    def _read_box_loss(self, B):
        """The unweighted batch value of the step just issued, behind the metric row."""
        if self.box_loss is None:
            return
        per = torch.empty(B, device=self.params.device)
        self.model.ctx.call("phx_debug_last_box_loss", per.data_ptr(), None, None, None, _stream())
        torch.sum(per, 0, keepdim=True, out=self._box_val)

    # ---- reference methods -------------------------------------------------------------------
    def first_pass(self, images):
        return self.model.first_pass(images)

    def call(self, images, *, training=True, boxes=None, add_tv=None):
        """PatchAttacker.call (attacker.py:172-219).  training=True: the attack step, returns
        [d scale, d patch] (attacker.py:217).  training=False: the victim in inference mode, returns
        the second pass's soft-NMS person detections (boxes_pred, scores_pred) as padded [B,100,4],
        [B,100] plus counts [B].  `boxes` optionally replaces the first-pass detections for
        placement (injected boxes).  The metric row of the step is left in metrics_buf."""
        images = self.model._check_images(images)
        B = images.shape[0]
        self._last_B = B
        if add_tv is None:
            add_tv = ddp.rank() == 0  # TV counted once per global step
        if boxes is not None:
            bx, cnt = _pad_boxes(boxes, B, images.device)
            bp, cp, maxb = bx.data_ptr(), cnt.data_ptr(), bx.shape[1]
            self._keep = (bx, cnt)
        else:
            bp, cp, maxb = None, None, 0
        self._select_matcher()
        self._select_box_loss()
        if not training:
            ob = torch.empty(B, _lib.MAX_OUT, 4, device=images.device)
            os_ = torch.empty(B, _lib.MAX_OUT, device=images.device)
            oc = torch.empty(B, dtype=torch.int32, device=images.device)
            self.model.ctx.call("phx_eval_step", images.data_ptr(), B, bp, cp, maxb, self.params.data_ptr(),
                                int(self.cur_step), self.global_offset(B), int(bool(add_tv)),
                                self.metrics_buf.data_ptr(), ob.data_ptr(), os_.data_ptr(), oc.data_ptr(),
                                _stream())
            self._read_box_loss(B)
            return ob, os_, oc
        self.model.ctx.call("phx_step_grad", images.data_ptr(), B, bp, cp, maxb, self.params.data_ptr(),
                            int(self.cur_step), self.global_offset(B), int(bool(add_tv)), self.grad.data_ptr(),
                            self.metrics_buf.data_ptr(), _stream())
        self._read_box_loss(B)
        return [self.grad[_lib.NPATCH:], self.grad[:_lib.NPATCH].view(640, 640, 3)]

    __call__ = call

    def sync(self):
        """Makes the current stream wait for a prefetched first pass (train_step(next_inputs=...))."""
        self.model.ctx.call("phx_sync", _stream())

    def apply_gradients(self):
        """optimizer.apply_gradients + variable constraints (attacker.py:315, :51-54)."""
        self.iterations += 1
        self.model.ctx.call("phx_adam_clip", self.params.data_ptr(), self.grad.data_ptr(), self.m.data_ptr(),
                            self.v.data_ptr(), float(self.learning_rate), int(self.iterations), _stream())

    def allreduce_gradients(self):
        """SUM over ranks of [d patch | d scale | metric row] (the step's one collective)."""
        ddp.allreduce_sum_(self._red)

    def _metric_row(self):
        """Device row [metric row | scale | box-term value, when on] of the step just run (scale before the
        update, as the reference's add_metric(self._scale_regressor) inside call, attacker.py:197)."""
        return torch.cat([self.metrics_buf, self.params[_lib.NPATCH:], self._box_val])

    @staticmethod
    def _derive(v):
        """add_metric values (attacker.py:196-207) from a rank-summed [metrics | scale] row."""
        n, scale = float(v[_lib.M_NIMG]), float(v[_lib.NMETRIC])
        mean = v[_lib.M_SUM_M] / n
        var = max(v[_lib.M_SUM_M2] / n - mean * mean, 0.0)
        # calc_asr (attacker.py:253-255) divides tf.size of the flattened ragged [n,4] boxes, 4
        # floats per box, in float32: 1 - 4n / (4d + epsilon)
        asr = float(np.float32(1.0) - np.float32(4.0 * v[_lib.M_ASR_NUM])
                    / (np.float32(4.0 * v[_lib.M_ASR_DEN]) + np.float32(1e-7)))
        out = {"loss": float(v[_lib.M_LOSS]), "scale": scale, "scale_loss": float(v[_lib.M_SCALE_LOSS]),
               "tv_loss": float(v[_lib.M_TV]), "mean_max_score": mean, "std_max_score": math.sqrt(var),
               "asr": asr, "asr_to_scale": asr / scale if scale else float("inf"),
               "patches": float(v[_lib.M_NBOX])}
        if len(v) > _lib.NMETRIC + 1:  # the box-regression term's unweighted batch value (summed over ranks)
            out["box_loss"] = float(v[_lib.NMETRIC + 1])
        return out

    def step_metrics(self):
        """Per-step values of the reference's add_metric set (attacker.py:196-207) for the step
        just run: global over ranks after train_step (its all-reduce), this rank's after a bare
        call().  Synchronises with the device; issues no collective."""
        return self._derive(self._metric_row().cpu().numpy().astype(np.float64))

    def _flush_metrics(self):
        """Fold the queued per-step rows (already reduced by train_step's all-reduce) into the
        Keras-style running means with one device->host copy, so train_step never waits on the GPU
        and reading metrics never issues a collective (any rank may read them, or none)."""
        if not self._pending:
            return
        ids = [i for i, _ in self._pending]
        rows = torch.stack([r for _, r in self._pending]).cpu().numpy().astype(np.float64)
        self._pending.clear()
        for sid, v in zip(ids, rows):
            sm = self._derive(v)
            for k in self.METRICS:
                self.metrics[k].update(sm[k])
            self._snapshots[sid] = {k: m.result() for k, m in self.metrics.items()}
        for old in [k for k in self._snapshots if k < ids[-1] - 1024]:
            del self._snapshots[old]

    def vis_images(self, training=True):
        """PatchAttacker.vis_images (attacker.py:257-305) for the step just run (call() or
        call(training=False)), as arrays instead of TensorBoard summaries:

        "Patch"   uint8 [640,640,3], training only: clip(patch * stddev_rgb + mean_rgb, 0, 255), the
                  arithmetic of save_weights' patch.png
        "ASR"     (bins, asr): calc_asr at every threshold of self.bins, asr = 1 - 4n / (4d + 1e-7) in
                  float32 (_derive's rule) with d / n the step's first- / second-pass detections >= bin
        "Sample"  uint8 [B,S,S,3]: the patched batch with the first-pass boxes ([0,1,0]) and the
                  second-pass boxes ([0,0,1]) drawn, denormalised (phx_step_summary)

        Rank-local, like the reference's (it visualises on one GPU): the counts are this rank's shard's
        and no collective is issued.  Synchronises with the device."""
        ctx = self.model.ctx
        S = ctx.image_size
        dev = self.params.device
        bins = np.ascontiguousarray(self.bins, np.float32)
        if self._last_B is None:
            raise _lib.PhxError("vis_images: no step has run")
        B = self._last_B
        counts = torch.empty(2, len(bins), dtype=torch.int32, device=dev)
        sample = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
        ctx.call("phx_step_summary", bins.ctypes.data, len(bins), counts.data_ptr(), sample.data_ptr(), _stream())
        out = {}
        if training:
            patch = self.patch.detach().cpu().numpy()
            img = np.clip(patch * np.asarray(self.config.stddev_rgb, np.float32)
                          + np.asarray(self.config.mean_rgb, np.float32), 0, 255)
            out["Patch"] = img.astype(np.uint8)
        c = counts.cpu().numpy()
        asr = (np.float32(1.0) - (np.float32(4.0) * c[1].astype(np.float32))
               / (np.float32(4.0) * c[0].astype(np.float32) + np.float32(1e-7))).astype(np.float32)
        out["ASR"] = (bins.copy(), asr)
        out["Sample"] = sample.cpu().numpy()
        return out

    def _summarise(self, training, step):
        summaries.write(self.summary_writer, self.vis_images(training), step, "train" if training else "val")

    def train_step(self, inputs, boxes=None, next_inputs=None):
        """attacker.py:307-316: grads = self(inputs); apply_gradients; return metrics.  The metric
        dict is evaluated lazily (like the tensors Keras returns): reading it synchronises.
        next_inputs: the batch the next train_step will get (attacker_train.py's fit draws it from
        the generator).  With first-pass placement its clean first pass — a function of the images,
        not of the patch — then runs beside this step's second pass and backward (phx_set_next) and
        the next train_step places its patches by it; the results are the same either way."""
        # the batch the previous step prefetched, kept alive until this call (which joins its first
        # pass on the current stream) has been issued
        prev = getattr(self, "_next_keep", None)
        self._select_box_loss()  # (before a next batch is registered: the setter is refused while one is pending)
        _withdraw_if_refilled(self, lambda: self.model.ctx.call("phx_set_next", None, 0, 0))
        self._next_keep = self._next_rec = None
        if next_inputs is not None and boxes is None:
            nx = self.model._check_images(next_inputs)
            self._next_keep = nx  # alive until the step that consumes it
            self._next_rec = (nx, nx._version)
            self.model.ctx.call("phx_set_next", nx.data_ptr(), nx.shape[0], self.global_offset(nx.shape[0]))
        self.call(inputs, boxes=boxes)
        del prev
        # tf.cond(cur_step % visualize_freq == 0, vis_images) inside call (attacker.py:209-213): before the
        # update, with the step number the step ran with
        if summaries.due(self.summary_writer, self.cur_step, self.visualize_freq):
            self._summarise(True, self.cur_step)
        sid = self._step_id
        self._step_id += 1
        self.allreduce_gradients()
        self._pending.append((sid, self._metric_row()))
        if len(self._pending) >= 256:  # bound the queue when nobody reads the metrics
            self._flush_metrics()
        self.apply_gradients()
        self.cur_step += 1
        return _StepMetrics(self, sid)

    def test_step(self, inputs, boxes=None):
        """attacker.py:318-326: self(inputs, training=False) — the victim in inference mode (BN
        from the moving statistics, no drop connect), the same EOT paste, loss and metrics, no
        gradient and no update.  Returns (metrics, (boxes_pred, scores_pred, count)) where the
        predictions are call()'s soft-NMS person detections on the patched images."""
        preds = self.call(inputs, training=False, boxes=boxes)
        if summaries.due(self.summary_writer, self._val_step, self.visualize_freq):
            self._summarise(False, self._val_step)
        self._val_step += 1
        # every rank, same point: the one collective of the metric row (and the box-term value behind it)
        ddp.allreduce_sum_(self._red[_lib.NPARAM:])
        return self.step_metrics(), preds

    def reset_metrics(self):
        """Keras reset at epoch boundaries: queued steps are folded first (they belong to the
        finished epoch)."""
        self._flush_metrics()
        for m in self.metrics.values():
            m.total, m.count = 0.0, 0
        self._snapshots = {}

    def save_weights(self, dirpath, **kwargs):
        """attacker.py:328-341, same three files: scale.txt (str of the float32 scale), patch.png
        (clip(patch*std + mean, 0, 255) as uint8) and patch.tiff (the raw float32 normalised patch,
        written by our own baseline-TIFF writer since tifffile is not installed)."""
        os.makedirs(dirpath)
        with open(os.path.join(dirpath, "scale.txt"), "w") as f:
            f.write(str(np.float32(self.scale.item())))
        patch = self.patch.detach().cpu().numpy()
        tiff.write_float_tiff(os.path.join(dirpath, "patch.tiff"), patch)
        img = np.clip(patch * np.asarray(self.config.stddev_rgb, np.float32)
                      + np.asarray(self.config.mean_rgb, np.float32), 0, 255)
        from PIL import Image
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(dirpath, "patch.png"))


def load_patch(dirpath):
    """initial_patch=dir (attacker.py:46-48): tifffile.imread(patch.tiff) + float(scale.txt)."""
    import ast
    patch = tiff.read_float_tiff(os.path.join(dirpath, "patch.tiff"))
    if patch.shape != (640, 640, 3):
        raise ValueError(f"patch.tiff holds {patch.shape}, expected (640, 640, 3)")
    with open(os.path.join(dirpath, "scale.txt")) as f:
        scale = ast.literal_eval(f.read())
    return patch, float(scale)


class ReduceLROnPlateau:
    """keras ReduceLROnPlateau(monitor='loss', factor=.5, patience=50, min_lr=1e-4) used by
    attacker_train.py:70-71, stepped once per epoch."""

    def __init__(self, attacker: PatchAttacker, factor=0.5, patience=50, min_lr=1e-4, min_delta=1e-4):
        self.a, self.factor, self.patience, self.min_lr, self.min_delta = attacker, factor, patience, min_lr, min_delta
        self.best, self.wait = float("inf"), 0

    def on_epoch_end(self, loss):
        if loss < self.best - self.min_delta:
            self.best, self.wait = loss, 0
        else:
            self.wait += 1
            if self.wait >= self.patience and self.a.learning_rate > self.min_lr:
                self.a.learning_rate = max(self.a.learning_rate * self.factor, self.min_lr)
                self.wait = 0
