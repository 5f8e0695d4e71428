/*
 * phx.h — C ABI of libphx.so, the MI355X-native (gfx950) adversarial-patch optimisation step.
 *
 * This is the drop-in boundary for the inner step of tiiuae/MLAdversarialObjectDetection's
 * attacker_train.py.  Each entry point replaces one reference interface; the reference
 * file:line it stands in for is given next to it (paths relative to the reference root).
 *
 * Conventions
 *  - Plain pointers and sizes only.  Device pointers are HIP device memory (e.g. PyTorch-ROCm
 *    tensors' data_ptr()); every launch is enqueued on the caller's stream (`stream`, a
 *    hipStream_t passed as void*; NULL = the null stream).  No entry point synchronises the
 *    device unless its comment says so.
 *  - Layouts: images NHWC float32 [B,H,W,3] in the victim's normalised space; boxes
 *    [ymin,xmin,ymax,xmax] float32 pixels; the trainable parameter buffer is the contiguous
 *    float32 vector [patch 640*640*3 | scale 1] (`PHX_NPARAM` floats), gradients use the same
 *    layout (the reference's `_trainable_variables = [scale, patch]`, attacker.py:63, in a
 *    flat order that lets one RCCL all-reduce cover both).
 *  - Errors: every int-returning call returns 0 on success and a negative PHX_E* code on
 *    failure; phx_last_error() returns the message.  No C++ exception crosses the ABI.
 */
#ifndef PHX_H_
#define PHX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_ABI_VERSION 4

#define PHX_PATCH_SIZE 640                               /* attacker.py:43 */
#define PHX_NPATCH (PHX_PATCH_SIZE * PHX_PATCH_SIZE * 3)
#define PHX_NPARAM (PHX_NPATCH + 1)                      /* [patch | scale] */
#define PHX_MAX_OUT 100                                  /* nms max_output_size, hparams_config.py:264 */

enum {
  PHX_OK = 0,
  PHX_EINVAL = -1,   /* bad argument / shape */
  PHX_EHIP = -2,     /* HIP runtime error */
  PHX_ESTATE = -3,   /* call order (e.g. weights not loaded) */
  PHX_ECAP = -4,     /* capacity exceeded (batch > max_batch, ...) */
};

/* BN modes.  LOCAL = training-mode batch statistics over the rank's batch, as
 * the reference's attack step (victim inherits training=True, attacker.py:172); FROZEN =
 * inference BN with moving statistics (attacker.py:325 test_step); SYNC = training-mode
 * statistics over the global batch of all ranks (SyncBN: the per-channel [n, sum x, sum x^2]
 * of every BN forward and [n, sum dz, sum dz*xhat] of every BN backward are SUM-reduced through
 * the caller's collective, phx_set_allreduce), equal to one reference step on the whole batch. */
enum { PHX_BN_LOCAL = 0, PHX_BN_FROZEN = 1, PHX_BN_SYNC = 2 };

/* Arithmetic of the victim's 1x1 convolutions ("C4: bf16 act, fp32 acc").
 * F32: fp32 matrix cores (the reference's precision, BASELINE configs 1-3).  BF16: bf16 matrix
 * cores with fp32 accumulation; BN statistics, depthwise convs, EOT and the loss stay fp32. */
enum { PHX_DTYPE_F32 = 0, PHX_DTYPE_BF16 = 1 };

typedef struct phx_config {
  const char* model_name;   /* "efficientdet-d0" ... "-d7", "efficientdet-lite0".."-lite4"
                               (hparams_config.py:301-467)                                  */
  int image_size;           /* 0 = model default; square images only                         */
  int max_batch;            /* per-rank batch capacity (workspace is sized for it)            */
  int bn_mode;              /* PHX_BN_LOCAL / PHX_BN_FROZEN / PHX_BN_SYNC                     */
  float score_thresh;       /* nms_configs.score_thresh (hparams_config.py:258-266 default 0;
                               attacker_train.py:31 override 0.5).  As the reference: the first
                               pass keeps scores >= it (attacker.py:83-84) and gaussian soft-NMS
                               keeps scores > (it, or 0.001 when it is 0) (postprocess.py:186-188) */
  uint64_t seed;            /* Philox key for all EOT randomness                              */
  int compute_dtype;        /* PHX_DTYPE_F32 / PHX_DTYPE_BF16                                  */
} phx_config;

typedef struct phx_ctx phx_ctx;

/* bn=sync's collective: SUM-reduce n doubles at device address buf across the ranks, in place,
 * ordered on `stream` after the library's work so far and before its next launch (an RCCL
 * all-reduce enqueued on the stream, or a blocking one).  Returns 0 on success.  The library calls
 * it from phx_step_grad / phx_detect / phx_first_pass of a PHX_BN_SYNC context, once per BN (per
 * head group) and pass; every rank must run the same steps.  Replaces the cross-replica sums of
 * the reference's SyncBatchNormalization (automl/efficientdet/utils.py:205-241). */
typedef int (*phx_allreduce_fn)(void* user, double* buf, size_t n, void* stream);
int phx_set_allreduce(phx_ctx* ctx, phx_allreduce_fn fn, void* user);

/* Per-step metrics written by phx_step_grad (host-readable device or host memory, PHX_NMETRIC
 * floats), the reference's add_metric set, attacker.py:196-207. */
enum {
  PHX_M_LOSS = 0,        /* sum_b m_b^2 + scale_loss (+ 1e-5*TV on the rank that owns TV)
                            (+ weight * the box-regression term, phx_set_box_loss)          */
  PHX_M_SCALE_LOSS = 1,  /* sum_b (m_b - s)^2                                              */
  PHX_M_TV = 2,          /* total_variation(patch) (written by the rank that owns TV, else 0)  */
  PHX_M_SUM_M = 3,       /* sum_b m_b      (mean_max_score = SUM_M / B)                    */
  PHX_M_SUM_M2 = 4,      /* sum_b m_b^2    (std_max_score)                                 */
  PHX_M_ASR_NUM = 5,     /* #second-pass boxes >= 0.5 after soft-NMS                       */
  PHX_M_ASR_DEN = 6,     /* #first-pass boxes >= 0.5                                       */
  PHX_M_NBOX = 7,        /* #patches pasted                                                */
  PHX_M_NIMG = 8,        /* #images of the step (B): the metric row is SUM-all-reducible     */
  PHX_NMETRIC = 9
};

/* ---- lifetime --------------------------------------------------------------------------- */
/* Replaces util.get_victim_model (util.py:177) + infer_lib.KerasDriver.__init__
 * (infer_lib.py:385-403): builds the EfficientDet program for `cfg` on `device`. */
int phx_create(const phx_config* cfg, int device, phx_ctx** out);
void phx_destroy(phx_ctx* ctx);
/* ctx == NULL: the message of this thread's last failed phx_create or phx_ingest_dims. */
const char* phx_last_error(const phx_ctx* ctx);
int phx_abi_version(void);
/* The effective model configuration as JSON (hparams_config.get_efficientdet_config,
 * hparams_config.py:301-480, + the BiFPN node list of fpn_configs.get_fpn_config,
 * tf2/fpn_configs.py:166-176): name, backbone_name, image_size, fpn_num_filters,
 * fpn_cell_repeats, box_class_repeats, anchor_scale, num_scales, aspect_ratios, min_level,
 * max_level, act_type, fpn_weight_method, mean_rgb, stddev_rgb, num_classes, survival_prob,
 * fpn_nodes, score_thresh, nms_score_thresh (null when a hard NMS keeps every score), nms_method,
 * nms_iou_thresh, nms_sigma, nms_max_output_size, post_mode.  Buffer protocol as phx_weight_manifest. */
int phx_model_info(const phx_ctx* ctx, char* buf, size_t cap, size_t* needed);
/* Config.override({'nms_configs': {'score_thresh': t}}) (hparams_config.py:91-109) after
 * creation: first-pass filter >= t, soft-NMS threshold t (0.001 when t == 0, method gaussian). */
int phx_set_score_thresh(phx_ctx* ctx, float score_thresh);
/* The rest of nms_configs (hparams_config.py:258-266), as postprocess.nms reads it (postprocess.py:175-200):
 *   method PHX_NMS_HARD ('hard', '' or None): NonMaxSuppressionV5 with iou_threshold = "iou_thresh or 0.5"
 *     (an iou_thresh of 0 means unset), score_threshold = "score_thresh or -inf", soft_nms_sigma 0;
 *   method PHX_NMS_GAUSSIAN: iou_threshold 1, score_threshold = "score_thresh or 0.001", soft_nms_sigma =
 *     sigma / 2.
 * max_output_size selections at most; every output array keeps its [B,100] shape (rows at and beyond the
 * count are zero), so max_output_size > 100 is refused.  PHX_EINVAL with a message: an unknown method,
 * max_output_size outside [1, 100], iou_thresh outside [0, 1], sigma not positive and finite.  The thresholds
 * in force are the same whichever of phx_set_score_thresh and phx_set_nms_config is called first.  Every
 * NMS of the context follows it: phx_first_pass, the step's first pass and its second-pass ASR counters, the
 * defender's odet_model, phx_soft_nms, phx_nms_global, phx_nms_per_class and phx_serve.  The step's gradient
 * does not pass through NMS (the loss reads pre-NMS maxima).  Drops a pending phx_set_next prefetch.  The
 * default, {PHX_NMS_GAUSSIAN, 0, 0.5, 100}, is the reference's. */
enum { PHX_NMS_GAUSSIAN = 0, PHX_NMS_HARD = 1 };
typedef struct phx_nms_config {
  int32_t method;           /* PHX_NMS_GAUSSIAN | PHX_NMS_HARD */
  float iou_thresh;         /* hard: the IoU threshold, 0 = unset (0.5) */
  float sigma;              /* gaussian: the paper's sigma (TF's soft_nms_sigma is half of it) */
  int32_t max_output_size;  /* 1..PHX_MAX_OUT */
} phx_nms_config;
int phx_set_nms_config(phx_ctx* ctx, const phx_nms_config* cfg);
int phx_get_nms_config(const phx_ctx* ctx, phx_nms_config* cfg);
/* EfficientDetModel.call's post_mode for phx_serve: PHX_POST_GLOBAL (postprocess_global, the default) or
 * PHX_POST_PER_CLASS (postprocess_per_class).  phx_get_post_mode returns the mode (PHX_EINVAL: null ctx). */
enum { PHX_POST_GLOBAL = 0, PHX_POST_PER_CLASS = 1 };
int phx_set_post_mode(phx_ctx* ctx, int mode);
int phx_get_post_mode(const phx_ctx* ctx);

/* JSON list of the victim's tensors in blob order: [{"name","shape","offset","kind"}...].
 * kind: "kernel","bias","gamma","beta","moving_mean","moving_variance","wsm".
 * Writes at most `cap` bytes (NUL-terminated); *needed = full length + 1. */
int phx_weight_manifest(const phx_ctx* ctx, char* buf, size_t cap, size_t* needed);
size_t phx_weight_count(const phx_ctx* ctx);   /* floats in the blob */
/* Copies a host float32 blob laid out per the manifest (restore_ckpt, util_keras.py:108). */
int phx_load_weights(phx_ctx* ctx, const float* host_blob, size_t nfloats);
/* Copies the (possibly updated) BN moving statistics back into a host blob. */
int phx_read_weights(phx_ctx* ctx, float* host_blob, size_t nfloats);

/* ---- victim ----------------------------------------------------------------------------- */
/* EfficientDetModel.call(images, pre_mode=None, post_mode=None) (efficientdet_keras.py:966)
 * followed by postprocess.pre_nms (postprocess.py:119): per anchor max logit score (sigmoid),
 * argmax class and decoded box.  scores [B,A], classes [B,A] int32, boxes [B,A,4].
 * A = phx_num_anchors(). BN statistics per cfg.bn_mode (moving stats are updated in LOCAL). */
int phx_detect(phx_ctx* ctx, const float* images, int B, float* scores, int32_t* classes,
               float* boxes, void* stream);
int phx_num_anchors(const phx_ctx* ctx);
int phx_image_size(const phx_ctx* ctx);
/* Device bytes of the executor for batch B (activations, gradients, statistics, EOT and
 * post-processing buffers); builds (allocates) it if it does not exist yet.  SURVEY §8b's
 * phx_workspace_bytes; the library owns the workspace, no step allocates. */
int phx_workspace_bytes(phx_ctx* ctx, int B, size_t* bytes);

/* PatchAttacker.first_pass (attacker.py:91-116): detect + person/valid/threshold filter +
 * gaussian soft-NMS (postprocess.nms, postprocess.py:159-205 → NonMaxSuppressionV5) +
 * clip_boxes.  out_boxes [B,100,4], out_scores [B,100], out_count [B] (device). */
int phx_first_pass(phx_ctx* ctx, const float* images, int B, float* out_boxes,
                   float* out_scores, int32_t* out_count, void* stream);

/* Soft-NMS alone over caller-provided candidates (postprocess.nms with padded=True):
 * boxes [B,N,4], scores [B,N], count [B] valid candidates per row. */
int phx_soft_nms(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* count,
                 int B, int N, float* out_boxes, float* out_scores, int32_t* out_count,
                 void* stream);

/* ---- serving raw frames ------------------------------------------------------------------
 * EfficientDetModel.call(raw_frames, training=False, pre_mode='infer', post_mode='global')
 * (efficientdet_keras.py:912-994), what KerasDriver.serve runs for detector.Detector.infer
 * (infer_lib.py:408-421, detector.py:35-60), in three entry points.  Frames are a packed batch of
 * HWC uint8 RGB images of any sizes: src (device) with offsets [B] int64 byte offsets and dims
 * [B,2] int32 (h, w) — both HOST arrays, so every argument is checked before anything is launched.
 * PHX_EINVAL with a message naming the argument, nothing launched: B < 1 or B > max_batch, a null
 * pointer, h or w < 1, a scaled side that truncates to 0 (tf.image.resize raises there), images
 * not 16-byte aligned.  The first serving call reserves the frame tables (and phx_serve the batch
 * size's image buffer; both synchronous, counted by phx_workspace_bytes); later calls allocate
 * nothing and do not synchronise — unless 8 serving calls are still in flight, when the host
 * waits for the oldest one's frame table.
 *
 * _preprocessing(mode='infer') -> DetectionInputProcessor (dataloader.py:59-65, 115-142, 199-201):
 * (x - mean_rgb) / stddev_rgb in fp32 with the model's own constants; image_scale =
 * min(fp32(S)/fp32(h), fp32(S)/fp32(w)); tf.image.resize(antialias=True, bilinear) to
 * [int(h * image_scale), int(w * image_scale)] (truncating fp32 products); top-left placement on a
 * zero [S,S,3] canvas.  images [B,S,S,3] float32 and scales [B] = image_scale_to_original =
 * 1 / image_scale (device).  Works in a context of either compute dtype (its output is fp32). */
int phx_serve_preprocess(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims,
                         int B, float* images, float* scales, void* stream);
/* postprocess_global over caller-provided candidates (postprocess.py:375-406), the class-carrying
 * sibling of phx_soft_nms: nms(padded=True) on every candidate with score > the context's NMS
 * threshold (score_thresh, or 0.001 when it is 0) — no person, validity or >= filter —, clip_boxes
 * to [0, S], then x scales[b] (NULL: boxes stay in model pixels), classes + 1 (CLASS_OFFSET) as
 * float32.  boxes [B,N,4], scores [B,N], classes [B,N] int32, count [B] valid candidates per row
 * (NULL: N); out_boxes [B,100,4], out_scores [B,100], out_classes [B,100], out_count [B] (all
 * device).  Rows at and beyond out_count are zero in every output (TF's padded
 * NonMaxSuppressionV5 gathers candidate 0 there: read the first out_count rows only). */
int phx_nms_global(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* classes,
                   const int32_t* count, int B, int N, const float* scales, float* out_boxes,
                   float* out_scores, float* out_classes, int32_t* out_count, void* stream);
/* per_class_nms over caller-provided candidates (postprocess.py:409-467), phx_nms_global's sibling: for each
 * class cid in [0, num_classes) nms(padded=False) under the context's nms_configs over the candidates with
 * classes == cid (at most max_output_size selections per class); the classes' selections concatenated in class
 * order, and the max_output_size best by (possibly decayed) score taken, ties to the lower position of that
 * concatenation (tf.math.top_k); out_count = min(max_output_size, selections of all classes).  Boxes x scales[b]
 * (NULL: as they are) and NOT clipped (the reference's per-class path has no clip_boxes); classes cid + 1 as
 * float32.  Arguments and output shapes as phx_nms_global; rows at and beyond out_count are zero. */
int phx_nms_per_class(phx_ctx* ctx, const float* boxes, const float* scores, const int32_t* classes,
                      const int32_t* count, int B, int N, const float* scales, float* out_boxes,
                      float* out_scores, float* out_classes, int32_t* out_count, void* stream);
/* The whole call: preprocess, forward, postprocess_global (or, after phx_set_post_mode(PHX_POST_PER_CLASS),
 * postprocess_per_class: boxes not clipped) with the frames' image_scale_to_original,
 * so boxes are in frame pixels.  The forward always runs inference BN from the moving statistics,
 * without drop connect or moving-statistics update, whatever the context's bn_mode (KerasDriver
 * forces is_training_bn=False, infer_lib.py:171).  out_scales [B] (NULL = skip) receives
 * image_scale_to_original.  Needs loaded weights (PHX_ESTATE).  PHX_ESTATE while a phx_set_next
 * prefetch is in flight (run or withdraw it first).  fp32 contexts only: a PHX_DTYPE_BF16 context is
 * refused with PHX_EINVAL (phx_serve_preprocess and phx_nms_global work in either). */
int phx_serve(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
              float* out_boxes, float* out_scores, float* out_classes, int32_t* out_count,
              float* out_scales, void* stream);

/* ---- stream ingest (streaming.py:53-62 Stream.change_frame_size, :75 the video path's BGR -> RGB) --
 * What the reference's streaming.Stream does to every frame before anything else sees it: for one
 * uint8 frame [h,w,3] and a target width set_width
 *   scale = set_width / w                       a float64 division
 *   dh = int(h * scale)                         a truncated float64 product, NOT h * set_width // w:
 *                                               77x77 at 640 becomes 639x640, 117x78 959x640
 *   cv2.resize(frame, (set_width, dh))          the default INTER_LINEAR on an 8UC3 frame: equal size
 *                                               copies, w == 2 set_width and h == 2 dh takes the 2x2 box
 *                                               mean (sum + 2) >> 2, everything else is the 11-bit
 *                                               fixed-point bilinear (fx in float32 from a double
 *                                               expression, horizontal pass into int rows, vertical
 *                                               ((b0 * (S0 >> 4)) >> 16 + (b1 * (S1 >> 4)) >> 16 + 2) >> 2)
 * set_width == 0 means no rescaling.  Results are exact (uint8 equality with cv2's arithmetic).
 *
 * phx_ingest_dims: the ingest size of B frames, host arithmetic only (no context, nothing launched):
 * dims [B,2] int32 (h, w) -> out_dims [B,2] (int(h * ((double)set_width / w)), set_width), or the dims
 * unchanged when set_width is 0.  PHX_EINVAL (message: phx_last_error(NULL)): a null pointer, B < 1,
 * set_width < 0, h or w < 1, a height that truncates to 0 (cv2.resize raises there) or leaves the int
 * range. */
int phx_ingest_dims(int set_width, const int32_t* dims, int B, int32_t* out_dims);
/* One launch for a packed batch of frames of mixed sizes, passed as for phx_serve (src device; offsets,
 * dims host).  Frame b is written at out + out_offsets[b] (out device; out_offsets a HOST array of byte
 * offsets, any alignment) with phx_ingest_dims' size, rows packed; nothing outside the frames is
 * written.  flags: PHX_INGEST_BGR reads channel 2 - c (the reference's cvtColor BGR2RGB on decoded
 * video); set_width == 0 copies, with the swap if asked.
 * Every argument is checked on the host before anything is launched: PHX_EINVAL with a message naming
 * the argument for what phx_ingest_dims refuses, an unknown flag bit, a negative offset, an output frame
 * whose bytes overlap any source frame's or another output frame's (as addresses: src + offsets[k] against
 * out + out_offsets[b]); PHX_ECAP for B > max_batch.  Runs on the caller's stream without synchronising;
 * the host tables may be freed on return.  Shares phx_serve's frame tables: the first serving or ingest
 * call reserves them (synchronous), and the host waits only when 8 such calls are still in flight. */
enum { PHX_INGEST_BGR = 1 };
int phx_ingest(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
               int set_width, int flags, uint8_t* out, const int64_t* out_offsets, void* stream);

/* The person rows of phx_serve's outputs, on the device: Detector.infer's loop (detector.py:48-57)
 * followed by util.filter_by_thresh (util.py:163-174), and the score the demos report (demo.py:81,
 * max(sc) before the * 100.).  boxes [B,100,4], scores [B,100], classes [B,100] float32, valid [B]
 * are phx_serve's outputs (device).  best [B] = the fp32 maximum score over all rows below valid[b]
 * whose class is 1, thresholded or not; 0 when there is none.  pboxes [B,100,4] = the rows with
 * class 1 and score >= (float)min_score_thresh (an fp32 compare, as numpy's float32 >= Python
 * float), compacted in NMS order, zero at and beyond pcount [B].  Rows at and beyond valid[b] are
 * never read.  boxes and pboxes are 16-byte aligned and do not alias.  One wave per frame, no
 * atomics: the result is deterministic.  Allocates nothing and does not synchronise. */
int phx_persons(phx_ctx* ctx, const float* boxes, const float* scores, const float* classes,
                const int32_t* valid, int B, double min_score_thresh, float* pboxes, int32_t* pcount,
                float* best, void* stream);

/* ---- EOT patch pipeline ----------------------------------------------------------------- */
/* BrightnessMatcher.call((src, tgt)) (brightness_matcher.py:43-73) for one src per image:
 * src [B,P,P,3], tgt [B,H,W,3] -> out [B,P,P,3]. */
int phx_brightness_match(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W,
                         int B, float* out, void* stream);

/* The patch-to-scene matcher of the attack's Patcher (attacker.py:362: one word swaps
 * BrightnessMatcher for HistogramMatcher).  MEAN (the default) transfers the Y-channel mean
 * (brightness_matcher.py:14-73); HISTOGRAM does a full histogram specification of the printed
 * patch's Y channel onto the scene's (brightness_matcher.py:76-162), whose gradient treats the
 * lookup table as a constant, as TF autodiff does (the histogram op has no gradient).  The choice
 * is read by phx_patch_images, phx_step_grad and phx_eval_step.  The defender's Masker
 * (phx_def_*) and the inference compositor (phx_adv_patch) keep the mean matcher.  Any other
 * value is PHX_EINVAL with a message; no device call is made.  The setting belongs to the context
 * and is read when a call is issued: like every other call on one context it is not thread-safe, so
 * callers that share a context (two attackers on one victim) set it before each call they issue and
 * do not interleave calls from several threads.  Any batch size up to max_batch runs with either. */
enum { PHX_MATCH_MEAN = 0, PHX_MATCH_HISTOGRAM = 1 };
int phx_set_matcher(phx_ctx* ctx, int matcher);
/* HistogramMatcher.call((src, tgt)) (brightness_matcher.py:82-115), same contract as
 * phx_brightness_match: one src per image, no print variation.  P >= 2, H*W >= 2. */
/* An opt-in box-regression term of the attack objective: the reference's InverseDIOULoss
 * (regression_loss.py:16-142), which the reference kept but never wired in ("unused ... kept for future
 * reuse", :7).  The wiring is this library's: inside the tape of PatchAttacker.call,
 *   loss += weight * InverseDIOULoss()(boxes_pred, boxes)
 * in phx_step_grad (training) and phx_eval_step (test_step) alike, where boxes_pred are the second pass's
 * anchors of argmax class 0 that pass filter_valid_boxes(thresh=False) (attacker.py:118-141: the set the
 * score loss reads) and boxes are the boxes the patches were placed by (the first pass's soft-NMS output, or
 * the caller's boxes / count).  The module is taken as written (regression_loss.py:27-68, :101-142): per
 * (gt g, pred p) 1 - diou_loss(b1 = g, b2 = p) with divide_no_nan twice, the pred's width / height clamped at
 * 0 and the gt's not, the "centres" (ymin + height, xmin + width) and enclose_diag as written; per image
 * sum_g max_p (0 without a pred) + Keras epsilon 1e-7; the batch value is the sum over images.  Gradient
 * rules [TF-recall]: reduce_max splits among exact ties; tf.maximum / tf.minimum send a tie to their first
 * argument (never the pred here) and maximum(0., v) passes only v > 0; divide_no_nan has zero gradient
 * where its denominator is 0.  The masks are not differentiable: the gradient reaches the network through
 * decode_box_outputs (tf2/anchors.py:30-58) only, and the box head then runs backward beside the class head.
 * kind PHX_BOX_LOSS_NONE (the default): every plan, workspace size and result is what it is without this
 * call.  PHX_DTYPE_F32 contexts only.  A change of kind drops the planned executors (the backward plan and
 * the gradient arena change; the next call plans again).  PHX_EINVAL with a message: an unknown kind, a
 * non-finite weight, a PHX_DTYPE_BF16 context; PHX_ESTATE while a phx_set_next batch or its prefetched first
 * pass is pending. */
enum { PHX_BOX_LOSS_NONE = 0, PHX_BOX_LOSS_INV_DIOU = 1 };
int phx_set_box_loss(phx_ctx* ctx, int kind, float weight);
int phx_get_box_loss(const phx_ctx* ctx, int* kind, float* weight);
int phx_histogram_match(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W,
                        int B, float* out, void* stream);
/* Its intermediates, for exact tests: hist [B,2,256] int32 (the 256-bin Y histograms of source
 * and target, tf.histogram_fixed_width(Y, [0,1], 256); NULL = skip) and lut [B,256], the table
 * interpolate(cdf_tgt, floating_space, cdf_src) the pixels are remapped through (device). */
int phx_histogram_lut(phx_ctx* ctx, const float* src, int P, const float* tgt, int H, int W, int B,
                      int32_t* hist, float* lut, void* stream);

/* Patcher.call([boxes, images]) (attacker.py:490-498): print variation, brightness match,
 * placement, antialiased resize, noise, brightness jitter, ±20° rotate, composite, paste.
 * boxes [B,maxb,4] with count [B]; params = [patch | scale]; `step` keys the RNG.
 * Also returns per-box placements [B,maxb,8] (ymin,xmin,ps,diag,angle,delta,valid,-) if
 * `placements` is non-NULL. */
int phx_patch_images(phx_ctx* ctx, const float* images, int B, const float* boxes,
                     const int32_t* count, int maxb, const float* params, int64_t step,
                     int global_image_offset, float* out_images, float* placements,
                     void* stream);

/* ---- the step --------------------------------------------------------------------------- */
/* PatchAttacker.call(images, training=True) (attacker.py:172-219): first pass (or the
 * caller's boxes when `boxes` != NULL: "injected" placement), EOT paste, second pass, loss,
 * and the gradient of the loss w.r.t. [patch | scale] written to `grad` (PHX_NPARAM floats,
 * overwritten).  `add_tv` = 1 adds the 1e-5*TV term (rank 0 only under data parallelism).
 * metrics: PHX_NMETRIC floats (device pointer).  `global_image_offset` = rank * B keys the
 * RNG so draws are independent of the GPU count. */
int phx_step_grad(phx_ctx* ctx, const float* images, int B, const float* boxes,
                  const int32_t* count, int maxb, const float* params, int64_t step,
                  int global_image_offset, int add_tv, float* grad, float* metrics,
                  void* stream);
/* Cross-step first-pass prefetch (first-pass placement, bn=local).  The clean first pass of a step
 * depends on its images, the step (drop connect) and the image offset, not on the patch, so the
 * training loop (attacker_train.py's fit, whose generator has the next batch ready) may name the
 * next batch: the next phx_step_grad without caller boxes then also runs the first pass of
 * next_images — for step + 1 at global_image_offset — on a stream of its own beside its second pass
 * and backward, deferring that pass's BN moving-statistics updates; the phx_step_grad call for
 * exactly those images, B, step and offset applies them (after the previous step's, as in the
 * one-stream order) and places its patches by those detections (attacker.py:180-184), bit for bit
 * the result of running the first pass itself.  next_images must keep its contents until then.
 * NULL withdraws a named batch and also a first pass already prefetched for it (a caller that
 * refilled that device buffer in place: the Python mirror does this when the tensor's version
 * counter moved); the next phx_step_grad consumes a prefetch either way (one with caller boxes
 * drops it).  phx_load_weights and phx_set_score_thresh drop a pending prefetch; phx_sync makes
 * `stream` wait for one. */
int phx_set_next(phx_ctx* ctx, const float* next_images, int B, int32_t global_image_offset);
int phx_sync(phx_ctx* ctx, void* stream);

/* PatchAttacker.call(images, training=False) as run by test_step (attacker.py:318-326): the
 * victim in inference mode (BN from the moving statistics, no drop connect, moving statistics
 * unchanged), first pass (or injected boxes), EOT paste, second pass, loss and the metric row; no
 * gradient.  Optional outputs (NULL = skip): the second pass's soft-NMS person boxes / scores /
 * counts ([B,100,4], [B,100], [B]) that call returns as (boxes_pred, scores_pred). */
int phx_eval_step(phx_ctx* ctx, const float* images, int B, const float* boxes,
                  const int32_t* count, int maxb, const float* params, int64_t step,
                  int global_image_offset, int add_tv, float* metrics, float* out_boxes,
                  float* out_scores, int32_t* out_count, void* stream);

/* ---- training summaries (PatchAttacker.vis_images, attacker.py:257-305) -------------------------
 * What the reference's call hands to TensorBoard every visualize_freq steps, computed on the device.
 * All three calls work in a context of either compute dtype: what they read — images, the patched
 * batch, soft-NMS boxes and scores — is fp32 in both.  Arguments are checked on the host before
 * anything is launched (PHX_EINVAL with a message naming the argument); no call allocates or
 * synchronises, and no workspace is added (the first phx_set_next reserves two label slots of 2.4 KB
 * per image of max_batch for the prefetched detections, counted by phx_workspace_bytes from then on).
 *
 * phx_vis_sample: the "Sample" image of a batch, the box-drawing sibling of phx_soft_nms:
 *   images = tf.image.draw_bounding_boxes(images, convert_format(boxes_a), [[0., 1., 0.]])
 *   images = tf.image.draw_bounding_boxes(images, convert_format(boxes_b), [[0., 0., 1.]])
 *   tf.cast(tf.clip_by_value(images * stddev_rgb + mean_rgb, 0., 255.), tf.uint8)      (truncating)
 * in one pass with the model's own constants; every multiply and add rounds on its own.  images
 * [B,H,W,3] float32; a box set is boxes [B,n,4] pixels (ymin, xmin, ymax, xmax) with count [B] valid
 * rows (1 <= n <= 511; boxes NULL = no such set); image b is written as H*W*3 bytes at out_u8 +
 * b * out_stride + out_offset (bytes; out_stride >= H*W*3), so two calls can interleave their images.
 * The colours are TF float colours written into the normalised image, so drawn pixels come out as
 * mean_rgb (0) or mean_rgb + stddev_rgb (1) per channel, as the reference's do.
 * draw_bounding_boxes as restated here ([TF-recall], parity unpinned): convert_format divides in fp32
 * (ymin / h, xmin / w, ...); the op takes min_row = trunc((ymin / h) * (H - 1)) in fp32, likewise
 * max_row, min_col, max_col; a box with min > max on an axis or wholly outside the image draws
 * nothing; otherwise the top line is drawn if min_row >= 0, the bottom if max_row < H, the left if
 * min_col >= 0, the right if max_col < W, each over the clamped range of the other axis, one pixel
 * thick.  box.to_tensor() pads every image's list with zero boxes up to the batch's longest count (taken
 * from `count` on the device), and a zero box paints pixel (0, 0). */
int phx_vis_sample(phx_ctx* ctx, const float* images, int B, int H, int W, const float* boxes_a,
                   const int32_t* count_a, int n_a, const float* boxes_b, const int32_t* count_b, int n_b,
                   uint8_t* out_u8, int64_t out_stride, int64_t out_offset, void* stream);
/* The counts behind calc_asr (attacker.py:238-255) at T thresholds: out_counts[t] = number of
 * scores[b][j] >= thresholds[t] over j < count[b] (count NULL: N).  scores [B,N] float32 and out_counts
 * [T] int32 are device memory; thresholds [T] is a HOST array, 1 <= T <= 128.  Exact integers. */
int phx_score_curve(phx_ctx* ctx, const float* scores, const int32_t* count, int B, int N, const float* thresholds,
                    int T, int32_t* out_counts, void* stream);
/* Both for the last phx_step_grad or phx_eval_step on this context, from what that step left in its
 * executor: curve_counts int32 [2,T] = the counts of its first-pass detections (row 0: the labels, also
 * with injected placement boxes, exactly what PHX_M_ASR_DEN counts at 0.5) and of its second-pass
 * soft-NMS output (row 1: PHX_M_ASR_NUM at 0.5) at thresholds [T] (host); sample_u8 [B,S,S,3] = its
 * patched batch with the first-pass boxes as set a and the second-pass boxes as set b.  Either output
 * may be NULL.  A step that placed its patches by a phx_set_next prefetch is read where it read: a
 * prefetch's detections go to one of two label slots of the context that no other entry point writes,
 * and the prefetch a step issues itself goes to the other one.  PHX_ESTATE when no step has run, or when its
 * executor was rebuilt (evicted) or used by another call that runs the victim or pastes patches
 * (phx_detect, phx_first_pass, phx_patch_images, phx_serve, a defender on this context) since.
 * The step itself is unchanged: it issues the launches it issued without this call. */
int phx_step_summary(phx_ctx* ctx, const float* thresholds, int T, int32_t* curve_counts, uint8_t* sample_u8,
                     void* stream);

/* Keras Adam (ResourceApplyAdam, beta1 .9, beta2 .999, eps 1e-7; attacker_train.py:38) on
 * [patch | scale] followed by the variable constraints clip(patch,-1,1), clip(scale,0,1)
 * (attacker.py:51-54).  m, v: PHX_NPARAM floats each.  t = 1-based iteration. */
int phx_adam_clip(phx_ctx* ctx, float* params, const float* grad, float* m, float* v,
                  float lr, int64_t t, void* stream);

/* ---- input pipeline (off the attack step) ----------------------------- */
/* DataSequence._map_fn (train_data_generator.py:55-77) for a batch of decoded RGB uint8 images:
 * (x - mean_rgb) / stddev_rgb, resize by min(out_h/h, out_w/w) to (int(h*s), int(w*s)) with
 * cv2.resize INTER_LINEAR semantics, pasted at the top-left of a zero [out_h,out_w,3] canvas.
 * src: packed HWC uint8 images; offsets [B] int64 byte offsets into src; dims [B,2] int32
 * (h, w) — all three device pointers.  mean_rgb / stddev_rgb: 3 floats each (host).
 * out [B,out_h,out_w,3] float32 (device); out_h*out_w*3 must be a multiple of 4. */
int phx_letterbox(phx_ctx* ctx, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
                  const float* mean_rgb, const float* stddev_rgb, int out_h, int out_w, float* out,
                  void* stream);
/* The train-set map chain of partition() (train_data_generator.py:201-204, 222-225):
 * tf.image.random_flip_left_right -> RandomFlip('horizontal') -> RandomContrast(0.2) ->
 * tf.image.random_brightness(0.2) -> clip [-1, 1], on in [B,H,W,3] -> out (must not alias).
 * Flips are drawn per image (Philox keyed by ctx seed, step, global image index), the contrast
 * factor and brightness delta once per step (shared by every rank).  The first call for a
 * batch size allocates a small scratch (synchronous). */
int phx_augment(phx_ctx* ctx, const float* in, int B, int H, int W, int64_t step, int global_image_offset,
                float* out, void* stream);

/* Inference-time patch compositor: AdversarialPatch.add_adv_to_img (adv_patch.py:16-201) for a batch
 * of uint8 RGB images [B,H,W,3] on the device, modified in place.  boxes / count are HOST arrays:
 * boxes [B][max_boxes][4] (ymin, xmin, ymax, xmax in pixels), count [B].  patch [P,P,3] uint8
 * (device) is the unprinted patch (patch.png); the library prints it (print_patch, :40-58).  Boxes
 * are pasted in order, each brightness-matched (cv2 YUV, :110-131) against the image as patched so
 * far rescaled into out_h x out_w (:93-108), resized to the box's patch (cv2 INTER_AREA down,
 * INTER_CUBIC up, :151-164), with U(-0.01, 0.01) noise (:140-149; Philox keyed by ctx seed, step,
 * global image index, box slot).  A patch side below 1 or beyond the image is PHX_EINVAL (the
 * reference's cv2 / numpy raise there).  The first call allocates a small scratch (synchronous). */
int phx_adv_patch(phx_ctx* ctx, uint8_t* images, int B, int H, int W, const float* boxes, const int32_t* count,
                  int max_boxes, const uint8_t* patch, int patch_size, double scale, int out_h, int out_w,
                  int64_t step, int global_image_offset, void* stream);

/* phx_adv_patch with the boxes on the device: the three composites of the demos' loop
 * (demo.py:116, 177 on the boxes of demo.py:72-76) without a host round trip.  Same contract and the
 * same bytes as phx_adv_patch for the same boxes, step and global_image_offset, except:
 *  - boxes [B,max_boxes,4] and count [B] are DEVICE pointers (e.g. phx_persons' pboxes / pcount);
 *  - rounds (host) is the number of paste rounds issued: box k of every frame is pasted in round k,
 *    so rounds >= the largest count pastes everything (phx_adv_patch derives it from its host counts);
 *  - status [B] int32 (device) is overwritten with PHX_AP_* bits.  What phx_adv_patch refuses with
 *    PHX_EINVAL cannot be seen on the host here: such a box is not pasted (the frame's other boxes
 *    are) and its frame's status says why.
 * The placements (AdversarialPatch._create, adv_patch.py:60-91) are computed by a kernel with the host
 * path's arithmetic; a frame without a box in a round skips that round's brightness sum.  Does not
 * synchronise and keeps no host table; the first call (or a larger B, rounds or patch) allocates the
 * scratch it shares with phx_adv_patch (synchronous). */
enum {
  PHX_AP_REFUSED = 1,   /* a box's patch side is below 1 pixel or beyond the frame: not pasted */
  PHX_AP_OVERFLOW = 2,  /* the frame has a box in a slot >= rounds: not pasted                 */
  PHX_AP_BADCOUNT = 4,  /* count[b] outside [0, max_boxes]: clamped                           */
};
int phx_adv_patch_dev(phx_ctx* ctx, uint8_t* images, int B, int H, int W, const float* boxes,
                      const int32_t* count, int max_boxes, int rounds, const uint8_t* patch, int patch_size,
                      double scale, int out_h, int out_w, int64_t step, int global_image_offset,
                      int32_t* status, void* stream);

/* Per-launch-group device timing (HIP events on the launch stream).  enable=1 clears and
 * starts recording; phx_profile_report synchronises and writes JSON
 * {kind: {count, ms, flops, bytes}} with the algorithmic FLOPs / bytes of the launches. */
int phx_profile(phx_ctx* ctx, int enable);
int phx_profile_report(phx_ctx* ctx, char* buf, size_t cap, size_t* needed);

/* Debug / test hooks (parity tests call these; not on the timed path).
 * phx_debug_last_patched: copies the last step's patched images [B,H,W,3] (device->device). */
int phx_debug_last_patched(phx_ctx* ctx, float* out, void* stream);
/* Last step's per-image max scores m_b [B] and loss-anchor index [B] (device->device). */
int phx_debug_last_maxscores(phx_ctx* ctx, float* m, int32_t* anchor, void* stream);
/* Last step's box-regression term (phx_set_box_loss), unweighted: per_image [B] (sum over the image's gts of
 * max_p + 1e-7, regression_loss.py:54-59), and per (image, gt slot) [B,100] the maximum, its lowest anchor
 * index and the number of anchors that reach it exactly (slots at or past the image's gt count, and every
 * slot of an image without a kept anchor: 0, -1, 0).  Any pointer may be NULL (device->device).  PHX_ESTATE
 * when no step with the term has run. */
int phx_debug_last_box_loss(phx_ctx* ctx, float* per_image, float* gt_max, int32_t* gt_anchor,
                            int32_t* gt_nties, void* stream);
/* Last step's second-pass pre_nms outputs (postprocess.pre_nms, postprocess.py:119-156): per-anchor
 * scores [B,A], classes [B,A] and decoded boxes [B,A,4] (ymin, xmin, ymax, xmax px) — the values
 * the loss's person / validity masks read (attacker.py:118-141).  Any pointer may be NULL
 * (device->device). */
int phx_debug_last_detections(phx_ctx* ctx, float* scores, int32_t* classes, float* boxes, void* stream);
/* Last step's d loss / d patched images [B,H,W,3] as the EOT backward reads it (the stem dgrad
 * writes it only at pixels a paste owns; elsewhere 0) (device->device). */
int phx_debug_last_image_grad(phx_ctx* ctx, float* out, void* stream);
/* Per-layer diagnostics of the last step.  `op_name` names an op of the program: a batch norm by
 * its weight prefix (e.g. "efficientnet-b0/blocks_3/tpu_batch_normalization_1"), a BiFPN fuse as
 * "<node>/fuse", a resampling max-pool / upsample as "<resample prefix>/max_pool" / "/upsample".
 * which = 0 copies the op's output (for a batch norm, which is never materialised: its input), which
 * = 1 the loss gradient w.r.t. its output (a batch norm's after its activation); NHWC [B,h,w,C] =
 * nfloats floats (device->device).  PHX_EINVAL if the name or size is wrong, or no gradient exists. */
int phx_debug_tap(phx_ctx* ctx, const char* op_name, int which, float* out, size_t nfloats, void* stream);
/* Stream-hazard diagnostics.  With PHX_CKSUM=1 in the environment (read per call), every
 * phx_step_grad takes an order-independent 64-bit hash of each tensor / statistics slot an op
 * writes, on the op's stream right after it.  This copies the last step's list ("name\thex\n" lines,
 * launch order) of the executor with `tag` (0: the step's, 1: the concurrent first pass's) into buf
 * (synchronising); *needed = bytes including the NUL.  Two steps on the same inputs must give the
 * same list; the first differing line names the launch that broke. */
int phx_debug_checksums(phx_ctx* ctx, int tag, char* buf, size_t cap, size_t* needed);
/* The raw storage (bf16 words in a PHX_DTYPE_BF16 context) of op `op_index`'s output (which = 0) or
 * input which - 1 in the last step's executor `tag`; nbytes must equal its size (device->device). */
int phx_debug_tensor(phx_ctx* ctx, int tag, int op_index, int which, void* out, size_t nbytes, void* stream);

/* ---- defender step (BASELINE C5) ------------------------------------------
 * attack_detection.PatchAttackDefender (attack_detection.py:31-206, training) over a frozen
 * victim ctx: first pass (inference BN, person anchors, soft-NMS, filter_valid_boxes), Masker
 * (self-supervised patches, attack_detection.py:321-498), 2 * PatchNeutralizer(images)
 * (generator.py:17-277: attention U-Net, n_filters 8, dropout 0.2, batch norm) and
 * loss = sum_b mean((targets - updates)^2) with its gradient w.r.t. the U-Net variables.
 * The variables are one flat float buffer in phx_def_manifest order (Keras shapes and layouts:
 * conv kernels [k,k,in,out], transposed-conv kernels [k,k,out,in]); the library owns the BN moving
 * statistics (updated by every step, as Keras training-mode BN).  Replaces generator.define_model
 * + PatchAttackDefender.__init__ (attack_detection.py:34-71). */
typedef struct phx_def phx_def;
/* the U-Net at the victim's image size (a multiple of 16, >= 240); seed keys the Masker's and
 * Dropout's Philox draws */
int phx_def_create(phx_ctx* victim, int max_batch, uint64_t seed, phx_def** out);
void phx_def_destroy(phx_def* d);
/* d == NULL: the message of this thread's last failed phx_def_create. */
const char* phx_def_last_error(phx_def* d);
int64_t phx_def_num_params(phx_def* d);
int64_t phx_def_num_moving(phx_def* d);
/* JSON {n_params, n_moving, params: [{name, shape, offset}], bn: [{name, channels, moving_mean,
 * moving_variance}]} (offsets in floats) */
int phx_def_manifest(phx_def* d, char* buf, size_t cap, size_t* needed);
/* BN moving statistics: src != NULL loads them, dst != NULL copies them out (any memory) */
int phx_def_moving(phx_def* d, float* dst, const float* src, void* stream);
/* Device bytes of the batch-B workspace a training step uses (built if needed). */
int phx_def_workspace_bytes(phx_def* d, int B, size_t* bytes);
/* Device bytes the first phx_def_eval_step at batch B adds to that workspace (the evaluation
 * Masker's matched patches and worst-case resized-patch store, reserved on first use and freed with
 * the workspace); a run that only trains never holds them. */
int phx_def_eval_workspace_bytes(phx_def* d, int B, size_t* bytes);
/* PatchAttackDefender.call(images, training=True) + tape.gradient (attack_detection.py:168-206).
 * boxes [B,100,4] + count [B] (device) place the patches; NULL = the victim's first pass.
 * grad: num_params floats followed by the metric row [loss] (SUM-all-reducible). */
int phx_def_step_grad(phx_def* d, const float* images, int B, const float* boxes, const int32_t* count,
                      const float* params, float* grad, int64_t step, int32_t global_image_offset, void* stream);
/* Cross-step first-pass prefetch.  The first pass of a training step depends only on its images
 * (the protege is frozen), so the host loop (defender_train.py's fit over the generator, which has
 * the next batch ready) may name the next batch: the next phx_def_step_grad then also runs the
 * victim's first pass of next_images — for step + 1 at global_image_offset — on the defender's own
 * stream beside its U-Net work, into a second box buffer, and the phx_def_step_grad call for exactly
 * those images, B, step and offset (without caller boxes) uses those boxes instead of running the
 * first pass (attack_detection.py:174-178: the same boxes either way).  next_images must keep its
 * contents until that call; NULL withdraws it, and a prefetch already made (a refilled buffer).  A
 * prefetch made at another victim generation (a weight load, a training pass or new score thresholds
 * on the victim ctx since) is not used.  A prefetch ties up the victim ctx until it
 * finishes: the defender's own calls wait for it, other users of the victim ctx call phx_def_sync
 * on their stream first. */
int phx_def_set_next(phx_def* d, const float* next_images, int B, int32_t global_image_offset);
/* makes `stream` wait for the first pass a phx_def_set_next prefetch has in flight */
int phx_def_sync(phx_def* d, void* stream);
/* PatchAttackDefender.call(images, training=False) as test_step runs it (attack_detection.py:168-198,
 * 320-326): first pass (or the caller's boxes), the Masker's evaluation branch with the attacker's
 * trained patch — eval_patch = [patch 640*640*3 | scale] (device; the PatchAttackDefender eval_patch
 * directory's patch.tiff / scale.txt, :57-61) — print variation, brightness match, centred placement
 * at the fixed scale (:454-456), the second detector pass odet_model(images, score_thresh=0.)
 * (:185-187, soft-NMS threshold 0.001, filter_valid_boxes at the config's threshold), updates =
 * 2 * PatchNeutralizer(images, training=False) (inference BN, no Dropout) and the loss.  metrics:
 * [loss] (1 float, device).  out_boxes [B,100,4] / out_scores [B,100] / out_count [B]: the second
 * pass's detections (NULL = skip).  No variable or moving statistic changes. */
int phx_def_eval_step(phx_def* d, const float* images, int B, const float* boxes, const int32_t* count,
                      const float* params, const float* eval_patch, float* metrics, float* out_boxes,
                      float* out_scores, int32_t* out_count, int64_t step, int32_t global_image_offset,
                      void* stream);
/* PatchAttackDefender.vis_images (attack_detection.py:239-288) for the last phx_def_step_grad (without
 * caller boxes) or phx_def_eval_step, from what that step left in the workspace.  "Original" is the
 * step's first pass (training) or its attacked second pass (evaluation); "recovered" is
 * odet_model(clip(patched + updates, -1, 1), score_thresh=0.) with the step's own updates, run here with
 * the victim in inference mode (inference BN, no drop connect, no moving statistic changed).
 * sample_u8 [2B,S,S,3]: the attacked image b with the original boxes in [0,1,0] at slot 2b, the
 * recovered image with the recovered boxes in [0,0,1] at slot 2b + 1 (phx_vis_sample's arithmetic).
 * orig_* / rec_*: boxes [B,100,4], scores [B,100], count [B] (device; rows beyond count are zero).  Any
 * output may be NULL, not all.  params is not read (the step's updates are): it may be NULL.
 * Nothing a step computes changes: no variable, no moving statistic, no later gradient.  Waits for a
 * phx_def_set_next prefetch as phx_def_eval_step does and leaves it valid.  Works over a victim of
 * either compute dtype (the buffers read and written are fp32).  PHX_ESTATE when no such step has run
 * since the workspace was built, after a step with caller boxes (they carry no scores) and after a
 * phx_def_recover (it reuses the step's buffers).  The first call of a workspace reserves the recovered
 * batch [B,S,S,3] and its detections (synchronous); from then on phx_def_workspace_bytes counts them.
 * The 3.2 KB per image of detections every step retains for this call are part of the workspace from
 * its creation and counted from there. */
int phx_def_summary(phx_def* d, const float* params, uint8_t* sample_u8, float* orig_boxes, float* orig_scores,
                    int32_t* orig_count, float* rec_boxes, float* rec_scores, int32_t* rec_count, void* stream);
/* ---- frame recovery (demo_v2.py:151-169 RecoveryDemo.serve, :133-134 run's uint8 cast) ----------
 * The trained U-Net applied to raw frames.  For one uint8 RGB frame [h,w,3] at the victim's image size
 * S with its mean_rgb / stddev_rgb:
 *   x, scale = driver._preprocess(frame)            what phx_serve_preprocess writes (scale =
 *                                                   image_scale_to_original, fp32)
 *   y = clip(2 * PatchNeutralizer(x, training=False) + x, -1, 1) * stddev_rgb + mean_rgb   (fp32)
 *   d = int(fp32(S) * scale)                        a truncating fp32 product
 *   cv2.resize(y, (d, d))                           INTER_LINEAR on a CV_32FC3 source: fp32 weights
 *                                                   (1 - f, f), f from float((o + .5) * (S / d) - .5)
 *                                                   in double, taps clamped to the image, horizontal
 *                                                   pass first; S == 2 d takes the 2x2 box mean
 *   [:h, :w]                                        the float image serve returns; run then takes
 *                                                   clip(., 0, 255).astype('uint8'), which truncates
 * The recovered frame is (min(h, d), min(w, d)): the fp32 truncation can leave d one below the frame's
 * longer side (50 x 211 -> 50 x 210, 90 x 120 -> 90 x 119), and the crop then returns a frame one row
 * or column smaller than the input, as the reference does.
 *
 * phx_recover_dims: that size for B frames, host arithmetic only (no context, nothing launched):
 * dims [B,2] int32 (h, w) -> out_dims [B,2] (min(h, d), min(w, d)).  PHX_EINVAL: a null pointer,
 * image_size or B < 1, h or w < 1, a scaled side int(h * image_scale) or int(w * image_scale) of 0,
 * d < 1 (tf.image.resize / cv2.resize raise there). */
int phx_recover_dims(int image_size, const int32_t* dims, int B, int32_t* out_dims);
/* The whole chain for a packed batch of frames, passed as for phx_serve (src device; offsets, dims
 * host).  out_u8 (the clipped, truncated frame) and out_f32 (the float image) are packed device
 * buffers, either may be NULL but not both; frame b starts at element out_offsets[b] (a HOST array,
 * the same element offset in both buffers) and has phx_recover_dims' size, rows packed.  One kernel
 * writes both, so out_u8 is exactly trunc(clip(out_f32, 0, 255)); nothing outside the frames is
 * written.  params: the U-Net variables (phx_def_manifest order); inference BN from the moving
 * statistics, no Dropout; no variable and no moving statistic changes, and the victim is not run.
 * Every argument is checked on the host before anything is launched: PHX_EINVAL with a message naming
 * the argument (phx_def_last_error) for B < 1, a null pointer, both outputs null, a negative offset
 * and what phx_serve_preprocess refuses; PHX_ECAP for B > max_batch.  Runs on the caller's stream
 * without synchronising; the host tables may be freed on return.  The first call reserves the frame
 * tables and the first call at a batch size the workspace (both synchronous); later calls allocate
 * nothing — unless 8 calls are still in flight, when the host waits for the oldest one's table.  Waits
 * for a phx_def_set_next prefetch as phx_def_eval_step does and leaves it valid.
 * The call reuses the training workspace: the preprocess writes the U-Net's input buffer and the
 * output layer the `updates` buffer, so afterwards phx_def_debug(PHX_DEF_PATCHED / PHX_DEF_UPDATES)
 * and phx_def_debug_tap show this call's canvas [B,S,S,3] and forward (PHX_DEF_TARGETS keeps the last
 * step's). */
int phx_def_recover(phx_def* d, const uint8_t* src, const int64_t* offsets, const int32_t* dims, int B,
                    const float* params, uint8_t* out_u8, float* out_f32, const int64_t* out_offsets,
                    void* stream);
/* debug copies of the last step (device->device): patched images / targets / updates [B,H,W,3],
 * first-pass boxes [B,100,4], counts [B] (int32 bits) */
enum { PHX_DEF_PATCHED = 0, PHX_DEF_TARGETS = 1, PHX_DEF_UPDATES = 2, PHX_DEF_BOXES = 3, PHX_DEF_COUNTS = 4 };
int phx_def_debug(phx_def* d, int what, float* dst, size_t nfloats, void* stream);
/* Read-only tap of a tensor the U-Net forward of the last step (training or evaluation) stored; the
 * backward reads these and leaves them as they are.  Copies the named tensor, NHWC float32
 * [B,h,w,C], to dst (any memory, nfloats >= its size); nothing but the copy is launched.  Names, in
 * program order (i = 0..3; the encoder level i works at S >> i, decoder i at S >> (3 - i)):
 *   conv<i>/y1, /a1, /y2, /a2     encoder block i: y* = the 3x3 conv outputs with bias, before BN;
 *                                 a* = leaky_relu(BN(y*))
 *   conv<i>/pool                  max-pool 2x2 of a2, after Dropout in training [B,h/2,w/2,C]
 *   conv4/y1, /a1, /y2, /a2       the bottleneck block
 *   deconv<i>/up                  the transposed conv's output with bias
 *   deconv<i>/att_g, /att_x       the attention's 1x1 conv outputs (of up / of the skip) with bias,
 *                                 before their BN
 *   deconv<i>/att_s               leaky_relu(BN1(att_g) + BN2(att_x))
 *   deconv<i>/att_t               the 1-channel 1x1 conv of att_s with bias, before bn3 [B,h,w,1]
 *   deconv<i>/cat                 concat(up, skip * sigmoid(bn3(att_t))), after Dropout in training
 *   deconv<i>/convblock/y1, /a1, /y2, /a2   the decoder's conv block
 *   updates                       2 * tanh(output conv) [B,S,S,3]
 * PHX_EINVAL: unknown name; PHX_ESTATE: no U-Net forward has run since the workspace was (re)built (a
 * new batch size rebuilds it); PHX_ECAP: destination too small. */
int phx_def_debug_tap(phx_def* d, const char* name, float* dst, size_t nfloats, void* stream);
/* Keras Adam without constraints (the defender's optimizer, defender_train.py:35) */
int phx_adam(float* params, const float* grad, float* m, float* v, int64_t n, float lr, int64_t t, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PHX_H_ */
