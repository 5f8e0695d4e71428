"""GPU: the training summaries (kernels_vis.hip, phx_vis_sample / phx_score_curve / phx_step_summary /
phx_def_summary, the vis_images hooks) against tests/vis_oracle.py.  Every comparison is exact: uint8
bytes and integer counts.  The step-level tests feed the oracle the device's own fp32 tensors (the
patched batch, the detections), so nothing depends on detector rounding."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vis_oracle as VO

pytestmark = pytest.mark.gpu

MEAN = np.array([0.485 * 255, 0.456 * 255, 0.406 * 255], np.float32)
STD = np.array([0.229 * 255, 0.224 * 255, 0.225 * 255], np.float32)
GUARD = 0xCD


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(scope="module")
def ctx():
    from mladversarialobjectdetection_amd import _lib
    return _lib.Context("efficientdet-d0", image_size=128, max_batch=4)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _vis(ctx, img, a, b, out, stride, offset):
    """phx_vis_sample on device tensors; a / b: (boxes [B,n,4], count [B]) or None"""
    B, H, W, _ = img.shape
    args = []
    for s in (a, b):
        args += [None, None, 0] if s is None else [s[0].data_ptr(), s[1].data_ptr(), s[0].shape[1]]
    ctx.call("phx_vis_sample", img.data_ptr(), B, H, W, *args, out, int(stride), int(offset), _stream())


# ---- phx_vis_sample ------------------------------------------------------------------------------
SPLIT_Y, SPLIT_X = np.float32(36 / 11), np.float32(70 / 9)  # fp32 and exact arithmetic disagree here


def _small_case():
    H, W = 12, 10
    rng = np.random.default_rng(3)
    img = rng.uniform(-4, 4, (3, H, W, 3)).astype(np.float32)  # beyond +-3: both clips fire
    a = np.zeros((3, 4, 4), np.float32)
    a[0, 0] = [0, 0, 12, 10]                   # touches all four edges
    a[0, 1] = [-3, -2, 6, 5]                   # partly outside: top and left
    a[0, 2] = [SPLIT_Y, SPLIT_X, 9, 9.5]       # the fp32 / exact split on both axes
    a[2, 0] = [5, 4, 15, 13]                   # partly outside: bottom and right
    a[1, 0] = [1, 1, 3, 3]                     # beyond its count: never drawn
    ca = np.array([3, 0, 1], np.int32)
    b = np.zeros((3, 3, 4), np.float32)
    b[0, 0] = [13.5, 1, 20, 5]                 # wholly outside
    b[0, 1] = [8, 2, 3, 6]                     # inverted
    b[0, 2] = [0, 0, 6, 5]                     # overlaps A's lines
    b[1, 0] = [5, 5, 5, 5]                     # zero area, inside
    b[1, 1] = [2, 2, 7, 7]
    b[1, 2] = [20, 20, 30, 30]
    cb = np.array([3, 3, 0], np.int32)
    return img, a, ca, b, cb


def test_split_coordinate_really_splits():
    from fractions import Fraction
    assert VO.extents([SPLIT_Y, SPLIT_X, 0, 0], 12, 10)[:2] == (3, 7)
    assert (int(Fraction(float(SPLIT_Y)) * 11 / 12), int(Fraction(float(SPLIT_X)) * 9 / 10)) == (2, 6)


@pytest.mark.parametrize("lead", [16, 5])  # an aligned output (16-B loads, dword stores) and an unaligned one
def test_vis_sample_small_matches_oracle(ctx, lead):
    img, a, ca, b, cb = _small_case()
    n = 12 * 10 * 3
    want = VO.sample(img, a, ca, b, cb, mean=MEAN, std=STD)
    # the padding pixel: image 1 has no A box (its B list is full), image 2 neither a full A list nor a B
    # box, so B's padding paints over A's; the batch's longest lists have 3
    assert (want[1, 0, 0] == [123, 173, 103]).all() and (want[2, 0, 0] == [123, 116, 160]).all()
    assert want.min() == 0 and want.max() == 255
    buf = torch.full((lead + 3 * n + 16,), GUARD, dtype=torch.uint8, device="cuda")
    _vis(ctx, _dev(img), (_dev(a), _dev(ca)), (_dev(b), _dev(cb)), buf.data_ptr() + lead, n, 0)
    got = buf.cpu().numpy()
    assert (got[:lead] == GUARD).all() and (got[lead + 3 * n:] == GUARD).all()
    np.testing.assert_array_equal(got[lead:lead + 3 * n].reshape(3, 12, 10, 3), want)


def test_vis_sample_interleaved_layout_matches_oracle(ctx):
    """H = W = 128, 100 random boxes per set, two calls interleaving into one [2B,S,S,3] buffer (the
    defender's layout): several workgroups per image, boxes staged per row band."""
    B, S, N = 2, 128, 100
    rng = np.random.default_rng(8)
    img = rng.uniform(-1.5, 1.5, (2, B, S, S, 3)).astype(np.float32)
    sets = []
    for k in range(2):
        y0, x0 = rng.uniform(-20, 120, (2, B, N)).astype(np.float32)
        hh, ww = rng.uniform(-10, 80, (2, B, N)).astype(np.float32)  # some inverted
        sets.append(np.stack([y0, x0, y0 + hh, x0 + ww], -1).astype(np.float32))
    cnt = [np.array([100, 57], np.int32), np.array([31, 100], np.int32)]
    n = S * S * 3
    lead = 64
    buf = torch.full((lead + 2 * B * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    _vis(ctx, _dev(img[0]), (_dev(sets[0]), _dev(cnt[0])), None, buf.data_ptr() + lead, 2 * n, 0)
    _vis(ctx, _dev(img[1]), None, (_dev(sets[1]), _dev(cnt[1])), buf.data_ptr() + lead, 2 * n, n)
    got = buf.cpu().numpy()
    assert (got[:lead] == GUARD).all() and (got[lead + 2 * B * n:] == GUARD).all()
    got = got[lead:lead + 2 * B * n].reshape(B, 2, S, S, 3)
    np.testing.assert_array_equal(got[:, 0], VO.sample(img[0], sets[0], cnt[0], mean=MEAN, std=STD))
    np.testing.assert_array_equal(got[:, 1], VO.sample(img[1], None, None, sets[1], cnt[1], mean=MEAN, std=STD))


def test_vis_sample_checks_its_arguments(ctx):
    from mladversarialobjectdetection_amd import _lib
    x = torch.zeros(1, 4, 4, 3, device="cuda")
    out = torch.zeros(48, dtype=torch.uint8, device="cuda")
    bx = torch.zeros(1, 2, 4, device="cuda")
    for args, word in (((None, 1, 4, 4, None, None, 0, None, None, 0, out.data_ptr(), 48, 0), "images"),
                       ((x.data_ptr(), 1, 4, 4, None, None, 0, None, None, 0, None, 48, 0), "out_u8"),
                       ((x.data_ptr(), 1, 4, 4, bx.data_ptr(), None, 2, None, None, 0, out.data_ptr(), 48, 0), "count_a"),
                       ((x.data_ptr(), 2, 4, 4, None, None, 0, None, None, 0, out.data_ptr(), 47, 0), "out_stride"),
                       ((x.data_ptr(), 1, 4, 4, None, None, 0, None, None, 0, out.data_ptr(), 48, -1), "out_offset")):
        with pytest.raises(_lib.PhxError, match=word):
            ctx.call("phx_vis_sample", *args, _stream())


# ---- phx_score_curve -----------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 31, 128])
def test_score_curve_matches_numpy(ctx, T):
    B, N = 3, 100
    bins = np.arange(0.5, .805, .01, dtype="float32")
    th = {1: bins[:1], 31: bins, 128: np.linspace(0, 1, 128).astype(np.float32)}[T]
    assert len(th) == T
    rng = np.random.default_rng(T)
    sc = rng.uniform(0, 1, (B, N)).astype(np.float32)
    sc[0, :31] = bins            # the float32 bin values themselves, counted
    sc[2, 10:41] = bins          # partly beyond image 2's count
    sc[1, :31] = bins            # an empty image: never counted
    cnt = np.array([100, 0, 37], np.int32)
    out = torch.full((T + 2,), -7, dtype=torch.int32, device="cuda")
    dsc, dcnt = _dev(sc), _dev(cnt)
    ctx.call("phx_score_curve", dsc.data_ptr(), dcnt.data_ptr(), B, N, th.ctypes.data, T, out.data_ptr() + 4, _stream())
    got = out.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    np.testing.assert_array_equal(got[1:-1], VO.curve_counts(sc, cnt, th))


# ---- phx_step_summary ----------------------------------------------------------------------------
S, PB = 128, 4.0  # tests/test_gpu_firstpass.py's setting: >= 20 first-pass boxes per image


def _victim(person_bias=PB, **kw):
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    return EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=2, rng_seed=5,
                              person_bias=person_bias, **kw)


def _images(seed=1, B=2, size=S):
    return np.random.default_rng(seed).uniform(-1, 1, (B, size, size, 3)).astype(np.float32)


def _step_summary(att, B):
    bins = np.ascontiguousarray(att.bins, np.float32)
    counts = torch.full((2, len(bins)), -1, dtype=torch.int32, device="cuda")
    sample = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    att.model.ctx.call("phx_step_summary", bins.ctypes.data, len(bins), counts.data_ptr(), sample.data_ptr(), _stream())
    patched = torch.empty(B, S, S, 3, device="cuda")
    att.model.ctx.call("phx_debug_last_patched", patched.data_ptr(), _stream())
    return counts.cpu().numpy(), sample.cpu().numpy(), patched.cpu().numpy()


def _second_pass_of_last_step(victim, B):
    """The last step's second-pass soft-NMS detections, rebuilt from its own pre_nms outputs: person and
    valid anchors (attacker.py:203-205) through the device's soft-NMS."""
    from oracle import postprocess as pp
    A = victim.num_anchors
    sc = torch.empty(B, A, device="cuda")
    cl = torch.empty(B, A, dtype=torch.int32, device="cuda")
    bx = torch.empty(B, A, 4, device="cuda")
    victim.ctx.call("phx_debug_last_detections", sc.data_ptr(), cl.data_ptr(), bx.data_ptr(), _stream())
    sc, cl, bx = sc.cpu().numpy(), cl.cpu().numpy(), bx.cpu().numpy()
    keep = [(cl[b] == 0) & pp.valid_mask(bx[b], S, S) for b in range(B)]
    n = max(int(k.sum()) for k in keep)
    cb, cs, cc = np.zeros((B, n, 4), np.float32), np.zeros((B, n), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        cc[b] = keep[b].sum()
        cb[b, :cc[b]], cs[b, :cc[b]] = bx[b][keep[b]], sc[b][keep[b]]
    return [t.cpu().numpy() for t in victim.soft_nms(_dev(cb), _dev(cs), _dev(cc))]


def _check_summary(att, counts, sample, patched, first, second, met, min_first=20):
    from mladversarialobjectdetection_amd import _lib
    fb, fs, fc = first
    sb, ss, sc_ = second
    assert fc.min() >= min_first
    np.testing.assert_array_equal(counts[0], VO.curve_counts(fs, fc, att.bins))
    np.testing.assert_array_equal(counts[1], VO.curve_counts(ss, sc_, att.bins))
    assert att.bins[0] == np.float32(0.5)
    assert counts[0, 0] == met[_lib.M_ASR_DEN] and counts[1, 0] == met[_lib.M_ASR_NUM]
    want = VO.sample(patched, fb, fc, sb, sc_, mean=MEAN, std=STD)
    np.testing.assert_array_equal(sample, want)
    drawn = (want == [123, 173, 103]).all(-1) | (want == [123, 116, 160]).all(-1)
    assert drawn.sum() > 5 * min_first  # boxes were drawn


def test_step_summary_after_eval_step():
    """call(training=False) on a bn=frozen victim, whose phx_first_pass is the step's own first pass.
    Inference BN at the initial moving statistics keeps one person per image at person_bias 4; at 6 the
    oracle's inference-mode first pass fills all 100 slots, so the usual >= 20 boxes are asked for."""
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    v = _victim(person_bias=6.0, bn_mode="frozen")
    assert v.ctx.lib.phx_step_summary(v.ctx.h, None, 0, None, None, None) == -3  # no step yet: PHX_ESTATE
    att = PatchAttacker(v, seed=7)
    att.cur_step = 2
    x = _dev(_images(seed=6))
    second = [t.cpu().numpy() for t in att.call(x, training=False)]
    met = att.metrics_buf.cpu().numpy()
    counts, sample, patched = _step_summary(att, 2)
    first = [t.cpu().numpy() for t in v.first_pass(x)]
    _check_summary(att, counts, sample, patched, first, second, met)
    # the first pass just run reused the executor: the step's state is gone
    assert v.ctx.lib.phx_step_summary(v.ctx.h, None, 0, None, None, None) == -3


def test_step_summary_after_training_step_changes_nothing():
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    v = _victim()
    att = PatchAttacker(v, seed=7)
    att.cur_step = 4
    x = _dev(_images())
    att.call(x)
    g0, met = att.grad.clone(), att.metrics_buf.cpu().numpy()
    counts, sample, patched = _step_summary(att, 2)
    vis = att.vis_images()
    second = _second_pass_of_last_step(v, 2)
    # the same step again, after the summaries: gradient and metric row bit for bit
    att.call(x)
    assert torch.equal(att.grad, g0)
    np.testing.assert_array_equal(att.metrics_buf.cpu().numpy(), met)
    w_with = v.read_weights()
    first = [t.cpu().numpy() for t in v.first_pass(x)]
    _check_summary(att, counts, sample, patched, first, second, met)
    # vis_images returns the same sample, the curve by _derive's rule and the patch as save_weights does
    np.testing.assert_array_equal(vis["Sample"], sample)
    np.testing.assert_array_equal(vis["ASR"][0], att.bins)
    np.testing.assert_array_equal(vis["ASR"][1], VO.asr(counts[1], counts[0]))
    p = att.patch.cpu().numpy()
    np.testing.assert_array_equal(vis["Patch"], np.clip(p * STD + MEAN, 0, 255).astype(np.uint8))
    # and the moving statistics two steps leave are those of a run that never asked for a summary
    v2 = _victim()
    att2 = PatchAttacker(v2, seed=7)
    att2.cur_step = 4
    att2.call(x)
    att2.call(x)
    assert torch.equal(att2.grad, g0)
    np.testing.assert_array_equal(v2.read_weights(), w_with)


def test_step_summary_reads_a_prefetched_first_pass_where_the_step_read_it():
    """train_step(next_inputs=...): the second step places its patches by the first pass prefetched into
    the side executor and prefetches the third batch itself; its summary still shows its own labels."""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    xs = [_dev(_images(seed=20 + i)) for i in range(3)]
    v = _victim()
    att = PatchAttacker(v, seed=7)
    ws0 = v.ctx.workspace_bytes(2)
    att.train_step(xs[0], next_inputs=xs[1])
    att.train_step(xs[1], next_inputs=xs[2])
    # the side executor and the prefetch's two label slots (2 * 2.4 KB per image, rounded to 256 B) are counted
    assert v.ctx.workspace_bytes(2) - ws0 > 2 * 2 * 2404
    met = att._pending[-1][1].cpu().numpy()[:_lib.NMETRIC]
    counts, sample, patched = _step_summary(att, 2)
    second = _second_pass_of_last_step(v, 2)
    att.train_step(xs[2])
    att.sync()
    w = v.read_weights()
    # three steps with the prefetch end where three steps without it do
    v2 = _victim()
    att2 = PatchAttacker(v2, seed=7)
    for x in xs:
        att2.train_step(x)
    assert torch.equal(att2.params, att.params)
    np.testing.assert_array_equal(v2.read_weights(), w)
    first = [t.cpu().numpy() for t in v.first_pass(xs[1])]
    _check_summary(att, counts, sample, patched, first, second, met)


def test_eval_step_between_a_prefetch_and_its_consumer_leaves_the_prefetch_intact():
    """train_step(next), train_step(next), test_step, train_step: the validation pass at the same batch
    size runs between the second step's prefetch and the step that consumes it, and writes its executor's
    own first-pass buffers.  The prefetched labels live in the context's label slots, so the last step
    still places its patches by them: parameters, metric rows and moving statistics are bit for bit
    those of the same sequence without any prefetch."""
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    xs = [_dev(_images(seed=30 + i)) for i in range(3)]
    xv = _dev(_images(seed=40))

    def run(prefetch):
        v = _victim()
        att = PatchAttacker(v, seed=7)
        att.train_step(xs[0], next_inputs=xs[1] if prefetch else None)
        att.train_step(xs[1], next_inputs=xs[2] if prefetch else None)
        m, (vb, vs, vc) = att.test_step(xv)
        att.train_step(xs[2])
        att.sync()
        rows = torch.stack([r for _, r in att._pending]).cpu().numpy()
        return att.params.cpu().numpy(), rows, v.read_weights(), vb.cpu().numpy(), vc.cpu().numpy(), m

    a, b = run(True), run(False)
    from mladversarialobjectdetection_amd import _lib
    assert b[1][:, _lib.M_ASR_DEN].min() >= 40  # every step had first-pass labels to place by
    for got, want in zip(a[:5], b[:5]):
        np.testing.assert_array_equal(got, want)
    assert a[5] == b[5]


def test_visualize_freq_zero_means_never(tmp_path):
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    from mladversarialobjectdetection_amd.summaries import DirWriter
    att = PatchAttacker(_victim(), seed=7, visualize_freq=0, summary_writer=DirWriter(tmp_path / "log"))
    x = _dev(_images())
    att.train_step(x)
    att.test_step(x)
    assert not (tmp_path / "log").exists()


# ---- hooks ---------------------------------------------------------------------------------------
def _counts(ctx):
    return {k: r["count"] for k, r in ctx.profile_report().items()}


def test_writer_hook_writes_every_visualize_freq_steps_and_costs_nothing_otherwise(tmp_path):
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    from mladversarialobjectdetection_amd.summaries import DirWriter
    v = _victim()
    x = _dev(_images())
    att = PatchAttacker(v, seed=7, visualize_freq=2, summary_writer=DirWriter(tmp_path / "log"))
    for _ in range(3):
        att.train_step(x)
    att.test_step(x)
    files = sorted(os.listdir(tmp_path / "log" / "train"))
    want = []
    for step in (0, 2):
        want += [f"ASR_{step:08d}.npz", f"Patch_{step:08d}_0.png", f"Sample_{step:08d}_0.png", f"Sample_{step:08d}_1.png"]
    assert files == sorted(want)
    assert sorted(os.listdir(tmp_path / "log" / "val")) == ["ASR_00000000.npz", "Sample_00000000_0.png",
                                                            "Sample_00000000_1.png"]
    from PIL import Image
    z = np.load(tmp_path / "log" / "train" / "ASR_00000002.npz")
    assert z["x"].dtype == np.float32 and len(z["x"]) == len(z["y"]) == len(att.bins)
    assert np.asarray(Image.open(tmp_path / "log" / "train" / "Sample_00000002_1.png")).shape == (S, S, 3)
    # launch groups of one step: no writer == a writer on a step it skips; a summarised step adds its two
    plain = PatchAttacker(v, seed=7, visualize_freq=2)
    v.ctx.profile(True)
    plain.train_step(x)
    base = _counts(v.ctx)
    v.ctx.profile(True)
    att.train_step(x)  # cur_step 3: skipped
    assert _counts(v.ctx) == base
    v.ctx.profile(True)
    att.train_step(x)  # cur_step 4: summarised
    with_vis = _counts(v.ctx)
    v.ctx.profile(False)
    assert with_vis == {**base, "score_curve": 1, "vis_sample": 1}
    assert os.listdir(tmp_path) == ["log"]  # the attacker without a writer wrote nothing


# ---- phx_def_summary -----------------------------------------------------------------------------
DS, DB = 256, 2  # tests/test_gpu_defender.py's size and overrides
OV = {"nms_configs": {"iou_thresh": .5, "score_thresh": .5}}


@pytest.fixture(scope="module")
def dvictim():
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    return EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=DS, max_batch=DB, rng_seed=5,
                              person_bias=4.0, bn_mode="frozen")


def _defender(dvictim, **kw):
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    epatch = np.random.default_rng(12).uniform(-1, 1, (640, 640, 3)).astype(np.float32)
    return PatchAttackDefender(dvictim, protege_config_override=OV, seed=9, eval_patch=(epatch, 0.4), **kw)


def _recovered_detections(victim, rec):
    """odet_model(rec, score_thresh=0.) by an independent route on the same context: its per-anchor
    detections, person anchors through the device's soft-NMS at threshold 0 (0.001), then
    filter_valid_boxes at the config's 0.5 on the host (attack_detection.py:79-127)."""
    B = rec.shape[0]
    bx, sc, cl = (t.cpu().numpy() for t in victim.detect(_dev(rec)))
    keep = [cl[b] == 0 for b in range(B)]
    n = max(int(k.sum()) for k in keep)
    cb, cs, cc = np.zeros((B, n, 4), np.float32), np.zeros((B, n), np.float32), np.zeros(B, np.int32)
    for b in range(B):
        cc[b] = keep[b].sum()
        cb[b, :cc[b]], cs[b, :cc[b]] = bx[b][keep[b]], sc[b][keep[b]]
    victim.ctx.set_score_thresh(0.0)
    try:
        nb, ns, nc = (t.cpu().numpy() for t in victim.soft_nms(_dev(cb), _dev(cs), _dev(cc)))
    finally:
        victim.ctx.set_score_thresh(0.5)
    ob, os_, oc = np.zeros((B, 100, 4), np.float32), np.zeros((B, 100), np.float32), np.zeros(B, np.int32)
    f = np.float32
    for b in range(B):
        q, s = nb[b, :nc[b]], ns[b, :nc[b]]
        h, w = q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]
        ok = (w / f(DS) <= 1) & (h / f(DS) <= 1) & (h * w > f(100)) & (s >= f(.5))
        oc[b] = ok.sum()
        ob[b, :oc[b]], os_[b, :oc[b]] = q[ok], s[ok]
    return ob, os_, oc


def _check_def_summary(d, dvictim, orig_want=None):
    sample, orig, rec = d.summary()
    sample = sample.cpu().numpy().reshape(DB, 2, DS, DS, 3)
    orig = [t.cpu().numpy() for t in orig]
    rec = [t.cpu().numpy() for t in rec]
    patched = d.debug(0, DB).cpu().numpy()
    upd = d.debug(2, DB).cpu().numpy()
    if orig_want is not None:
        for got, want in zip(orig, orig_want):
            np.testing.assert_array_equal(got, want)
    assert orig[2].sum() > 0
    np.testing.assert_array_equal(sample[:, 0], VO.sample(patched, orig[0], orig[2], mean=MEAN, std=STD))
    updated = np.clip((patched + upd).astype(np.float32), np.float32(-1), np.float32(1))
    np.testing.assert_array_equal(sample[:, 1], VO.sample(updated, None, None, rec[0], rec[2], mean=MEAN, std=STD))
    for got, want in zip(rec, _recovered_detections(dvictim, updated)):
        np.testing.assert_array_equal(got, want)
    return orig, rec


def test_def_summary_after_training_and_eval_steps(dvictim):
    from mladversarialobjectdetection_amd import _lib
    d = _defender(dvictim)
    with pytest.raises(_lib.PhxError, match=r"\(-3\)"):
        d._last_B = DB
        d.summary()  # no step yet: PHX_ESTATE
    x, x2 = _dev(_images(1, DB, DS)), _dev(_images(2, DB, DS))
    d.cur_step = 3
    params0 = d.params.clone()
    d.call(x)
    boxes = d.debug(3, DB).cpu().numpy()
    count = d.debug(4, DB).cpu().numpy()
    orig, _ = _check_def_summary(d, dvictim)
    np.testing.assert_array_equal(orig[0], boxes)
    np.testing.assert_array_equal(orig[2], count)
    assert (orig[1][0, :count[0]] >= 0.5).all()
    d.cur_step = 4
    g = d.call(x2).clone()
    mv = d.moving_statistics()
    assert torch.equal(d.params, params0)
    # a run that never asks for a summary: same moving statistics, same following gradient
    e = _defender(dvictim)
    e.cur_step = 3
    e.call(x)
    e.cur_step = 4
    assert torch.equal(e.call(x2), g)
    np.testing.assert_array_equal(e.moving_statistics(), mv)
    # evaluation: "original" is the attacked second pass the step returned
    ob, os_, oc = (t.cpu().numpy() for t in d.call(x, training=False))
    _check_def_summary(d, dvictim, (ob, os_, oc))
    np.testing.assert_array_equal(d.moving_statistics(), mv)
    assert torch.equal(d.params, params0)
    vis = d.vis_images(False)
    assert vis["Sample"].shape == (2 * DB, DS, DS, 3) and vis["Sample"].dtype == np.uint8
    np.testing.assert_array_equal(vis["Scores"][0], np.concatenate([os_[b, :oc[b]] for b in range(DB)]))


def test_defender_writer_hook(dvictim, tmp_path):
    from mladversarialobjectdetection_amd.summaries import DirWriter
    d = _defender(dvictim, visualize_freq=2, summary_writer=DirWriter(tmp_path))
    x = _dev(_images(1, DB, DS))
    for _ in range(3):
        d.train_step(x)
    want = []
    for step in (0, 2):
        want += [f"Scores_{step:08d}.npz"] + [f"Sample_{step:08d}_{i}.png" for i in range(2 * DB)]
    assert sorted(os.listdir(tmp_path / "train")) == sorted(want)
    assert not (tmp_path / "val").exists()
