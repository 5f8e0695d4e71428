"""GPU: the histogram matcher (brightness_matcher.py:76-162) through libphx.so against its restatement
in tests/hist_oracle.py.

  histograms, lookup table   exact (integer counts; the table bit for bit)
  matched patch              |d| <= 2e-5 * max(1, largest segment slope of the image's table): 2e-5 is
                             the mean matcher's bound (test_gpu_parity.py), which covers slope 1; the
                             slope is what a one-ulp change of Y is multiplied by
  EOT paste, step gradient   the bounds of test_patch_images_matches_oracle / test_step_grad_matches_oracle
  default matcher            bit-identical before and after a histogram-matcher step

Every test prints its figures before it asserts (pytest -s).  On an MI355X the step test gave a
patch-gradient cosine of 1 - 4.7e-12 and a relative error of 3.1e-6 (128x128, seed 7, step 3, TV on),
and the matched patches sat within 2.6e-6 of the oracle in every case.
"""
import os

import numpy as np
import pytest
import torch

import hist_oracle as HO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 128
f32 = np.float32
SHAPES = [(37, 24, 40), (640, 128, 128)]  # P*P = 1369: no multiple of 4 or 256; the attack's own sizes


@pytest.fixture(scope="module")
def victim():
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    return EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=4, rng_seed=5)


def _images(B, seed=1, size=S):
    return np.random.default_rng(seed).uniform(-1, 1, (B, size, size, 3)).astype(np.float32)


def _boxes():
    return [np.array([[10, 20, 90, 70]], np.float32),
            np.array([[5, 5, 120, 60], [30, 40, 100, 110]], np.float32)]


_PAIRS = {}


def _pair(shape):
    """Bin-safe uniform sources and U(-1.5, 1.5) targets (end bins) of one shape, B = 2, with their
    restated (hist_src, hist_tgt, lut) per image; drawn once."""
    if shape not in _PAIRS:
        P, H, W = shape
        rng = np.random.default_rng(4)
        src = HO.bin_safe(rng.uniform(-1, 1, (2, P, P, 3)).astype(f32), rng)
        tgt = rng.uniform(-1.5, 1.5, (2, H, W, 3)).astype(f32)
        _PAIRS[shape] = (src, tgt, [HO.lut32(src[b], tgt[b]) for b in range(2)])
    return _PAIRS[shape]


def _gpu_lut(victim, src, tgt):
    from mladversarialobjectdetection_amd.attacker import HistogramMatcher
    hist, lut = HistogramMatcher(victim).lut((torch.as_tensor(src).cuda(), torch.as_tensor(tgt).cuda()))
    return hist.cpu().numpy(), lut.cpu().numpy()


def _gpu_match(victim, src, tgt):
    from mladversarialobjectdetection_amd.attacker import HistogramMatcher
    return HistogramMatcher(victim)((torch.as_tensor(src).cuda(), torch.as_tensor(tgt).cuda())).cpu().numpy()


def _ref_match(src, tgt):
    return HO.hist_match(torch.as_tensor(src, dtype=torch.float64), torch.as_tensor(tgt, dtype=torch.float64)).numpy()


@pytest.mark.parametrize("shape", SHAPES)
def test_histograms_and_lut_exact(victim, shape):
    P, H, W = shape
    src, tgt, refs = _pair(shape)
    hist, lut = _gpu_lut(victim, src, tgt)
    for b, (hs, ht, rl) in enumerate(refs):
        assert hist[b, 0].sum() == P * P and hist[b, 1].sum() == H * W
        assert np.array_equal(hist[b, 0], hs) and np.array_equal(hist[b, 1], ht)
        assert ht[0] > 0 and ht[255] > 0  # the end bins took the out-of-range values
        assert np.array_equal(lut[b].view(np.uint32), rl.view(np.uint32)), np.abs(lut[b] - rl).max()


def _check_forward(victim, src, tgt):
    out = _gpu_match(victim, src, tgt)
    assert np.isfinite(out).all()
    for b in range(src.shape[0]):
        bound = 2e-5 * max(1.0, HO.max_slope(HO.lut32(src[b], tgt[b])[2]))
        err = np.abs(out[b] - _ref_match(src[b], tgt[b])).max()
        print(f"histogram match {src.shape[1]}px image {b}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_oracle(victim, shape):
    src, tgt, _ = _pair(shape)
    _check_forward(victim, src, tgt)


def _burj():
    d = np.load(os.path.join(ROOT, "tests", "golden", "burj_khalifa_96.npz"))
    return [((d[k].astype(f32) - f32(127.0)) / f32(127.0)).astype(f32)
            for k in ("burj_khalifa_day", "burj_khalifa_sunset")]


@pytest.mark.parametrize("case", ["constant target", "black source", "beyond range", "burj", "burj crop"])
def test_edge_inputs(victim, case):
    P, H, W = SHAPES[0]
    rng = np.random.default_rng(6)
    src = HO.bin_safe(rng.uniform(-1, 1, (2, P, P, 3)).astype(f32), rng)
    tgt = rng.uniform(-1, 1, (2, H, W, 3)).astype(f32)
    if case == "constant target":
        tgt = np.stack([np.full((H, W, 3), 0.25, f32), np.full((H, W, 3), -1.0, f32)])
    elif case == "black source":  # Y = 0: the x <= dx[0] branch
        src = np.full((2, P, P, 3), -1.0, f32)
    elif case == "beyond range":  # Y below 0 and above 1: both end branches
        src = HO.bin_safe(rng.uniform(-1.6, 1.6, (2, P, P, 3)).astype(f32), rng, lo=-1.6, hi=1.6)
        assert HO.y32(src).min() < 0.0 and HO.y32(src).max() > 1.0
    elif case == "burj":  # photographs: most pixels in a few bins (LDS counter contention)
        day, sunset = _burj()
        src, tgt = np.stack([day, sunset]), np.stack([sunset, day])
    elif case == "burj crop":
        day, sunset = _burj()
        src, tgt = np.stack([day[:P, :P], sunset[-P:, -P:]]), np.stack([sunset, day])
    hist, lut = _gpu_lut(victim, src, tgt)
    for b in range(2):
        hs, ht, rl = HO.lut32(src[b], tgt[b])
        assert np.array_equal(hist[b, 0], hs) and np.array_equal(hist[b, 1], ht)
        assert np.array_equal(lut[b].view(np.uint32), rl.view(np.uint32))
    _check_forward(victim, src, tgt)


@pytest.fixture(scope="module")
def step_setup(victim):
    """The inputs of test_patch_images_matches_oracle / test_step_grad_matches_oracle made bin-safe (the
    images, and the patch under both images' print parameters), one attacker with the histogram
    matcher, and the oracle's step with its matcher swapped for hist_match (computed once)."""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd import weights as W
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    from oracle import eot
    from oracle import step as ST
    rng = np.random.default_rng(8)
    imgs = np.stack([HO.bin_safe(im, rng) for im in _images(2)])
    att = PatchAttacker(victim, seed=7, matcher="histogram")
    att.cur_step = 3
    prints = [eot.print_params(5, 3, b) for b in range(2)]
    patch = HO.bin_safe(att.patch.cpu().numpy(), rng, prints=prints)
    att.params[:_lib.NPATCH].copy_(torch.as_tensor(patch.reshape(-1)))
    mp = pytest.MonkeyPatch()
    mp.setattr(eot, "brightness_match", HO.hist_match)
    try:
        ref = ST.attack_step(W.unpack(victim.manifest, victim.blob), imgs, patch, np.float32(0.4), boxes=_boxes(),
                             seed=5, step=3, image_size=S, add_tv=True)
    finally:
        mp.undo()
    return att, imgs, ref


def test_patch_images_match_oracle(victim, step_setup):
    att, imgs, ref = step_setup
    out = att._patcher([_boxes(), torch.as_tensor(imgs).cuda()]).cpu().numpy()
    pl = att._patcher.last_placements.cpu().numpy()
    for b in range(2):
        for k, p in enumerate(ref["places"][b]):
            assert [p["ymin"], p["xmin"], p["ps"], p["diag"], int(p["valid"])] == \
                [int(pl[b, k, 0]), int(pl[b, k, 1]), int(pl[b, k, 2]), int(pl[b, k, 3]), int(pl[b, k, 6])]
            assert abs(p["angle"] - pl[b, k, 4]) <= 1e-7 and abs(p["delta"] - pl[b, k, 5]) <= 1e-7
        d = np.abs(out[b] - ref["patched"][b])
        print(f"histogram EOT paste image {b}: share within 1e-4 {(d <= 1e-4).mean():.6f}, max {d.max():.3e}")
        assert (d <= 1e-4).mean() >= 0.9999, d.max()


def test_step_grad_matches_oracle(victim, step_setup):
    from mladversarialobjectdetection_amd import _lib
    att, imgs, ref = step_setup
    att.call(torch.as_tensor(imgs).cuda(), boxes=_boxes(), add_tv=True)
    g = att.grad.cpu().numpy().astype(np.float64)
    met = att.metrics_buf.cpu().numpy()
    gp, rp = g[:-1], ref["grad"][:-1]
    cos = gp @ rp / (np.linalg.norm(gp) * np.linalg.norm(rp))
    rel = np.linalg.norm(gp - rp) / np.linalg.norm(rp)
    print(f"histogram step: loss {met[_lib.M_LOSS]:.7f} vs {ref['loss']:.7f}, cosine 1 - {1 - cos:.3e}, rel {rel:.3e}")
    assert np.isfinite(g).all()
    assert abs(met[_lib.M_LOSS] - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert abs(g[-1] - ref["grad"][-1]) <= 1e-5 * max(1.0, abs(ref["grad"][-1]))
    assert cos >= 0.99999, cos
    assert rel <= 1e-3, rel


@pytest.mark.parametrize("matcher", ["brightness", "histogram"])
def test_batch_beyond_one_table_tile(matcher):
    """The histogram backward passes the images' tables through LDS 16 at a time: a batch of 18 crosses
    the tile boundary.  With inference BN (bn=frozen) the images of a step do not interact, and every
    random draw is keyed by the global image index, so the gradient of the 18-image step equals the sum
    of the gradients of images 0-15 and of images 16-17 (run at image offset 16).  TV is left out: its
    gradient does not pass through the matcher and would only dilute the comparison.
    Both sides are fp32 evaluations of the same sum in another order (and the victim's GEMMs tile 18,
    16 and 2 images differently), each within the step test's bounds of the exact value, so they are
    held to those bounds against each other: cosine >= 0.99999, relative error <= 1e-3.  A tile that
    dropped or mixed up images 16-17 would miss them by their share of the gradient (0.32 here; measured
    relative error 7.8e-7).
    The mean matcher runs the same comparison as a control of the method."""
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim, PatchAttacker
    B = 18
    v = EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=B, rng_seed=5,
                           bn_mode="frozen")
    x = torch.as_tensor(_images(B, seed=11)).cuda()
    boxes = [_boxes()[b % 2] for b in range(B)]
    att = PatchAttacker(v, seed=7, matcher=matcher)
    att.cur_step = 3

    def grad(lo, hi):
        att.global_offset = lambda n: lo
        att.call(x[lo:hi], boxes=boxes[lo:hi], add_tv=False)
        return att.grad.cpu().numpy().astype(np.float64)

    full, head, tail = grad(0, B), grad(0, 16), grad(16, B)
    parts = head + tail
    share = np.linalg.norm(tail[:-1]) / np.linalg.norm(full[:-1])
    assert np.isfinite(full).all() and share > 0
    cos = full[:-1] @ parts[:-1] / (np.linalg.norm(full[:-1]) * np.linalg.norm(parts[:-1]))
    rel = np.linalg.norm(full[:-1] - parts[:-1]) / np.linalg.norm(parts[:-1])
    print(f"{matcher} 18 = 16 + 2 images: |g| {np.linalg.norm(full[:-1]):.3e}, share of images 16-17 {share:.3f}, cosine 1 - {1 - cos:.3e}, rel {rel:.3e}, d scale {full[-1]:.6e} vs {parts[-1]:.6e}")
    assert cos >= 0.99999, cos
    assert rel <= 1e-3, rel
    assert abs(full[-1] - parts[-1]) <= 1e-5 * max(1.0, abs(parts[-1]))


def test_default_matcher_untouched(victim):
    """One context: the default step, the same step after phx_set_matcher(MEAN), and once more after a
    histogram-matcher step in between: gradients and metrics bit for bit the same."""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    x = torch.as_tensor(_images(2)).cuda()
    att = PatchAttacker(victim, seed=7)
    att.cur_step = 3

    def run(a):
        a.call(x, boxes=_boxes(), add_tv=True)
        return a.grad.cpu().numpy().copy(), a.metrics_buf.cpu().numpy().copy()

    g1, m1 = run(att)
    victim.ctx.call("phx_set_matcher", _lib.MATCH_MEAN)
    g2, m2 = run(att)
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)) and np.array_equal(m1.view(np.uint32), m2.view(np.uint32))
    ath = PatchAttacker(victim, seed=7, matcher="histogram")
    ath.cur_step = 3
    gh, _ = run(ath)
    assert np.isfinite(gh).all() and not np.array_equal(gh, g1)  # the other matcher did run
    victim.ctx.call("phx_set_matcher", _lib.MATCH_MEAN)
    g3, m3 = run(att)
    assert np.array_equal(g1.view(np.uint32), g3.view(np.uint32)) and np.array_equal(m1.view(np.uint32), m3.view(np.uint32))
