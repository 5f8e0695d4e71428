"""BASELINE C5 at its own size: the defender step on a D0 victim at 512^2 (parity ran
only at 256^2).  The U-Net (generator.py:17-277) then has its full five-level depth at 512 / 256 /
128 / 64 / 32 pixels, the levels the 256^2 case never reaches.

  * B = 2 against the fp64 oracle (oracle/defender.py): Masker pixels, loss, every variable's
    gradient and stored tensor (unet_parity.py's bounds), moving statistics — the tolerances of
    tests/test_gpu_defender.py;
  * B = 8 (C5's per-GPU share of 64 images over 8 GPUs): bit-identical on rerun, and the loss the
    library reports equals sum_b mean((t - u)^2) recomputed in fp64 from its own targets and
    U-Net updates (2 * unet(x), attack_detection.py:189-193), a size-independent consistency check.
"""
import numpy as np
import pytest
import torch

import unet_parity as UP

pytestmark = pytest.mark.gpu

S = 512
MEASURED_REL = 3.486e-4  # test_defender_512_step_matches_oracle's overall ||g - g64|| / ||g64|| on an MI355X


def _victim(B):
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    return EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=B, rng_seed=5,
                              person_bias=4.0, bn_mode="frozen")


def _defender(v, seed=9):
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    return PatchAttackDefender(v, protege_config_override={"nms_configs": {"iou_thresh": .5, "score_thresh": .5}},
                               seed=seed)


def _images(B, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (B, S, S, 3)).astype(np.float32)


def _boxes():
    return [np.array([[40, 60, 400, 240], [200, 200, 500, 500]], np.float32),
            np.array([[10, 10, 480, 280]], np.float32)]


@pytest.mark.timeout(900)
def test_defender_512_step_matches_oracle():
    from oracle import defender as DF
    B = 2
    d = _defender(_victim(B))
    mv = d.moving_statistics()
    mv0 = {b["name"]: (mv[b["moving_mean"]:b["moving_mean"] + b["channels"]].astype(np.float64),
                       mv[b["moving_variance"]:b["moving_variance"] + b["channels"]].astype(np.float64))
           for b in d.manifest["bn"]}
    imgs = _images(B, 3)
    params = d.params.cpu().numpy().copy()
    d.cur_step = 5
    d.call(torch.as_tensor(imgs).cuda(), boxes=_boxes())
    torch.cuda.synchronize()
    g = d.grad.cpu().numpy().astype(np.float64)
    loss = float(d.loss_buf.item())
    patched = d.debug(0, B).cpu().numpy()
    targets = d.debug(1, B).cpu().numpy()
    upd = d.debug(2, B).cpu().numpy()
    fwd = UP.gpu_taps(d, B)
    torch.set_num_threads(16)
    rp, rt = DF.masker(imgs, _boxes(), 9, 5, 0)
    for got, ref in ((patched, rp), (targets, rt)):
        dd = np.abs(got - ref)
        assert (dd <= 1e-4).mean() >= 0.9999, f"{(dd > 1e-4).mean():.2e} off, max {dd.max():.3e}"
    full = UP.reference(params, mv0, patched, targets, seed=9, step=5)  # the oracle in fp64 and in fp32
    ref = full.r64
    assert abs(loss - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert np.abs(upd - ref["updates"]).max() <= 1e-4
    rel, cos = UP.overall(g, full)
    print(f"overall rel {rel:.3e} (fp32 oracle {full.overall32:.3e}) cos {cos:.9f}")
    assert cos >= 0.99999, cos
    # 4x the rel measured on an MI355X, or the fp32 oracle's own where that is smaller, and never above
    # the 1e-3 this test held before
    assert rel <= min(1e-3, 4 * MEASURED_REL, full.overall32), (rel, full.overall32)
    # per tap and per variable, within a multiple of the fp32 oracle's own deviation (unet_parity.py)
    rep = UP.sweep(full, fwd, g, var_cap=2e-2)  # (and never above the 2e-2 this test held before)
    print(rep.table())
    rep.check()
    assert rep.counts() == dict(fwd=UP.N_FWD, var=UP.N_VAR, zero=UP.N_ZERO)
    mv = d.moving_statistics()
    for b in d.manifest["bn"]:
        rm, rv = ref["moving"][b["name"]]
        np.testing.assert_allclose(mv[b["moving_mean"]:b["moving_mean"] + b["channels"]], rm, rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(mv[b["moving_variance"]:b["moving_variance"] + b["channels"]], rv,
                                   rtol=1e-4, atol=1e-6)


@pytest.mark.timeout(600)
def test_defender_512_batch8_deterministic_and_consistent():
    B = 8
    v = _victim(B)
    imgs = torch.as_tensor(_images(B, 4)).cuda()
    runs = []
    for _ in range(2):
        d = _defender(v, seed=11)
        d.cur_step = 2
        d.call(imgs)   # the victim's own first pass places the patches
        torch.cuda.synchronize()
        runs.append((d.grad.cpu().numpy().copy(), float(d.loss_buf.item()),
                     d.debug(1, B).cpu().numpy().astype(np.float64), d.debug(2, B).cpu().numpy().astype(np.float64),
                     d.debug(4, B).cpu().numpy()))
    (g0, l0, t0, u0, c0), (g1, l1, _, _, _) = runs
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    assert np.array_equal(g0, g1) and l0 == l1
    assert c0.sum() > 0   # the first pass found persons to patch
    ref = sum(float(((t0[b] - u0[b]) ** 2).mean()) for b in range(B))  # updates = 2 * unet(x)
    assert abs(l0 - ref) <= 1e-5 * abs(ref), (l0, ref)
