"""GPU: every stored tensor of the defender's U-Net forward and every variable's gradient against the fp64
oracle (tests/unet_parity.py; phx_def_debug_tap against oracle.defender.UNet.taps), away from the
variables as initialised and at row counts that are no multiple of a tile.

test_unet_step_matches_oracle and test_defender_512_step_matches_oracle start from zero biases, gamma 1,
beta 0 and moving statistics (0, 1), at M = B * H^2 a multiple of 64 on every level.  A kernel that
drops a bias add, takes the leaky-ReLU sign without beta, loses gamma from a data gradient or mishandles
a partial tile passes both (tests/test_unet_parity.py shows the first three passing unnoticed).  Here:

  case  S    B  variables                 mode   reaches
  A     256  2  as initialised            train  test_unet_step_matches_oracle's case, now per layer
  B     240  3  randomised                train  M = 172800 .. 2700, 675 (= 42 * 16 + 3): a partial last
                                                 weight-gradient slice, a partial 16-row conv tile, column
                                                 reductions with a short last block; Masker crop P = S;
                                                 no power-of-two side, so every wide conv takes the
                                                 column-matrix GEMM
  C     272  2  randomised                train  17 x 17 bottleneck (M = 578), odd H into the stride-2
                                                 transposed conv and its gathers
  D     256  3  randomised, moving        eval   inference BN (launch_bn_frozen_stats), no Dropout: forward
                statistics = the fp64            taps, updates and loss only; variables and moving
                oracle's batch statistics        statistics bit-unchanged

Randomised (fixed seeds, unet_parity.case_variables): kernels as init_unet_params draws them, gamma ~
U(0.5, 1.5), beta ~ N(0, 0.3), every bias ~ N(0, 0.3); in B and C moving mean ~ N(0, 0.5) and variance ~
U(0.5, 2) through phx_def_moving, so the momentum update is checked away from (0, 1).  All cases inject
boxes and feed the library's own Masker output to the oracle; neither the victim's first pass nor the
oracle's detector runs in the training cases.

Per case: the forward sweep (65 taps), the gradient sweep (100 variables) and the analytically-zero
class (30 biases) are clean at unet_parity's multiples, the counts are pinned, loss rel <=
1e-5, the updated moving statistics within rtol 1e-4 / atol 1e-6.

Measured on an MI355X (worst ratio to max(o32, f) per class; overall ||g - g64|| / ||g64|| of the device
and of the fp32 oracle run on that machine's CPU, 16 threads; relative loss error):
  case  fwd    var    zero   overall rel (fp32 oracle)  loss err
  A     0.83   1.03   0.92   3.08e-4 (4.02e-4)          2.5e-8
  B     0.79   0.76   2.00   6.57e-5 (5.69e-4)          6.0e-9
  C     0.82   7.25   0.68   4.03e-4 (1.88e-4)          8.5e-9
  D     0.90   -      -      -                          1.5e-8   (max |d updates| 1.3e-5, 0.45 % saturated)
512^2 (test_defender_512_step_matches_oracle): 0.81 / 0.86 / 0.45, overall 3.49e-4 (5.66e-4).
K = ceil(2 x worst), capped at 4 / 16 / 16: K_FWD = 2, K_ZERO = 4, and for the variables K_VAR = 8 (worst
3.65, case C's conv0/bn1/beta) except the four attention bn3/gamma, which have K_VAR_BN3_GAMMA = 15
(unet_parity.py).  Case C's 7.25 is deconv1/attention/bn3/gamma alone (e_dev 1.1e-1 against the fp32 oracle's 1.5e-2): the
gamma of a one-channel BN in front of a sigmoid, a single number whose gradient sum_m dz xhat cancels to
6.9e-5 beside a whole gradient of norm 2.5 (the error is 3e-6 of that); it is the fp32 oracle's own
worst variable of the case by a factor of ten.
No sweep exposed a kernel error.
"""
import numpy as np
import pytest
import torch

import unet_parity as UP

pytestmark = pytest.mark.gpu

OVERRIDE = {"nms_configs": {"iou_thresh": .5, "score_thresh": .5}}
_victims = {}


def victim(S):
    """a D0 victim context at S: with injected boxes only a handle (case D's second pass runs it)"""
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    if S not in _victims:
        _victims[S] = EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=3,
                                         rng_seed=5, person_bias=4.0, bn_mode="frozen")
    return _victims[S]


@pytest.mark.parametrize("case", [c for c in UP.CASES if UP.CASES[c]["mode"] == "train"])
def test_unet_layers_match_oracle(case):
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    S, B, imgs, boxes, step = UP.case_inputs(case)
    d = PatchAttackDefender(victim(S), protege_config_override=OVERRIDE, seed=UP.DEF_SEED)
    params, mv = UP.case_variables(case, d.manifest)
    UP.load_variables(d, params, mv)
    mv0 = UP.moving_dict(d.manifest, d.moving_statistics())
    d.cur_step = step
    d.call(torch.as_tensor(imgs).cuda(), boxes=boxes)
    torch.cuda.synchronize()
    g = d.grad.cpu().numpy().astype(np.float64)
    loss = float(d.loss_buf.item())
    patched = d.debug(0, B).cpu().numpy()
    targets = d.debug(1, B).cpu().numpy()
    fwd = UP.gpu_taps(d, B)
    assert np.array_equal(fwd["updates"], d.debug(2, B).cpu().numpy())
    assert np.array_equal(d.params.cpu().numpy(), params)

    torch.set_num_threads(16)
    ref = UP.reference(params, mv0, patched, targets, step=step)
    rep = UP.sweep(ref, fwd, g)
    print(rep.table())
    rel, cos = UP.overall(g, ref)
    loss_err = abs(loss - ref.r64["loss"]) / abs(ref.r64["loss"])
    print(f"case {case}: worst ratio " + " ".join(f"{c} {rep.worst_ratio(c):.3f}" for c in UP.CLASSES)
          + " (floors " + " ".join(f"{c} {v:.3e}" for c, v in rep.floors.items())
          + f"); overall rel {rel:.3e} (fp32 oracle {ref.overall32:.3e}) cos {cos:.9f} loss err {loss_err:.3e}")

    assert np.abs(targets).max() > 0.1  # patches were pasted
    assert set(ref.zero) == UP.expected_zero_names()
    rep.check()
    assert rep.counts() == dict(fwd=UP.N_FWD, var=UP.N_VAR, zero=UP.N_ZERO)
    assert loss_err <= 1e-5
    assert cos >= 0.99999 and rel <= 1e-3  # test_unet_step_matches_oracle's overall bounds
    UP.check_moving(d.manifest, d.moving_statistics(), ref.r64["moving"])


def test_unet_layers_match_oracle_eval():
    """case D"""
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    case = "D"
    S, B, imgs, boxes, step = UP.case_inputs(case)
    d = PatchAttackDefender(victim(S), protege_config_override=OVERRIDE, seed=UP.DEF_SEED,
                            eval_patch=(UP.eval_patch(), UP.EVAL_SCALE))
    params, _ = UP.case_variables(case, d.manifest)
    UP.load_variables(d, params, None)
    d.cur_step = step
    x = torch.as_tensor(imgs).cuda()
    # the Masker's output does not depend on the U-Net: a first evaluation yields the patched images
    # the moving statistics are taken from
    d.call(x, training=False, boxes=boxes)
    torch.cuda.synchronize()
    patched = d.debug(0, B).cpu().numpy()
    torch.set_num_threads(16)
    UP.load_variables(d, params, UP.batch_statistics(d.manifest, params, patched, UP.DEF_SEED, step))
    mv_before = d.moving_statistics()
    d.call(x, training=False, boxes=boxes)
    torch.cuda.synchronize()
    loss = float(d.eval_loss.item())
    assert np.array_equal(d.debug(0, B).cpu().numpy(), patched)
    targets = d.debug(1, B).cpu().numpy()
    fwd = UP.gpu_taps(d, B)
    assert np.array_equal(fwd["updates"], d.debug(2, B).cpu().numpy())
    # nothing may change
    assert np.array_equal(d.params.cpu().numpy(), params)
    assert np.array_equal(d.moving_statistics(), mv_before)

    ref = UP.reference(params, UP.moving_dict(d.manifest, mv_before), patched, targets, step=step, training=False)
    rep = UP.sweep(ref, fwd)
    print(rep.table())
    loss_err = abs(loss - ref.r64["loss"]) / abs(ref.r64["loss"])
    pre = np.arctanh(np.clip(ref.r64["updates"] / 2.0, -1 + 1e-15, 1 - 1e-15))
    sat = float((np.abs(pre) > 3).mean())
    print(f"case D: worst ratio fwd {rep.worst_ratio('fwd'):.3f} (floor {rep.floors['fwd']:.3e}); "
          f"loss err {loss_err:.3e}; |pre-tanh| > 3 at {sat:.4f} of the outputs; "
          f"max |d updates| {np.abs(fwd['updates'] - ref.r64['updates']).max():.3e}")
    assert np.abs(targets).max() > 0.1
    assert sat <= 0.10  # the parity is not of saturated values
    rep.check()
    assert rep.counts() == dict(fwd=UP.N_FWD, var=0, zero=0)
    assert loss_err <= 1e-5


def test_tap_refusals():
    """unknown name, destination too small, no forward yet in this workspace: an error text, nothing
    copied"""
    import ctypes
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    S, B, imgs, boxes, step = UP.case_inputs("A")
    d = PatchAttackDefender(victim(S), seed=UP.DEF_SEED)
    buf = torch.full((B * S * S * 8,), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    with pytest.raises(_lib.PhxError, match="no U-Net forward has run"):
        d.handle.call("phx_def_debug_tap", b"conv0/y1", buf.data_ptr(), buf.numel(), st)
    d.call(torch.as_tensor(imgs).cuda(), boxes=boxes)
    with pytest.raises(_lib.PhxError, match="no tensor named conv0/y3"):
        d.handle.call("phx_def_debug_tap", b"conv0/y3", buf.data_ptr(), buf.numel(), st)
    with pytest.raises(_lib.PhxError, match="destination too small"):
        d.handle.call("phx_def_debug_tap", b"conv0/y1", buf.data_ptr(), buf.numel() - 1, st)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
    d.handle.call("phx_def_debug_tap", b"conv0/y1", buf.data_ptr(), buf.numel(), st)
    assert np.array_equal(buf.cpu().numpy().reshape(B, S, S, 8), d.debug_tap("conv0/y1", B).cpu().numpy())
    # another batch size rebuilds the workspace: nothing to tap until a forward has written it
    buf.fill_(7.0)
    n = ctypes.c_size_t()
    d.handle.call("phx_def_workspace_bytes", B - 1, ctypes.byref(n))
    with pytest.raises(_lib.PhxError, match="no U-Net forward has run"):
        d.handle.call("phx_def_debug_tap", b"conv0/y1", buf.data_ptr(), buf.numel(), st)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
