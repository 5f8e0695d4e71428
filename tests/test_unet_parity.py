"""CPU: the defender's per-layer / per-variable sweep (tests/unet_parity.py) with the fp32 oracle as the
stand-in for a device.

The clean stand-in passes at the chosen multiples (and at 1: it is the yardstick itself).  Each seeded
error in a stand-in U-Net, of the kind a kernel could have, fails with the expected first failing tap
or variable at case B's randomised variables (240^2, B = 3: the bottleneck has M = 675 rows).  The bias,
beta and gamma errors are then shown to pass unnoticed at case A's variables as initialised (zero
biases, gamma 1, beta 0), the only variables the gradient parity saw before.

The conditions on the cases' inputs are checked here against the oracle alone: patches were pasted,
every Dropout layer keeps 75 % .. 85 %, case D's outputs are not saturated, and the analytically-zero
class holds exactly the 30 expected biases.  The Masker here is the oracle's (the GPU test feeds the
library's own output, which test_masker_matches_oracle holds within 1e-4 of it).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import unet_parity as UP
from oracle import defender as DF


def masked_inputs(case):
    S, B, imgs, boxes, step = UP.case_inputs(case)
    if UP.CASES[case]["mode"] == "train":
        patched, targets = DF.masker(imgs, boxes, UP.DEF_SEED, step, 0)
    else:
        patched, targets = DF.masker_eval(imgs, boxes, UP.eval_patch(), UP.EVAL_SCALE, UP.DEF_SEED, step, 0)
    return patched.astype(np.float32), targets.astype(np.float32), step


class Case:
    def __init__(self, name):
        torch.set_num_threads(min(16, torch.get_num_threads()))
        self.man = UP.cpu_manifest()
        self.params, mv = UP.case_variables(name, self.man)
        self.moving = UP.moving_dict(self.man, UP.initial_moving(self.man) if mv is None else mv)
        self.patched, self.targets, self.step = masked_inputs(name)
        self.ref = UP.reference(self.params, self.moving, self.patched, self.targets, step=self.step)

    def standin(self, unet):
        """an fp32 step of a (faulty) U-Net in the form of a device result"""
        r = DF.defender_step(self.params, self.moving, self.patched, seed=UP.DEF_SEED, step=self.step,
                             masked=(self.patched, self.targets), dtype=torch.float32, taps={}, unet=unet)
        return UP.standin(r)


@pytest.fixture(scope="module")
def case_a():
    return Case("A")


@pytest.fixture(scope="module")
def case_b():
    return Case("B")


# ---- seeded errors --------------------------------------------------------------------------------
class BiasDropped(DF.UNet):
    """the transposed conv of deconv1 without its bias add (the backward, which never reads the bias,
    as it is)"""

    def tconv(self, x, name):
        y = super().tconv(x, name)
        if name == "deconv1/cnv":
            y = y - self.p[f"{name}/bias"].detach()[None, :, None, None]
        return y


class BetaOutOfLeakySign(DF.UNet):
    """conv2/bn1's backward takes the leaky-ReLU slope from the sign of z - beta"""

    def bn_act(self, x, name):
        if name != "conv2/bn1":
            return super().bn_act(x, name)
        z = self.bn(x, name)
        b = self.p[f"{name}/beta"][None, :, None, None]
        zm = z * torch.where(z - b > 0, 1.0, 0.2).to(z.dtype).detach()
        return self.leaky(z).detach() + (zm - zm.detach())


class GammaOutOfDataGradient(DF.UNet):
    """conv2/bn2's data gradient without gamma (sc = gamma * rstd taken as rstd); d gamma, d beta intact"""

    def bn_affine(self, x, mean, inv, g, b, name):
        if name != "conv2/bn2":
            return super().bn_affine(x, mean, inv, g, b, name)
        xhat = (x - mean[None, :, None, None]) * inv[None, :, None, None]
        wrong = xhat.detach() * g[None, :, None, None] + b[None, :, None, None] + (xhat - xhat.detach())
        # (the forward value bit for bit as the clean one)
        return super().bn_affine(x, mean, inv, g, b, name).detach() + (wrong - wrong.detach())


class TconvShifted(DF.UNet):
    """deconv2's transposed conv cropped one pixel down and right"""

    def tconv(self, x, name):
        if name != "deconv2/cnv":
            return super().tconv(x, name)
        w = self.p[f"{name}/kernel"].permute(3, 2, 0, 1)
        H, W = x.shape[2], x.shape[3]
        return F.conv_transpose2d(x, w, self.p[f"{name}/bias"], stride=2)[:, :, 1:2 * H + 1, 1:2 * W + 1]


class GateDetached(DF.UNet):
    """no gradient through deconv1's attention gate"""

    def gate(self, skip, a, name):
        if name != "deconv1/attention":
            return super().gate(skip, a, name)
        return skip * (a.detach() + 0.0 * a)


class DropoutUnscaled(DF.UNet):
    """Dropout layer 5 (deconv1's concatenation) without the 1 / (1 - rate)"""

    def dropout_scale(self, layer):
        return 1.0 if layer == 5 else super().dropout_scale(layer)


class WgradTailRows(DF.UNet):
    """conv4/cnv2's kernel gradient without the last 3 of its M rows (forward and data gradient intact)"""

    def conv(self, x, name, k):
        y = super().conv(x, name, k)
        if name != "conv4/cnv2":
            return y
        w = self.p[f"{name}/kernel"].detach().permute(3, 2, 0, 1)
        y_nograd = F.conv2d(x, w, self.p[f"{name}/bias"], padding=k // 2)
        B, _, H, W = y.shape
        tail = (torch.arange(B * H * W) >= B * H * W - 3).reshape(B, 1, H, W)
        return torch.where(tail, y_nograd, y)


# (stand-in, class of the first failure, first failing row, last passing row before it)
FAULTS = [
    (BiasDropped, "fwd", "deconv1/up", "deconv0/convblock/a2"),
    (BetaOutOfLeakySign, "var", "conv2/bn1/gamma", "conv2/cnv2/kernel"),
    (GammaOutOfDataGradient, "var", "conv2/cnv2/kernel", "conv2/bn2/beta"),
    (TconvShifted, "fwd", "deconv2/up", "deconv1/convblock/a2"),
    (GateDetached, "var", "deconv1/attention/bn3/gamma", "deconv1/convblock/cnv1/kernel"),
    (DropoutUnscaled, "fwd", "deconv1/cat", "deconv1/att_t"),
    (WgradTailRows, "var", "conv4/cnv2/kernel", "conv4/bn2/beta"),
]


def test_case_b_reaches_the_tails(case_b):
    # 3 * 15 * 15 = 675 = 42 * 16 + 3 rows at the bottleneck
    assert case_b.ref.fwd["conv4/y2"].shape == (3, 15, 15, 128) and 3 * 15 * 15 == 42 * 16 + 3


@pytest.mark.parametrize("case", ["a", "b"])
def test_clean_standin_passes(case, case_a, case_b):
    c = case_a if case == "a" else case_b
    fwd, grad = c.standin(None)
    for k in (None, 1):  # at the chosen multiples, and as the yardstick itself
        rep = UP.sweep(c.ref, fwd, grad, k, k, k)
        rep.check()
        assert rep.counts() == dict(fwd=UP.N_FWD, var=UP.N_VAR, zero=UP.N_ZERO)
    assert set(c.ref.zero) == UP.expected_zero_names()
    assert UP.overall(grad, c.ref)[0] == pytest.approx(c.ref.overall32)


@pytest.mark.parametrize("unet,cls,first,last", FAULTS, ids=[f[0].__name__ for f in FAULTS])
def test_seeded_error_is_found(unet, cls, first, last, case_b):
    fwd, grad = case_b.standin(unet)
    rep = UP.sweep(case_b.ref, fwd, grad)
    ff = rep.first_failure(cls)
    assert ff is not None, f"{unet.__name__} passed unnoticed"
    assert (ff[0].name, ff[1].name) == (first, last), rep.table()
    if cls == "var":  # an error of the backward alone: the forward sweep stays clean
        assert not rep.failures("fwd")
    with pytest.raises(AssertionError, match=f"first failing row, {cls} sweep: {cls} {first}"):
        rep.check()


@pytest.mark.parametrize("unet", [BiasDropped, BetaOutOfLeakySign, GammaOutOfDataGradient],
                         ids=lambda u: u.__name__)
def test_seeded_error_unnoticed_at_initial_variables(unet, case_a):
    """the gap: zero biases, gamma 1 and beta 0 hide these three from any gradient parity"""
    fwd, grad = case_a.standin(unet)
    UP.sweep(case_a.ref, fwd, grad).check()
    rel, cos = UP.overall(grad, case_a.ref)
    assert rel <= 1e-3 and cos >= 0.99999  # test_unet_step_matches_oracle's overall bounds


def test_zero_class_bound_has_teeth(case_b):
    """a bias gradient that is not the analytically-zero one (here: the kernel's norm times 1e-4) fails"""
    fwd, grad = case_b.standin(None)
    sl = case_b.ref.sl
    name = "conv3/cnv1/bias"
    grad = grad.copy()
    grad[sl[name]] = 1e-4 * np.linalg.norm(grad[sl["conv3/cnv1/kernel"]]) / np.sqrt(64)
    ff = UP.sweep(case_b.ref, fwd, grad).first_failure("zero")
    assert ff is not None and ff[0].name == name


@pytest.mark.parametrize("case", list(UP.CASES))
def test_case_input_conditions(case, case_a, case_b):
    S, B, _, _, _ = UP.case_inputs(case)
    c = {"A": case_a, "B": case_b}.get(case)
    if c is not None:
        targets, step = c.targets, c.step
    else:
        patched, targets, step = masked_inputs(case)
    assert np.abs(targets).max() > 0.1  # patches were pasted
    for f in UP.dropout_keep_fractions(S, B, UP.DEF_SEED, step):
        assert 0.75 <= f <= 0.85
    if UP.CASES[case]["mode"] == "eval":
        man = UP.cpu_manifest()
        params, _ = UP.case_variables(case, man)
        mv = UP.batch_statistics(man, params, patched, UP.DEF_SEED, step)
        r = DF.defender_eval(params, UP.moving_dict(man, mv), patched, None, None, None, masked=(patched, targets),
                             seed=UP.DEF_SEED, step=step)
        pre = np.arctanh(np.clip(r["updates"] / 2.0, -1 + 1e-15, 1 - 1e-15))
        assert (np.abs(pre) > 3).mean() <= 0.10  # the parity is not of saturated values
