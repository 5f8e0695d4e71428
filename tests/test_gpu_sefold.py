"""GPU: the squeeze-excite backward whose input gradient is formed on load by the depthwise dgrad
(PHX_SEFOLD) against the path that stores it (PHX_SEFOLD=0) and the fp64 oracle.

One D0 step at 128^2 with 2 images (test_step_grad_matches_oracle's inputs: case A of tests/layer_parity.py)
under each setting, each in a victim of its own (the knob is read when the executor is planned):

  * [d patch | d scale] of both against the fp64 oracle step: the new path's relative deviation may exceed
    the storing path's own, measured here, by at most a quarter.  Both values are printed (DESIGN.md
    section 4 records them).  The new path performs the same operations on the same operands in the same
    order, so the two gradients are also required to be equal bit for bit.
  * the gradient tap of a depthwise BN's output, which the new path never stores and materialises for
    the tap as fma(dy, s, dpool / HW): under both settings it lies within the layer sweep's bound
    K_BWD * max(e32, f) of the oracle's gradient at that layer (tests/layer_parity.py), e32 the fp32 oracle
    run's own deviation there and f its median over the layers; and the two taps are equal bit for bit.
  * the executor's workspace is the same size under both settings (dpool is kept in the gradient slot of
    the tensor that is no longer written).
  * each step did take its path: the PHX_CKSUM names of such an SE are its dpool, those of the storing
    path its input's gradient.
"""
import numpy as np
import pytest
import torch

import layer_parity as LP

pytestmark = pytest.mark.gpu

# depthwise BNs (the second BN of an MBConv block with an expand conv): the last block's, whose incoming
# gradient is the same under both settings up to the block's own SE, and one in the middle of the
# backbone, downstream of ten other folded blocks in the reverse sweep
TAPS = ["efficientnet-b0/blocks_15/tpu_batch_normalization_1", "efficientnet-b0/blocks_5/tpu_batch_normalization_1"]
N_SE = 16  # MBConv blocks of EfficientNet-b0, each with one SE


@pytest.fixture(scope="module")
def inputs():
    return LP.case_inputs("A")


def _step(inputs, sefold, monkeypatch):
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim, PatchAttacker
    S, B, imgs, boxes, _ = inputs
    if sefold is None:
        monkeypatch.delenv("PHX_SEFOLD", raising=False)
    else:
        monkeypatch.setenv("PHX_SEFOLD", sefold)
    monkeypatch.setenv("PHX_CKSUM", "1")
    v = EfficientDetVictim(LP.MODEL, "synthetic", seed=0, image_size=S, max_batch=B, rng_seed=LP.RNG_SEED)
    att = PatchAttacker(v, seed=LP.PATCH_SEED)
    att.cur_step = LP.STEP
    att.call(torch.as_tensor(imgs).cuda(), boxes=boxes)
    torch.cuda.synchronize()
    return v, att


@pytest.fixture(scope="module")
def runs(inputs):
    from mladversarialobjectdetection_amd import weights as W
    S, B, imgs, boxes, _ = inputs
    mp = pytest.MonkeyPatch()
    try:
        out = {}
        for key, val in (("fold", None), ("apply", "0")):
            v, att = _step(inputs, val, mp)
            shapes = None
            out[key] = dict(v=v, grad=att.grad.cpu().numpy().astype(np.float64), names=[n for n, _ in v.ctx.checksums()],
                            ws=v.ctx.workspace_bytes(B), patch=att.patch.cpu().numpy())
        v = out["fold"]["v"]
        wd = W.unpack(v.manifest, v.blob.copy())
        torch.set_num_threads(16)
        ref = LP.reference(wd, imgs, out["fold"]["patch"], boxes, S)
        for key in out:
            fwd, bwd = LP.gpu_taps(out[key]["v"], {n: ref.fwd[n].shape for n in TAPS})
            out[key]["taps"] = bwd
        out["ref"] = ref
        return out
    finally:
        mp.undo()


def test_each_setting_takes_its_path(runs):
    q = [n for n in runs["fold"]["names"] if n.startswith("b ") and n.endswith(" dpool")]
    assert len(q) == N_SE, q
    assert not [n for n in runs["apply"]["names"] if n.endswith(" dpool")]
    # the storing path checksums the SE input's gradient (" se... d0"), the other must not: nothing is there
    se_d0 = lambda names: [n for n in names if n.startswith("b ") and "/se" in n and n.endswith(" d0")]
    assert len(se_d0(runs["apply"]["names"])) == N_SE and not se_d0(runs["fold"]["names"])


def test_workspace_is_unchanged(runs):
    assert runs["fold"]["ws"] == runs["apply"]["ws"]


def test_step_gradient_against_the_oracle(runs):
    """measured on an MI355X: see the printed line"""
    r = runs["ref"].r64["grad"]
    rel = {k: float(np.linalg.norm(runs[k]["grad"] - r) / np.linalg.norm(r)) for k in ("fold", "apply")}
    print(f"[d patch | d scale] rel. deviation from the fp64 oracle: folded {rel['fold']:.4e}, apply pass {rel['apply']:.4e}")
    assert np.isfinite(runs["fold"]["grad"]).all()
    assert rel["fold"] <= 1.25 * rel["apply"], rel
    assert np.array_equal(runs["fold"]["grad"], runs["apply"]["grad"])


@pytest.mark.parametrize("name", TAPS)
def test_depthwise_bn_gradient_tap(runs, name):
    ref = runs["ref"]
    floor = float(np.median(list(ref.e32_bwd.values())))
    bound = LP.K_BWD * max(ref.e32_bwd[name], floor)
    for key in ("fold", "apply"):
        t = runs[key]["taps"][name]
        assert not isinstance(t, LP.Refused), (key, t)
        e = LP._rel(np.asarray(t, np.float64), ref.bwd[name])
        print(f"{name} {key}: e_dev {e:.3e} bound {bound:.3e}")
        assert e <= bound, (key, e, bound)
    assert np.array_equal(runs["fold"]["taps"][name], runs["apply"]["taps"][name])
