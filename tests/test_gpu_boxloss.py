"""The box-regression attack term (phx_set_box_loss: the reference's InverseDIOULoss) end to end on the GPU against
tests/idiou_oracle.py's fp64 step: D0 at 128^2, B = 2, injected boxes and the fixture weights of
tests/test_gpu_parity.py's step test.

Bounds (those of the 128^2 step test, the added path runs the same kinds of kernels): loss rel <= 1e-5, d patch
cosine >= 0.99999 and ||d - d_ref|| / ||d_ref|| <= 1e-3.

Weights, chosen on the CPU from the fp64 oracle so that the box term's gradient is within a factor 10 of the score
loss's (||g(0)|| is the norm of d patch without the term, ||g_box|| of the unweighted term's):
  bn=local   ||g(0)|| = 3.139e-2, ||g_box|| = 4.686e-1 -> w = 0.0625: ||w g_box|| = 2.93e-2
  bn=frozen  ||g(0)|| = 3.131e-2, ||g_box|| = 6.519e-5 -> w = 64:     ||w g_box|| = 4.17e-3
(the tests assert the factor-10 rule on the oracle's norms again).

Stable argmax: with these inputs (images seed 1, patch seed 7, step 3) every (image, gt)'s best diou is at least 1.8e-2
above its runner-up in the fp64 oracle, bn=local (gaps 9.2e-2, 6.3e-2, 1.9e-2), and asserted below to exceed KERNEL_BOUND for every pair; the
kernel's own bound on one diou at coordinates up to 256 px and a kept box side of 10 px or more is 2e-5 (DESIGN.md
section 22)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

S = 128
W_LOCAL = 0.0625
W_FROZEN = 64.0
KERNEL_BOUND = 1e-4  # five times the 2e-5 derived in DESIGN.md section 22: a stricter margin


def _images(B=2, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, (B, S, S, 3)).astype(np.float32)


def _boxes():
    return [np.array([[10, 20, 90, 70]], np.float32),
            np.array([[5, 5, 120, 60], [30, 40, 100, 110]], np.float32)]


def _victim(bn_mode="local", dtype="f32"):
    from mladversarialobjectdetection_amd.attacker import EfficientDetVictim
    return EfficientDetVictim("efficientdet-d0", "synthetic", seed=0, image_size=S, max_batch=4, rng_seed=5,
                              bn_mode=bn_mode, dtype=dtype)


@pytest.fixture(scope="module")
def victim():
    return _victim()


@pytest.fixture(scope="module")
def victim_frozen():
    return _victim("frozen")


@pytest.fixture(scope="module")
def wdict(victim):
    from mladversarialobjectdetection_amd import weights as W
    return W.unpack(victim.manifest, victim.blob)


def _patch(seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(640, 640, 3)).astype(np.float32)


def _oracle(wdict, **kw):
    import idiou_oracle as IO
    return IO.attack_step(wdict, _images(), _patch(), np.float32(0.4), _boxes(), seed=5, step=3, image_size=S, **kw)


@pytest.fixture(scope="module")
def ref_local(wdict):
    return _oracle(wdict)


@pytest.fixture(scope="module")
def ref_frozen(wdict):
    return _oracle(wdict, bn_frozen=True)


@pytest.fixture(scope="module")
def ref_eval(wdict):
    return _oracle(wdict, training=False)


def _attacker(victim, box_loss="inv_diou", weight=W_LOCAL):
    from mladversarialobjectdetection_amd.attacker import PatchAttacker
    att = PatchAttacker(victim, seed=7, box_loss=box_loss, box_loss_weight=weight)
    att.cur_step = 3
    return att


def _step(victim, box_loss="inv_diou", weight=W_LOCAL, training=True):
    """One step; returns (grad fp64 copy, metric row copy, attacker)."""
    att = _attacker(victim, box_loss, weight)
    att.call(torch.as_tensor(_images()).cuda(), boxes=_boxes(), training=training)
    torch.cuda.synchronize()
    return att.grad.cpu().numpy().copy(), att.metrics_buf.cpu().numpy().copy(), att


def _debug(victim, B=2):
    per = torch.empty(B, device="cuda")
    gmax = torch.empty(B, 100, device="cuda")
    ganc = torch.empty(B, 100, dtype=torch.int32, device="cuda")
    gnt = torch.empty(B, 100, dtype=torch.int32, device="cuda")
    victim.ctx.call("phx_debug_last_box_loss", per.data_ptr(), gmax.data_ptr(), ganc.data_ptr(), gnt.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return per.cpu().numpy(), gmax.cpu().numpy(), ganc.cpu().numpy(), gnt.cpu().numpy()


def _check_parity(g, met, ref, w):
    from mladversarialobjectdetection_amd import _lib
    loss = ref["loss0"] + w * ref["box"]
    rg = ref["grad0"] + w * ref["grad_box"]
    gp, rp = g[:-1].astype(np.float64), rg[:-1]
    cos = gp @ rp / (np.linalg.norm(gp) * np.linalg.norm(rp))
    rel = np.linalg.norm(gp - rp) / np.linalg.norm(rp)
    print(f"loss {met[_lib.M_LOSS]!r} ref {loss!r} rel {abs(met[_lib.M_LOSS] - loss) / abs(loss):.3g}; "
          f"d patch cosine {cos:.9f} rel {rel:.3g}; d scale {g[-1]!r} ref {rg[-1]!r}")
    assert abs(met[_lib.M_LOSS] - loss) <= 1e-5 * abs(loss)
    assert cos >= 0.99999, cos
    assert rel <= 1e-3, rel
    assert abs(g[-1] - rg[-1]) <= 1e-5 * max(1.0, abs(rg[-1]))


def _factor10(ref, w):
    n0, nb = np.linalg.norm(ref["grad0"][:-1]), w * np.linalg.norm(ref["grad_box"][:-1])
    print(f"w {w}: ||g(0)|| {n0:.4g}, ||w g_box|| {nb:.4g}")
    assert n0 / 10 <= nb <= n0 * 10, (n0, nb)


def test_parity_local(victim, ref_local):
    """bn=local: loss and gradient with the term at w = 0.0625 against the fp64 oracle."""
    _factor10(ref_local, W_LOCAL)
    g, met, _ = _step(victim)
    _check_parity(g, met, ref_local, W_LOCAL)


def test_parity_frozen(victim_frozen, ref_frozen):
    """bn=frozen: one parity case (w = 64: the term's gradient through inference BN is small here)."""
    _factor10(ref_frozen, W_FROZEN)
    g, met, _ = _step(victim_frozen, weight=W_FROZEN)
    _check_parity(g, met, ref_frozen, W_FROZEN)


def test_isolation_box_term_alone(victim, ref_local):
    """g(w) - g(0) is the box term's gradient alone: its cosine against the oracle's w g_box meets the step's bound."""
    _factor10(ref_local, W_LOCAL)
    gw, _, _ = _step(victim)
    g0, _, _ = _step(victim, box_loss=None)
    d = (gw.astype(np.float64) - g0.astype(np.float64))[:-1]
    r = W_LOCAL * ref_local["grad_box"][:-1]
    cos = d @ r / (np.linalg.norm(d) * np.linalg.norm(r))
    rel = np.linalg.norm(d - r) / np.linalg.norm(r)
    print(f"box term alone: cosine {cos:.9f} rel {rel:.3g}; ||g(w) - g(0)|| {np.linalg.norm(d):.4g}, ||w g_box|| "
          f"{np.linalg.norm(r):.4g}")
    assert cos >= 0.99999, cos
    # and without the term the step is the oracle's plain step
    r0 = ref_local["grad0"][:-1]
    c0 = g0[:-1].astype(np.float64) @ r0 / (np.linalg.norm(g0[:-1].astype(np.float64)) * np.linalg.norm(r0))
    assert c0 >= 0.99999, c0


def test_stable_argmax_and_values(victim, ref_local):
    """Every (image, gt)'s best diou beats its runner-up by more than the kernel bound in the fp64 oracle (asserted
    for every pair); the device's anchors then equal the oracle's exactly, with one winner each, and the per-image
    values and the box_loss metric follow."""
    _, met, att = _step(victim)
    per, gmax, ganc, gnt = _debug(victim)
    boxes = _boxes()
    npairs = 0
    for b in range(2):
        pairs, kept = ref_local["pairs"][b], ref_local["kept"][b]
        assert pairs.shape == (len(boxes[b]), len(kept)) and len(kept) >= 2
        for g in range(pairs.shape[0]):
            s = np.sort(pairs[g])
            assert s[-1] - s[-2] > KERNEL_BOUND, (b, g, s[-1], s[-2])
            assert ganc[b, g] == kept[np.argmax(pairs[g])], (b, g, ganc[b, g], kept[np.argmax(pairs[g])])
            assert gnt[b, g] == 1
            # the decoded boxes carry the detector's fp32 error (test_gpu_parity.py bounds it at 5e-4 of box size +
            # anchor size); a diou moves by at most ~4 / side per pixel: far inside the margin, loosely 1e-3 here
            assert abs(gmax[b, g] - s[-1]) <= 1e-3, (b, g, gmax[b, g], s[-1])
            npairs += 1
        assert (ganc[b, len(boxes[b]):] == -1).all() and (gnt[b, len(boxes[b]):] == 0).all()
        assert (gmax[b, len(boxes[b]):] == 0).all()
    assert npairs == 3
    # per image: the fp32 sum of the maxima in gt order + 1e-7, from the device's own maxima
    for b in range(2):
        v = np.float32(0)
        for g in range(len(boxes[b])):
            v = np.float32(v + gmax[b, g])
        assert per[b] == np.float32(v + np.float32(1e-7))
    m = att.step_metrics()
    assert m["box_loss"] == float(np.float32(per[0] + per[1]))
    # the budget the loss check leaves the term: 1e-5 of the loss, over w
    from mladversarialobjectdetection_amd import _lib
    assert abs(m["box_loss"] - ref_local["box"]) <= 1e-5 * abs(met[_lib.M_LOSS]) / W_LOCAL
    assert "box_loss" not in _attacker(victim, box_loss=None).METRICS


def test_default_path_is_byte_equal_and_same_size(victim):
    """kind NONE — never set, set explicitly, or the term set and then reset — gives phx_step_grad's bytes of a fresh
    context and its phx_workspace_bytes."""
    fresh = _victim()
    gf, mf, _ = _step(fresh, box_loss=None)
    wf = fresh.ctx.workspace_bytes(2)
    # on a context that ran the term: reset through the attacker, and explicitly
    _step(victim)
    won = victim.ctx.workspace_bytes(2)
    g1, m1, _ = _step(victim, box_loss=None)
    assert victim.ctx.get_box_loss()[0] is None
    assert victim.ctx.workspace_bytes(2) == wf
    assert won > wf  # (the term's buffers and the larger gradient arena are the term's alone)
    victim.ctx.set_box_loss("inv_diou", 3.0)
    victim.ctx.set_box_loss(None, 3.0)
    g2, m2, _ = _step(victim, box_loss=None, weight=3.0)
    assert gf.tobytes() == g1.tobytes() == g2.tobytes()
    assert mf.tobytes() == m1.tobytes() == m2.tobytes()
    assert victim.ctx.workspace_bytes(2) == wf


def test_abi_and_setter(victim):
    from mladversarialobjectdetection_amd import _lib
    ctx = victim.ctx
    assert _lib.load().phx_abi_version() == _lib.ABI_VERSION == 4
    ctx.set_box_loss(None)
    for kind, w in ((7, 1.0), (-1, 1.0), (_lib.BOX_LOSS_INV_DIOU, float("nan")), (_lib.BOX_LOSS_INV_DIOU, float("inf"))):
        with pytest.raises(_lib.PhxError, match=r"phx_set_box_loss failed \(-1\): box_loss"):
            ctx.call("phx_set_box_loss", kind, w)
    assert ctx.get_box_loss() == (None, 1.0)
    bf = _victim(dtype="bf16")
    with pytest.raises(_lib.PhxError, match=r"\(-1\).*PHX_DTYPE_F32"):
        bf.ctx.set_box_loss("inv_diou", 1.0)
    bf.ctx.set_box_loss(None, 1.0)  # (the default stays settable)
    # no step with the term has run on a fresh context
    with pytest.raises(_lib.PhxError, match=r"phx_debug_last_box_loss failed \(-3\)"):
        _debug(_victim())
    # PHX_ESTATE while a phx_set_next batch (or its prefetched first pass) is pending
    nxt = torch.as_tensor(_images(seed=2)).cuda()
    ctx.call("phx_set_next", nxt.data_ptr(), 2, 0)
    try:
        with pytest.raises(_lib.PhxError, match=r"phx_set_box_loss failed \(-3\)"):
            ctx.set_box_loss("inv_diou", 1.0)
    finally:
        ctx.call("phx_set_next", None, 0, 0)
    ctx.set_box_loss("inv_diou", 0.5)
    assert ctx.get_box_loss() == ("inv_diou", 0.5)
    ctx.set_box_loss(None)


def test_eval_step_includes_the_term(ref_eval):
    """phx_eval_step (test_step: inference BN, no gradient): PHX_M_LOSS includes w * the term.  On a fresh context:
    the shared one's training steps have moved its moving statistics away from the oracle's."""
    from mladversarialobjectdetection_amd import _lib
    victim = _victim()
    _, met, att = _step(victim, training=False)
    loss = ref_eval["loss0"] + W_LOCAL * ref_eval["box"]
    print(f"eval loss {met[_lib.M_LOSS]!r} ref {loss!r}; box_loss {att.step_metrics()['box_loss']!r} ref {ref_eval['box']!r}")
    assert abs(met[_lib.M_LOSS] - loss) <= 1e-5 * abs(loss)
    _, met0, _ = _step(victim, box_loss=None, training=False)
    assert abs((met[_lib.M_LOSS] - met0[_lib.M_LOSS]) - W_LOCAL * ref_eval["box"]) <= 2e-5 * abs(loss)
    assert abs(att.step_metrics()["box_loss"] - ref_eval["box"]) <= 1e-5 * abs(loss) / W_LOCAL


def test_train_and_test_step_metric_dicts_carry_box_loss(victim):
    att = _attacker(victim)
    imgs = torch.as_tensor(_images()).cuda()
    m = att.train_step(imgs, boxes=_boxes())
    assert np.isfinite(dict(m)["box_loss"]) and dict(m)["box_loss"] != 0.0 and "loss" in dict(m)
    tm, _ = att.test_step(imgs, boxes=_boxes())
    assert np.isfinite(tm["box_loss"]) and tm["box_loss"] != 0.0  # (a diou, and so the value, may be negative)
    plain = _attacker(victim, box_loss=None)
    tm0, _ = plain.test_step(imgs, boxes=_boxes())
    assert "box_loss" not in tm0


def test_determinism_and_stream_order(victim, monkeypatch):
    """Two steps with the term give the same bytes, with the concurrent first pass on and off."""
    outs = []
    for conc in ("1", "1", "0", "0"):
        monkeypatch.setenv("PHX_CONC", conc)
        g, met, _ = _step(victim)
        outs.append((g.tobytes(), met.tobytes(), _debug(victim)[2].tobytes()))
    assert outs[0] == outs[1] == outs[2] == outs[3]
