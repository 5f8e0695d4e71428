"""GPU: frame recovery — phx_def_recover, PatchAttackDefender.recover and the Recovery mirror of
RecoveryDemo (demo_v2.py:99-169) — against the fp64 restatement in tests/recover_oracle.py.

The victim is D0 (and efficientdet-lite0, for its mean 127 / std 128) at 256^2, the defender's
smallest practical size, with synthetic weights; the frames and U-Net variables are recover_cases.py's.
Every frame goes through mixed-size B = 3 calls whose output offsets are deliberately unaligned (the
byte-store paths) and leave gaps.

Measured on an MI355X (the tests print each figure before asserting it): the
epilogue alone 1.1e-5 ... 3.5e-5 levels from fp64 against 1.22e-4, out_u8 different from the
restatement's at 0-2 near-threshold pixels per frame; end to end 4.0e-5 ... 1.57e-4 levels against
6.1e-3 (D0 constants) / 1.3e-2 (lite0); B = 1 and B = 3 calls bit-equal.
"""
import numpy as np
import pytest
import torch

import recover_cases as RC
import recover_oracle as ro
import serve_oracle as so

pytestmark = pytest.mark.gpu

S = RC.S
U8_FILL, F32_FILL = 0xAB, -777.0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _raw(defender, frames, *, u8=True, f32=True, lead=5, gap=7, B=None, src=True, dims=None):
    """One phx_def_recover call into pre-filled buffers whose frames start at unaligned offsets with
    gaps between and after them -> (out_u8, out_f32 host arrays or None, offsets, recovered dims)."""
    from mladversarialobjectdetection_amd.defender import recovered_dims
    from mladversarialobjectdetection_amd.detector import pack_frames
    p = pack_frames(frames, torch.device("cuda", 0))
    rd = recovered_dims(S, p.dims)
    sizes = rd[:, 0].astype(np.int64) * rd[:, 1] * 3
    offsets = lead + np.concatenate([[0], np.cumsum(sizes + gap)[:-1]]).astype(np.int64)
    total = int(offsets[-1] + sizes[-1] + gap)
    o8 = torch.full((total,), U8_FILL, dtype=torch.uint8, device="cuda") if u8 else None
    o32 = torch.full((total,), F32_FILL, dtype=torch.float32, device="cuda") if f32 else None
    d = p.dims if dims is None else np.ascontiguousarray(dims, np.int32)
    defender.handle.call("phx_def_recover", p.src.data_ptr() if src else None, p.offsets.ctypes.data, d.ctypes.data,
                         len(p.offsets) if B is None else B, defender.params.data_ptr(),
                         o8.data_ptr() if u8 else None, o32.data_ptr() if f32 else None, offsets.ctypes.data, _stream())
    torch.cuda.synchronize()
    return (o8.cpu().numpy() if u8 else None), (o32.cpu().numpy() if f32 else None), offsets, rd


def _split(flat, offsets, rd):
    return [flat[o:o + h * w * 3].reshape(h, w, 3) for o, (h, w) in zip(offsets.tolist(), rd.tolist())]


def _outside(flat, offsets, rd):
    keep = np.ones(flat.shape, bool)
    for o, (h, w) in zip(offsets.tolist(), rd.tolist()):
        keep[o:o + h * w * 3] = False
    return flat[keep]


@pytest.fixture(scope="module", params=["d0", "lite"])
def rig(request):
    """The detector, the defender with recover_cases' variables, and what two B = 3 recovery calls
    over the six frames wrote, with the canvas and `updates` each call left in the workspace."""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    from mladversarialobjectdetection_amd.detector import Detector
    fam = request.param
    model, consts = RC.MODELS[fam]
    det = Detector(params={"image_size": S, "nms_configs": {"score_thresh": 0.5}}, model=model, max_batch=3,
                   rng_seed=5, person_bias=4.0)
    victim = det.driver.model
    p, mv = RC.variables()
    defender = PatchAttackDefender(victim, initial_weights=p, seed=9)
    assert defender.manifest["n_params"] == p.size
    defender.handle.call("phx_def_moving", None, mv.ctypes.data, None)
    frames = RC.frames()
    out = []
    raw = []
    for k in (0, 3):
        o8, o32, offsets, rd = _raw(defender, frames[k:k + 3])
        canvas = defender.debug(_lib.DEF_PATCHED, 3).cpu().numpy()
        upd = defender.debug(_lib.DEF_UPDATES, 3).cpu().numpy()
        np.testing.assert_array_equal(upd, defender.debug_tap("updates", 3).cpu().numpy())
        raw.append((o8, o32, offsets, rd))
        for b, (a8, a32) in enumerate(zip(_split(o8, offsets, rd), _split(o32, offsets, rd))):
            out.append(dict(u8=a8, f32=a32, canvas=canvas[b], upd=upd[b]))
    return dict(fam=fam, consts=RC.mean_std(consts), det=det, victim=victim, defender=defender, frames=frames, out=out,
                raw=raw, params=p, moving=mv)


def test_epilogue_matches_fp64_over_the_librarys_canvas(rig):
    """Steps 2-6 alone: the restated epilogue in fp64 over the library's own canvas and `updates`
    (phx_def_debug after the call).  out_f32 within EPS = 8 * 2^-24 * 256 levels (one rounding per
    product and sum of the two passes and the denormalise, at magnitude <= 256); out_u8 exactly
    trunc(clip(out_f32)) of the same call, and different from the restatement's uint8 only where the
    fp64 value is within EPS of a threshold of the cast."""
    mean, std = rig["consts"]
    for fr, got in zip(rig["frames"], rig["out"]):
        h, w, _ = fr.shape
        ref = ro.epilogue(got["canvas"], got["upd"], h, w, S, mean, std)
        assert got["f32"].shape == ref.shape == ro.dims(h, w, S) + (3,)
        err = np.abs(got["f32"].astype(np.float64) - ref).max()
        np.testing.assert_array_equal(got["u8"], ro.to_uint8(got["f32"]))
        share, ndiff = RC.check_uint8(got["u8"], ref, identity=ro.side(h, w, S) == S)
        clipped = ((ref <= 0) | (ref >= 255)).mean()
        print(f"{rig['fam']} {h}x{w} -> {ref.shape[0]}x{ref.shape[1]}: max |out_f32 - fp64| {err:.3e} (eps {ro.EPS:.3e}), "
              f"near-threshold share {share:.4%}, uint8 differs at {ndiff} px, [0, 255] clip bites at {clipped:.3%}")
        assert err <= ro.EPS, (fr.shape, err)
    if rig["fam"] == "lite":  # only these constants reach the [0, 255] clip
        assert any(((ro.epilogue(g["canvas"], g["upd"], f.shape[0], f.shape[1], S, mean, std) >= 255).any())
                   for f, g in zip(rig["frames"], rig["out"]))


def test_recover_matches_fp64_end_to_end(rig):
    """The whole chain against serve_oracle.preprocess64 -> oracle U-Net (fp64, inference mode) ->
    the restated epilogue: out_f32 within (1e-4 + preprocess bound) * max(stddev) + EPS, 1e-4 being
    test_unet_step_matches_oracle's bound on `updates` and the preprocess bound
    test_gpu_serve._check_preprocess's."""
    mean, std = rig["consts"]
    ref = RC.reference(RC.MODELS[rig["fam"]][1])
    for fr, got, (img, x, u) in zip(rig["frames"], rig["out"], ref):
        h, w, _ = fr.shape
        ty, tx = so.taps(h, w, S)
        pre = (ty + tx + 8) * 2.0 ** -24 * 2.65
        bound = (1e-4 + pre) * max(std) + ro.EPS
        e_pre = np.abs(got["canvas"] - x).max()
        e_upd = np.abs(got["upd"] - u).max()
        err = np.abs(got["f32"].astype(np.float64) - img).max()
        print(f"{rig['fam']} {h}x{w}: max |d canvas| {e_pre:.3e} (bound {pre:.3e}), |d updates| {e_upd:.3e}, "
              f"|out_f32 - fp64| {err:.3e} levels (bound {bound:.3e})")
        assert e_pre <= pre
        assert err <= bound, (fr.shape, err, bound)


def test_shapes_gaps_and_batch_independence(rig):
    """Outputs have phx_recover_dims' sizes (50x211 -> 50x210, 90x120 -> 90x119), the bytes before,
    between and after the frames keep their fill, a call with one output null writes the same values,
    and a mixed-size B = 3 call agrees with three B = 1 calls within the end-to-end bound."""
    d, frames = rig["defender"], rig["frames"]
    assert [g["u8"].shape[:2] for g in rig["out"]] == [(50, 210), (90, 119), (128, 128), (300, 200), (256, 256), (96, 160)]
    for o8, o32, offsets, rd in rig["raw"]:
        assert (_outside(o8, offsets, rd) == U8_FILL).all() and _outside(o8, offsets, rd).size >= 5 + 3 * 7
        assert (_outside(o32, offsets, rd) == np.float32(F32_FILL)).all()
    o8, o32, offsets, rd = rig["raw"][0]
    only8, none32, _, _ = _raw(d, frames[:3], f32=False)
    none8, only32, _, _ = _raw(d, frames[:3], u8=False)
    assert none32 is None and none8 is None
    np.testing.assert_array_equal(only8, o8)
    np.testing.assert_array_equal(only32, o32)
    # other alignments of the output offsets: every lead-in of the dword / 16-byte groups
    for lead in (0, 2, 16):
        a8, a32, off, _ = _raw(d, frames[:3], lead=lead, gap=lead + 1)
        for x, y in zip(_split(a8, off, rd) + _split(a32, off, rd), _split(o8, offsets, rd) + _split(o32, offsets, rd)):
            np.testing.assert_array_equal(x, y)
        assert (_outside(a8, off, rd) == U8_FILL).all() and (_outside(a32, off, rd) == np.float32(F32_FILL)).all()
    mean, std = rig["consts"]
    equal = True
    for b in range(3):
        s8, s32, off1, rd1 = _raw(d, frames[b:b + 1])
        one = _split(s32, off1, rd1)[0]
        h, w, _ = frames[b].shape
        ty, tx = so.taps(h, w, S)
        bound = (1e-4 + (ty + tx + 8) * 2.0 ** -24 * 2.65) * max(std) + ro.EPS
        diff = np.abs(one.astype(np.float64) - rig["out"][b]["f32"]).max()
        equal &= bool(np.array_equal(one, rig["out"][b]["f32"]) and np.array_equal(_split(s8, off1, rd1)[0], rig["out"][b]["u8"]))
        print(f"{rig['fam']} frame {b}: B = 1 vs B = 3 max |d| {diff:.3e} levels (bound {bound:.3e})")
        assert diff <= bound
    print(f"{rig['fam']}: B = 1 and B = 3 results bit-equal: {equal}")


def test_recover_changes_no_state(rig):
    """The variables and moving statistics are bit-identical after a recovery, and a train_step after a
    recovery gives the same loss and gradient as one without it."""
    from mladversarialobjectdetection_amd.defender import PatchAttackDefender
    d = rig["defender"]
    np.testing.assert_array_equal(d.params.cpu().numpy(), rig["params"])
    np.testing.assert_array_equal(d.moving_statistics(), rig["moving"])
    imgs = torch.as_tensor(np.random.default_rng(8).uniform(-1, 1, (2, S, S, 3)).astype(np.float32)).cuda()
    res = []
    for with_recover in (False, True):
        t = PatchAttackDefender(rig["victim"], initial_weights=rig["params"], seed=9)
        t.handle.call("phx_def_moving", None, rig["moving"].ctypes.data, None)
        if with_recover:
            t.recover(rig["frames"][:2])
            np.testing.assert_array_equal(t.moving_statistics(), rig["moving"])
        loss = t.train_step(imgs)["loss"]
        torch.cuda.synchronize()
        res.append((float(loss.item()), t.grad.cpu().numpy().copy(), t.params.cpu().numpy().copy(), t.moving_statistics()))
    assert np.isfinite(res[0][0]) and res[0][0] == res[1][0]
    for a, b in zip(res[0][1:], res[1][1:]):
        assert a.tobytes() == b.tobytes()


def test_refusals_launch_nothing(rig):
    """Every argument is checked on the host: the message names the argument, the code is PHX_EINVAL
    (PHX_ECAP for B > max_batch), and neither the output buffers nor the workspace were written."""
    from mladversarialobjectdetection_amd import _lib
    from mladversarialobjectdetection_amd._lib import PhxError
    d, frames = rig["defender"], rig["frames"]
    _raw(d, frames[3:6])  # (the state the fixture left)
    before = d.debug(_lib.DEF_PATCHED, 3).cpu().numpy()
    cases = [(dict(src=False), r"\(-1\).*src is null"),
             (dict(u8=False, f32=False), r"\(-1\).*out_u8 and out_f32 are both null"),
             (dict(B=0), r"\(-1\).*B = 0"),
             (dict(B=4), r"\(-4\).*B = 4 exceeds max_batch = 3"),
             (dict(dims=[[0, 211], [90, 120], [128, 128]]), r"\(-1\).*dims\[0\] = 0x211: h and w must be >= 1")]
    for kw, match in cases:
        with pytest.raises(PhxError, match=match):
            _raw(d, frames[:3], **kw)
    # a refused call with outputs: they keep their fill
    from mladversarialobjectdetection_amd.detector import pack_frames
    p = pack_frames(frames[:3], torch.device("cuda", 0))
    o8 = torch.full((200000,), U8_FILL, dtype=torch.uint8, device="cuda")
    offs = np.array([0, 60000, 120000], np.int64)
    bad = p.dims.copy()
    bad[2] = (1, 1000)  # the scaled height int(1 * 0.256) is 0
    rc = d.handle.lib.phx_def_recover(d.handle.h, p.src.data_ptr(), p.offsets.ctypes.data, bad.ctypes.data, 3,
                                      d.params.data_ptr(), o8.data_ptr(), None, offs.ctypes.data, _stream())
    assert rc == -1 and b"dims[2] = 1x1000" in d.handle.lib.phx_def_last_error(d.handle.h)
    torch.cuda.synchronize()
    assert bool((o8 == U8_FILL).all())
    np.testing.assert_array_equal(d.debug(_lib.DEF_PATCHED, 3).cpu().numpy(), before)


def test_recovery_run(rig, tmp_path):
    """Recovery.run equals the manual composition of AdversarialPatch.add_adv_to_img, recover and
    Detector.infer; recover's device PackedFrames through infer_batch equal the host round trip; a
    U-Net loaded from an antipatch.h5 written by save_weights recovers the same bytes."""
    from mladversarialobjectdetection_amd.adv_patch import AdversarialPatch
    from mladversarialobjectdetection_amd.detector import filter_by_thresh
    from mladversarialobjectdetection_amd.recovery import Recovery, unpack_frames
    det, d = rig["det"], rig["defender"]
    d.save_weights(str(tmp_path / "w"))
    patch = AdversarialPatch(scale=0.4, seed=3, ctx=rig["victim"].ctx)
    rec = Recovery(str(tmp_path / "w" / "antipatch.h5"), patch, det, min_score_thresh=0.5)
    frame = np.random.default_rng(12).integers(0, 256, (200, 300, 3), dtype=np.uint8)
    bb = [(30.0, 50.0, 170.0, 250.0)]
    step = patch._calls
    got_frame, got_bb, got_sc, detected = rec.run(frame, bb, 0.0, 100.0)
    # the manual composition
    mal = patch.add_adv_to_img(frame, bb, step=step)
    assert (mal != frame).any()
    direct = d.recover([mal])[0]
    loaded = rec.recover([mal])
    assert loaded.src.cpu().numpy().tobytes() == direct.src.cpu().numpy().tobytes()  # antipatch.h5 round trip
    recovered = unpack_frames(direct)[0]
    assert recovered.dtype == np.uint8 and recovered.shape == ro.dims(200, 300, S) + (3,)
    np.testing.assert_array_equal(got_frame, recovered)
    host = det.infer(recovered)  # the host round trip
    assert det.infer_batch(direct) == [host]
    wb, ws = filter_by_thresh(*host, 0.5)
    want_sc = max(ws) * 100.0 if ws else 0.0
    print(f"{rig['fam']} Recovery.run: {len(wb)} person box(es) on the recovered frame, best score {want_sc:.1f} %")
    assert got_bb == wb and got_sc == want_sc
    assert detected == (want_sc - 0.0 > 10.0)
    assert rec.run(frame, bb, 0.0, 40.0)[3] is False  # the score before the attack was below the threshold
    # serve: the float images of the same call
    fl = rec.serve([mal])[0]
    assert fl.dtype == np.float32 and fl.shape == recovered.shape
    np.testing.assert_array_equal(ro.to_uint8(fl), recovered)
