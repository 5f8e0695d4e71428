"""GPU: phx_serve_preprocess where a canvas row has several column blocks.

k_serve_pre gives a workgroup 1024 consecutive floats of a canvas row (blockIdx.x) and stages source pixels in
chunks of 1024.  At the sizes tests/test_gpu_serve.py runs (S = 128: 384 floats) there is one block; every
production size from S = 344 up has more, and with block index >= 1 come a pixel whose channels two blocks
share (pixel 341), blocks that are all padding (p_lo > p_hi), staging that starts inside a source row (x_lo > 0,
a lead of 1 to 3 bytes that changes per row) and chunk loops that start at x_lo.  The frames below are chosen
for those paths; `_geometry` restates which one a frame reaches from the oracle's resize matrices and the
tests assert it, so the table cannot drift off its edges.

Reference, bound and side checks are tests/test_gpu_serve.py's: serve_oracle.preprocess64 (fp64), the derived
(ty + tx + 8) * 2^-24 * 2.65 per frame, padding exactly 0, scales equal to the fp32
restatement, the canvas prefilled with 7.0 so that an unwritten element shows.

Measured on an MI355X (each figure is printed before it is asserted; DESIGN.md section 15, "Preprocess at several
column blocks", lists them all): max |d| 1.1e-7 ... 4.0e-7 against bounds of 1.6e-6 ... 8.7e-6, the closest the 7x5
upscale at 0.21 of its bound; the module takes 6 s, most of it the fp64 references on the host.  The 1080p frame's
reference alone takes 2.9 s, so it appears in one test only.
"""
import numpy as np
import pytest
import torch

import serve_oracle as so
from oracle import eot

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mean_std():
    from mladversarialobjectdetection_amd.attacker import MEAN_RGB, STDDEV_RGB
    return MEAN_RGB["efficientdet"], STDDEV_RGB["efficientdet"]


def _frames(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


_CTX = {}


def _ctx(S, max_batch=12):
    """Bare contexts (the preprocess needs no weights), one per size for the module."""
    from mladversarialobjectdetection_amd import _lib
    if S not in _CTX:
        _CTX[S] = _lib.Context("efficientdet-d0", image_size=S, max_batch=max_batch)
    return _CTX[S]


def _run(S, frames, offsets=None, fill=0, total=None):
    """phx_serve_preprocess over frames packed at `offsets` (default: back to back) in a buffer of `total`
    bytes holding `fill` wherever no frame lies -> (images, scales)."""
    sizes = [int(f.size) for f in frames]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    offsets = np.ascontiguousarray(offsets, np.int64)
    total = int(max(o + n for o, n in zip(offsets, sizes))) if total is None else total
    flat = np.full(total, fill, np.uint8)
    for o, fr in zip(offsets, frames):
        flat[o:o + fr.size] = fr.reshape(-1)
    dims = np.ascontiguousarray([f.shape[:2] for f in frames], np.int32).reshape(-1, 2)
    src = torch.as_tensor(flat).cuda()
    assert src.data_ptr() % 4 == 0
    B = len(frames)
    images = torch.full((B, S, S, 3), 7.0, device="cuda")
    scales = torch.empty(B, device="cuda")
    _ctx(S).call("phx_serve_preprocess", src.data_ptr(), offsets.ctypes.data, dims.ctypes.data, B, images.data_ptr(),
                 scales.data_ptr(), _stream())
    torch.cuda.synchronize()
    return images.cpu().numpy(), scales.cpu().numpy()


def _check(S, images, scales, frames):
    """test_gpu_serve._check_preprocess at any S."""
    mean, std = _mean_std()
    worst = 0.0
    for b, fr in enumerate(frames):
        h, w, _ = fr.shape
        sh, sw, _ = so.dims(h, w, S)
        ref = so.preprocess64(fr, S, mean, std)
        ty, tx = so.taps(h, w, S)
        bound = (ty + tx + 8) * 2.0 ** -24 * 2.65
        err = np.abs(images[b].astype(np.float64) - ref).max()
        print(f"preprocess S={S} {h}x{w} -> {sh}x{sw}: taps ({ty}, {tx}) max |d| {err:.3e} bound {bound:.3e}")
        assert np.abs(ref).max() <= 2.65
        assert err <= bound, (S, fr.shape, err, bound)
        worst = max(worst, err / bound)
        assert np.array_equal(images[b, sh:], np.zeros_like(images[b, sh:]))
        assert np.array_equal(images[b, :, sw:], np.zeros_like(images[b, :, sw:]))
        assert scales[b] == so.scale_to_original(h, w, S)
    return worst


def _geometry(h, w, S, offset=0):
    """Per column block of k_serve_pre: None for a block that is all padding, else dict(p_lo, p_hi, x_lo, x_hi,
    chunks, lead) from the non-zeros of the oracle's horizontal resize matrix; lead = the staging offset mod 4
    on source rows 0, 1, 2 for a frame at byte `offset` of a dword-aligned buffer."""
    sh, sw, _ = so.dims(h, w, S)
    Wx = eot.resize_matrix(sw, w)
    out = []
    for bx in range((S * 3 + 1023) // 1024):
        p_lo, p_hi = bx * 1024 // 3, min(sw - 1, (bx * 1024 + 1023) // 3)
        if p_lo > p_hi:
            out.append(None)
            continue
        x_lo = int(np.flatnonzero(Wx[p_lo])[0])
        x_hi = int(np.flatnonzero(Wx[p_hi])[-1]) + 1
        out.append(dict(p_lo=p_lo, p_hi=p_hi, x_lo=x_lo, x_hi=x_hi, chunks=-(-(x_hi - x_lo) // 1024),
                        lead=[(offset + (y * w + x_lo) * 3) % 4 for y in range(min(h, 3))]))
    return out


# S = 344: two blocks, the second of 8 floats (2 lanes) holding channels 1 and 2 of pixel 341 and pixels 342, 343
S344 = [(344, 344), (344, 342), (900, 300), (41, 3501), (40, 3500), (100, 1375), (343, 1029), (7, 5), (1, 1)]


def test_table_reaches_the_block_paths():
    """Every frame reaches the path it was chosen for (host arithmetic on the oracle's matrices)."""
    g = {s: _geometry(*s, 344) for s in S344}
    assert all(len(v) == 2 for v in g.values())
    assert g[(344, 342)][1]["p_lo"] == g[(344, 342)][1]["p_hi"] == 341  # block 1 owns two channels of one pixel
    assert g[(344, 342)][1]["lead"] == [3, 1, 3]
    assert g[(900, 300)][1] is None and so.dims(900, 300, 344)[:2] == (344, 114)  # padding only
    a = g[(41, 3501)]
    assert (a[0]["x_lo"], a[0]["chunks"]) == (0, 4) and a[1]["x_lo"] == 3465 and so.taps(41, 3501, 344) == (21, 21)
    assert a[0]["lead"] == [0, 3, 2] and a[1]["lead"] == [3, 2, 1]
    assert [so.dims(*s, 344)[0] % 4 for s in ((40, 3500), (100, 1375), (343, 1029))] == [3, 1, 2]
    assert g[(100, 1375)][0]["chunks"] == 2
    b = g[(343, 1029)]
    assert b[0]["chunks"] == 2 and b[0]["x_hi"] - b[0]["x_lo"] - 1024 == 1  # the second chunk covers one source pixel
    assert b[0]["lead"] == [0, 3, 2] and b[1]["lead"] == [1, 0, 3]
    assert so.dims(7, 5, 344)[:2] == (344, 245)
    c = _geometry(61, 2051, 684)
    assert len(c) == 3 and [x["chunks"] for x in c[:2]] == [2, 2] and 684 * 3 - 2048 == 4  # the last block: one lane
    assert [x["lead"] for x in c] == [[0, 1, 2], [3, 0, 1], [0, 1, 2]]
    assert so.dims(1080, 1920, 512)[:2] == (288, 512) and so.dims(720, 1280, 640)[:2] == (360, 640)


@pytest.fixture(scope="module")
def s344():
    frames = _frames(S344, 11)
    images, scales = _run(344, frames)
    return frames, images, scales


def test_preprocess_two_blocks_matches_fp64(s344):
    frames, images, scales = s344
    worst = _check(344, images, scales, frames)
    print(f"S=344: worst err / bound {worst:.3f}")
    # the identity: exactly the fp32 normalised frame
    mean, std = (np.asarray(v, np.float32) for v in _mean_std())
    np.testing.assert_array_equal(images[0], ((frames[0].astype(np.float32) - mean) / std).astype(np.float32))
    # 344 x 342: pixel 341 is image (its channel 0 in block 0, channels 1 and 2 in block 1), pixel 342 padding
    assert images[1, :, 341].all() and not images[1, :, 342:].any()


def test_preprocess_three_blocks_matches_fp64():
    frames = _frames([(61, 2051)], 12)
    images, scales = _run(684, frames)
    _check(684, images, scales, frames)


@pytest.mark.parametrize("S,shape", [(512, (1080, 1920)), (640, (720, 1280))])
def test_preprocess_production_sizes_match_fp64(S, shape):
    frames = _frames([shape], 13)
    images, scales = _run(S, frames)
    _check(S, images, scales, frames)


def test_canvas_does_not_depend_on_neighbours_alignment_or_batch(s344):
    """Bit for bit: a frame's canvas with all-zero and all-255 bytes around it (the dword loads that straddle the
    frame's first and last bytes), at the four alignments of its byte offset, alone and in the batch."""
    frames, images, _ = s344
    for k in (1, 3, 6, 7):  # 344x342, 41x3501, 343x1029 (sizes = 0, 1, 3 mod 4 bytes and an odd lead), 7x5
        fr = frames[k]
        for align in range(4):
            for fill in (0, 255):
                got, _ = _run(344, [fr], offsets=[8 + align], fill=fill, total=8 + align + fr.size + 11)
                assert np.array_equal(got[0], images[k]), (fr.shape, align, fill)
