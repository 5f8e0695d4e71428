"""HistogramMatcher.call (brightness_matcher.py:82-162) restated for the tests (a helper, not a test).

Two layers, as the library computes it:

* numpy fp32, operation by operation in the reference's order (no fused multiply-add): the Y channel,
  the 256-bin histograms (tf.histogram_fixed_width(v, [0, 1], 256) = clamp(floor(256 v), 0, 255)), the
  CDFs f32(c[k] - c[0]) / f32(n - 1), the grid FS[k] = clamp(f32(k) * f32(1/255), 0, 1) and the lookup
  table lut = interp(cdf_t, FS, cdf_s).  The library's histograms and table must equal these exactly.
* torch fp64 `hist_match(src, tgt)`: the per-pixel remap interp(FS, lut, Y) and the colour conversions
  in torch ops, with the table taken from the fp32 layer under no_grad (the histogram op has no
  gradient in TF), so autograd yields the selected segment's slope as Y's gradient.

`bin_safe` redraws the pixels whose Y sits within 1e-3 (in bin units) of a histogram bin edge or of a
knot of FS; fp32 rounding of Y is about 3e-5 in those units, so on bin-safe inputs the histograms and
the selected segments do not depend on rounding or on the precision Y was computed in.
"""
import numpy as np
import torch

f32 = np.float32
K01 = f32(127.0 / 255.0)
KB = f32(255.0 / 127.0)
KY = (f32(0.299), f32(0.587), f32(0.114))
NB = 256


def fs_grid():
    """floating_space: clip(range(0, 1.00001, 1/255), 0, 1) taken as k * f32(1/255) (fp32)."""
    return np.clip(np.arange(NB, dtype=f32) * (f32(1.0) / f32(255.0)), f32(0), f32(1)).astype(f32)


def y32(x):
    """Y of an image [..., 3] in [-1, 1] space, fp32, each multiply and add rounded on its own."""
    x = np.asarray(x, f32)
    r, g, b = ((x[..., c] + f32(1.0)) * K01 for c in range(3))
    return ((r * KY[0] + g * KY[1]) + b * KY[2]).astype(f32)


def y64(x):
    x = np.asarray(x, np.float64)
    s = (x + 1.0) * float(K01)
    return s[..., 0] * 0.299 + s[..., 1] * 0.587 + s[..., 2] * 0.114


def histogram(v):
    k = np.clip(np.floor(f32(256.0) * np.asarray(v, f32).reshape(-1)), 0, NB - 1).astype(np.int64)
    return np.bincount(k, minlength=NB)


def cdf(h, n):
    c = np.cumsum(h.astype(np.int64))
    return ((c - c[0]).astype(f32) / f32(n - 1)).astype(f32)


def interp(dx, dy, x):
    """interpolate(dx_T, dy_T, x) (brightness_matcher.py:135-162), fp32: dy[0] at or below dx[0],
    dy[255] at or above dx[255], else on the segment whose right knot is the first dx > x."""
    dx, dy, x = np.asarray(dx, f32), np.asarray(dy, f32), np.asarray(x, f32)
    i1 = np.clip(np.searchsorted(dx, x, side="right"), 1, NB - 1)
    i0 = i1 - 1
    with np.errstate(divide="ignore", invalid="ignore"):
        v = dy[i0] + ((dy[i1] - dy[i0]) * (x - dx[i0])) / (dx[i1] - dx[i0])
    return np.where(x <= dx[0], dy[0], np.where(x >= dx[-1], dy[-1], v)).astype(f32)


def lut32(src, tgt):
    """(hist_src, hist_tgt, lut) of one image pair, src [P,P,3], tgt [H,W,3] (fp32 restatement)."""
    ys, yt = y32(src), y32(tgt)
    hs, ht = histogram(ys), histogram(yt)
    return hs, ht, interp(cdf(ht, yt.size), fs_grid(), cdf(hs, ys.size))


def max_slope(lut):
    fs = fs_grid()
    return float(np.max(np.diff(lut.astype(np.float64)) / np.diff(fs.astype(np.float64))))


def _mats(dtype):
    from oracle import eot
    return eot.RGB2YUV.to(dtype), eot.YUV2RGB.to(dtype)


def hist_match(src, tgt):
    """HistogramMatcher.call((src, tgt)) for one image, torch (fp64) src [P,P,3], tgt [H,W,3]."""
    with torch.no_grad():
        _, _, lut = lut32(src.detach().numpy().astype(f32), tgt.detach().numpy().astype(f32))
    lut = torch.as_tensor(lut.astype(np.float64), dtype=src.dtype)
    fs = torch.as_tensor(fs_grid().astype(np.float64), dtype=src.dtype)
    m_fwd, m_back = _mats(src.dtype)
    s = ((src + 1.0) * float(K01)) @ m_fwd
    y = s[..., 0]
    i1 = torch.searchsorted(fs, y.detach().contiguous(), right=True).clamp(1, NB - 1)
    i0 = i1 - 1
    v = lut[i0] + ((lut[i1] - lut[i0]) * (y - fs[i0])) / (fs[i1] - fs[i0])
    pxmap = torch.where(y <= fs[0], lut[0].expand_as(y), torch.where(y >= fs[-1], lut[-1].expand_as(y), v))
    res = torch.stack([pxmap, s[..., 1], s[..., 2]], -1) @ m_back
    return torch.clamp(res, 0.0, 1.0) * float(KB) - 1.0


def _unsafe(x, prints, tol):
    bad = np.zeros(x.shape[:-1], bool)
    for w, b in prints:
        p = x.astype(np.float64)
        if w is not None:
            p = np.clip(np.asarray(w, np.float64) * p + np.asarray(b, np.float64), -1.0, 1.0)
        y = y64(p)
        for m in (256.0, 255.0):
            bad |= np.abs(m * y - np.round(m * y)) < tol
    return bad


def bin_safe(x, rng, lo=-1.0, hi=1.0, prints=((None, None),), tol=1e-3, stats=None):
    """x [..., 3] float32 with every pixel whose fp64 256*Y or 255*Y lies within tol of an integer
    redrawn from U(lo, hi), until none remains.  prints: (w, b) print parameters (attacker.py:365-372)
    under each of which clip(w * x + b, -1, 1) must be bin-safe; (None, None) = x itself.
    stats (a list) receives the redrawn share of every round."""
    x = np.array(x, f32)
    while True:
        bad = _unsafe(x, prints, tol)
        if stats is not None:
            stats.append(float(bad.mean()))
        if not bad.any():
            return x
        x[bad] = rng.uniform(lo, hi, (int(bad.sum()), 3)).astype(f32)
