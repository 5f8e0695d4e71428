"""An independent pin of oracle.eot.resize_matrix, on which serve_oracle.preprocess64 and the whole EOT oracle rest.

resize_matrix restates one axis of tf.image.resize(antialias=True) (ScaleAndTranslate's triangle kernel) in fp32,
as TF computes it.  torch.nn.functional.interpolate(mode="bilinear", antialias=True, align_corners=False) is the
same filter written by other people: a triangle of half-width max(1, in/out) source pixels around the half-pixel
sample centre, normalised to sum 1.  On a float64 identity input it returns its weight matrix in float64.

This makes nothing "parity pinned" against TensorFlow: no TensorFlow runs here, and the two libraries may still
differ from TF in the same way.  It only says that two independent statements of the filter agree to the rounding
of the fp32 one.

The bound, per weight, with u = 2^-24, k = max(1, in/out) and the triangle's slope 1/k:
  the sample coordinate (i + 0.5) * fp32(1 / fp32(out / in)) has magnitude up to `in` and carries the roundings of
  the scale, its reciprocal and the product: 3.5 u in; the tap offset src + 0.5 - sample rounds once more at that
  magnitude: u in; so the triangle's argument moves by 4.5 u in / k, and its own scaling by fp32(1 / k) and the
  subtraction from 1 add 5 u:                    d_raw = 4.5 u in / k + 5 u
  the normalisation divides by the sum of the T <= 2k + 1 raw weights, which is at least k / 2 (a clamped edge
  keeps half the triangle): each weight's own error, the sum's error (T d_raw, weight / sum <= 2 / T ... 2 / k) and
  two roundings:                                 bound = 6 d_raw / k + 2 u
Measured (printed below): 6.8e-6 against 1.9e-4 at 1000 -> 341, 4.8e-7 against 1.3e-5 at 7 -> 512, 0 at the
identity, which is also asserted exactly: there the sample centres are exact and every neighbour sits at |x| = 1."""
import numpy as np
import pytest
import torch

from oracle import eot

U = 2.0 ** -24
PAIRS = [(3, 40), (33, 3500), (341, 1000), (342, 1003), (512, 7), (344, 344)]


def _torch_matrix(out, inn):
    # channel c holds the unit vector e_c along H; the width (2 -> 2, two equal columns) is untouched.  (At a
    # width of 1 this torch build repeats output row 0 in every row, so the width is 2.)
    x = torch.eye(inn, dtype=torch.float64).reshape(1, inn, inn, 1).expand(1, inn, inn, 2).contiguous()
    y = torch.nn.functional.interpolate(x, size=(out, 2), mode="bilinear", antialias=True, align_corners=False)
    assert torch.equal(y[..., 0], y[..., 1])
    return y[0, :, :, 0].T.numpy()  # [out, in]


@pytest.mark.parametrize("out,inn", PAIRS)
def test_resize_matrix_agrees_with_torch_antialias(out, inn):
    got = eot.resize_matrix(out, inn).astype(np.float64)
    ref = _torch_matrix(out, inn)
    assert got.shape == ref.shape == (out, inn)
    k = max(1.0, inn / out)
    bound = 6 * (4.5 * U * inn / k + 5 * U) / k + 2 * U
    err = np.abs(got - ref).max()
    print(f"resize_matrix {inn} -> {out}: max |d weight| {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    np.testing.assert_allclose(ref.sum(1), 1.0, atol=1e-12)
    np.testing.assert_allclose(got.sum(1), 1.0, atol=(2 * k + 3) * U)  # fp32 weights, each rounded once
    if out == inn:
        np.testing.assert_array_equal(got, np.eye(out))
        np.testing.assert_array_equal(ref, np.eye(out))
