"""CPU: the layer-parity sweep of tests/layer_parity.py, run with the oracle's fp32 run standing in for
the device.

The reference alone passes: the fp32 run is the yardstick, so at k = 1 it passes its own sweep by
construction; what the tests pin is the plumbing — 158 taps of D0, 15 of them (box_net) without a
gradient, the exactly-zero levels, the residual chains, the loss-anchor gap condition.

Seeded errors are caught and localised: five mutants of the fp32 run on case A, each an error a kernel
rewrite could make, must fail the sweep at the K_FWD / K_BWD the GPU tests use, with the expected first
failing layer and every layer before it in sweep order passing.
"""
import numpy as np
import pytest
import torch

import layer_parity as LP

NO_GRAD = {f"box_net/box-{i}-bn-{lv}" for i in range(3) for lv in range(3, 8)}
# exactly-zero gradients: the class head's BNs at the levels without a loss anchor (3 each), and the
# last cell's bottom-up nodes above the highest such level (fuse, BN, and the max-pool feeding it)
COUNTS = {  # case: (loss-anchor levels, exactly-zero layers)
    "A": ({4}, 4 * 3 + 3 * 3),
    "B": ({3, 5}, 3 * 3 + 2 * 3),
    "C": ({3, 4}, 3 * 3 + 3 * 3),
    "D": ({3}, 4 * 3 + 4 * 3),
}


@pytest.fixture(scope="module")
def refs():
    torch.set_num_threads(16)
    cache = {}

    def get(case):
        if case not in cache:
            S, B, imgs, boxes, _ = LP.case_inputs(case)
            wd, patch = LP.cpu_weights(S)
            cache[case] = (LP.reference(wd, imgs, patch, boxes, S), (wd, imgs, patch, boxes, S))
        return cache[case]
    return get


def test_alias_chains_follow_the_block_table():
    assert LP.derive_alias_chains() == LP.ALIAS_CHAINS
    assert len(LP.alias_map()) == 9  # b0's nine residual blocks


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_reference_passes_its_own_sweep(refs, case):
    ref, (_, _, _, _, S) = refs(case)
    assert len(ref.names) == 158
    assert {n for n in ref.names if ref.bwd[n] is None} == NO_GRAD
    # the argmax cannot flip within the score tolerance, and fp32 agrees on it
    assert min(g for _, g in ref.r64["anchor"]) >= LP.MIN_GAP, ref.r64["anchor"]
    assert [i for i, _ in ref.r32["anchor"]] == [i for i, _ in ref.r64["anchor"]]
    levels, nzero = COUNTS[case]
    assert set(LP.anchor_levels(ref.r64["anchor"], S)) == levels
    fwd, bwd = LP.standin(ref.fwd32, ref.bwd32)
    rep = LP.sweep(ref, fwd, bwd, k_fwd=1, k_bwd=1)
    rep.check()
    assert rep.counts("fwd") == dict(compared=158, refused=0)
    assert rep.counts("bwd") == dict(compared=158 - 15 - nzero, refused=15, zero=nzero)
    # the chain members are expected to hold their head's gradient, which is not their own
    for m, h in LP.alias_map().items():
        assert ref.bwd[m] is ref.bwd[h]
        assert not np.array_equal(ref.bwd32[m], ref.bwd32[h])


def test_sweep_refusal_rules(refs):
    """What may be refused, and that a refusal elsewhere, a non-zero where the oracle has an exact zero
    and an un-aliased chain member each fail."""
    ref, _ = refs("A")
    fwd, bwd = LP.standin(ref.fwd32, ref.bwd32)
    fuse = "fpn_cells/cell_1/fnode3/fuse"
    node_bn = "fpn_cells/cell_1/fnode3/op_after_combine8/bn"
    never = LP.Refused("tap: this fuse is computed on load by its depthwise conv, never stored")
    rep = LP.sweep(ref, dict(fwd, **{fuse: never}), bwd, 1, 1)
    rep.check()
    assert rep.counts("fwd") == dict(compared=157, refused=1)
    # ... but not when its node's BN input is not compared, not for another kind, not with another message
    for f in (dict(fwd, **{fuse: never, node_bn: never}), dict(fwd, **{node_bn: never}),
              dict(fwd, **{fuse: LP.Refused("tap: size mismatch")})):
        with pytest.raises(AssertionError):
            LP.sweep(ref, f, bwd, 1, 1).check()
    zero = "class_net/class-1-bn-7"
    assert zero in ref.zero
    member = LP.bn_project(6)
    own = ref.bwd32[member]
    tiny = np.zeros_like(bwd[zero])
    tiny.flat[0] = 1e-30
    for b in (dict(bwd, **{zero: tiny}), dict(bwd, **{member: own}),
              dict(bwd, **{"box_net/box-0-bn-3": np.zeros_like(fwd["box_net/box-0-bn-3"])}),
              dict(bwd, **{node_bn: LP.Refused("tap: " + LP.NO_GRADIENT)})):
        with pytest.raises(AssertionError):
            LP.sweep(ref, fwd, b, 1, 1).check()


# ---- mutants --------------------------------------------------------------------------------------
BB = "efficientnet-b0"


def _mutant_se_gate_detached(D, block=5):
    class M(D.Detector):
        def conv(self, x, kname, stride=1, bias=None):
            y = super().conv(x, kname, stride, bias)
            return y.detach() if kname == f"{BB}/blocks_{block}/se/conv2d_1/kernel" else y
    return M, None, ("bwd", f"{BB}/blocks_{block}/tpu_batch_normalization_1")


def _mutant_bn_backward_term_missing(D, block=8):
    pfx = f"{BB}/blocks_{block}/tpu_batch_normalization_1"

    class BnNoXhatTerm(torch.autograd.Function):
        """training BN whose input gradient lacks xh * mean(dz * xh)"""

        @staticmethod
        def forward(ctx, x, g, b):
            mean = x.mean(dim=(0, 2, 3), keepdim=True)
            var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
            rstd = 1.0 / torch.sqrt(var + D.BN_EPS)
            ctx.save_for_backward(g, rstd)
            return (x - mean) * rstd * g.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)

        @staticmethod
        def backward(ctx, dy):
            g, rstd = ctx.saved_tensors
            dz = dy * g.view(1, -1, 1, 1)
            return rstd * (dz - dz.mean(dim=(0, 2, 3), keepdim=True)), None, None

    class M(D.Detector):
        def _bn(self, x, p):
            if p == pfx and x.requires_grad:
                return BnNoXhatTerm.apply(x, self.w(p + "/gamma"), self.w(p + "/beta"))
            return super()._bn(x, p)
    return M, None, ("bwd", f"{BB}/blocks_{block}/tpu_batch_normalization")


def _mutant_depthwise_tap_zeroed(D, block=6):
    kname = f"{BB}/blocks_{block}/depthwise_conv2d/depthwise_kernel"

    class M(D.Detector):
        def w(self, name):
            t = super().w(name)
            if name == kname:
                t = t.clone()
                t[0, 1] = 0
            return t
    return M, None, ("fwd", f"{BB}/blocks_{block}/tpu_batch_normalization_1")


def _mutant_fuse_unnormalised(D, cell=1, node=4):
    calls = [0]
    orig = D.fuse_nodes

    def fuse_nodes(nodes, wsm, method):  # 8 nodes per cell, 3 cells, per pass
        i = calls[0] % 24
        calls[0] += 1
        if i != cell * 8 + node:
            return orig(nodes, wsm, method)
        out = nodes[0] * torch.relu(wsm[0])
        for x, w in zip(nodes[1:], wsm[1:]):
            out = out + x * torch.relu(w)
        return out
    return D.Detector, fuse_nodes, ("fwd", f"fpn_cells/cell_{cell}/fnode{node}/fuse")


def _mutant_upsample_shifted(D, pfx="fpn_cells/cell_1/fnode2/resample_1_6_7"):
    base = D.Detector

    class M(base):
        _shift = False

        def resample(self, x, th, tw, p):
            self._shift = p == pfx
            try:
                return super().resample(x, th, tw, p)
            finally:
                self._shift = False

        def upsample(self, x, th, tw):
            if not self._shift:
                return base.upsample(x, th, tw)
            h, w = x.shape[2], x.shape[3]  # every target pixel reads the source pixel one to the right
            iy = torch.arange(th) * h // th
            ix = torch.clamp(torch.arange(tw) * w // tw + 1, max=w - 1)
            return x[:, :, iy][:, :, :, ix]
    return M, None, ("fwd", pfx + "/upsample")


MUTANTS = {
    "se_gate_detached": _mutant_se_gate_detached,
    "bn_backward_term_missing": _mutant_bn_backward_term_missing,
    "depthwise_tap_zeroed": _mutant_depthwise_tap_zeroed,
    "fuse_unnormalised": _mutant_fuse_unnormalised,
    "upsample_shifted": _mutant_upsample_shifted,
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_seeded_error_is_caught_and_localised(refs, monkeypatch, mutant):
    from oracle import detector as D
    ref, (wd, imgs, patch, boxes, S) = refs("A")
    cls, fuse, (direction, first) = MUTANTS[mutant](D)
    monkeypatch.setattr(D, "Detector", cls)
    if fuse is not None:
        monkeypatch.setattr(D, "fuse_nodes", fuse)
    _, f32, b32 = LP.oracle_run(wd, imgs, patch, boxes, S, torch.float32)
    monkeypatch.undo()
    fwd, bwd = LP.standin(f32, b32)
    rep = LP.sweep(ref, fwd, bwd)  # at the committed K_FWD / K_BWD
    with pytest.raises(AssertionError, match="first failing layer"):
        rep.check()
    row, last = rep.first_failure(direction)
    print(row, "| last passing:", last)
    # the first failing layer is the expected one: every layer before it in sweep order passed (or is an
    # exact zero / has no gradient), and one did pass, to localise against
    assert row.name == first and row.status == "fail", str(row)
    assert last is not None
    if direction == "bwd":  # a backward-only error leaves the forward untouched
        assert not rep.failures("fwd")
        names = [r.name for r in rep.of("bwd")]
        assert names.index(last.name) < names.index(first)
