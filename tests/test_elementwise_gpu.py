"""sga_elu_fwd, sga_elu_bwd (gat.hip) and sga_relu_bwd (gcn.hip) called directly: exact where the operation is exact, within the measured
ulp bound of tests/fusion_gate.py against fp64 where it is not, at sizes on both sides of a workgroup and of the grid-stride loop's first
trip (8192 workgroups of 256 threads)."""
import math

import pytest
import torch

import fusion_gate as FG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', FG.EW_SIZES)
def test_elu(n):
    x, gy = FG.ew_inputs(n)
    y, gx = FG.elu_run(x, gy)
    pos = x > 0
    assert FG.same_bits(y[pos], x[pos]) and FG.same_bits(gx[pos], gy[pos])              # identity in bits for x > 0, both ways
    assert not torch.isnan(y).any() and not torch.isnan(gx).any()                         # every element written, none past the end read as one
    neg = ~pos
    if neg.any():
        fwd, bwd = FG.elu_worst_ulps(y, gx, x, gy)
        yy, yg = FG.elu_yardstick(x, gy)
        yf, yb = FG.elu_worst_ulps(yy, yg, x, gy)
        print(f'[elu] n {n}: forward {fwd:.3f} ulp (torch float32 {yf:.3f}), backward {bwd:.3f} ulp (torch float32 {yb:.3f}); '
              f"bounds {FG.ULP['elu_fwd']} / {FG.ULP['elu_bwd']}")
        assert fwd <= FG.ULP['elu_fwd'] and bwd <= FG.ULP['elu_bwd']
        inf = torch.isinf(x) & neg
        assert (y[inf] == -1.0).all() and (gx[inf] == 0.0).all()
        zero = x == 0
        assert (y[zero] == 0).all() and FG.same_bits(gx[zero], gy[zero])


@pytest.mark.parametrize('n', FG.EW_SIZES)
def test_relu_bwd(n):
    y, gy = FG.relu_inputs(n)
    gx = FG.relu_run(y, gy)
    want = torch.where(y > 0, gy, torch.zeros_like(gy))               # gy in bits where y > 0; +0.0 at y = -0.0, y = 0.0 and y < 0
    assert FG.same_bits(gx, want)
    if n >= 3000:
        off = ~(y > 0)
        assert (y[off] == 0).any() and torch.signbit(y[off]).any() and (y[off] < 0).any() and torch.signbit(gy[off]).any()


def _strided(n, gen):
    """A [n, 6] view of every second column of a [n, 12] tensor, values on both sides of zero with exact zeros."""
    base = torch.randn(n, 12, generator=gen)
    base[::5] = 0.0
    return base.cuda()[:, ::2]


def test_stacks_take_non_contiguous_tensors():
    """gat_ops.EluFn and gcn_ops._relu_bwd on a non-contiguous input and cotangent give what they give on contiguous copies."""
    from sgaligner_amd import gat_ops, gcn_ops
    gen = torch.Generator().manual_seed(3)
    x, gy = _strided(301, gen), _strided(301, gen)
    assert not x.is_contiguous() and not gy.is_contiguous()
    outs = []
    for a, g in ((x, gy), (x.contiguous(), gy.contiguous())):
        a = a.detach().requires_grad_(True)
        y = gat_ops.EluFn.apply(a)
        ga, = torch.autograd.grad(y, a, g)
        outs.append((y.detach(), ga, gcn_ops._relu_bwd(a.detach(), g)))
    torch.cuda.synchronize()
    for s, c in zip(*outs):
        assert s.shape == c.shape and FG.same_bits(s.cpu(), c.cpu())
    ref = torch.nn.functional.elu(x.cpu().double())
    assert (outs[0][0].cpu().double() - ref).abs().max().item() <= 2.0 ** -22
    assert math.isfinite(outs[0][2].sum().item())
    assert FG.same_bits(outs[0][2].cpu(), torch.where(x.cpu() > 0, gy.cpu(), torch.zeros(301, 6)))
