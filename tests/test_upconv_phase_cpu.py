"""The phase form of the up-sampler conv (tests/upconv_phase_refs.py) against torch in float64: four 2x2 phase convs + the
un-shuffle equal nearest-2x + 3x3 / pad 1, and the 4x4 / stride-2 conv over dy equals its autograd input gradient, to 1e-12
at every shape of the list (1 x 1: all taps but one are padding; odd H != W)."""
import pytest
import torch

import upconv_phase_refs as R

TOL = 1e-12


def data(nb, H, W, cin=5, cout=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nb, cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    return x, w, b


@pytest.mark.parametrize("nb", R.BATCHES)
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_phase_convs_equal_upsample_then_conv(nb, H, W):
    x, w, b = data(nb, H, W)
    ref = R.upconv_ref(x, w, b).permute(0, 2, 3, 1)
    planes = R.phase_planes(x.permute(0, 2, 3, 1).contiguous(), w, b)
    assert planes.shape == (4, nb, H, W, w.shape[0])
    got = R.unshuffle(planes)
    assert (got - ref).abs().max().item() <= TOL
    # the layout itself: plane 2a + b is the (a, b) sub-grid, and shuffle inverts unshuffle
    for a in range(2):
        for bb in range(2):
            assert torch.equal(planes[2 * a + bb], got[:, a::2, bb::2])
    assert torch.equal(R.shuffle(got), planes)


def test_phase_pack_order_and_sums():
    _, w, _ = data(1, 2, 2)
    pk = R.phase_pack(w)
    cout, cin = w.shape[:2]
    assert pk.shape == (4, cout, 4 * cin)
    # phase (0, 0), tap (1, 1) is the sum of the 3x3 rows {1, 2} x columns {1, 2}; phase (1, 1), tap (0, 0) rows {0, 1} x columns {0, 1}
    assert torch.allclose(pk[0, :, 3 * cin:], w[:, :, 1:, 1:].sum(dim=(2, 3)), rtol=0, atol=TOL)
    assert torch.allclose(pk[3, :, :cin], w[:, :, :2, :2].sum(dim=(2, 3)), rtol=0, atol=TOL)
    # every 3x3 weight lands in exactly one tap of each phase
    assert torch.allclose(pk.view(4, cout, 4, cin).sum(dim=2), w.sum(dim=(2, 3)).expand(4, -1, -1), rtol=0, atol=TOL)


@pytest.mark.parametrize("nb", R.BATCHES)
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_4x4_stride2_conv_is_the_input_gradient(nb, H, W):
    x, w, b = data(nb, H, W, seed=1)
    x.requires_grad_(True)
    y = R.upconv_ref(x, w, b)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (dx,) = torch.autograd.grad(y, x, dy)
    got = R.upconv_dx_4x4(dy, w)
    assert got.shape == dx.shape
    assert (got - dx).abs().max().item() <= TOL
