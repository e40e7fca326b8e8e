"""smi_nulltext_loss (the fused body of a null-text inner step) against its formula in fp64 on the same fp32 inputs:
    eps = eps_u + g (eps_c - eps_u);  x_prev = c_x x_t + c_eps eps;  loss = mean((x_prev - target)^2)
    d_eps_u = (1 - g) c_eps (2 / n) (x_prev - target)

Tolerances.  The loss is a sum of n non-negative fp32 terms reduced as a tree (per-thread strides, wave, workgroup, ordered
partials): rtol 1e-5.  The gradient is a handful of fp32 operations per element: rtol 1e-5 -- plus, per element, the absolute
error that the subtraction x_prev - target inherits from its operands: each of the five roundings in front of it is at most
2^-24 of a term no larger than A = |c_x x_t| + |c_eps| (|eps_u| + |g| (|eps_c| + |eps_u|)) + |target|, so
|error(d_eps_u)| <= |k| 5 x 2^-24 A with k = (1 - g) c_eps 2 / n.  (Where x_prev and target nearly cancel, a relative bound on
the difference alone is not something fp32 can meet.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from sliders_conceptmod_amd import _native

# 4 x 8 x 8 and 4 x 64 x 64 latents (one workgroup, one launch), a size that is no multiple of the 256-thread block, and one
# beyond 65536 elements, where the kernel switches to block partials and the ordered final sum
SIZES = [4 * 8 * 8, 4 * 64 * 64, 4 * 8 * 8 + 37, 65536 + 4 * 64 * 64 + 3]
C_X, C_EPS = 1.0371, -0.2468  # DDIM prev_step coefficients of a mid-schedule step (sqrt(a_prev / a_t), ...)


def run(n, g, seed=0):
    gen = torch.Generator().manual_seed(seed)
    eu, ec, xt, tg = (torch.randn(n, generator=gen) for _ in range(4))
    dev = [t.cuda() for t in (eu, ec, xt, tg)]
    loss = torch.full((1,), -1.0, device="cuda")
    grad = torch.full((n,), 3.0, device="cuda")
    scratch = torch.empty(256, device="cuda")
    _native.nulltext_loss(*dev, g, C_X, C_EPS, loss, grad, scratch)
    return (eu, ec, xt, tg), loss.cpu(), grad.cpu()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("g", [7.5, 1.0])
def test_loss_and_gradient_match_fp64(n, g):
    (eu, ec, xt, tg), loss, grad = run(n, g)
    eu64, ec64, xt64, tg64 = (t.double() for t in (eu, ec, xt, tg))
    cx, ce, g32 = (float(torch.tensor(v, dtype=torch.float32)) for v in (C_X, C_EPS, g))  # the fp32 values the kernel gets
    d = cx * xt64 + ce * (eu64 + g32 * (ec64 - eu64)) - tg64
    k = (1.0 - g32) * ce * 2.0 / n
    ref_loss, ref_grad = (d * d).mean(), k * d
    rl = abs(loss.double().item() - ref_loss.item()) / ref_loss.item()
    print(f"n={n} g={g}: loss {loss.item():.7f} ref {ref_loss.item():.7f} rel {rl:.2e}")
    assert rl < 1e-5
    if g == 1.0:
        assert bool((grad == 0).all()), "d_eps_u must be exactly zero at guidance scale 1"
        return
    A = (cx * xt64).abs() + abs(ce) * (eu64.abs() + abs(g32) * (ec64.abs() + eu64.abs())) + tg64.abs()
    err = (grad.double() - ref_grad).abs()
    bound = 1e-5 * ref_grad.abs() + abs(k) * 5 * 2.0 ** -24 * A
    worst = (err / bound).max().item()
    print(f"n={n} g={g}: gradient worst err / bound {worst:.3f}, max rel {(err / ref_grad.abs().clamp_min(1e-300)).max():.2e}")
    assert worst <= 1.0


@pytest.mark.parametrize("n", [SIZES[1], SIZES[3]])
def test_two_runs_are_bit_equal(n):
    _, l1, g1 = run(n, 7.5)
    _, l2, g2 = run(n, 7.5)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_gradient_is_optional():
    n = SIZES[0]
    gen = torch.Generator().manual_seed(0)
    dev = [torch.randn(n, generator=gen).cuda() for _ in range(4)]
    loss = torch.zeros(1, device="cuda")
    _native.nulltext_loss(*dev, 7.5, C_X, C_EPS, loss, None, torch.empty(256, device="cuda"))
    (_, _, _, _), ref, _ = run(n, 7.5)
    assert torch.equal(loss.cpu(), ref)
