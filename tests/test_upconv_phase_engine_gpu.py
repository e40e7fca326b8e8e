"""The UNet engine with its up-sampler convs as four 2x2 phase convs (SMI_UPCONV_PHASE, the default) against the same engine
with one 3x3 conv on the 2x grid, on tiny_sdxl at 128 x 128 pixels (16 x 16 latents): a batched 3 + 1 pass and its backward.

The two forms differ by one 16-bit rounding of the summed filters on two layers, so eps and the LoRA gradient must differ by
less than the project's own distance to the fp32 oracle (eps 1.8e-3 fp16 / 1.4e-2 bf16, global LoRA
gradient 4.7e-3 / 3.7e-2, the bars of tests/test_engine_gpu.py) -- a larger difference is a bug, not rounding.  The phase-major
temporary lives in the no-grad passes' alternating scratch regions as well as in the saved pass's arena: a no-grad forward
must give the frozen samples the bits the saving forward gave them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_engine_gpu import LOOSE, build_pair, inputs, rel

GRAD_BAR = {torch.float16: 4.7e-3, torch.bfloat16: 3.7e-2}
N = 2  # samples per prompt: the pass is [3 N frozen | N adapted]


def batched_pass(dtype, phase):
    """eps of the saving 3 + 1 pass, its flat LoRA gradient, and eps of a no-grad pass over the same samples"""
    from sliders_conceptmod_amd import _native
    lib = _native.lib()
    assert lib.smi_set_upconv_phase(phase) == 0
    try:
        ocfg, _, _, pu, pnet = build_pair("tiny_sdxl", dtype)
        xs, ctxs, tes, tids = [], [], [], []
        for i in range(4):
            x, _, _ = inputs(ocfg, N, 16, seed=3)
            _, ctx, add = inputs(ocfg, N, 16, seed=10 + i)
            xs.append(x), ctxs.append(ctx), tes.append(add["text_embeds"]), tids.append(add["time_ids"])
        x = torch.cat(xs).cuda()
        ctx = torch.cat(ctxs).cuda().to(dtype)
        te, tid = torch.cat(tes).cuda().to(dtype), torch.cat(tids).cuda().float()
        flat, n_down, _ = pnet.engine_params()
        down, up = flat[:n_down].detach(), flat[n_down:].detach()
        gy = torch.randn(N, 4, 16, 16, generator=torch.Generator().manual_seed(9)).cuda() * 1e-3
        eng = pu._ensure_engine(4 * N, 16, 16, 77, n_adapted=N)
        eps = eng.forward(x, 499.0, ctx, te, tid, down, up, 1.0, True, n_adapted=N).clone()
        frozen = eng.forward(x, 499.0, ctx, te, tid, None, None, 0.0, False, n_adapted=N).clone()
        g = torch.zeros_like(flat)
        eng.backward(gy, g[:n_down], g[n_down:])
        torch.cuda.synchronize()
        return eps, g.detach().clone(), frozen
    finally:
        lib.smi_set_upconv_phase(-1)


@pytest.fixture(scope="module", params=[torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def runs(request):
    dtype = request.param
    return dtype, batched_pass(dtype, 0), batched_pass(dtype, 1)


def test_eps_and_lora_gradient_within_the_oracle_bars(runs):
    dtype, (eps0, g0, _), (eps1, g1, _) = runs
    e, ge = rel(eps1, eps0), rel(g1, g0)
    print(f"\n{dtype}: phase form vs 3x3 form: eps rel L2 {e:.3e} (bar {LOOSE[dtype]:.1e}), LoRA gradient rel L2 {ge:.3e} "
          f"(bar {GRAD_BAR[dtype]:.1e})")
    assert float(g0.abs().max()) > 0 and float(g1.abs().max()) > 0
    assert e > 0, "the selector changed nothing: both engines ran the same form"
    assert e < LOOSE[dtype], f"eps differs by {e:.3e}"
    assert ge < GRAD_BAR[dtype], f"LoRA gradient differs by {ge:.3e}"


def test_default_keeps_maps_under_the_floor_on_the_3x3_form(runs):
    """8 x 8 and 4 x 4 input maps are under the default floor of 32 x 32 pixels per sample: the default selection (-1) must
    give the bits of the 3x3 form; the two tests beside this one force the phase form with the override 1"""
    dtype, (eps0, g0, _), _ = runs
    eps, g, _ = batched_pass(dtype, -1)
    assert torch.equal(eps, eps0) and torch.equal(g, g0)


def test_no_grad_pass_gives_the_saved_pass_its_frozen_rows(runs):
    _, (eps0, _, frozen0), (eps1, _, frozen1) = runs
    for eps, frozen in ((eps0, frozen0), (eps1, frozen1)):
        assert torch.equal(frozen[:3 * N], eps[:3 * N])
        assert not torch.equal(frozen[3 * N:], eps[3 * N:])  # (the adapted rows carry the LoRA delta in the saved pass only)
