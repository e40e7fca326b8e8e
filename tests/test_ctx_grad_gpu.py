"""d(loss)/d(encoder_hidden_states) of the HIP engine (smi_unet_backward_ctx, through the product UNet's autograd seam)
against the CPU oracle's autograd.

Inputs: the build_pair / inputs recipe of tests/test_engine_gpu.py (tiny_sd1x and tiny_sdxl, fp16 and bf16, n = 2, 16 x 16
latents, ctx_len 77, t = 499) and an output gradient randn x 1e-4 with sample 1 multiplied by 8 -- the two samples then get
different power-of-two loss scales, and a wrong unscale shows.

The bar is a relative L2 norm over the whole d_ctx tensor: 3 x e_q + 1e-4, where e_q is the distance between the oracle's
d_ctx with the forward rounded to the storage dtype and its fp32 one, computed here.  The factor is the project's: the rounded
oracle rounds the forward only, and the global LoRA-gradient error sits at 2.6 x the forward's rounding floor
(tests/test_engine_gpu.py).  Each sample is held to the same formula on its own rows as well: sample 1 carries 8 x the
gradient, so the whole-tensor figure alone would not see a mistake confined to sample 0
(tests/test_ctx_grad_refs_cpu.py shows what the bar can and cannot see)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctx_grad_refs as R
from tests.test_engine_gpu import build_pair, cuda_add, inputs

MODELS = ["tiny_sd1x", "tiny_sdxl"]
DTYPES = [torch.float16, torch.bfloat16]


def check_bar(tag, got, ref32, refq):
    e_eng, e_q = R.rel(got, ref32), R.rel(refq, ref32)
    print(f"{tag}: e_eng {e_eng:.3e}  e_q {e_q:.3e}  ratio {e_eng / e_q:.2f}  bar {R.bar(e_q):.3e}")
    per = []
    for s in range(got.shape[0]):
        es, qs = R.rel(got[s], ref32[s]), R.rel(refq[s], ref32[s])
        print(f"{tag}: sample {s}: e_eng {es:.3e}  e_q {qs:.3e}  ratio {es / qs:.2f}")
        per.append((s, es, qs))
    assert torch.isfinite(got).all()
    assert e_eng < R.bar(e_q), f"{tag}: d_ctx rel err {e_eng:.3e} above 3 x {e_q:.3e} + 1e-4"
    for s, es, qs in per:
        assert es < R.bar(qs), f"{tag}: sample {s} d_ctx rel err {es:.3e} above 3 x {qs:.3e} + 1e-4"


def product_d_ctx(pu, pnet, x, ctx, add, gy):
    c = ctx.cuda().requires_grad_()
    if pnet is not None:
        pnet.flat.grad = None
        with pnet:
            out = pu(x.cuda(), R.T, encoder_hidden_states=c, added_cond_kwargs=cuda_add(add)).sample
    else:
        out = pu(x.cuda(), R.T, encoder_hidden_states=c, added_cond_kwargs=cuda_add(add)).sample
    assert out.requires_grad
    (out * gy.cuda()).sum().backward()
    assert c.grad is not None and c.grad.dtype == torch.float32 and c.grad.shape == ctx.shape
    return out.detach(), c.grad.detach().cpu()


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_network_grouped_path(model, dtype):
    """(i) no adaptor at all: grouped k|v projection, d_ctx as one GEMM, and the first cross-attention of the net runs the
    dK / dV-only attention backward (its q has no gradient)."""
    ocfg, ou, pu = R.build_plain_pair(model, dtype)
    x, ctx, add = inputs(ocfg, R.N, R.HW)
    gy = R.output_grad()
    with torch.no_grad():
        plain = pu(x.cuda(), R.T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
    wbytes = pu._engine.stats()["weights_bytes"]
    out, got = product_d_ctx(pu, None, x, ctx, add, gy)
    assert torch.equal(out, plain)  # the differentiated forward computes the same bits
    assert pu._engine.stats()["weights_bytes"] == wbytes  # the transposed k|v copy lives in the extra buffer
    check_bar(f"{model} {dtype} no network", got, R.plain_refs(model), R.plain_refs(model, dtype))
    # written, not accumulated; and reproducible
    _, again = product_d_ctx(pu, None, x, ctx, add, gy)
    assert torch.equal(again, got)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("method", ["xattn", "noxattn"])
def test_with_lora_network(model, dtype, method):
    """(ii) xattn: LoRA on to_k / to_v -- per-layer k|v projections, their d_ctx terms summed in fp32, adapted K / V;
    (iii) noxattn: grouped path with LoRA gradients in the same backward.  The LoRA gradients must not notice."""
    ocfg, ou, onet, pu, pnet = build_pair(model, dtype, method=method)
    x, ctx, add = inputs(ocfg, R.N, R.HW)
    gy = R.output_grad()
    # the parent's entry points, on the fresh engine: eps and LoRA gradients
    flat, n_down, _ = pnet.engine_params()
    eng = pu._ensure_engine(R.N, R.HW, R.HW, 77)
    te = None if add is None else add["text_embeds"].cuda().to(dtype)
    ti = None if add is None else add["time_ids"].cuda().float()
    eps0 = eng.forward(x.cuda(), R.T, ctx.cuda().to(dtype), te, ti, flat[:n_down].detach(), flat[n_down:].detach(), 1.0, True)
    g0 = torch.zeros_like(flat)
    eng.backward(gy.cuda(), g0[:n_down], g0[n_down:])
    assert float(g0.abs().max()) > 0
    # no embedding requires a gradient: the seam takes the same launches
    pnet.flat.grad = None
    with pnet:
        out1 = pu(x.cuda(), R.T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
    (out1 * gy.cuda()).sum().backward()
    assert torch.equal(out1.detach(), eps0) and torch.equal(pnet.flat.grad, g0)
    # with the context gradient
    out2, got = product_d_ctx(pu, pnet, x, ctx, add, gy)
    assert torch.equal(out2, eps0)
    assert torch.equal(pnet.flat.grad, g0), "the LoRA gradients changed with the context gradient on"
    ref32 = R.oracle_d_ctx(ou, onet, x, ctx, add, gy)
    refq = R.oracle_d_ctx(ou, onet, x, ctx, add, gy, storage=dtype)
    check_bar(f"{model} {dtype} {method}", got, ref32, refq)
    # and back: a pass without it is the parent's again
    pnet.flat.grad = None
    with pnet:
        out3 = pu(x.cuda(), R.T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
    (out3 * gy.cuda()).sum().backward()
    assert torch.equal(out3.detach(), eps0) and torch.equal(pnet.flat.grad, g0)


@pytest.mark.parametrize("model", MODELS)
def test_batched_pass_with_frozen_samples_in_front(model):
    """smi_unet_forward_batched with two frozen samples in front of the two differentiated ones: d_ctx covers the adapted
    samples only, matches the oracle on them, and nothing is written for the frozen ones."""
    dtype = torch.float16
    ocfg, ou, pu = R.build_plain_pair(model, dtype)
    x, ctx, add = inputs(ocfg, R.N, R.HW)
    xf, ctxf, addf = inputs(ocfg, R.N, R.HW, seed=11)
    gy = R.output_grad()
    cat = lambda a, b: torch.cat([a, b]).cuda().contiguous()
    te = None if add is None else cat(addf["text_embeds"], add["text_embeds"]).to(dtype)
    ti = None if add is None else cat(addf["time_ids"], add["time_ids"]).float()
    eng = pu._ensure_engine(2 * R.N, R.HW, R.HW, 77, n_adapted=R.N)
    eng.set_ctx_grad(True)
    eps = eng.forward(cat(xf, x), R.T, cat(ctxf, ctx).to(dtype), te, ti, None, None, 0.0, True, n_adapted=R.N)
    buf = torch.full((2 * R.N, 77, ocfg.cross_attention_dim), 7.0, device="cuda")
    eng.backward_ctx(gy.cuda(), None, None, buf[R.N:])
    assert torch.isfinite(eps).all()
    assert bool((buf[:R.N] == 7.0).all()), "something was written for the frozen samples"
    check_bar(f"{model} batched", buf[R.N:].cpu(), R.plain_refs(model), R.plain_refs(model, dtype))
    eng.set_ctx_grad(False)


def test_refusals():
    from sliders_conceptmod_amd._native import SmiError
    ocfg, ou, pu = R.build_plain_pair("tiny_sd1x", torch.float16)
    x, ctx, add = inputs(ocfg, R.N, R.HW)
    eng = pu._ensure_engine(R.N, R.HW, R.HW, 77)
    d = torch.empty(R.N, 77, ocfg.cross_attention_dim, device="cuda")
    eng.forward(x.cuda(), R.T, ctx.cuda().half(), None, None, None, None, 0.0, True)
    with pytest.raises(SmiError, match="does not differentiate the context"):
        eng.backward_ctx(R.output_grad().cuda(), None, None, d)
    eng.set_ctx_grad(True)
    eng.forward(x.cuda(), R.T, ctx.cuda().half(), None, None, None, None, 0.0, True)
    g = torch.zeros(8, device="cuda")
    with pytest.raises(SmiError, match="tail backward is not offered"):
        eng.backward_tail(R.output_grad().cuda()[1:], g, g)
