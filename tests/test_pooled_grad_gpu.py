"""d(loss)/d(added_cond_kwargs["text_embeds"]) of the HIP engine (smi_unet_backward_cond, through the product UNet's
autograd seam) against the CPU oracle's autograd, on tiny_sdxl in fp16 and bf16.

Inputs, output gradient and bar are those of tests/test_ctx_grad_gpu.py: relative L2 over the whole tensor and over each
sample under 3 x e_q + 1e-4, e_q the distance between the oracle's gradient with the forward rounded to the storage dtype
and its fp32 one (tests/test_pooled_grad_refs_cpu.py shows what that bar can and cannot see).

Measured on an MI355X, e_eng / e_q: no network fp16 2.18e-3 / 1.90e-3 (ratio 1.15), bf16 1.57e-2 / 1.64e-2 (0.96); noxattn
network fp16 1.25, bf16 1.22; worst sample 1.25."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ctx_grad_refs as CR
from tests import pooled_grad_refs as R
from tests.test_engine_gpu import build_pair, cuda_add, inputs

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
    assert e_eng < R.bar(e_q), f"{tag}: d(text_embeds) rel err {e_eng:.3e} above 3 x {e_q:.3e} + 1e-4"
    for s, es, qs in per:
        assert es < R.bar(qs), f"{tag}: sample {s} d(text_embeds) rel err {es:.3e} above 3 x {qs:.3e} + 1e-4"


def product_grads(pu, pnet, x, ctx, add, gy, pooled=True):
    """(eps, d_ctx, d_text_embeds or None) through the seam; both embeddings are fp32 leaves."""
    c = ctx.cuda().requires_grad_()
    a = cuda_add(add)
    if pooled:
        a["text_embeds"] = a["text_embeds"].requires_grad_()
    if pnet is not None:
        pnet.flat.grad = None
        with pnet:
            out = pu(x.cuda(), R.T, encoder_hidden_states=c, added_cond_kwargs=a).sample
    else:
        out = pu(x.cuda(), R.T, encoder_hidden_states=c, added_cond_kwargs=a).sample
    (out * gy.cuda()).sum().backward()
    te = a["text_embeds"]
    assert a["time_ids"].grad is None
    if pooled:
        assert te.grad is not None and te.grad.dtype == torch.float32 and te.grad.shape == add["text_embeds"].shape
    return out.detach(), c.grad.detach().cpu(), (te.grad.detach().cpu() if pooled else None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_parity_and_bit_equalities_without_a_network(dtype):
    ocfg, ou, pu = CR.build_plain_pair(R.MODEL, dtype)
    x, ctx, add = R.std_inputs()
    gy = R.output_grad()
    with torch.no_grad():
        plain = pu(x.cuda(), R.T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
    stats = pu._engine.stats()
    _, d_ctx_alone, _ = product_grads(pu, None, x, ctx, add, gy, pooled=False)  # backward_ctx alone
    out, d_ctx, got = product_grads(pu, None, x, ctx, add, gy)
    assert torch.equal(out, plain)  # the differentiated forward computes the same bits
    assert pu._engine.stats()["weights_bytes"] == stats["weights_bytes"]  # the transposed copy lives in the extra buffer
    assert torch.equal(d_ctx, d_ctx_alone), "d_ctx changed with the pooled gradient on"
    check_bar(f"{R.MODEL} {dtype} no network", got, R.plain_refs(), R.plain_refs(dtype))
    # written, not accumulated; and reproducible
    _, _, again = product_grads(pu, None, x, ctx, add, gy)
    assert torch.equal(again, got)
    # only the pooled embedding requires a gradient: the same d(text_embeds), the context gets none
    a = cuda_add(add)
    a["text_embeds"].requires_grad_()
    c = ctx.cuda()
    out = pu(x.cuda(), R.T, encoder_hidden_states=c, added_cond_kwargs=a).sample
    (out * gy.cuda()).sum().backward()
    assert c.grad is None and torch.equal(a["text_embeds"].grad.cpu(), got)


def test_batched_pass_with_frozen_samples_in_front():
    """Two frozen samples in front of the two differentiated ones: d(text_embeds) covers the adapted samples only, matches
    the oracle on them, and nothing is written for the frozen ones."""
    dtype = torch.float16
    ocfg, ou, pu = CR.build_plain_pair(R.MODEL, dtype)
    x, ctx, add = R.std_inputs()
    xf, ctxf, addf = inputs(ocfg, R.N, R.HW, seed=11)
    gy = R.output_grad()
    cat = lambda a, b: torch.cat([a, b]).cuda().contiguous()
    te = cat(addf["text_embeds"], add["text_embeds"]).to(dtype)
    ti = cat(addf["time_ids"], add["time_ids"]).float()
    eng = pu._ensure_engine(2 * R.N, R.HW, R.HW, 77, n_adapted=R.N)
    eng.set_ctx_grad(True)
    eng.set_pooled_grad(True)
    eps = eng.forward(cat(xf, x), R.T, cat(ctxf, ctx).to(dtype), te, ti, None, None, 0.0, True, n_adapted=R.N)
    P = add["text_embeds"].shape[1]
    buf = torch.full((2 * R.N, P), 7.0, device="cuda")
    d_ctx = torch.empty(R.N, 77, ocfg.cross_attention_dim, device="cuda")
    eng.backward_cond(gy.cuda(), None, None, d_ctx, buf[R.N:])
    assert torch.isfinite(eps).all()
    assert bool((buf[:R.N] == 7.0).all()), "something was written for the frozen samples"
    check_bar(f"{R.MODEL} batched", buf[R.N:].cpu(), R.plain_refs(), R.plain_refs(dtype))
    eng.set_ctx_grad(False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lora_gradients_do_not_notice(dtype):
    """noxattn LoRA network: the LoRA gradients of a call with the pooled gradient equal, bit for bit, those of the same
    call without it; and with both switches off eps and the LoRA gradients are those of smi_unet_forward / smi_unet_backward
    called directly, before and after a pass with the switch on."""
    ocfg, ou, onet, pu, pnet = build_pair(R.MODEL, dtype, method="noxattn")
    x, ctx, add = R.std_inputs()
    gy = R.output_grad()
    flat, n_down, _ = pnet.engine_params()
    eng = pu._ensure_engine(R.N, R.HW, R.HW, 77)
    te, ti = add["text_embeds"].cuda().to(dtype), add["time_ids"].cuda().float()
    eps0 = eng.forward(x.cuda(), R.T, ctx.cuda().to(dtype), te, ti, flat[:n_down].detach(), flat[n_down:].detach(), 1.0, True)
    g0 = torch.zeros_like(flat)
    eng.backward(gy.cuda(), g0[:n_down], g0[n_down:])
    assert float(g0.abs().max()) > 0

    def switches_off():
        pnet.flat.grad = None
        with pnet:
            out = pu(x.cuda(), R.T, encoder_hidden_states=ctx.cuda(), added_cond_kwargs=cuda_add(add)).sample
        (out * gy.cuda()).sum().backward()
        assert torch.equal(out.detach(), eps0) and torch.equal(pnet.flat.grad, g0)

    switches_off()
    _, d_ctx1, _ = product_grads(pu, pnet, x, ctx, add, gy, pooled=False)
    g_ctx_only = pnet.flat.grad.clone()
    out2, d_ctx2, got = product_grads(pu, pnet, x, ctx, add, gy)
    assert torch.equal(out2, eps0)
    assert torch.equal(pnet.flat.grad, g_ctx_only), "the LoRA gradients changed with the pooled gradient on"
    assert torch.equal(pnet.flat.grad, g0) and torch.equal(d_ctx2, d_ctx1)
    ref = R.oracle_grads(ou, onet, x, ctx, add, gy)[1]
    refq = R.oracle_grads(ou, onet, x, ctx, add, gy, storage=dtype)[1]
    check_bar(f"{R.MODEL} {dtype} noxattn", got, ref, refq)
    switches_off()


def test_refusals_leave_the_engine_working():
    from sliders_conceptmod_amd import _native
    from sliders_conceptmod_amd._native import SmiError
    gy = R.output_grad().cuda()
    # an SD-1.x engine has no pooled embedding
    ocfg1, _, pu1 = CR.build_plain_pair("tiny_sd1x", torch.float16)
    x1, ctx1, _ = inputs(ocfg1, R.N, R.HW)
    eng1 = pu1._ensure_engine(R.N, R.HW, R.HW, 77)
    eng1.set_ctx_grad(True)
    with pytest.raises(SmiError, match="no added conditioning"):
        eng1.set_pooled_grad(True)
    with pytest.raises(SmiError, match="no added conditioning"):
        _native.check(_native.lib().smi_unet_pooled_grad(eng1.handle, 1), "smi_unet_pooled_grad")
    eng1.forward(x1.cuda(), R.T, ctx1.cuda().half(), None, None, None, None, 0.0, True)
    d1 = torch.empty(R.N, 77, ocfg1.cross_attention_dim, device="cuda")
    eng1.backward_ctx(gy, None, None, d1)
    assert torch.isfinite(d1).all() and float(d1.abs().max()) > 0

    ocfg, _, pu = CR.build_plain_pair(R.MODEL, torch.float16)
    x, ctx, add = R.std_inputs()
    te, ti = add["text_embeds"].cuda().half(), add["time_ids"].cuda().float()
    eng = pu._ensure_engine(R.N, R.HW, R.HW, 77)
    fwd = lambda: eng.forward(x.cuda(), R.T, ctx.cuda().half(), te, ti, None, None, 0.0, True)
    d_ctx = torch.empty(R.N, 77, ocfg.cross_attention_dim, device="cuda")
    d_te = torch.empty(R.N, te.shape[1], device="cuda")
    # no buffer attached (with and without the context gradient's)
    with pytest.raises(SmiError, match="needs set_ctx_grad"):
        eng.set_pooled_grad(True)
    eng.set_ctx_grad(True)
    with pytest.raises(SmiError, match="no pooled-gradient buffer is attached"):
        _native.check(_native.lib().smi_unet_pooled_grad(eng.handle, 1), "smi_unet_pooled_grad")
    # a pass saved without the switch has no pooled gradient to give
    eps0 = fwd()
    with pytest.raises(SmiError, match="does not differentiate the pooled embedding"):
        eng.backward_cond(gy, None, None, d_ctx, d_te)
    eng.backward_ctx(gy, None, None, d_ctx)
    ref_ctx = d_ctx.clone()
    # the tail backward
    eng.set_pooled_grad(True)
    eps1 = fwd()
    g = torch.zeros(8, device="cuda")
    with pytest.raises(SmiError, match="tail backward is not offered"):
        eng.backward_tail(gy[1:], g, g)
    eng.backward_cond(gy, None, None, d_ctx, d_te)
    assert torch.equal(eps1, eps0) and torch.equal(d_ctx, ref_ctx)
    check_bar("after the refusals", d_te.cpu(), R.plain_refs(), R.plain_refs(torch.float16))
    # the switch needs the context gradient's
    eng.set_ctx_grad(False)
    with pytest.raises(SmiError, match="context gradient is off"):
        _native.check(_native.lib().smi_unet_pooled_grad(eng.handle, 1), "smi_unet_pooled_grad")

    # c3lier puts an adaptor on every time_emb_proj: refused, the site named; the engine still trains
    ocfg, ou, onet, puc, pnetc = build_pair(R.MODEL, torch.float16, method="noxattn", c3lier=True)
    flat, n_down, _ = pnetc.engine_params()
    engc = puc._ensure_engine(R.N, R.HW, R.HW, 77)
    engc.set_ctx_grad(True)
    with pytest.raises(SmiError, match=r"adaptor on a time_emb_proj: .*resnets\.0\.time_emb_proj"):
        engc.set_pooled_grad(True)
    engc.set_ctx_grad(False)
    epsc = engc.forward(x.cuda(), R.T, ctx.cuda().half(), te, ti, flat[:n_down].detach(), flat[n_down:].detach(), 1.0, True)
    gc = torch.zeros_like(flat)
    engc.backward(gy, gc[:n_down], gc[n_down:])
    assert torch.isfinite(epsc).all() and torch.isfinite(gc).all() and float(gc.abs().max()) > 0
