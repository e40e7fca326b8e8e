"""Shared references of the pooled-embedding gradient tests (tests/test_pooled_grad_gpu.py,
tests/test_pooled_grad_refs_cpu.py): the CPU oracle's d(loss)/d(text_embeds) through its own autograd, in fp32 and with the
forward rounded to a storage dtype, and the split of that gradient into the terms of the single time_emb_proj layers
(backward hooks on every resnet's time_emb_proj, each term then taken back through the embedding chain, which is the same
for all of them; oracle/ itself is untouched).

Model, inputs, output gradient and bar are those of tests/ctx_grad_refs.py: tiny_sdxl, n = 2, 16 x 16 latents, ctx_len 77,
t = 499, randn x 1e-4 with sample 1 multiplied by 8, 3 x e_q + 1e-4."""
import contextlib

import torch
import torch.nn.functional as F

from tests import ctx_grad_refs as R
from tests.test_engine_gpu import CFGS, inputs

MODEL = "tiny_sdxl"
T, N, HW = R.T, R.N, R.HW
rel, bar, output_grad, plain_oracle = R.rel, R.bar, R.output_grad, R.plain_oracle


def std_inputs():
    return inputs(CFGS[MODEL](), N, HW)


def oracle_grads(ou, onet, x, ctx, add, gy, storage=None):
    """(d_ctx, d_text_embeds) of (out * gy).sum() on the oracle; storage: the forward's rounding dtype or None."""
    c = ctx.clone().requires_grad_()
    te = add["text_embeds"].clone().requires_grad_()
    ou.storage_dtype = storage
    try:
        with (onet if onet is not None else contextlib.nullcontext()):
            out = ou(x, T, c, {"text_embeds": te, "time_ids": add["time_ids"]}).sample
    finally:
        ou.storage_dtype = None
    (out * gy).sum().backward()
    return c.grad.detach(), te.grad.detach()


_CACHE = {}


def plain_refs(storage=None, boost=True):
    """d(text_embeds) of the network-free oracle on the standard inputs (cached: computed once per process, left unchanged)."""
    key = (storage, boost)
    if key not in _CACHE:
        x, ctx, add = std_inputs()
        _CACHE[key] = oracle_grads(plain_oracle(MODEL), None, x, ctx, add, output_grad(boost), storage)[1]
    return _CACHE[key]


def embedding_chain(ou, text_embeds, time_ids, n):
    """silu(emb) as a function of text_embeds: the fp32 oracle's own modules in the order of its forward."""
    t = torch.full((n,), T, dtype=torch.float32)
    emb = ou.time_embedding(ou.time_proj(t))
    te = ou.add_time_proj(time_ids.float().flatten()).reshape(n, -1)
    return F.silu(emb + ou.add_embedding(torch.cat([text_embeds, te], dim=-1)))


def term_contributions(boost=True):
    """({resnet name: its time_emb_proj's term of d(text_embeds)}, the full d(text_embeds)), fp32 oracle, no network."""
    ou = plain_oracle(MODEL)
    x, ctx, add = std_inputs()
    grads, handles = {}, []
    for name, m in ou.named_modules():
        if name.endswith(".time_emb_proj"):

            def hook(_mod, grad_in, _grad_out, blk=name[:-len(".time_emb_proj")]):
                grads[blk] = grad_in[0].detach().clone()  # d(loss)/d(silu(emb)) through this projection alone

            handles.append(m.register_full_backward_hook(hook))
    full = oracle_grads(ou, None, x, ctx, add, output_grad(boost))[1]
    for h in handles:
        h.remove()
    te = add["text_embeds"].clone().requires_grad_()
    temb = embedding_chain(ou, te, add["time_ids"], N)
    parts = {b: torch.autograd.grad(temb, te, g, retain_graph=True)[0] for b, g in grads.items()}
    return parts, full
