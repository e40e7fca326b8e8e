"""Shared references of the context-gradient tests (tests/test_ctx_grad_gpu.py, tests/test_ctx_grad_refs_cpu.py): the CPU
oracle's d(loss)/d(ctx) through its own autograd, in fp32 and with the forward rounded to a storage dtype, and the split of
that gradient into the contributions of the single cross-attention blocks (backward hooks on attn2.to_k / attn2.to_v;
oracle/ itself is untouched).

Inputs are the recipe of tests/test_engine_gpu.py: n = 2, 16 x 16 latents, ctx_len 77, t = 499.  The output gradient is
randn x 1e-4 with sample 1 multiplied by 8, so that the two samples get different power-of-two loss scales in the engine."""
import contextlib
import dataclasses

import torch

from oracle import unet_ref as OU
from tests.test_engine_gpu import CFGS, inputs

T = 499.0
N, HW = 2, 16
BAR_FACTOR, BAR_FLOOR = 3.0, 1e-4  # d_ctx bar = 3 x e_q + 1e-4 (relative L2 over the whole tensor)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def output_grad(boost=True):
    gy = torch.randn(N, 4, HW, HW, generator=torch.Generator().manual_seed(9)) * 1e-4
    if boost:
        gy[1] *= 8
    return gy


def plain_oracle(model):
    return OU.init_synthetic_(OU.UNet2DConditionModel(CFGS[model]()), seed=0).requires_grad_(False).eval()


def build_plain_pair(model, dtype):
    """(ocfg, oracle UNet, product UNet on the GPU) with no LoRA network on either."""
    import sliders_conceptmod_amd.unet as PU
    ocfg = CFGS[model]()
    ou = plain_oracle(model)
    pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
    pu.load_state_dict(ou.state_dict())
    return ocfg, ou, pu.to("cuda", dtype).requires_grad_(False).eval()


def oracle_d_ctx(ou, onet, x, ctx, add, gy, storage=None):
    """ctx.requires_grad_() on the oracle, (out * gy).sum().backward(); storage: the forward's rounding dtype or None."""
    c = ctx.clone().requires_grad_()
    ou.storage_dtype = storage
    try:
        with (onet if onet is not None else contextlib.nullcontext()):
            out = ou(x, T, c, add).sample
    finally:
        ou.storage_dtype = None
    (out * gy).sum().backward()
    return c.grad.detach()


_CACHE = {}


def plain_refs(model, storage=None, boost=True):
    """d_ctx of the network-free oracle on the standard inputs (cached: computed once per process and left unchanged)."""
    key = (model, storage, boost)
    if key not in _CACHE:
        ou = plain_oracle(model)
        x, ctx, add = inputs(CFGS[model](), N, HW)
        _CACHE[key] = oracle_d_ctx(ou, None, x, ctx, add, output_grad(boost), storage)
    return _CACHE[key]


def bar(e_q):
    return BAR_FACTOR * e_q + BAR_FLOOR


def block_contributions(model, boost=True):
    """({block name: {'k': its to_k term of d_ctx, 'v': its to_v term}}, the full d_ctx), fp32 oracle, no network."""
    ou = plain_oracle(model)
    x, ctx, add = inputs(CFGS[model](), N, HW)
    parts, handles = {}, []
    for name, m in ou.named_modules():
        if name.endswith("attn2.to_k") or name.endswith("attn2.to_v"):
            blk, which = name.rsplit(".attn2.to_", 1)

            def hook(_mod, grad_in, _grad_out, blk=blk, which=which):
                parts.setdefault(blk, {})[which] = grad_in[0].detach().clone()

            handles.append(m.register_full_backward_hook(hook))
    full = oracle_d_ctx(ou, None, x, ctx, add, output_grad(boost))
    for h in handles:
        h.remove()
    return parts, full
