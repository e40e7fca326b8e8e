"""References for slider composition (sliders_conceptmod_amd/compose.py), in plain torch on the CPU:

  * the stacked layout of K state dicts (what the stack kernel must write, bit for bit);
  * the column-multiplied skinny product;
  * the oracle pair: two `LoRANetworkRef`s on ONE oracle UNet -- each patches `forward`, the deltas add, which is how
    the reference composes -- and the same two sliders as state dicts for the product side.
"""
import dataclasses
from typing import Dict, List, Sequence

import torch

from oracle import slider_ref as R
from oracle import unet_ref as OU

CFGS = {"tiny_sd1x": OU.tiny_sd1x_config, "tiny_sdxl": OU.tiny_sdxl_config}


# (train method, rank, alpha) of slider a and slider b
PAIRS = {
    "disjoint": (("noxattn", 4, 1.0), ("xattn", 8, 4.0)),
    "overlap": (("full", 4, 1.0), ("noxattn", 8, 4.0)),
}
PAIR_44 = (("full", 4, 1.0), ("noxattn", 4, 1.0))  # R = 8: 24 fused q|k|v rows, the 32-row class
SEEDS = (1, 5)          # torch.manual_seed before each network's init (lora_down)
UP_SEED = 2             # lora_up ~ 0.05 randn, one generator over slider a then slider b
SCALES = (2.0, -2.0)


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def oracle_state(onet) -> Dict[str, torch.Tensor]:
    """The state dict LoRANetwork.save_weights writes, from an oracle network."""
    sd = {}
    for l in onet.unet_loras:
        sd[f"{l.lora_name}.alpha"] = l.alpha.detach().clone()
        sd[f"{l.lora_name}.lora_down.weight"] = l.lora_down.weight.detach().clone()
        sd[f"{l.lora_name}.lora_up.weight"] = l.lora_up.weight.detach().clone()
    return sd


def oracle_pair(model: str, pair, c3lier: bool = False):
    """(config, oracle UNet, [network a, network b] chained on it, [state dict a, state dict b])."""
    ocfg = CFGS[model]()
    ou = OU.init_synthetic_(OU.UNet2DConditionModel(ocfg), seed=0).requires_grad_(False).eval()
    g = torch.Generator().manual_seed(UP_SEED)
    nets = []
    for (method, rank, alpha), seed in zip(pair, SEEDS):
        torch.manual_seed(seed)
        kw = {"target_replace": R.C3LIER_TARGET_REPLACE} if c3lier else {}
        net = R.LoRANetworkRef(ou, rank, 1.0, alpha, method, **kw)
        with torch.no_grad():
            for l in net.unet_loras:
                l.lora_up.weight.copy_(torch.randn(l.lora_up.weight.shape, generator=g) * 0.05)
        net.requires_grad_(False)
        nets.append(net)
    return ocfg, ou, nets, [oracle_state(n) for n in nets]


def product_unet(ocfg, ou, dtype=None, device="cpu"):
    import sliders_conceptmod_amd.unet as PU
    pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
    pu.load_state_dict(ou.state_dict())
    if dtype is not None:
        pu = pu.to(device, dtype)
    return pu.requires_grad_(False).eval()


def oracle_eps(ou, nets, scales: Sequence[float], x, t, ctx, add, storage_dtype=None):
    """eps of the oracle with network k entered at scales[k] (None: that network stays off)."""
    for net, s in zip(nets, scales):
        if s is None:
            net.__exit__(None, None, None)
        else:
            net.set_lora_slider(s)
            net.__enter__()
    ou.storage_dtype = storage_dtype
    try:
        with torch.no_grad():
            return ou(x, t, ctx, add).sample
    finally:
        ou.storage_dtype = None
        for net in nets:
            net.set_lora_slider(1)
            net.__exit__(None, None, None)


def inputs(ocfg, n, hw, seed=3):
    """tests/test_engine_gpu.py inputs()."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 4, hw, hw, generator=g)
    ctx = torch.randn(n, 77, ocfg.cross_attention_dim, generator=g)
    add = None
    if ocfg.addition_embed_type == "text_time":
        pdim = ocfg.projection_class_embeddings_input_dim - 6 * ocfg.addition_time_embed_dim
        add = {"text_embeds": torch.randn(n, pdim, generator=g),
               "time_ids": torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * n)}
    return x, ctx, add


# ---- the stacked layout ------------------------------------------------------------------------------------------
def stack_site_reference(downs: Sequence, ups: Sequence, ranks: Sequence[int], coefs: Sequence[float], row_len: int,
                         n_out: int):
    """One site: downs[k] [r_k, row_len] / ups[k] [n_out, r_k] (None: slider k does not adapt the site) ->
    (down [R, row_len], up [n_out, R]) with up's block k = fp32(coef_k) * up_k (ONE fp32 multiply) and zero blocks for the
    absent sliders."""
    R_ = sum(ranks)
    down = torch.zeros(R_, row_len, dtype=torch.float32)
    up = torch.zeros(n_out, R_, dtype=torch.float32)
    c = 0
    for d, u, r, coef in zip(downs, ups, ranks, coefs):
        if d is not None:
            down[c:c + r] = d.detach().float().reshape(r, row_len)
            up[:, c:c + r] = torch.tensor(coef, dtype=torch.float32) * u.detach().float().reshape(n_out, r)
        c += r
    return down, up


def stack_reference(plan, sliders, coefs_of_site):
    """The flat stacked buffers (down, up) of a compose.StackPlan; coefs_of_site(site) -> [c_k]."""
    down = torch.zeros(plan.n_down, dtype=torch.float32)
    up = torch.zeros(plan.n_up, dtype=torch.float32)
    for s in plan.sites:
        ds = [p.state[f"{s.lora_name}.lora_down.weight"] if here else None for p, here in zip(sliders, s.present)]
        us = [p.state[f"{s.lora_name}.lora_up.weight"] if here else None for p, here in zip(sliders, s.present)]
        d, u = stack_site_reference(ds, us, s.ranks, coefs_of_site(s), s.row_len, s.n_out)
        down[s.off_down:s.off_down + d.numel()] = d.reshape(-1)
        up[s.off_up:s.off_up + u.numel()] = u.reshape(-1)
    return down, up


def col_mul_reference(out: torch.Tensor, table: torch.Tensor, rows_per_mul: int, period: int) -> torch.Tensor:
    """out[m][c] * table[m // rows_per_mul][c % period] in fp32 (one multiply per element)."""
    m = torch.arange(out.shape[0], device=out.device) // rows_per_mul
    c = torch.arange(out.shape[1], device=out.device) % period
    return out * table[m][:, c]
