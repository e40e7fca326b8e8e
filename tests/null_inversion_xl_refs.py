"""CPU restatement of SD-XL null-text optimisation (sliders_conceptmod_amd/null_inversion_xl.py: the notebook's
NullInversion.ddim_loop and .null_optimization with the added conditioning carried through, and the unconditional pooled
embedding as a second Adam parameter) on the fp32 oracle UNet with torch autograd: the reference of
tests/test_null_inversion_xl_gpu.py.  Recipe: that of tests/null_inversion_refs.py on tiny_sdxl -- 8 x 8 latents, 4 DDIM
steps, 5 inner steps, early stop disabled, guidance 7.5; seed 5 draws x0, uncond, cond, pooled_uncond [1, P], pooled_cond
[1, P] in this order; time_ids = [64, 64, 0, 0, 64, 64]."""
import torch
import torch.nn.functional as nnf

from sliders_conceptmod_amd.null_inversion import step_coefficients
from tests.null_inversion_refs import GUIDANCE, HW, INNER, NO_EARLY_STOP, STEPS, ddim_scheduler  # noqa: F401

MODEL = "tiny_sdxl"
IMAGE_SIZE = 64
TIME_IDS = [64.0, 64.0, 0.0, 0.0, 64.0, 64.0]
GOLDEN = "null_inversion_xl_oracle.json"  # under tests/golden/: {"timesteps", "losses_pooled_off", "losses_pooled_on"}


def recipe(ctx_dim, pooled_dim, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(1, 4, HW, HW, generator=g)
    uncond = torch.randn(1, 77, ctx_dim, generator=g)
    cond = torch.randn(1, 77, ctx_dim, generator=g)
    pooled_u = torch.randn(1, pooled_dim, generator=g)
    pooled_c = torch.randn(1, pooled_dim, generator=g)
    return x0, uncond, cond, pooled_u, pooled_c


def pooled_dim(cfg):
    return cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim


def oracle_null_optimization(ou, x0, uncond, cond, pooled_u, pooled_c, optimize_pooled, steps=STEPS, inner=INNER, g=GUIDANCE,
                             epsilon=NO_EARLY_STOP, only_first=False):
    """-> (losses [timestep][inner step], timesteps); only_first: stop after the first timestep's inner loop"""
    sched = ddim_scheduler(steps)
    tid = torch.tensor([TIME_IDS])
    unet = lambda x, t, c, p: ou(x, float(t), c, {"text_embeds": p, "time_ids": tid}).sample
    with torch.no_grad():
        latents = [x0]
        lat = x0.clone()
        for i in range(steps):
            t = int(sched.timesteps[len(sched.timesteps) - i - 1])
            cx, ce = step_coefficients(sched, t, True)
            lat = cx * lat + ce * unet(lat, t, cond, pooled_c)
            latents.append(lat)
    losses, ts = [], []
    cur = latents[-1]
    u, p = uncond, pooled_u
    for i in range(steps):
        u = u.clone().detach().requires_grad_(True)
        p = p.clone().detach().requires_grad_(optimize_pooled)
        opt = torch.optim.Adam([u, p] if optimize_pooled else [u], lr=1e-2 * (1. - i / 100.))
        prev = latents[len(latents) - i - 2]
        t = int(sched.timesteps[i])
        cx, ce = step_coefficients(sched, t, False)
        with torch.no_grad():
            eps_c = unet(cur, t, cond, pooled_c)
        losses.append([])
        ts.append(t)
        for _j in range(inner):
            eps_u = unet(cur, t, u, p)
            rec = cx * cur + ce * (eps_u + g * (eps_c - eps_u))
            loss = nnf.mse_loss(rec, prev)
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses[-1].append(loss.item())
            if loss.item() < epsilon + i * 2e-5:
                break
        if only_first:
            break
        with torch.no_grad():
            e_u, e_c = unet(cur, t, u.detach(), p.detach()), unet(cur, t, cond, pooled_c)
            cur = cx * cur + ce * (e_u + g * (e_c - e_u))
    return losses, ts


if __name__ == "__main__":  # python -m tests.null_inversion_xl_refs: rewrites the golden file
    import json
    import os
    from tests.ctx_grad_refs import plain_oracle
    ou = plain_oracle(MODEL)
    args = recipe(ou.cfg.cross_attention_dim, pooled_dim(ou.cfg))
    off, ts = oracle_null_optimization(ou, *args, optimize_pooled=False)
    on, ts_on = oracle_null_optimization(ou, *args, optimize_pooled=True)
    assert ts == ts_on
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    json.dump({"timesteps": ts, "losses_pooled_off": off, "losses_pooled_on": on}, open(path, "w"), indent=1)
    print(path)
