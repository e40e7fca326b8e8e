"""CPU restatement of the notebook's null-text optimisation (demo_image_editing.ipynb, NullInversion.ddim_loop and
.null_optimization) on the fp32 oracle UNet with torch autograd: the reference of tests/test_null_inversion_gpu.py.
Recipe: tiny_sd1x, 8 x 8 latents, 4 DDIM steps, 5 inner steps, early stop disabled, guidance 7.5, seeded random cond /
uncond embeddings and start latent."""
import torch
import torch.nn.functional as nnf

from sliders_conceptmod_amd import model_util
from sliders_conceptmod_amd.null_inversion import step_coefficients

STEPS, INNER, GUIDANCE, HW = 4, 5, 7.5, 8
NO_EARLY_STOP = -1.0  # loss < epsilon + i 2e-5 is then never true


def recipe(ctx_dim, seed=5):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(1, 4, HW, HW, generator=g)
    uncond = torch.randn(1, 77, ctx_dim, generator=g)
    cond = torch.randn(1, 77, ctx_dim, generator=g)
    return x0, uncond, cond


def ddim_scheduler(steps=STEPS):
    s = model_util.create_noise_scheduler("ddim")
    s.set_timesteps(steps)
    return s


GOLDEN = "null_inversion_oracle.json"  # under tests/golden/: {"timesteps": [...], "losses": [[...], ...]} of this recipe


XL_TIME_IDS = [64.0, 64.0, 0.0, 0.0, 64.0, 64.0]  # of the SD-XL recipe (tests/null_inversion_xl_refs.py: a 64 x 64 image)


def oracle_null_optimization(ou, x0, uncond, cond, pooled_u=None, pooled_c=None, optimize_pooled=False, steps=STEPS,
                             inner=INNER, g=GUIDANCE, epsilon=NO_EARLY_STOP, only_first=False):
    """-> (losses [timestep][inner step], timesteps); only_first: stop after the first timestep's inner loop.
    pooled_u / pooled_c None: SD-1.x.  Given (SD-XL): they and XL_TIME_IDS go through every UNet call, and optimize_pooled
    makes pooled_u a second Adam parameter."""
    sched = ddim_scheduler(steps)
    tid = torch.tensor([XL_TIME_IDS])
    unet = lambda x, t, c, p: ou(x, float(t), c, None if p is None else {"text_embeds": p, "time_ids": tid}).sample
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
        if p is not None:
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
            e_u, e_c = unet(cur, t, u.detach(), None if p is None else p.detach()), unet(cur, t, cond, pooled_c)
            cur = cx * cur + ce * (e_u + g * (e_c - e_u))
    return losses, ts


if __name__ == "__main__":  # python -m tests.null_inversion_refs: rewrites the golden file
    import json
    import os
    from tests.ctx_grad_refs import plain_oracle
    ou = plain_oracle("tiny_sd1x")
    losses, ts = oracle_null_optimization(ou, *recipe(ou.cfg.cross_attention_dim))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)
    json.dump({"timesteps": ts, "losses": losses}, open(path, "w"), indent=1)
    print(path)
