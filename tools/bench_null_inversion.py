"""Time one null-text inversion at real shapes on the MI355X: SD-1.x, 512^2 (64 x 64 latents), synthetic weights and a
seeded random latent / embeddings, DDIM steps x inner steps with the early stop disabled (every inner step runs).

    python tools/bench_null_inversion.py [--steps 50] [--inner 10] [--rounds 3] [--out bench_out/null_inversion.json]

`fused=True` (smi_unet_backward_ctx + smi_nulltext_loss + smi_clip_adamw) and `fused=False` (torch autograd through the same
UNet) run in the same process, alternating `--rounds` times after one warm-up each; a time is a host clock around
null_optimization ending in a device synchronise, divided by the inner steps taken (so it carries the per-timestep
conditional pass and guided step, 2 of 12 UNet passes at 10 inner steps).  Then, with SMI_PROF_DUMP=1 in the environment,
one profiled timestep of the fused route: per-class device time (smi_profile_read) and, on stderr, the per-shape table whose
`f32` GEMM of N = cross_attention_dim and K = sum of the k|v widths is the d_ctx GEMM and whose `attn_bwd dK|dV` lines are the
cross-attention backward launches that produce dK / dV (`no dQ`: the first block of the net).

`--base xl`: the SD-XL loop (null_inversion_xl.NullInversionXL; defaults synthetic://sdxl, 1024^2 = 128 x 128 latents) with
four arms -- fused and autograd, the pooled optimisation on and off -- alternating `--rounds` times; the profiled timestep
is the fused route with the pooled optimisation on, whose `f32` GEMM of M = 1, N = 1280 and K = the sum of the time_emb_proj
widths is the grouped d(temb_act) product of smi_unet_backward_cond."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", choices=["1.4", "xl"], default="1.4")
    ap.add_argument("--model", default=None, help="default synthetic://sd1x, with --base xl synthetic://sdxl")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--hw", type=int, default=None, help="latent side: default 64, with --base xl 128")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    xl = a.base == "xl"
    a.model = a.model or ("synthetic://sdxl" if xl else "synthetic://sd1x")
    a.hw = a.hw or (128 if xl else 64)
    if xl:
        return main_xl(a)
    from sliders_conceptmod_amd import model_util
    from sliders_conceptmod_amd.null_inversion import NullInversion
    _tok, _enc, unet, sched = model_util.load_models(a.model, "ddim", weight_dtype=torch.float16)
    unet = unet.to("cuda", torch.float16).requires_grad_(False).eval()
    g = torch.Generator().manual_seed(0)
    D = unet.cfg.cross_attention_dim
    x0 = torch.randn(1, 4, a.hw, a.hw, generator=g).cuda()
    ctx = torch.randn(2, 77, D, generator=g).cuda()
    inv = {f: NullInversion(unet, sched, num_ddim_steps=a.steps, guidance_scale=7.5, fused=f) for f in (True, False)}
    for i in inv.values():
        i.context = ctx
    latents = inv[True].ddim_loop(x0)
    torch.cuda.synchronize()

    def run(fused, steps_limit=None):
        i = inv[fused]
        if steps_limit is not None:  # a short run: warm-up / profile
            i.num_ddim_steps = steps_limit
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i.null_optimization(latents, a.inner, -1.0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = sum(len(l) for l in i.losses)
        i.num_ddim_steps = a.steps
        return dt, n, [l[0] for l in i.losses[:2]], [l[-1] for l in i.losses[:2]]

    for f in (True, False):  # warm-up: every shape, the GEMM tile tuner
        run(f, 2)
    res = {"fused": [], "autograd": []}
    for r in range(a.rounds):
        for f in (True, False):
            dt, n, first, last = run(f)
            ms = 1e3 * dt / n
            res["fused" if f else "autograd"].append(ms)
            print(f"round {r} fused={f}: {dt:.2f} s for {n} inner steps = {ms:.2f} ms per inner step; first losses {first} "
                  f"-> {last}", flush=True)
    # profiled timestep of the fused route
    eng = unet._engine
    eng.profile_enable(True)
    dt, n, _, _ = run(True, 1)
    prof = eng.profile_read()
    eng.profile_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    print(f"profiled fused timestep ({n} inner steps + conditional pass + guided step): device time by class, ms "
          f"(total {tot:.2f}): " + ", ".join(f"{k} {v['ms']:.2f}" for k, v in prof.items()), flush=True)
    out = {"model": a.model, "steps": a.steps, "inner": a.inner, "latent": a.hw, "ms_per_inner_step": res,
           "profiled_timestep_ms_by_class": {k: v["ms"] for k, v in prof.items()}, "profiled_inner_steps": n}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


def main_xl(a):
    from sliders_conceptmod_amd import model_util
    from sliders_conceptmod_amd.null_inversion_xl import NullInversionXL
    _tok, _enc, unet, sched = model_util.load_models(a.model, "ddim", weight_dtype=torch.float16, xl=True)
    unet = unet.to("cuda", torch.float16).requires_grad_(False).eval()
    g = torch.Generator().manual_seed(0)
    cfg = unet.cfg
    P = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    x0 = torch.randn(1, 4, a.hw, a.hw, generator=g).cuda()
    ctx = torch.randn(2, 77, cfg.cross_attention_dim, generator=g).cuda()
    pooled = torch.randn(2, P, generator=g).cuda()
    inv = {f: NullInversionXL(unet, sched, num_ddim_steps=a.steps, guidance_scale=7.5, fused=f, image_size=8 * a.hw)
           for f in (True, False)}
    for i in inv.values():
        i.context, i.pooled = ctx, pooled
    latents = inv[True].ddim_loop(x0)
    torch.cuda.synchronize()

    def run(fused, pool, steps_limit=None):
        i = inv[fused]
        if steps_limit is not None:
            i.num_ddim_steps = steps_limit
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        i.null_optimization(latents, a.inner, -1.0, optimize_pooled=pool)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = sum(len(l) for l in i.losses)
        i.num_ddim_steps = a.steps
        return dt, n, [l[0] for l in i.losses[:2]], [l[-1] for l in i.losses[:2]]

    arms = [(f, p) for f in (True, False) for p in (True, False)]
    name = lambda f, p: ("fused" if f else "autograd") + ("_pooled" if p else "_sequence_only")
    for f, p in arms:  # warm-up: every shape, the GEMM tile tuner, both gradient buffers
        run(f, p, 2)
    res = {name(f, p): {"ms_per_inner_step": [], "s_per_inversion": []} for f, p in arms}
    for r in range(a.rounds):
        for f, p in arms:
            dt, n, first, last = run(f, p)
            res[name(f, p)]["ms_per_inner_step"].append(1e3 * dt / n)
            res[name(f, p)]["s_per_inversion"].append(dt)
            print(f"round {r} {name(f, p)}: {dt:.2f} s per inversion, {n} inner steps = {1e3 * dt / n:.2f} ms per inner step; "
                  f"first losses {first} -> {last}", flush=True)
    eng = unet._engine
    eng.profile_enable(True)
    dt, n, _, _ = run(True, True, 1)
    prof = eng.profile_read()
    eng.profile_enable(False)
    tot = sum(v["ms"] for v in prof.values())
    print(f"profiled fused timestep, pooled on ({n} inner steps + conditional pass + guided step): device time by class, ms "
          f"(total {tot:.2f}): " + ", ".join(f"{k} {v['ms']:.2f}" for k, v in prof.items()), flush=True)
    out = {"model": a.model, "steps": a.steps, "inner": a.inner, "latent": a.hw, "arms": res,
           "profiled_timestep_ms_by_class": {k: v["ms"] for k, v in prof.items()}, "profiled_inner_steps": n}
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
