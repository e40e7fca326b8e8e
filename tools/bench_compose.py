"""Time slider composition at real shapes on the MI355X: SD-XL widths, 1024^2 (128 x 128 latents), synthetic weights, seeded
random sliders and inputs, one UNet pass = one denoising step of the CFG-doubled batch.

    python tools/bench_compose.py [--rounds 5] [--iters 2] [--hw 128] [--out bench_out/compose.json]

Three comparisons, each with its arms alternating in one process after a warm-up of every shape, timed with device events
around the passes of an arm:
  (a) grid   one denoising step of a 3 x 3 grid of scales on a stack of two rank-4 sliders (R = 8) as ONE 18-sample
             smi_unet_forward_compose against nine 2-sample compose passes on the same engine;
  (b) stack  a `--small`-sample compose pass of that stack against the plain forward of ONE rank-8 adaptor on the same sites
             (what the column table costs);
  (c) rank   a `--small`-sample compose pass at R = 20 (ranks 4 + 16: past the MFMA epilogue's rank 16, the VALU form)
             against R = 16 (ranks 8 + 8).
Engines are driven directly (one per adaptor layout, sharing the UNet's weights).  An engine sizes its saved-pass arena for
every adapted sample, so the 18-sample SD-XL engine of (a) fills most of the card: (b) and (c) run after it is released."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_slider(unet, method, rank, alpha, seed):
    """A LoRA state dict as LoRANetwork.save_weights writes it, with random operands (lora_up ~ 0.05 randn)."""
    from sliders_conceptmod_amd import lora as LM
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, _path, child in LM.select_targets(unet, method, LM.DEFAULT_TARGET_REPLACE, LM.LORA_PREFIX_UNET, "_"):
        _r, dshape, ushape = LM.lora_shapes(child, rank)
        sd[f"{name}.alpha"] = torch.tensor(float(alpha))
        sd[f"{name}.lora_down.weight"] = torch.randn(dshape, generator=g) * dshape[1] ** -0.5
        sd[f"{name}.lora_up.weight"] = torch.randn(ushape, generator=g) * 0.05
    return sd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="synthetic://sdxl")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--hw", type=int, default=128)
    ap.add_argument("--small", type=int, default=4, help="samples of the passes of comparisons (b) and (c)")
    ap.add_argument("--method", default="noxattn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sliders_conceptmod_amd import _native, model_util
    from sliders_conceptmod_amd.compose import SliderStack
    dt = torch.float16
    _tok, _enc, unet, _sched = model_util.load_models(a.model, "ddim", weight_dtype=dt, xl=True)
    unet = unet.to("cuda", dt).requires_grad_(False).eval()
    state = {k: v.detach() for k, v in unet.state_dict().items()}
    cells = 9
    n = cells * 2
    g = torch.Generator().manual_seed(0)
    cfg = unet.cfg
    x = torch.randn(n, 4, a.hw, a.hw, generator=g).cuda()
    ctx = torch.randn(n, 77, cfg.cross_attention_dim, generator=g).cuda().to(dt)
    pdim = cfg.projection_class_embeddings_input_dim - 6 * cfg.addition_time_embed_dim
    te = torch.randn(n, pdim, generator=g).cuda().to(dt)
    ti = torch.tensor([[a.hw * 8.0, a.hw * 8.0, 0, 0, a.hw * 8.0, a.hw * 8.0]] * n).cuda()
    out = torch.empty(n, 4, a.hw, a.hw, device="cuda")

    def layout(ranks, batch):
        stack = SliderStack(unet, [random_slider(unet, a.method, r, 1.0, 10 + i) for i, r in enumerate(ranks)])
        eng = _native.Engine(cfg, dt, state, stack.engine_sites(), batch, a.hw, a.hw, 77, x.device)
        flat, nd, _ = stack.engine_params()
        return stack, eng, flat[:nd], flat[nd:]

    def measure(arms):
        for f in arms.values():  # warm-up: every shape, the GEMM tile tuner
            f()
            f()
        torch.cuda.synchronize()
        res = {k: [] for k in arms}
        for r in range(a.rounds):
            for k, f in arms.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.iters):
                    f()
                t1.record()
                torch.cuda.synchronize()
                res[k].append(t0.elapsed_time(t1) / a.iters)
            print(f"round {r}: " + ", ".join(f"{k} {v[-1]:.2f} ms" for k, v in res.items()), flush=True)
        return res

    # (a) the 3 x 3 grid: one engine (the engine sizes its saved-pass arena for every adapted sample, so an 18-sample SD-XL
    # engine at 1024^2 takes most of the card; the other comparisons run after it is released, at batch `small`)
    grid2 = [[float(p), float(q)] for p in (-2, 0, 2) for q in (-2, 0, 2)]
    rows2 = grid2 * 2  # [uncond of every cell ; cond of every cell]
    s8, e8, d8, u8 = layout([4, 4], n)
    pairs = [[t[[c, cells + c]].contiguous() for t in (x, ctx, te, ti)] for c in range(cells)]  # a cell's CFG pair

    def nine2():
        for c, (xc, cc, tec, tic) in enumerate(pairs):
            e8.forward_compose(xc, 499.0, cc, tec, tic, d8, u8, s8.ranks, [grid2[c], grid2[c]], out=out[:2])

    res = measure({
        f"grid_one_pass_{n}": lambda: e8.forward_compose(x, 499.0, ctx, te, ti, d8, u8, s8.ranks, rows2, out=out),
        "grid_nine_passes_2": nine2,
    })
    e8.close()
    del e8, d8, u8, s8
    torch.cuda.empty_cache()
    # (b), (c): `small` samples (cells of the grid, CFG-doubled), one engine per adaptor layout
    m = a.small
    xs, cs, tes, tis, outs = x[:m].contiguous(), ctx[:m].contiguous(), te[:m].contiguous(), ti[:m].contiguous(), out[:m]
    rows = (grid2 * 2)[:m]
    lay = {k: layout(r, m) for k, r in (("R8", [4, 4]), ("single8", [8]), ("R20", [4, 16]), ("R16", [8, 8]))}

    def compose_arm(k):
        st, eng, dn, up = lay[k]
        return lambda: eng.forward_compose(xs, 499.0, cs, tes, tis, dn, up, st.ranks, rows, out=outs)

    _st, e1, d1, u1 = lay["single8"]
    res.update(measure({
        f"stack_R8_{m}": compose_arm("R8"),
        f"single_rank8_plain_{m}": lambda: e1.forward(xs, 499.0, cs, tes, tis, d1, u1, 1.0, False, out=outs),
        f"stack_R20_{m}": compose_arm("R20"),
        f"stack_R16_{m}": compose_arm("R16"),
    }))
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    summary = {
        "a_grid_one_pass_over_nine_passes": med[f"grid_one_pass_{n}"] / med["grid_nine_passes_2"],
        "b_stack_R8_over_single_rank8": med[f"stack_R8_{m}"] / med[f"single_rank8_plain_{m}"],
        "c_R20_over_R16": med[f"stack_R20_{m}"] / med[f"stack_R16_{m}"],
    }
    o = {"model": a.model, "latent": a.hw, "grid_samples": n, "small_samples": m, "method": a.method, "rounds": a.rounds,
         "iters": a.iters, "ms": res, "median_ms": med, "ratios_of_medians": summary}
    print(json.dumps(o))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(o, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
