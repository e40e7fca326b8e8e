"""Saved passes and their backwards of the three differentiated engines (UNet, CLIP text tower with LoRA sites, MMDiT) on their
tiny models -> a SHA-256 of every output buffer and of both flat gradient buffers, one line each.  Every item runs twice in
the process: the second backward finds its weight-gradient job table already on the device, and in the second round an adapted
no-grad forward (other multipliers) runs between the saved forward and its backward.  Run under SMI_LIB=<another build> to
cross-check two builds of the library bit for bit; --out keeps the buffers themselves for a max |difference|."""
import argparse, dataclasses, hashlib, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KEPT = {}


def digest(name, t):
    t = t.detach().contiguous().cpu()
    KEPT[name] = t
    print(f"{hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()}  {name}", flush=True)


def unet_items():
    import sliders_conceptmod_amd.lora as L
    import sliders_conceptmod_amd.unet as PU
    from oracle import unet_ref as OU
    dt, n, na, hw = torch.float16, 3, 2, 16
    ocfg = OU.tiny_sdxl_config()
    ou = OU.init_synthetic_(OU.UNet2DConditionModel(ocfg), seed=0)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 4, hw, hw, generator=g).cuda()
    ctx = torch.randn(n, 77, ocfg.cross_attention_dim, generator=g).to(dt).cuda()
    pdim = ocfg.projection_class_embeddings_input_dim - 6 * ocfg.addition_time_embed_dim
    te = torch.randn(n, pdim, generator=g).to(dt).cuda()
    ti = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]] * n).cuda()
    d_eps = (torch.randn(na, 4, hw, hw, generator=g) * 1e-4 * torch.tensor([1.0, 3.0]).view(na, 1, 1, 1)).cuda()
    for form in ("lora", "c3lier"):
        pu = PU.UNet2DConditionModel(PU.UNetConfig(**dataclasses.asdict(ocfg)))
        pu.load_state_dict(ou.state_dict())
        pu = pu.to("cuda", dt).requires_grad_(False).eval()
        torch.manual_seed(1)
        targets = L.UNET_TARGET_REPLACE_MODULE_TRANSFORMER + (L.UNET_TARGET_REPLACE_MODULE_CONV if form == "c3lier" else [])
        net = L.LoRANetwork(pu, rank=4, multiplier=1.0, alpha=1.0, train_method="noxattn", target_replace=targets)
        with torch.no_grad():
            net.flat_up.copy_(torch.randn(net.flat_up.shape, generator=torch.Generator().manual_seed(2)) * 0.05)
        net.to("cuda")
        flat, n_down, _ = net.engine_params()
        down, up = flat[:n_down], flat[n_down:]
        eng = pu._ensure_engine(n, hw, hw, 77, n_adapted=na)
        # (multipliers of the saved pass, of the no-grad pass in between): per sample on Linear sites, one scalar with conv sites
        mults, other = ([1.0, -2.0], [0.5, 0.25]) if form == "lora" else (1.5, 0.5)
        kinds = ("full", "tail", "ctx") if form == "lora" else ("full",)
        for kind in kinds:
            eng.set_ctx_grad(kind == "ctx")
            for rnd in (1, 2):
                tag = f"unet/{form}/{kind}/round{rnd}"
                digest(f"{tag}/eps", eng.forward(x, 499.0, ctx, te, ti, down, up, mults, True, n_adapted=na))
                if rnd == 2:
                    digest(f"{tag}/eps_between", eng.forward(x, 250.0, ctx, te, ti, down, up, other, False, n_adapted=na))
                gd, gu = torch.zeros_like(down), torch.zeros_like(up)
                if kind == "full":
                    eng.backward(d_eps, gd, gu)
                elif kind == "tail":
                    eng.backward_tail(d_eps[1:].contiguous(), gd, gu)
                else:
                    d_ctx = torch.empty(na, 77, ocfg.cross_attention_dim, dtype=torch.float32, device="cuda")
                    eng.backward_ctx(d_eps, gd, gu, d_ctx)
                    digest(f"{tag}/d_ctx", d_ctx)
                torch.cuda.synchronize()
                digest(f"{tag}/d_down", gd)
                digest(f"{tag}/d_up", gu)
        pu._engine.close()


def clip_items():
    import notrigger_refs as R
    from sliders_conceptmod_amd import _native
    dt, rank, alpha = torch.float16, 4, 1.0
    cfg = R.tiny_config()
    state = {k: v.to(dt).cuda().contiguous() for k, v in R.tiny_state(cfg).items()}
    ids = R.tiny_ids(cfg, 2)
    eos = (ids == cfg.eos_token_id).int().argmax(dim=-1)
    names = R.site_names(cfg.num_hidden_layers)
    g = torch.Generator().manual_seed(11)
    lora = R.make_lora(names, cfg.hidden_size, rank, alpha, g)
    d_hidden = torch.randn((2, 77, cfg.hidden_size), generator=g, dtype=torch.float64).float().cuda()
    sites, n_down, n_up = R.flat_layout(names, cfg.hidden_size, rank, alpha)
    down, up = (t.cuda() for t in R.flatten_lora(lora, names))
    eng = _native.ClipLoraEngine(cfg, dt, state, sites, 2, torch.device("cuda"))
    for which in (0, 1):
        for rnd in (1, 2):
            tag = f"clip/which{which}/round{rnd}"
            for k, v in eng.forward_lora(ids, eos, down, up, [1.0, -2.0], save=True).items():
                digest(f"{tag}/{k}", v)
            if rnd == 2:
                for k, v in eng.forward_lora(ids, eos, down, up, [0.5, 0.25], save=False).items():
                    digest(f"{tag}/between/{k}", v)
            gd, gu = torch.zeros(n_down, device="cuda"), torch.zeros(n_up, device="cuda")
            eng.backward(d_hidden, gd, gu, which=which)
            torch.cuda.synchronize()
            digest(f"{tag}/d_down", gd)
            digest(f"{tag}/d_up", gu)
    eng.close()


def mmdit_items():
    import mmdit_bwd_refs as B
    from sliders_conceptmod_amd import mmdit as M
    dt, rank, alpha, h, w, nc, mults = torch.float16, 4, 2.0, 8, 6, 5, [0.0, 1.0, -2.0]
    cfg = M.tiny_sd3_config()
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=3)
    state = {k: v.to(dt).cuda().contiguous() for k, v in model.state_dict().items()}
    names = B.site_names(cfg.num_layers, True)  # the 191-module form: both streams
    lora = B.make_lora(names, cfg.inner_dim, rank, alpha, torch.Generator().manual_seed(11))
    x, ts, ctx, pooled, d_out = B.tiny_inputs(cfg, len(mults), h, w, nc, seed=13)
    sites, n_down, n_up = B.flat_layout(names, cfg.inner_dim, rank, alpha)
    down, up = (t.cuda() for t in B.flatten_lora(lora, names))
    eng = M.MMDiTEngine(cfg, dt, state, sites, len(mults), h, w, nc, torch.device("cuda", 0), trainable=True)
    args = (x.cuda(), list(ts), ctx.to(dt).cuda(), pooled.to(dt).cuda(), down, up)
    for rnd in (1, 2):
        tag = f"mmdit/191/round{rnd}"
        digest(f"{tag}/out_saved", eng.forward_save(*args, mults))
        if rnd == 2:
            digest(f"{tag}/out_between", eng.forward(*args, [0.5, 0.25, -1.0]))
        gd, gu = torch.zeros(n_down, device="cuda"), torch.zeros(n_up, device="cuda")
        eng.backward(d_out.cuda(), gd, gu)
        torch.cuda.synchronize()
        digest(f"{tag}/d_down", gd)
        digest(f"{tag}/d_up", gu)
        digest(f"{tag}/out_plain", eng.forward(*args, mults))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="keep every digested buffer in this .pt file")
    args = ap.parse_args()
    unet_items()
    clip_items()
    mmdit_items()
    if args.out:
        torch.save(KEPT, args.out)


if __name__ == "__main__":
    main()
