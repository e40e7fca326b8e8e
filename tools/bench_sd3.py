"""ms per forward of the SD3 MMDiT at `synthetic://sd3` (SD3-medium's architecture, seeded weights), n = 2, at 1024 x 1024 and
512 x 512 images (128 x 128 / 64 x 64 latents), 77 + 256 context tokens, fp16 and bf16: the engine next to a torch-ROCm
restatement of the same network in the same dtype on the same GPU (F.linear, F.layer_norm, scaled_dot_product_attention),
the two arms alternating in one process.  Prints one JSON line per (size, dtype) with the algorithmic FLOP of a forward
(GEMMs and attention, from the shapes) and the TF/s both arms reach, and writes them to --out.  No threshold.

`--train`: the slider step's differentiated part instead -- the trainable engine's saved forward + backward to the rank-4
LoRA matrices of the 96 image-stream sites (`--context_stream`: all 191) next to torch-ROCm autograd through the same
restatement with the same adaptor, same dtype, arms alternating; per (size, dtype) the ms of both arms, the engine's split
into forward_save and backward (forward_save timed alone; backward = the pair minus it), the workspace bytes and the
relative L2 distance of the two gradient vectors.

    python tools/bench_sd3.py [--rounds 3] [--iters 5] [--sizes 1024,512] [--dtypes fp16,bf16] [--out profiles/sd3_forward.json]
    python tools/bench_sd3.py --train [--sizes 512,1024] [--out profiles/sd3_train_n2_ctx333.json]"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sliders_conceptmod_amd import mmdit as M  # noqa: E402


def timed(fn, iters):
    fn()  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def forward_flop(cfg, n, Nx, Nc):
    """2 M N K of every GEMM + 4 B H L^2 D of every attention."""
    d, L = cfg.inner_dim, Nx + Nc
    f = 2.0 * n * Nx * d * (cfg.in_channels * cfg.patch_size ** 2) + 2.0 * n * Nc * d * cfg.joint_attention_dim
    f += 2.0 * n * d * (256 + d + cfg.pooled_projection_dim + d)
    for i in range(cfg.num_layers):
        last = i == cfg.num_layers - 1
        f += 2.0 * n * d * d * (6 + (2 if last else 6))              # modulations
        f += 2.0 * n * L * d * 3 * d + 4.0 * n * L * L * d           # q|k|v of both streams, the joint attention
        for rows in ((Nx,) if last else (Nx, Nc)):
            f += 2.0 * n * rows * d * d * (1 + 8)                    # to_out, ff up and down
    return f + 2.0 * n * d * 2 * d + 2.0 * n * Nx * d * cfg.patch_size ** 2 * cfg.out_channels


def torch_forward(sd, cfg, x, ts, ctx, pooled, lora=None, mults=None):
    """The network in torch ops, in the dtype of `sd` (tests/mmdit_refs.py is the float64 form of the same graph).
    lora: {module path: (down [r, in], up [out, r], alpha / r)} fp32 leaves, applied in the network's dtype at mults [n]."""
    n, dt = x.shape[0], ctx.dtype
    p, d, heads = cfg.patch_size, cfg.inner_dim, cfg.num_attention_heads
    gh, gw = x.shape[2] // p, x.shape[3] // p
    Nx = gh * gw

    def lin(t, k):
        y = F.linear(t, sd[k + ".weight"], sd[k + ".bias"])
        if lora is not None and k in lora:
            down, up, sc = lora[k]
            y = y + (mults.to(dt) * sc).reshape([n] + [1] * (t.dim() - 1)) * F.linear(F.linear(t, down.to(dt)), up.to(dt))
        return y
    half = torch.exp(-math.log(10000.0) * torch.arange(128, device=x.device, dtype=torch.float32) / 128)
    a = ts[:, None] * half[None]
    te = lin(F.silu(lin(torch.cat([a.cos(), a.sin()], 1).to(dt), "time_text_embed.timestep_embedder.linear_1")),
             "time_text_embed.timestep_embedder.linear_2")
    temb = te + lin(F.silu(lin(pooled, "time_text_embed.text_embedder.linear_1")), "time_text_embed.text_embedder.linear_2")
    st = F.silu(temb)
    h = F.conv2d(x.to(dt), sd["pos_embed.proj.weight"], sd["pos_embed.proj.bias"], stride=p).flatten(2).transpose(1, 2)
    S = cfg.pos_embed_max_size
    top, left = (S - gh) // 2, (S - gw) // 2
    h = h + sd["pos_embed.pos_embed"].reshape(S, S, d)[top:top + gh, left:left + gw].reshape(1, Nx, d)
    c = lin(ctx, "context_embedder")
    mod = lambda t, sc, sh: F.layer_norm(t, (d,), eps=1e-6) * (1 + sc[:, None]) + sh[:, None]
    hd = lambda t: t.reshape(n, -1, heads, d // heads).transpose(1, 2)
    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        last = i == cfg.num_layers - 1
        mx = lin(st, b + "norm1.linear").chunk(6, dim=1)
        mc = lin(st, b + "norm1_context.linear").chunk(2 if last else 6, dim=1)
        hn = mod(h, mx[1], mx[0])
        cn = mod(c, mc[0], mc[1]) if last else mod(c, mc[1], mc[0])
        q = torch.cat([lin(hn, b + "attn.to_q"), lin(cn, b + "attn.add_q_proj")], 1)
        k = torch.cat([lin(hn, b + "attn.to_k"), lin(cn, b + "attn.add_k_proj")], 1)
        v = torch.cat([lin(hn, b + "attn.to_v"), lin(cn, b + "attn.add_v_proj")], 1)
        o = F.scaled_dot_product_attention(hd(q), hd(k), hd(v)).transpose(1, 2).reshape(n, -1, d)
        h = h + mx[2][:, None] * lin(o[:, :Nx], b + "attn.to_out.0")
        f = lin(F.gelu(lin(mod(h, mx[4], mx[3]), b + "ff.net.0.proj"), approximate="tanh"), b + "ff.net.2")
        h = h + mx[5][:, None] * f
        if not last:
            c = c + mc[2][:, None] * lin(o[:, Nx:], b + "attn.to_add_out")
            f = lin(F.gelu(lin(mod(c, mc[4], mc[3]), b + "ff_context.net.0.proj"), approximate="tanh"), b + "ff_context.net.2")
            c = c + mc[5][:, None] * f
    mo = lin(st, "norm_out.linear").chunk(2, dim=1)
    y = lin(mod(h, mo[0], mo[1]), "proj_out")
    C = cfg.out_channels
    return y.reshape(n, gh, gw, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(n, C, gh * p, gw * p).float()


def train_rows(a, cfg, model):
    """--train (module docstring)."""
    from sliders_conceptmod_amd import lora as L
    n, Nc = 2, 77 + a.t5_tokens
    rows = []
    for dname in a.dtypes.split(","):
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        model = model.to("cuda", dt).requires_grad_(False)
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        torch.manual_seed(0)
        net = L.LoRANetwork(model, rank=4, multiplier=1.0, train_method="full", context_stream=a.context_stream).to("cuda")
        with torch.no_grad():
            net.flat[net._n_down:].normal_(0, 0.05)
        flat, nd = net.flat.detach(), net._n_down
        for size in (int(s) for s in a.sizes.split(",")):
            lat = size // 8
            g = torch.Generator().manual_seed(1)
            x = torch.randn(n, cfg.in_channels, lat, lat, generator=g).cuda()
            ctx = torch.randn(n, Nc, cfg.joint_attention_dim, generator=g).to(dt).cuda()
            pooled = torch.randn(n, cfg.pooled_projection_dim, generator=g).to(dt).cuda()
            d_out = torch.randn(n, cfg.out_channels, lat, lat, generator=g).cuda()
            ts, mults = [500.0] * n, [1.0, -2.0]
            tsd, md = torch.tensor(ts, device="cuda"), torch.tensor(mults, device="cuda")
            eng = model.engine(n, lat, lat, Nc, trainable=True)
            grad = torch.zeros_like(flat)

            def engine_pair():
                eng.forward_save(x, ts, ctx, pooled, flat[:nd], flat[nd:], mults)
                eng.backward(d_out, grad[:nd], grad[nd:])

            def leaves():
                return {l.target_path: (flat[l.off_down:l.off_down + 4 * l.in_dim].view(4, l.in_dim).clone().requires_grad_(True),
                                        flat[nd + l.off_up:nd + l.off_up + l.out_dim * 4].view(l.out_dim, 4).clone().requires_grad_(True),
                                        float(l.scale)) for l in net.unet_loras}
            lv = leaves()

            def torch_pair():
                for dn, up, _ in lv.values():
                    dn.grad = up.grad = None
                (torch_forward(sd, cfg, x, tsd, ctx, pooled, lv, md) * d_out).sum().backward()

            grad.zero_()
            engine_pair()
            torch.cuda.reset_peak_memory_stats()  # (the torch arm's peak, on top of what is resident: weights, the workspace)
            torch_pair()
            tg = torch.zeros_like(flat)
            for l in net.unet_loras:
                dn, up, _ = lv[l.target_path]
                tg[l.off_down:l.off_down + 4 * l.in_dim] = dn.grad.reshape(-1)
                tg[nd + l.off_up:nd + l.off_up + l.out_dim * 4] = up.grad.reshape(-1)
            rel = float((grad - tg).norm() / tg.norm())
            e_ms, f_ms, t_ms = [], [], []
            for _ in range(a.rounds):
                e_ms.append(timed(engine_pair, a.iters))
                f_ms.append(timed(lambda: eng.forward_save(x, ts, ctx, pooled, flat[:nd], flat[nd:], mults), a.iters))
                t_ms.append(timed(torch_pair, a.iters))
            row = {"model": a.model, "mode": "train", "image": size, "dtype": dname, "n": n, "context_tokens": Nc,
                   "lora_modules": len(net.unet_loras), "engine_ms": e_ms, "engine_forward_save_ms": f_ms,
                   "engine_backward_ms": min(e_ms) - min(f_ms), "torch_ms": t_ms, "engine_vs_torch_grad_rel_l2": rel,
                   "workspace_bytes": eng.workspace_bytes, "torch_peak_bytes": torch.cuda.max_memory_allocated()}
            print(json.dumps(row), flush=True)
            rows.append(row)
        model._close_engines()
        model.__dict__.pop("_lora_network", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="saved forward + backward to the LoRA matrices instead of the forward")
    ap.add_argument("--context_stream", action="store_true", help="--train: all 191 modules instead of the 96 image-stream ones")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--sizes", default="1024,512")
    ap.add_argument("--dtypes", default="fp16,bf16")
    ap.add_argument("--model", default="sd3", choices=["sd3", "tiny_sd3"])
    ap.add_argument("--t5_tokens", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = M.sd3_medium_config() if a.model == "sd3" else M.tiny_sd3_config()
    model = M.init_synthetic_(M.SD3Transformer2DModel(cfg), seed=0)
    if a.train:
        rows = train_rows(a, cfg, model)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(rows, open(a.out, "w"), indent=1)
        return rows
    n, Nc = 2, 77 + a.t5_tokens
    rows = []
    for dname in a.dtypes.split(","):
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        model = model.to("cuda", dt)
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        for size in (int(s) for s in a.sizes.split(",")):
            lat = size // 8
            g = torch.Generator().manual_seed(1)
            x = torch.randn(n, cfg.in_channels, lat, lat, generator=g).cuda()
            ctx = torch.randn(n, Nc, cfg.joint_attention_dim, generator=g).to(dt).cuda()
            pooled = torch.randn(n, cfg.pooled_projection_dim, generator=g).to(dt).cuda()
            ts = [500.0] * n
            tsd = torch.tensor(ts, device="cuda")
            eng = model.engine(n, lat, lat, Nc)
            with torch.no_grad():
                got, want = eng.forward(x, ts, ctx, pooled), torch_forward(sd, cfg, x, tsd, ctx, pooled)
                rel = float((got - want).norm() / want.norm())
                e_ms, t_ms = [], []
                for _ in range(a.rounds):
                    e_ms.append(timed(lambda: eng.forward(x, ts, ctx, pooled), a.iters))
                    t_ms.append(timed(lambda: torch_forward(sd, cfg, x, tsd, ctx, pooled), a.iters))
            flop = forward_flop(cfg, n, (lat // cfg.patch_size) ** 2, Nc)
            row = {"model": a.model, "image": size, "dtype": dname, "n": n, "context_tokens": Nc, "gflop": flop / 1e9,
                   "engine_ms": e_ms, "torch_ms": t_ms, "engine_tfs": flop / min(e_ms) / 1e9, "torch_tfs": flop / min(t_ms) / 1e9,
                   "engine_vs_torch_rel_l2": rel, "workspace_gib": eng.workspace_bytes / 2 ** 30}
            print(json.dumps(row), flush=True)
            rows.append(row)
        model._close_engines()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    return rows


if __name__ == "__main__":
    main()
