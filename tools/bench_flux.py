"""ms per forward of the Flux transformer at FLUX.1-schnell's architecture with random weights, n = 1, at 1024 x 1024 and
512 x 512 images (128 x 128 / 64 x 64 latents), 256 context tokens: the engine next to a torch-ROCm restatement of the same
network in the same dtype on the same GPU (F.linear, F.layer_norm, scaled_dot_product_attention), the two arms alternating
in one process, best of `--rounds` x `--iters` forwards.  Prints one JSON line per (size, dtype) with the algorithmic FLOP of
a forward (GEMMs and attention, from the shapes), the TF/s both arms reach and the workspace, plus the time of qk_norm_rope
alone at that shape (the double block's two launches and the single block's in-place one) next to its byte bound at the
8 TB/s HBM peak, and writes them to --out.  No threshold: no time is a pass or fail condition.

`--train`: the slider step's differentiated part instead -- the trainable engine's saved forward + backward to the rank-4
LoRA matrices of the attention projections (multiplier 1, d_out random) next to torch autograd through the same restatement
with the LoRA delta added to the adapted Linears, arms alternating; the gradient's distance between the two arms, the
trainable workspace in bytes and the torch arm's peak allocation are reported with the times.

The model is built on the device, so flux.init_synthetic_ draws its 12 billion parameters there (on the CPU: minutes).

    python tools/bench_flux.py [--rounds 2] [--iters 3] [--sizes 1024,512] [--dtypes bf16] [--out profiles/flux_forward_n1_ctx256.json]
    python tools/bench_flux.py --train [--sizes 512,1024] [--out profiles/flux_train_n1_ctx256.json]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sliders_conceptmod_amd import _native  # noqa: E402
from sliders_conceptmod_amd import flux as M  # noqa: E402

HBM_PEAK = 8.0e12


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
    K = cfg.in_channels * cfg.patch_size ** 2
    f = 2.0 * n * Nx * d * K + 2.0 * n * Nc * d * cfg.joint_attention_dim
    f += 2.0 * n * d * ((256 + d) * (2 if cfg.guidance_embeds else 1) + cfg.pooled_projection_dim + d)
    f += cfg.num_layers * (2.0 * n * d * d * 12 + 2.0 * n * L * d * 3 * d + 4.0 * n * L * L * d + 2.0 * n * L * d * d * 9)
    f += cfg.num_single_layers * (2.0 * n * d * d * 3 + 2.0 * n * L * d * d * (3 + 4 + 5) + 4.0 * n * L * L * d)
    return f + 2.0 * n * d * 2 * d + 2.0 * n * Nx * d * K


def rope_tables(cfg, gh, gw, Nc, device):
    """(cos, sin) [Nc + gh gw, head_dim / 2] fp32, angles in float64 (the engine's table)."""
    ids = torch.zeros(Nc + gh * gw, 3, dtype=torch.float64)
    r, c = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    ids[Nc:, 1], ids[Nc:, 2] = r.reshape(-1).double(), c.reshape(-1).double()
    ang = torch.cat([ids[:, a:a + 1] / cfg.rope_theta ** (2 * torch.arange(Da // 2, dtype=torch.float64) / Da)[None]
                     for a, Da in enumerate(cfg.axes_dims_rope)], dim=1)
    return ang.cos().float().to(device), ang.sin().float().to(device)


def torch_forward(sd, cfg, x, ts, guidance, ctx, pooled, cos, sin, lora=None, mults=None):
    """The network in torch ops, in the dtype of `sd` (tests/flux_refs.py is the float64 form of the same graph).  lora:
    {module path: (down [r, in], up [out, r], alpha / r)} fp32 leaves with mults [n] the per-sample multipliers."""
    n, dt = x.shape[0], ctx.dtype
    p, d, heads, hd_ = cfg.patch_size, cfg.inner_dim, cfg.num_attention_heads, cfg.attention_head_dim
    gh, gw = x.shape[2] // p, x.shape[3] // p
    Nx, Nc = gh * gw, ctx.shape[1]

    def lin(t, k):
        y = F.linear(t, sd[k + ".weight"], sd[k + ".bias"])
        if lora is not None and k in lora:
            dn, up, sc = lora[k]
            y = y + (mults.reshape([n] + [1] * (t.dim() - 1)) * sc * ((t.float() @ dn.t()) @ up.t())).to(dt)
        return y
    half = torch.exp(-math.log(10000.0) * torch.arange(128, device=x.device, dtype=torch.float32) / 128)

    def embed(v, k):
        a = v[:, None] * half[None]
        return lin(F.silu(lin(torch.cat([a.cos(), a.sin()], 1).to(dt), k + ".linear_1")), k + ".linear_2")
    temb = embed(ts, "time_text_embed.timestep_embedder")
    if cfg.guidance_embeds:
        temb = temb + embed(guidance * 1000.0, "time_text_embed.guidance_embedder")
    temb = temb + lin(F.silu(lin(pooled, "time_text_embed.text_embedder.linear_1")), "time_text_embed.text_embedder.linear_2")
    st = F.silu(temb)
    C_ = cfg.in_channels
    h = lin(x.reshape(n, C_, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(n, Nx, C_ * p * p).to(dt), "x_embedder")
    c = lin(ctx, "context_embedder")
    mod = lambda t, sc, sh: F.layer_norm(t, (d,), eps=1e-6) * (1 + sc[:, None]) + sh[:, None]

    def qk(t, w, lo, hi):  # RMSNorm per head in fp32, as diffusers' RMSNorm does, then the interleaved rotation
        t = t.reshape(n, -1, heads, hd_).float()
        t = t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float()
        t0, t1 = t[..., 0::2], t[..., 1::2]
        cc, ss = cos[lo:hi, None, :], sin[lo:hi, None, :]
        return torch.stack([t0 * cc - t1 * ss, t1 * cc + t0 * ss], dim=-1).flatten(-2).to(dt).transpose(1, 2)

    def attn(q, k, v):
        return F.scaled_dot_product_attention(q, k, v.reshape(n, -1, heads, hd_).transpose(1, 2)).transpose(1, 2).reshape(n, -1, d)
    L = Nc + Nx
    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        mx = lin(st, b + "norm1.linear").chunk(6, dim=1)
        mc = lin(st, b + "norm1_context.linear").chunk(6, dim=1)
        hn, cn = mod(h, mx[1], mx[0]), mod(c, mc[1], mc[0])
        w = lambda k: sd[b + "attn." + k + ".weight"]
        q = torch.cat([qk(lin(cn, b + "attn.add_q_proj"), w("norm_added_q"), 0, Nc), qk(lin(hn, b + "attn.to_q"), w("norm_q"), Nc, L)], 2)
        k = torch.cat([qk(lin(cn, b + "attn.add_k_proj"), w("norm_added_k"), 0, Nc), qk(lin(hn, b + "attn.to_k"), w("norm_k"), Nc, L)], 2)
        v = torch.cat([lin(cn, b + "attn.add_v_proj"), lin(hn, b + "attn.to_v")], 1)
        o = attn(q, k, v)
        h = h + mx[2][:, None] * lin(o[:, Nc:], b + "attn.to_out.0")
        h = h + mx[5][:, None] * lin(F.gelu(lin(mod(h, mx[4], mx[3]), b + "ff.net.0.proj"), approximate="tanh"), b + "ff.net.2")
        c = c + mc[2][:, None] * lin(o[:, :Nc], b + "attn.to_add_out")
        c = c + mc[5][:, None] * lin(F.gelu(lin(mod(c, mc[4], mc[3]), b + "ff_context.net.0.proj"), approximate="tanh"),
                                     b + "ff_context.net.2")
    s = torch.cat([c, h], dim=1)
    for i in range(cfg.num_single_layers):
        b = f"single_transformer_blocks.{i}."
        sh, sc, g = lin(st, b + "norm.linear").chunk(3, dim=1)
        z = mod(s, sc, sh)
        a = attn(qk(lin(z, b + "attn.to_q"), sd[b + "attn.norm_q.weight"], 0, L),
                 qk(lin(z, b + "attn.to_k"), sd[b + "attn.norm_k.weight"], 0, L), lin(z, b + "attn.to_v"))
        m = F.gelu(lin(z, b + "proj_mlp"), approximate="tanh")
        s = s + g[:, None] * lin(torch.cat([a, m], dim=-1), b + "proj_out")
    mo = lin(st, "norm_out.linear").chunk(2, dim=1)
    y = lin(mod(s[:, Nc:], mo[0], mo[1]), "proj_out")
    return y.reshape(n, gh, gw, C_, p, p).permute(0, 3, 1, 4, 2, 5).reshape(n, C_, gh * p, gw * p).float()


def qk_norm_rope_ms(cfg, dt, Nx, Nc, cos, sin, iters=20):
    """(ms of the double block's two launches, ms of the single block's in-place launch, their bytes)."""
    lib = _native.lib()
    d, H, D, L = cfg.inner_dim, cfg.num_attention_heads, cfg.attention_head_dim, Nx + Nc
    P = lambda t: C.c_void_p(t.data_ptr())
    code = _native.DTYPE_CODE[dt]
    qx, qc = torch.randn(Nx, 3 * d, device="cuda").to(dt), torch.randn(Nc, 3 * d, device="cuda").to(dt)
    j = torch.empty(L, 3 * d, device="cuda", dtype=dt)
    w = torch.ones(D, device="cuda", dtype=dt)
    tab = torch.cat([cos, sin], dim=1).contiguous()
    s = _native.stream_ptr()

    def pair():
        _native.check(lib.smi_op_qk_norm_rope(code, P(qc), 3 * d, P(j), 3 * d, P(w), P(w), P(tab), 1, Nc, L, 0, H, D, 1e-6, s), "qk")
        _native.check(lib.smi_op_qk_norm_rope(code, P(qx), 3 * d, P(j), 3 * d, P(w), P(w), P(tab), 1, Nx, L, Nc, H, D, 1e-6, s), "qk")

    def inplace():
        _native.check(lib.smi_op_qk_norm_rope(code, P(j), 3 * d, P(j), 3 * d, P(w), P(w), P(tab), 1, L, L, 0, H, D, 1e-6, s), "qk")
    pair_bytes = 2.0 * L * 3 * d * 2 + L * D * 4 * 2  # q|k|v read and written, the table once per part with arithmetic
    inplace_bytes = 2.0 * L * 2 * d * 2 + L * D * 4 * 2
    return timed(pair, iters), timed(inplace, iters), pair_bytes, inplace_bytes


def train_rows(a, cfg, model, dname, dt):
    """--train (module docstring): one row per size."""
    from sliders_conceptmod_amd import lora as L
    n, Nc = 1, a.context_tokens
    rows = []
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    torch.manual_seed(0)
    net = L.LoRANetwork(model, rank=4, multiplier=1.0, delimiter="-", target_replace=["Attention"], train_method="full",
                        context_stream=a.context_stream).to("cuda")
    with torch.no_grad():
        net.flat[net._n_down:].normal_(0, 0.05)
    flat, nd = net.flat.detach(), net._n_down
    for size in (int(s) for s in a.sizes.split(",")):
        lat = size // 8
        g = torch.Generator().manual_seed(1)
        x = torch.randn(n, cfg.in_channels, lat, lat, generator=g).cuda()
        ctx = torch.randn(n, Nc, cfg.joint_attention_dim, generator=g).to(dt).cuda()
        pooled = torch.randn(n, cfg.pooled_projection_dim, generator=g).to(dt).cuda()
        d_out = torch.randn(n, cfg.in_channels, lat, lat, generator=g).cuda()
        ts, gs, mults = [500.0] * n, ([3.5] * n if cfg.guidance_embeds else None), [1.0] * n
        tsd, md = torch.tensor(ts, device="cuda"), torch.tensor(mults, device="cuda")
        gsd = torch.tensor(gs, device="cuda") if gs else None
        cos, sin = rope_tables(cfg, lat // 2, lat // 2, Nc, "cuda")
        try:
            eng = model.engine(n, lat, lat, Nc, trainable=True)
        except (RuntimeError, _native.SmiError) as err:  # the plan does not fit the card: report it and go on
            row = {"model": a.model, "mode": "train", "image": size, "dtype": dname, "n": n, "context_tokens": Nc,
                   "error": str(err)[:200], "plan_bytes": M.train_workspace_bytes(cfg, dt, net.engine_sites(), n, lat, lat, Nc)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            continue
        grad = torch.zeros_like(flat)

        def engine_pair():
            eng.forward_save(x, ts, gs, ctx, pooled, flat[:nd], flat[nd:], mults)
            eng.backward(d_out, grad[:nd], grad[nd:])

        lv = {l.target_path: (flat[l.off_down:l.off_down + 4 * l.in_dim].view(4, l.in_dim).clone().requires_grad_(True),
                              flat[nd + l.off_up:nd + l.off_up + l.out_dim * 4].view(l.out_dim, 4).clone().requires_grad_(True),
                              float(l.scale)) for l in net.unet_loras}

        def torch_pair():
            for dn, up, _ in lv.values():
                dn.grad = up.grad = None
            (torch_forward(sd, cfg, x, tsd, gsd, ctx, pooled, cos, sin, lv, md) * d_out).sum().backward()

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
            f_ms.append(timed(lambda: eng.forward_save(x, ts, gs, ctx, pooled, flat[:nd], flat[nd:], mults), a.iters))
            t_ms.append(timed(torch_pair, a.iters))
        row = {"model": a.model, "mode": "train", "image": size, "dtype": dname, "n": n, "context_tokens": Nc,
               "lora_modules": len(net.unet_loras), "engine_ms": e_ms, "engine_forward_save_ms": f_ms,
               "engine_backward_ms": min(e_ms) - min(f_ms), "torch_ms": t_ms, "engine_vs_torch_grad_rel_l2": rel,
               "workspace_bytes": eng.workspace_bytes, "torch_peak_bytes": torch.cuda.max_memory_allocated()}
        print(json.dumps(row), flush=True)
        rows.append(row)
        model._close_engines()
        del lv, tg, grad
        torch.cuda.empty_cache()
    model.__dict__.pop("_lora_network", None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--sizes", default="1024,512")
    ap.add_argument("--dtypes", default="bf16")
    ap.add_argument("--model", default="flux_schnell", choices=["flux_schnell", "flux_dev", "tiny_flux"])
    ap.add_argument("--context_tokens", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--train", action="store_true", help="saved forward + backward to the LoRA matrices instead of the forward")
    ap.add_argument("--context_stream", action="store_true", help="--train: the context stream's modules too")
    a = ap.parse_args()
    cfg = {"flux_schnell": M.flux_schnell_config, "flux_dev": M.flux_dev_config, "tiny_flux": M.tiny_flux_config}[a.model]()
    n, Nc = 1, a.context_tokens
    rows = []
    for dname in a.dtypes.split(","):
        dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
        torch.set_default_dtype(dt)
        with torch.device("cuda"):
            model = M.FluxTransformer2DModel(cfg)
        torch.set_default_dtype(torch.float32)
        M.init_synthetic_(model.requires_grad_(False), seed=0)
        if a.train:
            rows += train_rows(a, cfg, model, dname, dt)
            model._close_engines()
            del model
            torch.cuda.empty_cache()
            continue
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        for size in (int(s) for s in a.sizes.split(",")):
            lat = size // 8
            g = torch.Generator().manual_seed(1)
            x = torch.randn(n, cfg.in_channels, lat, lat, generator=g).cuda()
            ctx = torch.randn(n, Nc, cfg.joint_attention_dim, generator=g).to(dt).cuda()
            pooled = torch.randn(n, cfg.pooled_projection_dim, generator=g).to(dt).cuda()
            ts, gs = [500.0] * n, ([3.5] * n if cfg.guidance_embeds else None)
            tsd = torch.tensor(ts, device="cuda")
            gsd = torch.tensor(gs, device="cuda") if gs else None
            cos, sin = rope_tables(cfg, lat // 2, lat // 2, Nc, "cuda")
            eng = model.engine(n, lat, lat, Nc)
            with torch.no_grad():
                got, want = eng.forward(x, ts, gs, ctx, pooled), torch_forward(sd, cfg, x, tsd, gsd, ctx, pooled, cos, sin)
                rel = float((got - want).norm() / want.norm())
                e_ms, t_ms = [], []
                for _ in range(a.rounds):
                    e_ms.append(timed(lambda: eng.forward(x, ts, gs, ctx, pooled), a.iters))
                    t_ms.append(timed(lambda: torch_forward(sd, cfg, x, tsd, gsd, ctx, pooled, cos, sin), a.iters))
            Nx = (lat // 2) ** 2
            flop = forward_flop(cfg, n, Nx, Nc)
            pair_ms, inpl_ms, pair_b, inpl_b = qk_norm_rope_ms(cfg, dt, Nx, Nc, cos, sin)
            row = {"model": a.model, "image": size, "dtype": dname, "n": n, "context_tokens": Nc, "gflop": flop / 1e9,
                   "engine_ms": e_ms, "torch_ms": t_ms, "engine_tfs": flop / min(e_ms) / 1e9, "torch_tfs": flop / min(t_ms) / 1e9,
                   "engine_vs_torch_rel_l2": rel, "workspace_gib": eng.workspace_bytes / 2 ** 30,
                   "qk_norm_rope_pair_us": pair_ms * 1e3, "qk_norm_rope_pair_bound_us": pair_b / HBM_PEAK * 1e6,
                   "qk_norm_rope_inplace_us": inpl_ms * 1e3, "qk_norm_rope_inplace_bound_us": inpl_b / HBM_PEAK * 1e6}
            print(json.dumps(row), flush=True)
            rows.append(row)
        model._close_engines()
        del model, sd
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(rows, open(a.out, "w"), indent=1)
    return rows


if __name__ == "__main__":
    main()
