"""References for the Flux transformer backward: per-element float64 references and bounds of the three backward kernels of
csrc/flux.hip (qk_norm_rope_bwd, gelu_tanh_cols_bwd, flux_unpack_bwd), and the model's LoRA gradients.  Torch only, no GPU
import, nothing from the package under test.  Imports flux_refs and mmdit_bwd_refs and changes nothing in them.

KERNEL BOUNDS, in the manner of mmdit_bwd_refs.adaln_bwd_bound / gelu_tanh_bwd_bound: u the storage rounding, U32 one fp32
rounding; the store's half ulp plus the counted fp32 roundings.  The GPU tests assert |got - ref| <= SLACK E.

MODEL GRADIENTS.  Form A: torch autograd through `flux_refs.forward(..., lora=, mults=)` in float64 (`grads_a`).  Form B:
`twin_forward`, the same network restated op by op so that (1) every tensor the engine stores in 16 bit is rounded on the
way forward AND its gradient on the way back (notrigger_refs' straight-through `_Store`), and (2) a backward can be mutated.
With dt=None and no mutation the twin IS form A (held to it at 1e-12); with a dt its output is flux_refs.forward(dt) bit for
bit.  Bar: 3 e_q + 1e-4 with e_q = rel(B, A), the project's standing margin for gradients.

What the engine differentiates: the LoRA matrices only.  scale / shift / gate depend on temb alone, the RMSNorm weights are
frozen, and nothing flows to the context, the pooled vector, the guidance or the latents."""
import math

import torch

import flux_refs as F
import mmdit_bwd_refs as B
import mmdit_refs as R
from mmdit_bwd_refs import (_AdaLN, _CutGrad, _Gate, _LoraDelta, _collect, _leaves, adaln_bwd_bound, adaln_bwd_ref,  # noqa: F401
                            flat_layout, flatten_lora, gelu_tanh_bwd_bound, gelu_tanh_bwd_ref, make_lora)
from norm_refs import FLOOR, SLACK, U32, sub_eta, unit_roundoff, worst  # noqa: F401
from notrigger_refs import bar, rel, store  # noqa: F401

F64 = torch.float64

BWD_MUTATIONS = ("rot_forward", "drop_xr2", "drop_w", "text_image_ids", "drop_mlp_to_z", "drop_attn_branch",
                 "cut_ctx_joint_pack")


def _store_e(ref, dt):
    return unit_roundoff(dt) * ref.abs() + sub_eta(dt)


# ---------------------------------------------------------------------------------------------------------------
# per-kernel references and bounds
# ---------------------------------------------------------------------------------------------------------------
def qk_norm_rope_bwd_ref(src, d_joint, wq, wk, cos, sin, eps=1e-6):
    """src, d_joint [n, tokens, 3, heads, D] (the pre-norm q | k | v rows and the joint gradient's rows of these tokens),
    wq / wk [D], (cos, sin) [tokens, D / 2].  Returns dict(dx, and the pieces the bound reads), float64, of src's shape."""
    x, do = src.double(), d_joint.double()
    D = x.shape[-1]
    out = {k: torch.zeros_like(x) for k in ("dx", "g", "k", "mag_dy", "r", "gx_abs")}
    out["dx"][:, :, 2] = do[:, :, 2]
    c, s = cos[:, None, :], sin[:, None, :]
    for part, w in ((0, wq), (1, wk)):
        xp, dp, wd = x[:, :, part], do[:, :, part], w.double()
        d0, d1 = dp[..., 0::2], dp[..., 1::2]
        dy = torch.stack([d0 * c + d1 * s, d1 * c - d0 * s], dim=-1).flatten(-2)
        mag = torch.stack([(d0 * c).abs() + (d1 * s).abs(), (d1 * c).abs() + (d0 * s).abs()], dim=-1).flatten(-2)
        g = dy * wd
        r = torch.rsqrt((xp * xp).mean(dim=-1, keepdim=True) + eps)
        k = r * r * (g * xp).mean(dim=-1, keepdim=True)
        out["dx"][:, :, part] = r * (g - xp * k)
        out["g"][:, :, part], out["k"][:, :, part] = g, k.expand_as(g)
        out["mag_dy"][:, :, part] = mag * wd.abs()
        out["r"][:, :, part] = r.expand_as(g)
        out["gx_abs"][:, :, part] = (g * xp).abs().mean(dim=-1, keepdim=True).expand_as(g)
    out["x"], out["D"] = x, D
    return out


def qk_norm_rope_bwd_bound(ref, dt):
    """v: a copy.  q and k, with r = rsqrt(mean(x^2) + eps) carrying the forward's relative error (flux_refs: the mean of
    squares 14 U32 halved by the root, v_rsq 2: 9 U32):
      dy: the two products and their sum, on the scale |do0 c| + |do1 s|: 2 U32; g = dy w one more: e_g = 3 U32 mag |w|
      sum g x: eight fused adds in the lane, a butterfly of up to 5, the product with 1 / D (14 U32 of mean |g x|), on terms
        that carry e_g: e_m = 14 U32 mean|g x| + mean(e_g |x|)
      k = r r m: r^2 (19 U32), the product (1): 20 U32 |k| + r^2 e_m
      g - x k as one fused multiply-add (1 at the size of its terms), then the product with r (10 U32 of the result)."""
    x, g, k, r = ref["x"], ref["g"], ref["k"], ref["r"]
    e_g = 3 * U32 * ref["mag_dy"]
    e_m = 14 * U32 * ref["gx_abs"] + (e_g * x.abs()).mean(dim=-1, keepdim=True)
    e_k = 20 * U32 * k.abs() + r * r * e_m
    inner = e_g + x.abs() * e_k + U32 * (g.abs() + (x * k).abs())
    e = r * inner + 10 * U32 * ref["dx"].abs()
    e[:, :, 2] = 0.0
    st = _store_e(ref["dx"], dt)
    st[:, :, 2] = 0.0
    return st + e + FLOOR


def flux_unpack_bwd_ref(d_out, scales, p=2):
    """d_out f32 [n, C, gh p, gw p], scales [n] (powers of two) -> rows [n gh gw, C p p], columns (c, py, px), float64."""
    n, C, H, W = d_out.shape
    gh, gw = H // p, W // p
    v = d_out.double() * torch.as_tensor(scales, dtype=F64)[:, None, None, None]
    return v.view(n, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(n * gh * gw, C * p * p)


def flux_unpack_bwd_bound(ref, dt):
    return _store_e(ref, dt) + FLOOR  # the product with a power of two is exact: the store alone


# ---------------------------------------------------------------------------------------------------------------
# the model: LoRA sites, form A, and the twin (form B and the mutants)
# ---------------------------------------------------------------------------------------------------------------
X_PARTS = ("to_q", "to_k", "to_v", "to_out.0")
C_PARTS = ("add_q_proj", "add_k_proj", "add_v_proj", "to_add_out")
S_PARTS = ("to_q", "to_k", "to_v")


def site_names(num_layers, num_single_layers, context_stream):
    """Engine targets in flat-buffer order: per double block to_q, to_k, to_v (adjacent: one fused GEMM), to_out.0 and, with
    context_stream, add_q_proj, add_k_proj, add_v_proj, to_add_out; per single block to_q, to_k, to_v."""
    out = []
    for i in range(num_layers):
        out += [f"transformer_blocks.{i}.attn.{p}" for p in X_PARTS]
        if context_stream:
            out += [f"transformer_blocks.{i}.attn.{p}" for p in C_PARTS]
    for i in range(num_single_layers):
        out += [f"single_transformer_blocks.{i}.attn.{p}" for p in S_PARTS]
    return out


def grads_a(sd, cfg, sample, timesteps, guidance, ctx, pooled, lora, names, mults, d_out):
    """Form A: float64 autograd through flux_refs.forward."""
    leaves = _leaves(lora)
    out = F.forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, lora=leaves, mults=mults)
    return _collect(out, d_out, leaves, names) + (out.detach(),)


def grads_twin(sd, cfg, sample, timesteps, guidance, ctx, pooled, lora, names, mults, d_out, dt=None, mut=None):
    """The twin's gradients: dt=None, mut=None is form A restated; dt a 16-bit type is form B; mut a mutated backward."""
    leaves = _leaves(lora)
    out = twin_forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, leaves, mults, dt=dt, mut=mut)
    if dt is not None:  # d_out enters the engine as 16-bit rows under the sample's loss scale
        out = store(out, dt)
    return _collect(out, d_out, leaves, names) + (out.detach(),)


class _QKNormRope(torch.autograd.Function):
    """Rot(x rsqrt(mean(x^2) + eps) w) on heads [n, T, heads, D]; the backward as the kernel forms it, with the table the
    BACKWARD reads given apart (cos_b, sin_b) and the terms a mutant changes."""

    @staticmethod
    def forward(ctx, x, w, cos, sin, cos_b, sin_b, mut):
        ctx.save_for_backward(x, w, cos_b, sin_b)
        ctx.mut = mut
        return F.rotate(F.rms(x, w), cos, sin)

    @staticmethod
    def backward(ctx, do):
        x, w, cos, sin = ctx.saved_tensors
        c, s = cos[:, None, :], sin[:, None, :]
        if ctx.mut == "rot_forward":
            s = -s
        d0, d1 = do[..., 0::2], do[..., 1::2]
        dy = torch.stack([d0 * c + d1 * s, d1 * c - d0 * s], dim=-1).flatten(-2)
        g = dy if ctx.mut == "drop_w" else dy * w
        r = torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + 1e-6)
        k = 0.0 if ctx.mut == "drop_xr2" else r * r * (g * x).mean(dim=-1, keepdim=True)
        return r * (g - x * k), None, None, None, None, None, None


def twin_forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, lora, mults, dt=None, mut=None):
    """flux_refs.forward restated with `store` (value and gradient rounded) at its rounding sites and the ops above."""
    st = (lambda t: t) if dt is None else (lambda t: store(t, dt))
    rnd = R._rounder(dt)
    # (as flux_refs.forward takes them: a float64 entry is the caller's, already rounded to the storage type)
    W = {k: (v if v.dtype == F64 else rnd(v.double())) for k, v in sd.items()}
    n = sample.shape[0]
    p, heads, hd = cfg.patch_size, cfg.num_attention_heads, cfg.attention_head_dim
    d = heads * hd
    gh, gw = sample.shape[2] // p, sample.shape[3] // p
    Nx, Nc = gh * gw, ctx.shape[1]
    L = Nc + Nx
    mv = torch.as_tensor(mults, dtype=F64)

    def lin(x, name, res=None):
        y = x @ W[name + ".weight"].t() + W[name + ".bias"]
        if name in lora:
            dn, up, sc = lora[name]
            y = y + _LoraDelta.apply(x, dn, up, mv.reshape([n] + [1] * (x.dim() - 1)), sc, None)
        if res is not None:
            y = y + res
        return st(y)

    def adaln(x, scale, shift):
        return st(_AdaLN.apply(x, scale, shift, None))

    def gate(h, g, f):
        return st(_Gate.apply(h, g, f, None))

    def embed(vals, name, res=None):
        s = rnd(R.timestep_sinusoid(torch.as_tensor(vals, dtype=F64)))
        return lin(rnd(R.silu(lin(s, name + ".linear_1"))), name + ".linear_2", res=res)

    with torch.no_grad():  # nothing adapted is upstream of these
        temb = embed(timesteps, "time_text_embed.timestep_embedder")
        if cfg.guidance_embeds:
            temb = embed(1000.0 * torch.as_tensor(guidance, dtype=F64), "time_text_embed.guidance_embedder", res=temb)
        temb = lin(rnd(R.silu(lin(rnd(pooled.double()), "time_text_embed.text_embedder.linear_1"))),
                   "time_text_embed.text_embedder.linear_2", res=temb)
        s_t = rnd(R.silu(temb))
        x = lin(rnd(R.patchify(sample.double(), p, "cpp")), "x_embedder")
        c = lin(rnd(ctx.double()), "context_embedder")
    cos, sin = F.rope_table(F.joint_ids(gh, gw, Nc), cfg.axes_dims_rope, cfg.rope_theta, f32=dt is not None)
    cos_b, sin_b = cos, sin
    if mut == "text_image_ids":  # the backward rotates the text rows by the image tokens' ids
        cos_b, sin_b = F.rope_table(F.joint_ids(gh, gw, Nc, "rope_text_rotated"), cfg.axes_dims_rope, cfg.rope_theta,
                                    f32=dt is not None)

    def heads_of(t):
        return t.reshape(n, -1, heads, hd)

    def qk(t, w, lo, hi):
        return st(_QKNormRope.apply(heads_of(t), w, cos[lo:hi], sin[lo:hi], cos_b[lo:hi], sin_b[lo:hi], mut))

    def attn(q, k, v):
        s = q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2) / math.sqrt(hd)
        return st((torch.softmax(s, dim=-1) @ heads_of(v).transpose(1, 2)).transpose(1, 2).reshape(n, -1, d))

    def nw(b, name):
        return W[b + "attn." + name + ".weight"]

    def tail(h, a, m6, b, out_name, ff):
        _sm, _scm, gm, sf, scf, gf = m6
        h = gate(h, gm, lin(a, b + out_name))
        f = lin(st(R.gelu_tanh(lin(adaln(h, scf, sf), b + ff + ".net.0.proj"))), b + ff + ".net.2")
        return gate(h, gf, f)

    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        with torch.no_grad():
            mx = lin(s_t, b + "norm1.linear").chunk(6, dim=1)
            mc = lin(s_t, b + "norm1_context.linear").chunk(6, dim=1)
        xn, cn = adaln(x, mx[1], mx[0]), adaln(c, mc[1], mc[0])
        qx, kx, vx = (lin(xn, b + "attn." + k) for k in ("to_q", "to_k", "to_v"))
        qc, kc, vc = (lin(cn, b + "attn." + k) for k in ("add_q_proj", "add_k_proj", "add_v_proj"))
        q = torch.cat([qk(qc, nw(b, "norm_added_q"), 0, Nc), qk(qx, nw(b, "norm_q"), Nc, L)], dim=1)
        k = torch.cat([qk(kc, nw(b, "norm_added_k"), 0, Nc), qk(kx, nw(b, "norm_k"), Nc, L)], dim=1)
        o = attn(q, k, torch.cat([vc, vx], dim=1))
        x = tail(x, o[:, Nc:], mx, b, "attn.to_out.0", "ff")
        c = tail(c, o[:, :Nc], mc, b, "attn.to_add_out", "ff_context")

    if mut == "cut_ctx_joint_pack":
        c = _CutGrad.apply(c)
    s = torch.cat([c, x], dim=1)
    for i in range(cfg.num_single_layers):
        b = f"single_transformer_blocks.{i}."
        with torch.no_grad():
            sh, sc, g = lin(s_t, b + "norm.linear").chunk(3, dim=1)
        z = adaln(s, sc, sh)
        q, k, v = (lin(z, b + "attn." + t) for t in ("to_q", "to_k", "to_v"))
        a = attn(qk(q, nw(b, "norm_q"), 0, L), qk(k, nw(b, "norm_k"), 0, L), v)
        if mut == "drop_attn_branch":
            a = _CutGrad.apply(a)
        m = st(R.gelu_tanh(lin(_CutGrad.apply(z) if mut == "drop_mlp_to_z" else z, b + "proj_mlp")))
        s = gate(s, g, lin(torch.cat([a, m], dim=-1), b + "proj_out"))
    x = s[:, Nc:]
    with torch.no_grad():
        sc_o, sh_o = lin(s_t, "norm_out.linear").chunk(2, dim=1)
    y = lin(adaln(x, sc_o, sh_o), "proj_out")
    return R.unpatchify(y, n, cfg.in_channels, gh, gw, p, "cpp")


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and GPU tests
# ---------------------------------------------------------------------------------------------------------------
def tiny_inputs(cfg, n, h, w, n_ctx, seed):
    """(sample, timesteps, guidance or None, ctx, pooled, d_out): float32 / 16-bit-representable values, so every form reads
    the same numbers."""
    g = torch.Generator().manual_seed(seed)
    sample = torch.randn((n, cfg.in_channels, h, w), generator=g)
    ts = [float(t) for t in torch.randint(1, 1000, (n,), generator=g)]
    ctx = torch.randn((n, n_ctx, cfg.joint_attention_dim), generator=g).half().float()
    pooled = torch.randn((n, cfg.pooled_projection_dim), generator=g).half().float()
    d_out = torch.randn((n, cfg.in_channels, h, w), generator=g)
    guidance = [3.5 - 0.5 * i for i in range(n)] if cfg.guidance_embeds else None
    return sample, ts, guidance, ctx.bfloat16().float(), pooled.bfloat16().float(), d_out
