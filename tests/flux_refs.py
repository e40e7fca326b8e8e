"""Float64 restatement of the Flux transformer forward (diffusers FluxTransformer2DModel 0.30, from a state dict), its
storage-dtype twin, the per-element bound of qk_norm_rope (csrc/flux.hip), the flow-matching scheduler's dynamic shift
and the Flux sweep loop.  Torch only, no GPU import, nothing from the package under test.  The restatement is UNPINNED:
diffusers is not a dependency, so this file is the one place a later pin has to check.

MODEL BAR, the rule of mmdit_refs.py.  `forward(..., dt=None)` is the network in float64.  `forward(..., dt=fp16 | bf16)` is the
storage-dtype twin: the same float64 arithmetic with the weights rounded to dt and a rounding to dt at exactly the sites where
the engine stores a 16-bit tensor -- the packed latents, the sinusoids, every GEMM output (a temb sum rides in the next
embedder's second GEMM: one rounding), every adaln_modulate / gate_residual / activation output, the q and k heads after
qk_norm_rope (v is copied: no rounding), the attention output; the rotary table is rounded to fp32, as the engine keeps it.
Everything between two sites stays float64.  bar(dt) = 2 x relative-L2(twin - float64) on the same inputs.

KERNEL BOUND of qk_norm_rope, in the manner of mmdit_refs.adaln_bound: u the storage rounding, U32 = 2^-24 one fp32 rounding;
the GPU tests assert |got - ref| <= SLACK E."""
import math

import torch

from mmdit_refs import (_rounder, _store, gelu_tanh, ln, patchify, rel_l2, silu, timestep_sinusoid,  # noqa: F401
                        unpatchify)
from norm_refs import FLOOR, SLACK, U32, worst  # noqa: F401

MUTATIONS = ("rope_dropped", "rope_half_split", "rope_axes_swapped", "rope_text_rotated", "rope_image_first",
             "drop_norm_q", "swap_norm_added", "rms_over_d", "drop_single_gate", "cat_order", "keep_first_rows",
             "drop_guidance", "swap_norm_out", "unpack_order")


# ---------------------------------------------------------------------------------------------------------------
# rotary table
# ---------------------------------------------------------------------------------------------------------------
def rope_angles(ids, axes, theta=10000.0):
    """ids [T, 3] -> float64 angles [T, sum(axes) / 2]: axis a of width D_a gives id_a / theta^(2 j / D_a), j < D_a / 2."""
    out = []
    for a, Da in enumerate(axes):
        j = torch.arange(Da // 2, dtype=torch.float64)
        out.append(ids[:, a].double()[:, None] / theta ** (2 * j / Da)[None])
    return torch.cat(out, dim=1)


def joint_ids(gh, gw, Nc, mut=None):
    """[Nc + gh gw, 3]: text rows (0, 0, 0), then image rows (0, row, col)."""
    r, c = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    img = torch.stack([torch.zeros_like(r), r, c], dim=-1).reshape(-1, 3)
    if mut == "rope_axes_swapped":
        img = img[:, [0, 2, 1]]
    txt = torch.zeros(Nc, 3, dtype=img.dtype)
    if mut == "rope_text_rotated":  # text token t takes the ids of image token t (of a grid as wide, continued downwards)
        t = torch.arange(Nc)
        txt = torch.stack([torch.zeros_like(t), t // gw, t % gw], dim=-1)
    if mut == "rope_image_first":
        return torch.cat([img, txt])
    return torch.cat([txt, img])


def rope_table(ids, axes, theta=10000.0, f32=False):
    """(cos, sin) [T, D / 2] in float64; f32: rounded to fp32 first, as the engine stores them."""
    a = rope_angles(ids, axes, theta)
    c, s = torch.cos(a), torch.sin(a)
    return (c.float().double(), s.float().double()) if f32 else (c, s)


def rotate(x, cos, sin, half_split=False):
    """x [..., T, heads, D] by (cos, sin) [T, D / 2]; pairs (2 j, 2 j + 1) -- or (j, j + D / 2) for the mutation."""
    c, s = cos[:, None, :], sin[:, None, :]
    if half_split:
        h = x.shape[-1] // 2
        x0, x1 = x[..., :h], x[..., h:]
        return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    return torch.stack([x0 * c - x1 * s, x1 * c + x0 * s], dim=-1).flatten(-2)


def rms(x, w, eps=1e-6):
    return x * torch.rsqrt((x * x).mean(dim=-1, keepdim=True) + eps) * w


# ---------------------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------------------
def forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, dt=None, mut=None, lora=None, mults=None):
    """sd: state dict (any float dtype); cfg: an object with the FluxConfig fields; sample [n, 16, H, W] un-packed,
    timesteps [n] (1000 sigma), guidance [n] or None, ctx [n, Nc, J], pooled [n, P].  lora: {module path: (down [r, in],
    up [out, r], alpha / r)} with mults [n] the per-sample multipliers.  Returns float64 [n, 16, H, W]."""
    rnd = _rounder(dt)

    class _Weights:  # converted at use, one at a time: the full-width blocks hold half a billion parameters.  A float64
        def __getitem__(self, k):  # entry is taken as it is: the caller has rounded it to the storage type already
            v = sd[k]
            return v if v.dtype == torch.float64 else rnd(v.double())
    W = _Weights()
    n = sample.shape[0]
    p, heads, hd = cfg.patch_size, cfg.num_attention_heads, cfg.attention_head_dim
    d = heads * hd
    gh, gw = sample.shape[2] // p, sample.shape[3] // p
    Nx, Nc = gh * gw, ctx.shape[1]
    mv = None if mults is None else torch.as_tensor(mults, dtype=torch.float64)

    def lin(x, name, res=None):
        y = x @ W[name + ".weight"].t() + W[name + ".bias"]
        if lora is not None and name in lora and mv is not None:
            dn, up, sc = lora[name]
            m = mv.reshape([n] + [1] * (x.dim() - 1))
            y = y + m * sc * ((x @ dn.double().t()) @ up.double().t())
        if res is not None:
            y = y + res
        return rnd(y)

    def adaln(x, scale, shift):
        return rnd(ln(x) * (1 + scale[:, None]) + shift[:, None])

    def gate(h, g, f):
        return rnd(h + g[:, None] * f)

    def embed(vals, name, res=None):
        s = rnd(timestep_sinusoid(torch.as_tensor(vals, dtype=torch.float64)))
        return lin(rnd(silu(lin(s, name + ".linear_1"))), name + ".linear_2", res=res)

    temb = embed(timesteps, "time_text_embed.timestep_embedder")
    if cfg.guidance_embeds and mut != "drop_guidance":
        temb = embed(1000.0 * torch.as_tensor(guidance, dtype=torch.float64), "time_text_embed.guidance_embedder", res=temb)
    temb = lin(rnd(silu(lin(rnd(pooled.double()), "time_text_embed.text_embedder.linear_1"))),
               "time_text_embed.text_embedder.linear_2", res=temb)
    st = rnd(silu(temb))

    x = lin(rnd(patchify(sample.double(), p, "cpp")), "x_embedder")
    c = lin(rnd(ctx.double()), "context_embedder")
    cos, sin = rope_table(joint_ids(gh, gw, Nc, mut), cfg.axes_dims_rope, cfg.rope_theta, f32=dt is not None)

    def heads_of(t):
        return t.reshape(n, -1, heads, hd)

    def qk(t, w, lo, hi):
        """RMS-normalise per head (or over d, the mutation) and rotate by table rows [lo, hi)."""
        if mut == "rms_over_d":
            t = heads_of(t * torch.rsqrt((t * t).mean(dim=-1, keepdim=True) + 1e-6)) * w
        else:
            t = rms(heads_of(t), w)
        if mut != "rope_dropped":
            t = rotate(t, cos[lo:hi], sin[lo:hi], mut == "rope_half_split")
        return rnd(t)

    def attn(q, k, v):
        s = q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2) / math.sqrt(hd)
        return rnd((torch.softmax(s, dim=-1) @ heads_of(v).transpose(1, 2)).transpose(1, 2).reshape(n, -1, d))

    def nw(b, name):
        if mut == "drop_norm_q" and name == "norm_q":
            return torch.ones(hd, dtype=torch.float64)
        if mut == "swap_norm_added" and b.startswith("transformer_blocks"):
            name = {"norm_q": "norm_added_q", "norm_k": "norm_added_k", "norm_added_q": "norm_q", "norm_added_k": "norm_k"}[name]
        return W[b + "attn." + name + ".weight"]

    def tail(h, a, m6, b, out_name, ff):
        _sm, _scm, gm, sf, scf, gf = m6
        h = gate(h, gm, lin(a, b + out_name))
        f = lin(rnd(gelu_tanh(lin(adaln(h, scf, sf), b + ff + ".net.0.proj"))), b + ff + ".net.2")
        return gate(h, gf, f)

    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        mx = lin(st, b + "norm1.linear").chunk(6, dim=1)
        mc = lin(st, b + "norm1_context.linear").chunk(6, dim=1)
        xn, cn = adaln(x, mx[1], mx[0]), adaln(c, mc[1], mc[0])
        qx, kx, vx = (lin(xn, b + "attn." + k) for k in ("to_q", "to_k", "to_v"))
        qc, kc, vc = (lin(cn, b + "attn." + k) for k in ("add_q_proj", "add_k_proj", "add_v_proj"))
        q = torch.cat([qk(qc, nw(b, "norm_added_q"), 0, Nc), qk(qx, nw(b, "norm_q"), Nc, Nc + Nx)], dim=1)
        k = torch.cat([qk(kc, nw(b, "norm_added_k"), 0, Nc), qk(kx, nw(b, "norm_k"), Nc, Nc + Nx)], dim=1)
        o = attn(q, k, torch.cat([vc, vx], dim=1))
        x = tail(x, o[:, Nc:], mx, b, "attn.to_out.0", "ff")
        c = tail(c, o[:, :Nc], mc, b, "attn.to_add_out", "ff_context")

    s = torch.cat([c, x], dim=1)
    L = Nc + Nx
    for i in range(cfg.num_single_layers):
        b = f"single_transformer_blocks.{i}."
        sh, sc, g = lin(st, b + "norm.linear").chunk(3, dim=1)
        z = adaln(s, sc, sh)
        q, k, v = (lin(z, b + "attn." + t) for t in ("to_q", "to_k", "to_v"))
        a = attn(qk(q, nw(b, "norm_q"), 0, L), qk(k, nw(b, "norm_k"), 0, L), v)
        m = rnd(gelu_tanh(lin(z, b + "proj_mlp")))
        f = lin(torch.cat([m, a] if mut == "cat_order" else [a, m], dim=-1), b + "proj_out")
        s = rnd(s + f) if mut == "drop_single_gate" else gate(s, g, f)
    x = s[:, :Nx] if mut == "keep_first_rows" else s[:, Nc:]
    sc_o, sh_o = lin(st, "norm_out.linear").chunk(2, dim=1)
    if mut == "swap_norm_out":
        sc_o, sh_o = sh_o, sc_o
    y = lin(adaln(x, sc_o, sh_o), "proj_out")
    return unpatchify(y, n, cfg.in_channels, gh, gw, p, "ppc" if mut == "unpack_order" else "cpp")


def model_bar(sd, cfg, sample, timesteps, guidance, ctx, pooled, dt, ref=None, **kw):
    """(bar, ref): 2 x the twin's relative-L2 distance from float64 on these inputs."""
    if ref is None:
        ref = forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, **kw)
    twin = forward(sd, cfg, sample, timesteps, guidance, ctx, pooled, dt=dt, **kw)
    return 2.0 * rel_l2(twin, ref), ref


# ---------------------------------------------------------------------------------------------------------------
# qk_norm_rope: reference, bound, fp32 emulation
# ---------------------------------------------------------------------------------------------------------------
def qk_norm_rope_ref(src, wq, wk, cos, sin, eps=1e-6):
    """src [n, tokens, 3, heads, D] (q | k | v), wq / wk [D], (cos, sin) [tokens, D / 2] the table rows of these tokens.
    Returns (out, mag) float64 of src's shape: mag is |y0 c| + |y1 s| per element of q and k (0 for v, a copy)."""
    x = src.double()
    out, mag = x.clone(), torch.zeros_like(x)
    c, s = cos[:, None, :], sin[:, None, :]
    for part, w in ((0, wq), (1, wk)):
        y = rms(x[:, :, part], w.double(), eps)
        y0, y1 = y[..., 0::2], y[..., 1::2]
        out[:, :, part] = torch.stack([y0 * c - y1 * s, y1 * c + y0 * s], dim=-1).flatten(-2)
        mag[:, :, part] = torch.stack([(y0 * c).abs() + (y1 * s).abs(), (y1 * c).abs() + (y0 * s).abs()], dim=-1).flatten(-2)
    return out, mag


QK_ROPE_ROUNDINGS = 14


def qk_norm_rope_bound(ref, mag, dt):
    """The store; on each of the two products of a rotated element, relative: the mean of squares (every term positive, so
    its relative error is at most the depth of the sum -- 8 fused adds in the lane, a butterfly of up to 5, the product with
    1 / D: 14 U32 -- and adding eps does not raise it; halved by the square root: 7), v_rsq_f32 (1 ulp: 2), x r and (x r) w
    (2), the fp32 table entry (1), the product with it (1): 13; their sum or difference 1 more, on the scale
    |y0 c| + |y1 s| = mag: 14 U32 mag."""
    return _store(ref, dt) + QK_ROPE_ROUNDINGS * U32 * mag + FLOOR


def qk_norm_rope_emulate(src, wq, wk, cos, sin, dt, eps=1e-6):
    """A correct kernel in fp32: inputs of dtype dt, fp32 arithmetic in the kernel's order of operations (torch's fp32 sum
    stands in for the lane chain + butterfly), fp32 table, one rounding to dt."""
    x = src.to(dt).float()
    out = x.clone()
    c, s = cos.float()[:, None, :], sin.float()[:, None, :]
    for part, w in ((0, wq), (1, wk)):
        h = x[:, :, part]
        r = torch.rsqrt((h * h).sum(dim=-1, keepdim=True) * (1.0 / h.shape[-1]) + eps)
        y = h * r * w.to(dt).float()
        y0, y1 = y[..., 0::2], y[..., 1::2]
        out[:, :, part] = torch.stack([y0 * c - y1 * s, y1 * c + y0 * s], dim=-1).flatten(-2)
    return out.to(dt)


# ---------------------------------------------------------------------------------------------------------------
# the scheduler's dynamic shift and the sweep loop, restated
# ---------------------------------------------------------------------------------------------------------------
def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=4096, base_shift=0.5, max_shift=1.15):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


def flux_sigmas(steps, mu=None, shift=1.0):
    """(timesteps [n], sigmas [n + 1]) of the Flux pipeline's set_timesteps(sigmas=linspace(1, 1 / n, n), mu=mu): with mu the
    exponential time shift e^mu / (e^mu + 1 / s - 1), else the static shift (1 for schnell: the identity).  Float64."""
    s = torch.linspace(1.0, 1.0 / steps, steps, dtype=torch.float64)
    s = math.exp(mu) / (math.exp(mu) + (1 / s - 1)) if mu is not None else shift * s / (1 + (shift - 1) * s)
    return s * 1000.0, torch.cat([s, torch.zeros(1, dtype=torch.float64)])


def sweep_loop(model_fn, latents, steps, mu=None, shift=1.0, start=0, total=None):
    """Euler loop over timesteps[start:total], one transformer pass per step: x += (sigma_{i+1} - sigma_i) model_fn(x, t_i)."""
    ts, sig = flux_sigmas(steps, mu, shift)
    total = steps if total is None else total
    x = latents.double()
    for i in range(start, total):
        x = x + (sig[i + 1] - sig[i]) * model_fn(x, float(ts[i]))
    return x
