"""Float64 restatement of the SD3 MMDiT forward (diffusers SD3Transformer2DModel, from a state dict), its storage-dtype
twin, the per-element bounds of the kernels of csrc/mmdit.hip, the restated flow-matching scheduler and the slider sweep
loop.  Torch only, no GPU import, nothing from the package under test.

MODEL BAR.  `forward(..., dt=None)` is the network in float64.  `forward(..., dt=torch.float16 | torch.bfloat16)` is the
storage-dtype twin: the same float64 arithmetic with the weights rounded to dt and a rounding to dt at exactly the sites
where the engine stores a 16-bit tensor -- the patch matrix, the sinusoid, every GEMM output (the temb sum rides in the
second text-embedder GEMM's epilogue: one rounding), every adaln_modulate / gate_residual / add_pos / activation output, and
the attention output (packing q|k|v moves bits and rounds nothing).  Everything between two sites stays float64.
bar(dt) = 2 x relative-L2(twin - float64) on the same inputs: the factor 2 is the project's own (clip_vision_refs.py,
lpips_refs.py).  It is computed from this file alone.

KERNEL BOUNDS, in the manner of norm_refs.py / elementwise_refs.py: u = 2^-11 (fp16) / 2^-8 (bf16) the storage rounding, eta
its absolute form below fp16's normal range, U32 = 2^-24 one fp32 rounding; the GPU tests assert |got - ref| <= SLACK E."""
import math

import torch

from norm_refs import FLOOR, SLACK, STAT_BAR, U32, sub_eta, unit_roundoff, worst  # noqa: F401

MUTATIONS = ("scale_no_one", "drop_gate", "swap_msa_mlp", "swap_norm_out", "swap_last_ctx", "skip_to_add_out",
             "own_stream_attn", "pos_crop0", "patch_order", "unpatch_order", "erf_gelu")


def _rounder(dt):
    return (lambda t: t) if dt is None else (lambda t: t.to(dt).double())


def timestep_sinusoid(t, dim=256):
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / half)
    a = t.double()[:, None] * f[None]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=1)


def gelu_tanh(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), written as x sigmoid(2 u): the same function, without the
    cancellation of 1 + tanh(u) for u << 0 (float64's tanh(-18) is -1 exactly; the true value there is 2e-16 x)."""
    return x * torch.sigmoid(2 * math.sqrt(2 / math.pi) * (x + 0.044715 * x ** 3))


def gelu_erf(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def silu(x):
    return x * torch.sigmoid(x)


def ln(x, eps=1e-6):
    m = x.mean(dim=-1, keepdim=True)
    v = ((x - m) ** 2).mean(dim=-1, keepdim=True)
    return (x - m) / torch.sqrt(v + eps)


def patchify(lat, p, order="cpp"):
    n, C, H, W = lat.shape
    t = lat.reshape(n, C, H // p, p, W // p, p)  # n c gy py gx px
    if order == "cpp":
        return t.permute(0, 2, 4, 1, 3, 5).reshape(n, (H // p) * (W // p), C * p * p)
    return t.permute(0, 2, 4, 3, 5, 1).reshape(n, (H // p) * (W // p), C * p * p)  # (py, px, c)


def unpatchify(rows, n, C, gh, gw, p, order="ppc"):
    if order == "ppc":
        t = rows.reshape(n, gh, gw, p, p, C).permute(0, 5, 1, 3, 2, 4)  # n c gy py gx px
    else:
        t = rows.reshape(n, gh, gw, C, p, p).permute(0, 3, 1, 4, 2, 5)
    return t.reshape(n, C, gh * p, gw * p)


def pos_window(pos, S, gh, gw, crop0=False):
    top, left = (0, 0) if crop0 else ((S - gh) // 2, (S - gw) // 2)
    return pos.reshape(S, S, -1)[top:top + gh, left:left + gw].reshape(gh * gw, -1)


def forward(sd, cfg, sample, timesteps, ctx, pooled, dt=None, mut=None, lora=None, mults=None):
    """sd: state dict (any float dtype); cfg: an object with the SD3Config fields; sample [n, Cin, H, W], timesteps [n],
    ctx [n, Nc, J], pooled [n, P].  lora: {module path: (down [r, in], up [out, r], alpha / r)} with mults [n] the
    per-sample multipliers: W + m (alpha / r) up down.  Returns float64 [n, Cout, H, W]."""
    rnd = _rounder(dt)
    W = {k: rnd(v.double()) for k, v in sd.items()}
    n = sample.shape[0]
    p, d, heads = cfg.patch_size, cfg.num_attention_heads * cfg.attention_head_dim, cfg.num_attention_heads
    gh, gw = sample.shape[2] // p, sample.shape[3] // p
    Nx = gh * gw
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
        one = 0.0 if mut == "scale_no_one" else 1.0
        return rnd(ln(x) * (one + scale[:, None]) + shift[:, None])

    def gate(h, g, f):
        if mut == "drop_gate":
            return rnd(h + f)
        return rnd(h + g[:, None] * f)

    act = gelu_erf if mut == "erf_gelu" else gelu_tanh
    # conditioning
    ts = rnd(timestep_sinusoid(torch.as_tensor(timesteps)))
    te = lin(rnd(silu(lin(ts, "time_text_embed.timestep_embedder.linear_1"))), "time_text_embed.timestep_embedder.linear_2")
    temb = lin(rnd(silu(lin(rnd(pooled.double()), "time_text_embed.text_embedder.linear_1"))),
               "time_text_embed.text_embedder.linear_2", res=te)
    st = rnd(silu(temb))
    # streams
    pm = rnd(patchify(sample.double(), p, "ppc" if mut == "patch_order" else "cpp"))
    pw = W["pos_embed.proj.weight"].reshape(d, -1)
    x = rnd(pm @ pw.t() + W["pos_embed.proj.bias"])
    x = rnd(x + pos_window(W["pos_embed.pos_embed"], cfg.pos_embed_max_size, gh, gw, mut == "pos_crop0")[None])
    c = lin(rnd(ctx.double()), "context_embedder")
    Nc = c.shape[1]

    def attn(q, k, v):
        def hd(t):
            return t.reshape(n, -1, heads, d // heads).transpose(1, 2)
        s = hd(q) @ hd(k).transpose(-1, -2) / math.sqrt(d // heads)
        return (torch.softmax(s, dim=-1) @ hd(v)).transpose(1, 2).reshape(n, -1, d)

    def tail(h, a, m6, b, out_name, ff):
        sm, scm, gm, sf, scf, gf = m6
        if mut == "swap_msa_mlp":
            sm, scm, gm, sf, scf, gf = sf, scf, gf, sm, scm, gm
        h = gate(h, gm, a if out_name is None else lin(a, b + out_name))
        f = lin(rnd(act(lin(adaln(h, scf, sf), b + ff + ".net.0.proj"))), b + ff + ".net.2")
        return gate(h, gf, f)

    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        last = i == cfg.num_layers - 1
        mx = lin(st, b + "norm1.linear").chunk(6, dim=1)
        mc = lin(st, b + "norm1_context.linear")
        if last:
            sc_c, sh_c = mc.chunk(2, dim=1)
            if mut == "swap_last_ctx":
                sc_c, sh_c = sh_c, sc_c
        else:
            mc = mc.chunk(6, dim=1)
            sh_c, sc_c = mc[0], mc[1]
        sh_x, sc_x = (mx[3], mx[4]) if mut == "swap_msa_mlp" else (mx[0], mx[1])
        if mut == "swap_msa_mlp" and not last:
            sh_c, sc_c = mc[3], mc[4]
        xn, cn = adaln(x, sc_x, sh_x), adaln(c, sc_c, sh_c)
        qx, kx, vx = (lin(xn, b + "attn." + k) for k in ("to_q", "to_k", "to_v"))
        qc, kc, vc = (lin(cn, b + "attn." + k) for k in ("add_q_proj", "add_k_proj", "add_v_proj"))
        if mut == "own_stream_attn":
            ox, oc = rnd(attn(qx, kx, vx)), rnd(attn(qc, kc, vc))
        else:
            o = rnd(attn(torch.cat([qx, qc], 1), torch.cat([kx, kc], 1), torch.cat([vx, vc], 1)))
            ox, oc = o[:, :Nx], o[:, Nx:]
        x = tail(x, ox, mx, b, "attn.to_out.0", "ff")
        if not last:
            c = tail(c, oc, mc, b, None if mut == "skip_to_add_out" else "attn.to_add_out", "ff_context")
    mo = lin(st, "norm_out.linear")
    sc_o, sh_o = mo.chunk(2, dim=1)
    if mut == "swap_norm_out":
        sc_o, sh_o = sh_o, sc_o
    y = lin(adaln(x, sc_o, sh_o), "proj_out")
    return unpatchify(y, n, cfg.out_channels, gh, gw, p, "cpp" if mut == "unpatch_order" else "ppc")


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def model_bar(sd, cfg, sample, timesteps, ctx, pooled, dt, ref=None, **kw):
    """(bar, ref): 2 x the twin's relative-L2 distance from float64 on these inputs."""
    if ref is None:
        ref = forward(sd, cfg, sample, timesteps, ctx, pooled, **kw)
    twin = forward(sd, cfg, sample, timesteps, ctx, pooled, dt=dt, **kw)
    return 2.0 * rel_l2(twin, ref), ref


# ---------------------------------------------------------------------------------------------------------------
# per-kernel references and bounds
# ---------------------------------------------------------------------------------------------------------------
def _store(ref, dt):
    return unit_roundoff(dt) * ref.abs() + sub_eta(dt)


def adaln_ref(x, mod, rps, off_scale, off_shift, eps):
    """x [M, C], mod [n, ldm] -> dict(y, mean, rstd, xh, scale, shift) in float64."""
    xd = x.double()
    M, C = xd.shape
    s = torch.arange(M) // rps
    sc = mod.double()[s, off_scale:off_scale + C]
    sh = mod.double()[s, off_shift:off_shift + C]
    mean = xd.mean(dim=1)
    var = ((xd - mean[:, None]) ** 2).mean(dim=1)
    rstd = (var + eps) ** -0.5
    xh = (xd - mean[:, None]) * rstd[:, None]
    return {"y": xh * (1 + sc) + sh, "mean": mean, "rstd": rstd, "xh": xh, "scale": sc, "shift": sh}


def adaln_bound(ref, dt):
    """The store; x - mean, times rstd, 1 + scale, the product, + shift (four fp32 roundings on the product, one on the sum);
    the statistics bar of norm_refs (d xh = xh S + S) through the factor (1 + scale)."""
    g = (1 + ref["scale"]).abs()
    y = ref["y"]
    return (_store(y, dt) + 4 * U32 * (ref["xh"] * g).abs() + U32 * y.abs()
            + STAT_BAR * g * (ref["xh"].abs() + 1) + FLOOR)


def gate_ref(h, f, mod, rps, off_gate):
    M, C = h.shape
    g = mod.double()[torch.arange(M) // rps, off_gate:off_gate + C]
    prod = g * f.double()
    return h.double() + prod, h.double().abs() + prod.abs()


def gate_bound(ref, mag, dt):
    return _store(ref, dt) + U32 * mag + FLOOR  # one fused multiply-add in fp32, one store


def add_pos_bound(ref, mag, dt):
    return _store(ref, dt) + U32 * mag + FLOOR  # one fp32 addition, one store


def gelu_tanh_bound(x, ref, dt):
    """x sigmoid(2u), 2u = 2 sqrt(2/pi) x (1 + 0.044715 x^2): the argument carries four fp32 roundings (4 U32 |2u| absolute on
    the exponent, so relative on e = exp(-2u)), __expf 2 ulp and its own argument product (|2u| U32), 1 + e and the division
    one each.  d y / y = (e / (1 + e)) d e / e + 2 U32."""
    xd = x.double()
    u2 = 2 * math.sqrt(2 / math.pi) * xd * (1 + 0.044715 * xd * xd)
    e_frac = torch.sigmoid(-u2)  # e / (1 + e)
    rel = U32 * (e_frac * (5 * u2.abs() + 4) + 3)
    return _store(ref, dt) + rel * ref.abs() + FLOOR


# ---------------------------------------------------------------------------------------------------------------
# the flow-matching scheduler and the sweep loop, restated
# ---------------------------------------------------------------------------------------------------------------
def shift_sigma(s, shift=3.0):
    return shift * s / (1 + (shift - 1) * s)


def flow_sigmas(num_inference_steps, num_train_timesteps=1000, shift=3.0):
    """(timesteps [n], sigmas [n + 1]) of FlowMatchEulerDiscreteScheduler.set_timesteps, float64."""
    base = torch.linspace(1, num_train_timesteps, num_train_timesteps, dtype=torch.float64).flip(0) / num_train_timesteps
    sig = shift_sigma(base, shift)
    t = torch.linspace(float(sig.max()) * num_train_timesteps, float(sig.min()) * num_train_timesteps, num_inference_steps,
                       dtype=torch.float64)
    s = shift_sigma(t / num_train_timesteps, shift)  # shifted once more, as the published class does
    return s * num_train_timesteps, torch.cat([s, torch.zeros(1, dtype=torch.float64)])


def sweep_loop(model_fn, latents, steps, guidance, start=0, total=None):
    """CFG Euler loop over timesteps[start:total]: model_fn(x2 [2n, ...], t) -> v [2n, ...] with the unconditional half
    first; x += (sigma_{i+1} - sigma_i) (u + g (c - u)).  Float64."""
    ts, sig = flow_sigmas(steps)
    total = steps if total is None else total
    x = latents.double()
    for i in range(start, total):
        v = model_fn(torch.cat([x, x]), float(ts[i]))
        u, c = v.chunk(2)
        x = x + (sig[i + 1] - sig[i]) * (u + guidance * (c - u))
    return x
