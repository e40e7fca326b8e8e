"""References for the SD3 MMDiT backward: per-element float64 references and bounds of the three backward kernels
(adaln_modulate_bwd, gate_residual_bwd, the tanh-GELU backward), and the model's LoRA gradients.  Torch only, no GPU
import, nothing from the package under test.  Imports mmdit_refs and changes nothing in it.

KERNEL BOUNDS, in the manner of mmdit_refs.adaln_bound / gelu_tanh_bound: u the storage rounding, U32 one fp32 rounding,
STAT_BAR what the forward's saved statistics may be off by; the GPU tests assert |got - ref| <= SLACK E.

MODEL GRADIENTS.  Form A: torch autograd through `mmdit_refs.forward(..., lora=, mults=)` in float64 (`grads_a`).
Form B: `twin_forward`, the same network restated here op by op so that (1) every tensor the engine stores in 16 bit is
rounded on the way forward AND its gradient on the way back (the straight-through `_Store` of notrigger_refs.py, under a
power-of-two scale as the engine's loss scale), and (2) a backward can be mutated.  With dt=None and no mutation the
twin IS form A (the CPU test holds its output and gradients to A at 1e-12), so the twin's rounded form and its mutants are
statements about the same function.  Bar: 3 e_q + 1e-4 with e_q = rel(B, A), the project's standing margin for gradients
(notrigger_refs.bar).

What the engine differentiates: the LoRA matrices only.  scale / shift / gate depend on temb alone and take no gradient."""
import math

import torch

import mmdit_refs as R
from mmdit_refs import FLOOR, SLACK, STAT_BAR, U32, sub_eta, unit_roundoff, worst  # noqa: F401
from notrigger_refs import bar, rel, store  # noqa: F401

F64 = torch.float64

BWD_MUTATIONS = ("drop_mean_g", "drop_mean_gx", "bwd_scale_no_one", "bwd_drop_gate", "cut_ctx_split", "drop_add", "abs_mult")


# ---------------------------------------------------------------------------------------------------------------
# per-kernel references and bounds
# ---------------------------------------------------------------------------------------------------------------
def _store_e(ref, dt):
    return unit_roundoff(dt) * ref.abs() + sub_eta(dt)


def adaln_bwd_ref(x, dy, mod, rps, off_scale, eps, add=None):
    """x, dy [M, C], mod [n, ldm] -> dict(dx, and the pieces the bound reads) in float64, statistics from x in float64."""
    f = R.adaln_ref(x, mod, rps, off_scale, off_scale, eps)
    xh, rstd, sc = f["xh"], f["rstd"][:, None], f["scale"]
    g = dy.double() * (1 + sc)
    m1 = g.mean(dim=1, keepdim=True)
    m2 = (g * xh).mean(dim=1, keepdim=True)
    d = rstd * (g - m1 - xh * m2)
    a = torch.zeros_like(d) if add is None else add.double()
    return {"dx": d + a, "d": d, "add": a, "g": g, "xh": xh, "m1": m1, "m2": m2, "rstd": rstd, "mean": f["mean"],
            "rstd_row": f["rstd"]}


def adaln_bwd_bound(ref, dt):
    """The store; g = dy (1 + scale) (two fp32 roundings); xhat (two roundings, and the statistics bar: d xh = xh S + S);
    the two row sums, each a chain of L fp32 additions (8 per 512 columns in a lane, 6 shuffle steps, the scaling by 1 / C)
    on terms that carry their own error; the combination (three roundings at the size of its terms); rstd (S relative);
    the addition of `add`."""
    g, xh, m1, m2, rstd = ref["g"], ref["xh"], ref["m1"], ref["m2"], ref["rstd"]
    C = g.shape[1]
    L = 8 * ((C + 511) // 512) + 6 + 1
    e_g = 2 * U32 * g.abs()
    e_xh = 2 * U32 * xh.abs() + STAT_BAR * (xh.abs() + 1)
    e_m1 = L * U32 * g.abs().mean(dim=1, keepdim=True) + e_g.mean(dim=1, keepdim=True)
    gx = (g * xh).abs()
    e_m2 = (L + 1) * U32 * gx.mean(dim=1, keepdim=True) + (g.abs() * e_xh + xh.abs() * e_g).mean(dim=1, keepdim=True)
    inner = e_g + e_m1 + xh.abs() * e_m2 + m2.abs() * e_xh + 3 * U32 * (g.abs() + m1.abs() + (xh * m2).abs())
    e_d = rstd * inner + (STAT_BAR + U32) * ref["d"].abs()
    return _store_e(ref["dx"], dt) + e_d + U32 * (ref["d"].abs() + ref["add"].abs()) + FLOOR


def gate_bwd_ref(dy, mod, rps, off_gate):
    M, C = dy.shape
    g = mod.double()[torch.arange(M) // rps, off_gate:off_gate + C]
    return g * dy.double()


def gate_bwd_bound(ref, dt):
    return _store_e(ref, dt) + U32 * ref.abs() + FLOOR  # one fp32 product, one store


_C = 2 * math.sqrt(2 / math.pi)
_A = 0.044715


def gelu_tanh_grad(x):
    """d/dx [x sigmoid(w)], w = c x (1 + a x^2): s + x s (1 - s) w', float64, through t = exp(-|w|) (no overflow, no
    cancellation in 1 - s).  Returns (act', s, B = x w' s (1 - s), w)."""
    xd = x.double()
    w = _C * xd * (1 + _A * xd * xd)
    t = torch.exp(-w.abs())
    r = 1 / (1 + t)
    s = torch.where(w >= 0, r, t * r)
    B = xd * _C * (1 + 3 * _A * xd * xd) * t * r * r
    return s + B, s, B, w


def gelu_tanh_bwd_ref(x, dy):
    return dy.double() * gelu_tanh_grad(x)[0]


def gelu_tanh_bwd_bound(x, dy, dt):
    """t = exp(-|w|) carries the relative error of mmdit_refs.gelu_tanh_bound's exponential, dt = U32 (5 |w| + 4): four fp32
    roundings in w, the exponent product, __expf 2 ulp.  s = 1 / (1 + t) or t / (1 + t): d s = s (1 - s) dt + 2 U32 s.
    B = x w' t / (1 + t)^2: |d B| <= |B| (dt + 10 U32) (w' three roundings, 1 + t, the reciprocal, its square, the products).
    The sum s + B one more at the size of its terms -- this is where act' cancels near x = -0.75 -- then the product with dy
    and the store."""
    d, s, B, w = gelu_tanh_grad(x)
    e_t = U32 * (5 * w.abs() + 4)
    e_d = e_t * (s * (1 - s) + B.abs()) + U32 * (3 * s + 11 * B.abs())
    ref = dy.double() * d
    return _store_e(ref, dt) + dy.double().abs() * e_d + U32 * ref.abs() + FLOOR


# ---------------------------------------------------------------------------------------------------------------
# the model: LoRA sites, form A, and the twin (form B and the mutants)
# ---------------------------------------------------------------------------------------------------------------
X_PARTS = ("to_q", "to_k", "to_v", "to_out.0")
C_PARTS = ("add_q_proj", "add_k_proj", "add_v_proj", "to_add_out")


def site_names(num_layers, context_stream):
    """Engine targets in flat-buffer order: per block to_q, to_k, to_v (adjacent: one fused GEMM), to_out.0 -- the reference's
    96 modules at 24 layers -- and with context_stream add_q_proj, add_k_proj, add_v_proj, to_add_out (not in the last block):
    191 at 24 layers."""
    out = []
    for i in range(num_layers):
        out += [f"transformer_blocks.{i}.attn.{p}" for p in X_PARTS]
        if context_stream:
            out += [f"transformer_blocks.{i}.attn.{p}" for p in (C_PARTS[:3] if i == num_layers - 1 else C_PARTS)]
    return out


def make_lora(names, d, rank, alpha, gen, up_std=0.05):
    """{name: (down [r, d], up [d, r], alpha / r)} float64 with fp32-representable values (the flat buffers are fp32); `up`
    seeded non-zero (a zero up gives a zero down gradient)."""
    out = {}
    for nm in names:
        down = (torch.randn((rank, d), generator=gen, dtype=F64) / math.sqrt(d)).float().to(F64)
        up = (torch.randn((d, rank), generator=gen, dtype=F64) * up_std).float().to(F64)
        out[nm] = (down, up, alpha / rank)
    return out


def flat_layout(names, d, rank, alpha):
    """The sites table of smi_mmdit_train_create and the sizes of the two flat buffers."""
    sites, od, ou = [], 0, 0
    for nm in names:
        sites.append(dict(target=nm, off_down=od, off_up=ou, rank=rank, scale=alpha / rank))
        od += rank * d
        ou += d * rank
    return sites, od, ou


def flatten_lora(lora, names):
    return (torch.cat([lora[n][0].reshape(-1) for n in names]).float(),
            torch.cat([lora[n][1].reshape(-1) for n in names]).float())


def _leaves(lora):
    return {k: (dn.clone().requires_grad_(True), up.clone().requires_grad_(True), sc) for k, (dn, up, sc) in lora.items()}


def _collect(out, d_out, leaves, names):
    """(flat d_down, flat d_up, {name: (d_down, d_up)}) of <d_out, out>, float64; sites the output does not reach get zeros."""
    ps = [t for n in names for t in leaves[n][:2]]
    gs = torch.autograd.grad((out * d_out.double()).sum(), ps, allow_unused=True)
    gs = [torch.zeros_like(p) if g is None else g for p, g in zip(ps, gs)]
    per = {n: (gs[2 * i], gs[2 * i + 1]) for i, n in enumerate(names)}
    return (torch.cat([per[n][0].reshape(-1) for n in names]), torch.cat([per[n][1].reshape(-1) for n in names]), per)


def grads_a(sd, cfg, sample, timesteps, ctx, pooled, lora, names, mults, d_out):
    """Form A: float64 autograd through mmdit_refs.forward."""
    leaves = _leaves(lora)
    out = R.forward(sd, cfg, sample, timesteps, ctx, pooled, lora=leaves, mults=mults)
    return _collect(out, d_out, leaves, names) + (out.detach(),)


def grads_twin(sd, cfg, sample, timesteps, ctx, pooled, lora, names, mults, d_out, dt=None, mut=None):
    """The twin's gradients: dt=None, mut=None is form A restated; dt a 16-bit type is form B; mut a mutated backward."""
    leaves = _leaves(lora)
    out = twin_forward(sd, cfg, sample, timesteps, ctx, pooled, leaves, mults, dt=dt, mut=mut)
    if dt is not None:  # d_out enters the engine as 16-bit rows under the sample's loss scale
        out = store(out, dt)
    return _collect(out, d_out, leaves, names) + (out.detach(),)


class _AdaLN(torch.autograd.Function):
    """LN(x) (1 + scale) + shift; the backward to x as the kernel forms it, with the terms a mutant drops."""

    @staticmethod
    def forward(ctx, x, scale, shift, mut):
        m = x.mean(dim=-1, keepdim=True)
        rstd = (((x - m) ** 2).mean(dim=-1, keepdim=True) + 1e-6) ** -0.5
        xh = (x - m) * rstd
        ctx.save_for_backward(xh, rstd, scale)
        ctx.mut = mut
        return xh * (1 + scale[:, None]) + shift[:, None]

    @staticmethod
    def backward(ctx, dy):
        xh, rstd, scale = ctx.saved_tensors
        g = dy if ctx.mut == "bwd_scale_no_one" else dy * (1 + scale[:, None])
        m1 = 0.0 if ctx.mut == "drop_mean_g" else g.mean(dim=-1, keepdim=True)
        m2 = 0.0 if ctx.mut == "drop_mean_gx" else (g * xh).mean(dim=-1, keepdim=True)
        return rstd * (g - m1 - xh * m2), None, None, None


class _Gate(torch.autograd.Function):
    """h + gate f.  dh = dy: in the engine it reaches h's slot as the `add` operand of the adaLN backward that follows (every
    h also feeds an adaLN), so a dropped `add` is a lost dh; df = gate dy."""

    @staticmethod
    def forward(ctx, h, gate, f, mut):
        ctx.save_for_backward(gate)
        ctx.mut = mut
        return h + gate[:, None] * f

    @staticmethod
    def backward(ctx, dy):
        (gate,) = ctx.saved_tensors
        dh = torch.zeros_like(dy) if ctx.mut == "drop_add" else dy
        df = dy if ctx.mut == "bwd_drop_gate" else gate[:, None] * dy
        return dh, None, df, None


class _CutGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return torch.zeros_like(g)


class _LoraDelta(torch.autograd.Function):
    """m s (x down^T) up^T per sample.  The engine applies sigma_i = m_i / max |m| to the rows of xa = x down^T on the way
    forward and to the rows of dxa = dy up on the way back: d(up) reads xa, d(down) and dx read dxa.  mut 'abs_mult': the
    backward's sigma without its sign."""

    @staticmethod
    def forward(ctx, x, down, up, m, sc, mut):
        xa = m * (x @ down.t())
        ctx.save_for_backward(x, down, up, xa, m)
        ctx.sc, ctx.mut = sc, mut
        return sc * (xa @ up.t())

    @staticmethod
    def backward(ctx, dy):
        x, down, up, xa, m = ctx.saved_tensors
        mb = m.abs() if ctx.mut == "abs_mult" else m
        dxa = mb * (dy @ up)
        d_up = ctx.sc * torch.einsum("bto,btr->or", dy, xa)
        d_down = ctx.sc * torch.einsum("btr,btk->rk", dxa, x)
        return ctx.sc * (dxa @ down), d_down, d_up, None, None, None


def twin_forward(sd, cfg, sample, timesteps, ctx, pooled, lora, mults, dt=None, mut=None):
    """mmdit_refs.forward restated with `store` (value and gradient rounded) at its rounding sites and the ops above."""
    st = (lambda t: t) if dt is None else (lambda t: store(t, dt))
    rnd = R._rounder(dt)
    W = {k: rnd(v.double()) for k, v in sd.items()}
    n = sample.shape[0]
    p, d, heads = cfg.patch_size, cfg.num_attention_heads * cfg.attention_head_dim, cfg.num_attention_heads
    gh, gw = sample.shape[2] // p, sample.shape[3] // p
    Nx = gh * gw
    mv = torch.as_tensor(mults, dtype=F64)

    def lin(x, name, res=None):
        y = x @ W[name + ".weight"].t() + W[name + ".bias"]
        if name in lora:
            dn, up, sc = lora[name]
            y = y + _LoraDelta.apply(x, dn, up, mv.reshape([n] + [1] * (x.dim() - 1)), sc, mut)
        if res is not None:
            y = y + res
        return st(y)

    def adaln(x, scale, shift):
        return st(_AdaLN.apply(x, scale, shift, mut))

    def gate(h, g, f):
        return st(_Gate.apply(h, g, f, mut))

    with torch.no_grad():  # nothing adapted is upstream of these
        ts = rnd(R.timestep_sinusoid(torch.as_tensor(timesteps)))
        te = lin(rnd(R.silu(lin(ts, "time_text_embed.timestep_embedder.linear_1"))), "time_text_embed.timestep_embedder.linear_2")
        temb = lin(rnd(R.silu(lin(rnd(pooled.double()), "time_text_embed.text_embedder.linear_1"))),
                   "time_text_embed.text_embedder.linear_2", res=te)
        s_t = rnd(R.silu(temb))
        pm = rnd(R.patchify(sample.double(), p))
        x = rnd(pm @ W["pos_embed.proj.weight"].reshape(d, -1).t() + W["pos_embed.proj.bias"])
        x = rnd(x + R.pos_window(W["pos_embed.pos_embed"], cfg.pos_embed_max_size, gh, gw)[None])
        c = lin(rnd(ctx.double()), "context_embedder")

    def attn(q, k, v):
        def hd(t):
            return t.reshape(n, -1, heads, d // heads).transpose(1, 2)
        s = hd(q) @ hd(k).transpose(-1, -2) / math.sqrt(d // heads)
        return (torch.softmax(s, dim=-1) @ hd(v)).transpose(1, 2).reshape(n, -1, d)

    def tail(h, a, m6, b, out_name, ff):
        _sm, _scm, gm, sf, scf, gf = m6
        h = gate(h, gm, lin(a, b + out_name))
        f = lin(st(R.gelu_tanh(lin(adaln(h, scf, sf), b + ff + ".net.0.proj"))), b + ff + ".net.2")
        return gate(h, gf, f)

    for i in range(cfg.num_layers):
        b = f"transformer_blocks.{i}."
        last = i == cfg.num_layers - 1
        with torch.no_grad():
            mx = lin(s_t, b + "norm1.linear").chunk(6, dim=1)
            mc = lin(s_t, b + "norm1_context.linear")
            if last:
                sc_c, sh_c = mc.chunk(2, dim=1)
            else:
                mc = mc.chunk(6, dim=1)
                sh_c, sc_c = mc[0], mc[1]
        xn, cn = adaln(x, mx[1], mx[0]), adaln(c, sc_c, sh_c)
        qx, kx, vx = (lin(xn, b + "attn." + k) for k in ("to_q", "to_k", "to_v"))
        qc, kc, vc = (lin(cn, b + "attn." + k) for k in ("add_q_proj", "add_k_proj", "add_v_proj"))
        o = st(attn(torch.cat([qx, qc], 1), torch.cat([kx, kc], 1), torch.cat([vx, vc], 1)))
        ox, oc = o[:, :Nx], o[:, Nx:]
        if mut == "cut_ctx_split":
            oc = _CutGrad.apply(oc)
        x = tail(x, ox, mx, b, "attn.to_out.0", "ff")
        if not last:
            c = tail(c, oc, mc, b, "attn.to_add_out", "ff_context")
    with torch.no_grad():
        sc_o, sh_o = lin(s_t, "norm_out.linear").chunk(2, dim=1)
    y = lin(adaln(x, sc_o, sh_o), "proj_out")
    return R.unpatchify(y, n, cfg.out_channels, gh, gw, p)


# ---------------------------------------------------------------------------------------------------------------
# seeded inputs shared by the CPU and GPU tests
# ---------------------------------------------------------------------------------------------------------------
def tiny_inputs(cfg, n, h, w, n_ctx, seed):
    """(sample, timesteps, ctx, pooled, d_out): float32 / 16-bit-representable values, so every form reads the same numbers."""
    g = torch.Generator().manual_seed(seed)
    sample = torch.randn((n, cfg.in_channels, h, w), generator=g)
    ts = [float(t) for t in torch.randint(1, 1000, (n,), generator=g)]
    ctx = torch.randn((n, n_ctx, cfg.joint_attention_dim), generator=g).half().float()
    pooled = torch.randn((n, cfg.pooled_projection_dim), generator=g).half().float()
    d_out = torch.randn((n, cfg.out_channels, h, w), generator=g)
    return sample, ts, ctx.bfloat16().float(), pooled.bfloat16().float(), d_out
