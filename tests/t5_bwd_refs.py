"""Float64 references for the backward kernels of the T5 tower (csrc/t5.hip rmsnorm_rows_bwd_kernel and
gated_gelu_tanh_bwd_kernel, the BIAS forms of attn_bwd_dq_body / attn_bwd_dkv_body in csrc/attention.hip): per-kernel
references, first-order error bounds, rounding emulations and the mutated references that show what each bound can see,
in the manner of t5_refs.py and attention_refs.py.  Torch only, no transformers module inside, no GPU import.

ROUNDING SITES, u = 2^-11 (fp16) or 2^-8 (bf16), U32 = 2^-24:
  rmsnorm_rows_bwd   dx = r g - x c (+ add), g = w dy, c = r^3 mean(x . g), all fp32, ONE 16-bit rounding at the store.  With
                     L = t5_refs.rms_sum_depth(C) the depth of the two fp32 row sums:
                       E = u |dx| + (L / 2 + 6) U32 t1 + (5 L / 2 + 15) U32 t2 + 2 U32 |add| + eta + FLOOR,
                       t1 = r |g|,  t2 = |x| r^3 mean|x g|
                     r carries (L / 2 + 3) U32 (the sum of squares halved, v_rsq, the mean and the eps add), r^3 three times
                     that; the sum x . g carries L U32 of mean|x g| (>= |mean(x g)|: the cancellation inside the sum is what the
                     absolute value pays for); the products and the FMA are the constants.
  gated_gelu_tanh_bwd  gate half dout up gelu_tanh'(gate), up half dout gelu_tanh(gate), fp32, ONE rounding each.
                       E = u |y| + 32 U32 (|y| + |dout up| [gate half]) + eta + FLOOR: gelu_tanh' = s + x w' t r^2 has a zero
                       near x = -0.75 where its two terms (each below 1) cancel, hence the absolute term on the gate half.
  attention (BIAS)   attention_refs' B1 .. B4 with P recomputed as exp(scale q.k + table[k - q + L - 1] - lse[q]): the bounds are
                     attention_refs.bounds on the BIASED reference (P, dS, dQ, dK, dV of the biased softmax) plus THE BIAS TERM:
                     the exponent's argument (scale s - lse) + bias is formed in fp32 from terms of size |scale s|, |lse| and
                     |bias| (100 in the inputs below), so P carries e_P = 4 U32 (|scale s| + |lse| + |bias|) P, which enters
                       E_dS += |dP - delta| e_P,   E_dV += e_P^T |dO|
                     and through E_dS both E_dQ and E_dK.
The assertion is elementwise |got - ref| <= SLACK E (+ attention_refs.TINY for the attention)."""
import torch

import attention_refs as A
import t5_refs as R
from norm_refs import FLOOR, SLACK, U32, sub_eta, unit_roundoff, worst  # noqa: F401  (re-exported for the tests)

# ---------------------------------------------------------------------------------------------------------------
# rmsnorm_rows_bwd
# ---------------------------------------------------------------------------------------------------------------
RMS_CASES = R.RMS_CASES
RMS_BWD_MUTANTS = ("projection_dropped", "r_not_cubed", "weight_dropped")
RMS_EPS = 1e-6


def rms_bwd_inputs(M, C, dt, seed=0):
    """x, w of t5_refs.rms_inputs (rows of magnitude 1, 1e-3, 60; in bf16 the last row at 3e4), dy = N + 0.5 x / rms(x): the
    part along x is what the projection term removes, so that term is of the size of the result; add = 0.7 N."""
    x, w = R.rms_inputs(M, C, dt, seed)
    g = torch.Generator().manual_seed(seed + 11 * M + C)
    xf = x.float()
    dy = torch.randn(M, C, generator=g) + 0.5 * xf / xf.pow(2).mean(-1, keepdim=True).sqrt()
    add = 0.7 * torch.randn(M, C, generator=g)
    return x, w, dy.to(dt), add.to(dt)


def rms_bwd_terms(x, w, dy, eps):
    x, g = x.double(), w.double() * dy.double()
    r = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return x, g, r


def rms_bwd_ref(x, w, dy, add=None, eps=RMS_EPS, fault=None):
    x, g, r = rms_bwd_terms(x, w, dy, eps)
    if fault == "weight_dropped":
        g = dy.double()
    proj = x * (r if fault == "r_not_cubed" else r ** 3) * (x * g).mean(-1, keepdim=True)
    dx = r * g - (0.0 if fault == "projection_dropped" else proj)
    return dx if add is None else dx + add.double()


def rms_bwd_autograd(x, w, dy, eps=RMS_EPS):
    """The same gradient from torch autograd through t5_refs.rms in float64 (what rms_bwd_ref's closed form must equal)."""
    xv = x.double().requires_grad_(True)
    y = R.rms(xv, w.double(), eps)
    return torch.autograd.grad(y, xv, dy.double())[0]


def rms_bwd_bound(x, w, dy, add, ref, C, dt, eps=RMS_EPS):
    xd, g, r = rms_bwd_terms(x, w, dy, eps)
    L = R.rms_sum_depth(C)
    t1 = r * g.abs()
    t2 = xd.abs() * r ** 3 * (xd * g).abs().mean(-1, keepdim=True)
    e = unit_roundoff(dt) * ref.abs() + (L / 2 + 6) * U32 * t1 + (5 * L / 2 + 15) * U32 * t2 + sub_eta(dt) + FLOOR
    return e if add is None else e + 2 * U32 * add.double().abs()


def rms_bwd_emulate(x, w, dy, add, dt, eps=RMS_EPS):
    """fp32 arithmetic in the kernel's order of operations (not of its sums), one rounding to dt."""
    xf, g = x.float(), w.float() * dy.float()
    r = torch.rsqrt((xf * xf).sum(-1, keepdim=True) * (1.0 / x.shape[-1]) + eps)
    c = r * r * r * ((xf * g).sum(-1, keepdim=True) * (1.0 / x.shape[-1]))
    t = r * g - xf * c
    return (t if add is None else t + add.float()).to(dt)


# ---------------------------------------------------------------------------------------------------------------
# gated_gelu_tanh_bwd
# ---------------------------------------------------------------------------------------------------------------
GG_CASES = R.GG_CASES
GG_BWD_MUTANTS = ("halves_swapped", "erf_derivative", "up_without_gelu")


def gg_bwd_inputs(M, F, dt, seed=0):
    """proj of t5_refs.gg_inputs (a quarter of the gates in [-4, -1], where the tanh and erf forms differ) and dout = N."""
    proj = R.gg_inputs(M, F, dt, seed)
    dout = torch.randn(M, F, generator=torch.Generator().manual_seed(seed + 3 * M + F))
    return proj, dout.to(dt)


def dgelu_tanh(x):
    """d/dx of t5_refs.gelu_tanh = x sigmoid(2 u): s + x s (1 - s) 2 u'."""
    k = 2.0 * (2.0 / torch.pi) ** 0.5
    s = torch.sigmoid(k * (x + 0.044715 * x ** 3))
    return s + x * s * (1.0 - s) * k * (1.0 + 3.0 * 0.044715 * x * x)


def dgelu_erf(x):
    return 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5


def gg_bwd_ref(proj, dout, fault=None):
    """dproj [M, 2 F] = gate half | up half in float64."""
    F = proj.shape[1] // 2
    g, v, d = proj[:, :F].double(), proj[:, F:].double(), dout.double()
    dg = d * v * (dgelu_erf(g) if fault == "erf_derivative" else dgelu_tanh(g))
    du = d * (1.0 if fault == "up_without_gelu" else R.gelu_tanh(g))
    return torch.cat([du, dg] if fault == "halves_swapped" else [dg, du], dim=1)


def gg_bwd_autograd(proj, dout):
    pv = proj.double().requires_grad_(True)
    return torch.autograd.grad(R.gg_ref(pv), pv, dout.double())[0]


def gg_bwd_bound(proj, dout, ref, dt):
    F = proj.shape[1] // 2
    e = unit_roundoff(dt) * ref.abs() + 32 * U32 * ref.abs() + sub_eta(dt) + FLOOR
    e[:, :F] += 32 * U32 * (dout.double() * proj[:, F:].double()).abs()
    return e


def gg_bwd_emulate(proj, dout, dt):
    """fp32, the kernel's expressions (dgelu_tanh_f of smi_common.h and the forward's GELU), one rounding to dt."""
    F = proj.shape[1] // 2
    x, v, d = proj[:, :F].float(), proj[:, F:].float(), dout.float()
    w = 1.5957691216057308 * x * (0.044715 * (x * x) + 1.0)
    t = torch.exp(-w.abs())
    r = 1.0 / (1.0 + t)
    s = torch.where(w >= 0, r, t * r)
    dw = 1.5957691216057308 * (3.0 * 0.044715 * (x * x) + 1.0)
    dg = (d * v) * (x * dw * (t * r * r) + s)
    du = d * (x / (1.0 + torch.exp(-w)))
    return torch.cat([dg, du], dim=1).to(dt)


# ---------------------------------------------------------------------------------------------------------------
# attention backward with the bias table
# ---------------------------------------------------------------------------------------------------------------
ATTN_B, ATTN_H, ATTN_D = R.ATTN_B, R.ATTN_H, R.ATTN_D
ATTN_BWD_LENGTHS = (1, 3, 63, 64, 65, 77, 128, 129, 130, 193, 256, 257)
ATTN_LONG = R.ATTN_LONG
ATTN_BWD_MUTANTS = ("bias_dropped", "bias_mirrored", "bias_after_lse_negated", "no_delta")
GRADS = ("q+kv", "q", "kv")


def attn_bwd_inputs(B, H, L, dt, seed=0):
    """q, k, v, table of t5_refs.attn_inputs (one table entry at BIG_BIAS) and d_o = N."""
    q, k, v, table = R.attn_inputs(B, H, L, dt, seed)
    d_o = torch.randn(B, L, H, ATTN_D, generator=torch.Generator().manual_seed(seed + 17 * L + H))
    return q, k, v, table, d_o.to(dt)


def attn_bias_bwd_ref(q, k, v, table, d_o, scale, fault=None):
    """{O, P, lse, dP, delta, dS, dQ, dK, dV} in float64: the forward on the biased scores, the backward with P recomputed
    from the forward's lse as the kernels do.  Faults are faults of the BACKWARD's recompute alone (O and lse stay right):
      bias_dropped             P = exp(scale s - lse)
      bias_mirrored            the table read at query - key
      bias_after_lse_negated   P = exp(scale s - (lse + bias)): the bias subtracted with the row statistic
      no_delta                 dS = P dP"""
    q, k, v, g = q.double(), k.double(), v.double(), d_o.double()
    L = q.shape[1]
    bias = R.expand_table(table.double(), L)[None]
    s0 = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    s = s0 + bias
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhqk,bkhd->bqhd", p, v)
    bb = {"bias_dropped": torch.zeros_like(bias), "bias_mirrored": bias.transpose(2, 3), "bias_after_lse_negated": -bias}.get(fault, bias)
    pb = p if fault in (None, "no_delta") else torch.exp(s0 + bb - lse[..., None])
    dp = torch.einsum("bqhd,bkhd->bhqk", g, v)
    delta = torch.einsum("bqhd,bqhd->bhq", g, o)
    ds = pb * (dp if fault == "no_delta" else dp - delta[..., None])
    return {"O": o, "P": p, "lse": lse, "dP": dp, "delta": delta, "dS": ds, "S0": s0, "bias": bias,
            "dQ": torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale,
            "dK": torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale,
            "dV": torch.einsum("bhqk,bqhd->bkhd", pb, g)}


def attn_bias_bwd_autograd(q, k, v, table, d_o, scale):
    """dQ, dK, dV from torch autograd through the biased softmax in float64 (the table a constant)."""
    qv, kv, vv = (t.double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", qv, kv) * scale + R.expand_table(table.double(), q.shape[1])[None]
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), vv)
    return dict(zip(("dQ", "dK", "dV"), torch.autograd.grad(o, (qv, kv, vv), d_o.double())))


def attn_bias_bwd_bounds(ref, q, k, v, d_o, scale, dt):
    """attention_refs.bounds on the biased reference, extended with the bias term of the module docstring."""
    e = A.bounds(ref, q, k, v, d_o, scale, dt)
    qa, ka, ga = q.double().abs(), k.double().abs(), d_o.double().abs()
    e_p = 4 * U32 * (ref["S0"].abs() + ref["lse"].abs()[..., None] + ref["bias"].abs()) * ref["P"]
    e_ds = (ref["dP"] - ref["delta"][..., None]).abs() * e_p
    e["dQ"] = e["dQ"] + scale * torch.einsum("bhqk,bkhd->bqhd", e_ds, ka)
    e["dK"] = e["dK"] + scale * torch.einsum("bhqk,bqhd->bkhd", e_ds, qa)
    e["dV"] = e["dV"] + torch.einsum("bhqk,bqhd->bkhd", e_p, ga)
    return e


def attn_bias_bwd_emulate(q, k, v, table, d_o, scale, dt):
    """Float64 arithmetic with the roundings B1 .. B4 of attention_refs on the biased scores, the backward on
    attention_refs.bwd_inputs of the float64 reference (O rounded to dt, lse to fp32), as the GPU test runs it."""
    ref = attn_bias_bwd_ref(q, k, v, table, d_o, scale)
    o16, lse32 = A.bwd_inputs(ref, dt)
    q, k, v, g = q.double(), k.double(), v.double(), d_o.double()
    pb = torch.exp(ref["S0"] + ref["bias"] - lse32.double()[..., None])
    delta = torch.einsum("bqhd,bqhd->bhq", g, o16.double())
    ds = A.rnd16(pb * (ref["dP"] - delta[..., None]), dt)
    return {"dQ": A.rnd16(torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale, dt),
            "dK": A.rnd16(torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale, dt),
            "dV": A.rnd16(torch.einsum("bhqk,bqhd->bkhd", A.rnd16(pb, dt), g), dt)}


def expected_bias_path(L, B, H, grads, fused):
    """bwd_bias of csrc/attention.hip restated: the kernel families of smi_attn_ran.family, in order.  grads as in
    attention_refs.expected_path; fused: sel_fused (0 = off, anything else = on)."""
    want_q, want_kv = "q" in grads.split("+"), "kv" in grads.split("+")
    fam = [] if want_q else [A.DELTA]
    if fused != 0 and want_q and want_kv and -(-L // 128) * H * B <= 1024:
        return fam + [A.BWD_FUSED]
    return fam + ([A.DQ] if want_q else []) + ([A.DKV] if want_kv else [])


# ---------------------------------------------------------------------------------------------------------------
# the tower with LoRA sites (smi_t5_forward_lora / smi_t5_backward), float64 under torch autograd
# ---------------------------------------------------------------------------------------------------------------
# Form A is exact float64; form B rounds every tensor the engine stores (each op's output: the two RMSNorms, q|k|v, the
# attention output, the residual stream after o and after wo, wi_0|wi_1, the gated GELU, the final norm) through
# notrigger_refs.store, values and gradients.  e_q = |B - A| / |A|; a native result is held to notrigger_refs.bar(e_q) for the
# whole (down | up) vector and for each site's pair.
import notrigger_refs as N  # noqa: E402

SITE_PARTS = ("q", "k", "v", "o")
TOWER_MUTANTS = ("bias_dropped_bwd", "bias_mirrored_dkv", "final_norm_bwd_skipped", "wi_1_grad_dropped", "residual_grad_dropped",
                 "o_site_fed_q_rows", "qkv_order_permuted")


def halved_state(cfg, seed=0):
    """t5_refs.seeded_state with the q and k weights halved: scores of standard deviation ~ 3 instead of ~ 11, where the
    softmax is not saturated and the bf16 form B sits 1.4e-2 .. 1.7e-2 from form A instead of 0.14 .. 0.17 -- a bar that a
    dropped or mirrored bias misses by an order of magnitude, not by a factor of two."""
    sd = R.seeded_state(cfg, seed)
    for k in sd:
        if k.endswith(("SelfAttention.q.weight", "SelfAttention.k.weight")):
            sd[k] = sd[k] * 0.5
    return sd


def site_names(num_layers, parts=SITE_PARTS, layers=None):
    """Engine targets in flat-buffer order: per block q, k, v (adjacent, as the fused projection needs), then o."""
    return [f"encoder.block.{i}.layer.0.SelfAttention.{p}" for i in (layers if layers is not None else range(num_layers))
            for p in parts]


def site_dims(cfg, name):
    """(in, out) of a site's Linear."""
    inner = cfg.num_heads * cfg.d_kv
    return (inner, cfg.d_model) if name.endswith(".o") else (cfg.d_model, inner)


def make_lora(cfg, names, rank, gen, up_std=0.05):
    """{name: (down [r, in], up [out, r])} float64 with fp32-representable values, `up` seeded non-zero."""
    out = {}
    for nm in names:
        i, o = site_dims(cfg, nm)
        out[nm] = ((torch.randn((rank, i), generator=gen, dtype=N.F64) / i ** 0.5).float().to(N.F64),
                   (torch.randn((o, rank), generator=gen, dtype=N.F64) * up_std).float().to(N.F64))
    return out


def flat_layout(cfg, names, rank, alpha):
    """The sites table of smi_t5_lora_create and the sizes of the two flat buffers."""
    sites, od, ou = [], 0, 0
    for nm in names:
        i, o = site_dims(cfg, nm)
        sites.append(dict(target=nm, off_down=od, off_up=ou, rank=rank, scale=alpha / rank))
        od += rank * i
        ou += o * rank
    return sites, od, ou


flatten_lora = N.flatten_lora


class _BiasAttention(torch.autograd.Function):
    """softmax(q k^T + bias) v on [n, L, H, D] with the backward written out as the kernels compute it (P recomputed from the
    row statistic, the bias a constant), so that a fault can sit in the backward alone."""

    @staticmethod
    def forward(ctx, q, k, v, bias, fault):
        s = torch.einsum("nqhd,nkhd->nhqk", q, k) + bias[None]
        lse = torch.logsumexp(s, dim=-1)
        o = torch.einsum("nhqk,nkhd->nqhd", torch.exp(s - lse[..., None]), v)
        ctx.save_for_backward(q, k, v, bias, lse, o)
        ctx.fault = fault
        return o

    @staticmethod
    def backward(ctx, g):
        q, k, v, bias, lse, o = ctx.saved_tensors
        s0 = torch.einsum("nqhd,nkhd->nhqk", q, k)
        b_q = torch.zeros_like(bias) if ctx.fault == "bias_dropped_bwd" else bias
        b_kv = bias.transpose(1, 2) if ctx.fault == "bias_mirrored_dkv" else b_q
        dp = torch.einsum("nqhd,nkhd->nhqk", g, v)
        delta = torch.einsum("nqhd,nqhd->nhq", g, o)[..., None]
        p_q, p_kv = torch.exp(s0 + b_q[None] - lse[..., None]), torch.exp(s0 + b_kv[None] - lse[..., None])
        return (torch.einsum("nhqk,nkhd->nqhd", p_q * (dp - delta), k), torch.einsum("nhqk,nqhd->nkhd", p_kv * (dp - delta), q),
                torch.einsum("nhqk,nqhd->nkhd", p_kv, g), None, None)


class _IdentityBackward(torch.autograd.Function):
    """y in the forward, the gradient handed to x unchanged: an op whose backward was skipped."""

    @staticmethod
    def forward(ctx, x, y):
        return y.clone()

    @staticmethod
    def backward(ctx, g):
        return g, None


def tower_forward(cfg, sd, ids, lora=None, mults=None, scale=1.0, dtype=None, mutate=None, autograd_attention=False):
    """The T5 encoder in float64 under torch autograd.  sd: transformers state dict; lora: {target: (down, up)} leaf tensors;
    mults [n]: sample i runs at effective weight W + mults[i] scale up down.  dtype: round every tensor the engine stores to
    it, values and gradients.  Returns dict(last_hidden = hidden_states[-1], after the final norm; penultimate =
    hidden_states[-2]).  mutate: one of TOWER_MUTANTS (qkv_order_permuted acts in tower_grads).  autograd_attention: plain
    torch ops instead of _BiasAttention (the check that its hand-written backward is the derivative)."""
    W = lambda k: sd[k].double()
    n, L = ids.shape
    H, dk, eps = cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
    st = lambda t: N.store(t, dtype)
    m = None if mults is None else torch.as_tensor(mults, dtype=N.F64)

    def lin(x, name, lora_x=None):
        y = torch.einsum("nld,ed->nle", x, W(name + ".weight"))
        if lora is not None and name in lora and m is not None:
            down, up = lora[name]
            y = y + m[:, None, None] * scale * (((x if lora_x is None else lora_x) @ down.t()) @ up.t())
        return y

    h = st(W("shared.weight")[ids])
    table = R.bias_table(W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"),
                         cfg.relative_attention_num_buckets, cfg.relative_attention_max_distance, L)
    bias = R.expand_table(table, L)
    pen = None
    for i in range(cfg.num_layers):
        b = f"encoder.block.{i}.layer."
        if i == cfg.num_layers - 1:
            pen = h
        x = st(R.rms(h, W(b + "0.layer_norm.weight"), eps))
        q, k, v = (st(lin(x, b + "0.SelfAttention." + c)).reshape(n, L, H, dk) for c in "qkv")
        if autograd_attention:
            s = torch.einsum("nqhd,nkhd->nhqk", q, k) + bias[None]
            o = torch.einsum("nhqk,nkhd->nqhd", torch.softmax(s, dim=-1), v)
        else:
            o = _BiasAttention.apply(q, k, v, bias, mutate)
        o = st(o.reshape(n, L, H * dk))
        h = st(h + lin(o, b + "0.SelfAttention.o", q.reshape(n, L, H * dk) if mutate == "o_site_fed_q_rows" else None))
        x = st(R.rms(h, W(b + "1.layer_norm.weight"), eps))
        g = st(torch.einsum("nld,fd->nlf", x, W(b + "1.DenseReluDense.wi_0.weight")))
        u = st(torch.einsum("nld,fd->nlf", x, W(b + "1.DenseReluDense.wi_1.weight")))
        f = st(R.gelu_tanh(g) * (u.detach() if mutate == "wi_1_grad_dropped" else u))
        res = h.detach() if (mutate == "residual_grad_dropped" and i == 0) else h
        h = st(res + torch.einsum("nlf,df->nld", f, W(b + "1.DenseReluDense.wo.weight")))
    fin = R.rms(h, W("encoder.final_layer_norm.weight"), eps)
    if mutate == "final_norm_bwd_skipped":
        fin = _IdentityBackward.apply(h, fin)
    return {"last_hidden": st(fin), "penultimate": pen}


def tower_grads(cfg, sd, ids, lora, names, mults, scale, d_hidden, which, dtype=None, mutate=None, autograd_attention=False):
    """Gradients of <d_hidden, output> with respect to every site's (down, up), concatenated in `names` order into the two
    flat vectors the engine fills; which: 'last_hidden' or 'penultimate'.  Sites the output does not depend on get zeros."""
    leaves = {nm: (lora[nm][0].clone().requires_grad_(True), lora[nm][1].clone().requires_grad_(True)) for nm in names}
    out = tower_forward(cfg, sd, ids, leaves, mults, scale, dtype, mutate, autograd_attention)[which]
    flat = [t for nm in names for t in leaves[nm]]
    grads = torch.autograd.grad((out * d_hidden).sum(), flat, allow_unused=True)
    grads = {nm: tuple(torch.zeros_like(t) if gr is None else gr for t, gr in zip(leaves[nm], grads[2 * j:2 * j + 2]))
             for j, nm in enumerate(names)}
    if mutate == "qkv_order_permuted":  # every block's q and k gradients land in each other's place
        for nm in names:
            if nm.endswith(".q") and nm[:-1] + "k" in grads:
                grads[nm], grads[nm[:-1] + "k"] = grads[nm[:-1] + "k"], grads[nm]
    return torch.cat([grads[nm][0].reshape(-1) for nm in names]), torch.cat([grads[nm][1].reshape(-1) for nm in names])


def per_site(cfg, names, rank, gd, gu):
    """[(name, down | up of that site as one vector)] from the two flat vectors."""
    out, od, ou = [], 0, 0
    for nm in names:
        i, o = site_dims(cfg, nm)
        out.append((nm, torch.cat([gd[od:od + rank * i].reshape(-1), gu[ou:ou + o * rank].reshape(-1)])))
        od += rank * i
        ou += o * rank
    return out


def distance(cfg, names, rank, got, ref):
    """(whole-vector relative distance, worst per-site relative distance over the sites whose reference is not zero, its site)
    of got = (gd, gu) from ref = (gd, gu)."""
    whole = N.rel(torch.cat([got[0].double().cpu(), got[1].double().cpu()]), torch.cat(ref))
    worst_site, at = 0.0, None
    for (nm, g), (_, r) in zip(per_site(cfg, names, rank, got[0].double().cpu(), got[1].double().cpu()),
                               per_site(cfg, names, rank, *ref)):
        if float(r.norm()) == 0.0:
            continue
        d = N.rel(g, r)
        if d > worst_site:
            worst_site, at = d, nm
    return whole, worst_site, at


def tower_case(cfg, sd, L, rank, mults, which, dtype, names=None, seed=0, alpha=None):
    """Inputs and both reference forms of one tower case: dict(ids, lora, names, scale, d_hidden, A, B, e_q, e_q_site)."""
    names = names if names is not None else site_names(cfg.num_layers)
    g = torch.Generator().manual_seed(100 * L + seed)
    ids = R.seeded_ids(cfg, len(mults), L)
    lora = make_lora(cfg, names, rank, g)
    scale = (alpha if alpha is not None else rank) / rank
    d_hidden = torch.randn((len(mults), L, cfg.d_model), generator=g).double()
    sdr = R.rounded_state(sd, dtype)
    A = tower_grads(cfg, sdr, ids, lora, names, mults, scale, d_hidden, which)
    B_ = tower_grads(cfg, sdr, ids, lora, names, mults, scale, d_hidden, which, dtype)
    whole, site, _ = distance(cfg, names, rank, B_, A)
    return dict(ids=ids, lora=lora, names=names, scale=scale, d_hidden=d_hidden, sd=sdr, A=A, B=B_, e_q=whole, e_q_site=site)
