"""float64 references for the differentiable CLIP text tower (test infrastructure, not shipped): the causal attention
backward of csrc/attention_causal.hip, the activation backward, and the text tower with a LoRA on its attention
projections (`smi_clip_forward_lora` / `smi_clip_backward`).

Every reference comes in two forms on the same 16-bit-representable inputs:
  A  exact float64 arithmetic;
  B  the same arithmetic with the values rounded to the storage dtype at the places where the native code rounds them.
`e_q = |B - A| / |A|` is the error the storage format alone costs; a native result is held to `BAR(e_q) = 3 e_q + 1e-4`
(the factor 3 is the project's standing margin, DESIGN sections 6 and 12, over rounding the references cannot see:
fp32 accumulation order, exp / erf approximations, the power-of-two loss scale).  tests/test_notrigger_refs_cpu.py shows on
the CPU that mutated references fall outside the bar and form B inside it."""
import math

import torch

F64 = torch.float64


def rnd(x, dtype):
    """x rounded to `dtype` (None: unchanged), back in float64."""
    return x if dtype is None else x.to(dtype).to(F64)


def rel(a, b):
    a, b = a.detach().to(F64).cpu(), b.detach().to(F64).cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def bar(e_q):
    return 3.0 * e_q + 1e-4


def representable(shape, gen, dtype, std=1.0):
    """Seeded normal values that `dtype` holds exactly, in float64."""
    return (torch.randn(shape, generator=gen, dtype=F64) * std).to(dtype).to(F64)


# ---------------------------------------------------------------------------------------------------------------
# causal self-attention, q / k / v / dO [b, L, h, D]
# ---------------------------------------------------------------------------------------------------------------
def causal_mask(L, mutate=None):
    """visible[i, j]: key j is visible to query i.  `mutate` builds the wrong masks the CPU test must reject."""
    i = torch.arange(L)[:, None]
    j = torch.arange(L)[None, :]
    vis = j <= i
    if mutate == "strict":
        vis = j < i
        vis[0, 0] = True  # (a row with no visible key has no softmax)
    elif mutate == "extra_cell":
        vis = vis.clone()
        vis[L // 2, L // 2 + 1] = True
    elif mutate == "tile_slip":  # keys >= 64 visible to queries 48..63
        vis = vis.clone()
        vis[48:64, 64:] = True
    return vis


def causal_attn_fwd(q, k, v, scale, dtype=None):
    """o [b, L, h, D] (rounded to dtype in form B) and lse [b, h, L] (natural log)."""
    L = q.shape[1]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    s = s.masked_fill(~causal_mask(L), -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhij,bjhd->bihd", p, v)
    return rnd(o, dtype), lse


def causal_attn_bwd(q, k, v, o, lse, do, scale, dtype=None, mutate=None):
    """dq, dk, dv from the forward's o and lse.  Form B (dtype given): P and dS are rounded to `dtype` before their matrix
    products (dS is formed from the unrounded P) and the three outputs are rounded.  `mutate`: see the CPU test."""
    L = q.shape[1]
    s = torch.einsum("bihd,bjhd->bhij", q, k) * scale
    bwd_mask = causal_mask(L, mutate if mutate in ("strict", "extra_cell", "tile_slip") else None)
    if mutate == "no_mask":
        bwd_mask = torch.ones(L, L, dtype=torch.bool)
    p = torch.exp(s - lse[..., None]) * bwd_mask
    delta = torch.einsum("bihd,bihd->bhi", do, o)
    if mutate == "no_delta":
        delta = torch.zeros_like(delta)
    dp = torch.einsum("bihd,bjhd->bhij", do, v)
    ds = rnd(p * (dp - delta[..., None]), dtype)
    p = rnd(p, dtype)
    dv = torch.einsum("bhij,bihd->bjhd", p, do)
    dq = torch.einsum("bhij,bjhd->bihd", ds, k) * scale
    dk = torch.einsum("bhij,bihd->bjhd", ds, q) * (1.0 if mutate == "no_dk_scale" else scale)
    return rnd(dq, dtype), rnd(dk, dtype), rnd(dv, dtype)


ATTN_MUTATIONS = ("strict", "no_mask", "extra_cell", "tile_slip", "no_delta", "no_dk_scale")


def causal_attn_case(L, dtype, b=2, h=2, D=64, seed=0):
    """Inputs of one kernel case and both reference forms: dict(q, k, v, do, scale, A=(o, lse, dq, dk, dv), B=(...))."""
    g = torch.Generator().manual_seed(1000 * L + seed)
    q, k, v, do = (representable((b, L, h, D), g, dtype) for _ in range(4))
    scale = D ** -0.5
    oA, lse = causal_attn_fwd(q, k, v, scale)
    A = (oA, lse) + causal_attn_bwd(q, k, v, oA, lse, do, scale)
    oB, _ = causal_attn_fwd(q, k, v, scale, dtype)
    B = (oB, lse) + causal_attn_bwd(q, k, v, oB, lse, do, scale, dtype)
    return dict(q=q, k=k, v=v, do=do, scale=scale, A=A, B=B)


# ---------------------------------------------------------------------------------------------------------------
# activation: kind 0 quick_gelu, 1 erf-gelu
# ---------------------------------------------------------------------------------------------------------------
def act_fwd(x, kind):
    return x * torch.sigmoid(1.702 * x) if kind == 0 else 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def act_bwd(x, dy, kind, dtype=None):
    if kind == 0:
        s = torch.sigmoid(1.702 * x)
        d = s * (1.0 + 1.702 * x * (1.0 - s))
    else:
        d = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return rnd(dy * d, dtype)


# ---------------------------------------------------------------------------------------------------------------
# the text tower with LoRA sites
# ---------------------------------------------------------------------------------------------------------------
class _Store(torch.autograd.Function):
    """A tensor the engine keeps in 16 bit: the value is rounded on the way forward and its gradient on the way back (the
    gradient under a power-of-two scale that brings its largest entry to [8, 16], as the engine's loss scale does)."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.dtype = dtype
        return x.to(dtype).to(F64)

    @staticmethod
    def backward(ctx, g):
        m = float(g.abs().max())
        if m == 0.0 or not math.isfinite(m):
            return g, None
        s = 2.0 ** math.floor(math.log2(16.0 / m))
        return (g * s).to(ctx.dtype).to(F64) / s, None


def store(x, dtype):
    return x if dtype is None else _Store.apply(x, dtype)


SITE_PARTS = ("q_proj", "k_proj", "v_proj", "out_proj")


def site_names(num_layers, layers=None):
    """Engine targets in flat-buffer order: per layer q, k, v (adjacent, as the fused projection needs), then out_proj."""
    return [f"text_model.encoder.layers.{i}.self_attn.{p}" for i in (layers if layers is not None else range(num_layers))
            for p in SITE_PARTS]


def make_lora(names, d, rank, alpha, gen, dtype=None, up_std=0.05):
    """{name: (down [r, d], up [d, r])} float64, `up` seeded non-zero (a zero up gives a zero down gradient); values
    fp32-representable (the flat buffers are fp32)."""
    out = {}
    for nm in names:
        down = (torch.randn((rank, d), generator=gen, dtype=F64) / math.sqrt(d)).float().to(F64)
        up = (torch.randn((d, rank), generator=gen, dtype=F64) * up_std).float().to(F64)
        out[nm] = (down, up)
    return out


def flat_layout(names, d, rank, alpha):
    """The sites table of smi_clip_lora_create and the sizes of the two flat buffers."""
    sites, od, ou = [], 0, 0
    for nm in names:
        sites.append(dict(target=nm, off_down=od, off_up=ou, rank=rank, scale=alpha / rank))
        od += rank * d
        ou += d * rank
    return sites, od, ou


def flatten_lora(lora, names):
    return (torch.cat([lora[n][0].reshape(-1) for n in names]).float(), torch.cat([lora[n][1].reshape(-1) for n in names]).float())


def tower_forward(sd, ids, num_heads, hidden_act, lora=None, mults=None, scale=1.0, dtype=None, mutate=None):
    """The CLIP text tower in float64 under torch autograd.  sd: transformers state dict (float64); lora: {target: (down,
    up)} leaf tensors; mults [n]: sample i runs at effective weight W + mults[i] * scale * up down.  dtype: round every
    tensor the engine stores (each op's output) to it, values and gradients.  Returns dict(last_layer_out =
    hidden_states[-1] without the final norm, penultimate = hidden_states[-2], last_hidden_state).
    mutate: 'drop_site' (layer 0 q_proj not applied), 'flip_sign' (sample 1's multiplier negated), 'drop_layer' (the last
    layer's sites not applied)."""
    import torch.nn.functional as Fn
    g = lambda k: sd[k]
    n, L = ids.shape
    x = g("text_model.embeddings.token_embedding.weight")[ids] + g("text_model.embeddings.position_embedding.weight")[:L]
    x = store(x, dtype)
    d = x.shape[-1]
    hd = d // num_heads
    nl = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("text_model.encoder.layers."))
    vis = causal_mask(L).to(x.device)
    m = None if mults is None else torch.as_tensor(mults, dtype=x.dtype).clone().to(x.device)
    if m is not None and mutate == "flip_sign":
        m[1] = -m[1]

    def lin(h, name, layer):
        y = Fn.linear(h, g(name + ".weight"), g(name + ".bias"))
        dropped = (mutate == "drop_site" and name.endswith("layers.0.self_attn.q_proj")) or (mutate == "drop_layer" and layer == nl - 1)
        if lora is not None and name in lora and m is not None and not dropped:
            down, up = lora[name]
            y = y + m[:, None, None] * scale * ((h @ down.t()) @ up.t())
        return y

    pen = None
    for i in range(nl):
        b = f"text_model.encoder.layers.{i}."
        if i == nl - 1:
            pen = x
        h = store(Fn.layer_norm(x, (d,), g(b + "layer_norm1.weight"), g(b + "layer_norm1.bias"), 1e-5), dtype)
        q, k, v = (store(lin(h, b + "self_attn." + p, i), dtype).view(n, L, num_heads, hd) for p in ("q_proj", "k_proj", "v_proj"))
        s = torch.einsum("bihd,bjhd->bhij", q, k) * hd ** -0.5
        p = torch.softmax(s.masked_fill(~vis, -math.inf), dim=-1)
        o = store(torch.einsum("bhij,bjhd->bihd", p, v).reshape(n, L, d), dtype)
        x = store(x + lin(o, b + "self_attn.out_proj", i), dtype)
        h = store(Fn.layer_norm(x, (d,), g(b + "layer_norm2.weight"), g(b + "layer_norm2.bias"), 1e-5), dtype)
        h = store(Fn.linear(h, g(b + "mlp.fc1.weight"), g(b + "mlp.fc1.bias")), dtype)
        h = store(act_fwd(h, 0 if hidden_act == "quick_gelu" else 1), dtype)
        x = store(x + Fn.linear(h, g(b + "mlp.fc2.weight"), g(b + "mlp.fc2.bias")), dtype)
    last = store(Fn.layer_norm(x, (d,), g("text_model.final_layer_norm.weight"), g("text_model.final_layer_norm.bias"), 1e-5), dtype)
    return {"last_layer_out": x, "penultimate": pen, "last_hidden_state": last}


def tower_grads(sd, ids, num_heads, hidden_act, lora, names, mults, scale, d_hidden, which, dtype=None, mutate=None):
    """Gradients of <d_hidden, output> with respect to every site's (down, up), concatenated in `names` order into the two
    flat vectors the engine fills; which: 'last_layer_out' or 'penultimate'.  Sites the output does not depend on get zeros."""
    leaves = {nm: (lora[nm][0].clone().requires_grad_(True), lora[nm][1].clone().requires_grad_(True)) for nm in names}
    out = tower_forward(sd, ids, num_heads, hidden_act, leaves, mults, scale, dtype, mutate)[which]
    flat = [t for nm in names for t in leaves[nm]]
    grads = torch.autograd.grad((out * d_hidden).sum(), flat, allow_unused=True)
    grads = [torch.zeros_like(t) if gr is None else gr for t, gr in zip(flat, grads)]
    return torch.cat([gr.reshape(-1) for gr in grads[0::2]]), torch.cat([gr.reshape(-1) for gr in grads[1::2]])


# ---------------------------------------------------------------------------------------------------------------
# the tiny tower of the engine tests: hidden 128, 2 heads (head_dim 64), 2 layers, intermediate 256, 77 positions
# ---------------------------------------------------------------------------------------------------------------
def tiny_config(hidden_act="quick_gelu", projection_dim=None):
    import sliders_conceptmod_amd.clip as PC
    return PC.CLIPTextConfig(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                             num_attention_heads=2, hidden_act=hidden_act, projection_dim=projection_dim, eos_token_id=999)


def tiny_state(cfg, seed=3):
    """A seeded transformers-layout state dict in float32 whose values bf16 holds exactly (every dtype sees the same
    weights)."""
    import sliders_conceptmod_amd.clip as PC
    model = (PC.CLIPTextModelWithProjection if cfg.projection_dim else PC.CLIPTextModel)(cfg)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, p in model.state_dict().items():
        if p.ndim >= 2:
            w = torch.randn(p.shape, generator=g) * (0.02 if "embedding" in name else 0.8 / p.shape[1] ** 0.5)
        elif name.endswith("weight"):
            w = 1.0 + 0.1 * torch.randn(p.shape, generator=g)
        else:
            w = 0.02 * torch.randn(p.shape, generator=g)
        sd[name] = w.to(torch.bfloat16).float()
    return sd


def tiny_ids(cfg, n=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg.eos_token_id - 2, (n, cfg.max_position_embeddings), generator=g)
    ids[:, 0] = cfg.eos_token_id - 1
    for i, e in enumerate((9, 33, 76, 50)[:n]):
        ids[i, e:] = cfg.eos_token_id
    return ids


# ---------------------------------------------------------------------------------------------------------------
# the loss and the training loop of the no-trigger trainer (conceptmod/notrigger/train_notrigger.py), float64
# ---------------------------------------------------------------------------------------------------------------
def _unit_axis_cos(a, b, eps=1e-8):
    """The reference's cosine_similarity(a.unsqueeze(0), b.unsqueeze(0)): torch's dim=1 is then an axis of length 1, so every
    element is its own vector: a b / max(|a| |b|, eps)."""
    return a * b / torch.clamp(a.abs() * b.abs(), min=eps)


def loss_ref(tp, tn, pos, neg, neu, norm_p, norm_n, lam):
    """The differentiated scalar of one two-sided step and its reconstruction MSE / curriculum loss, written out from the
    formulas (not from the package's code)."""
    def reg(t, own, other):
        v1, v1r, v2 = t - neu, own - neu, other - neu
        c = _unit_axis_cos(v1, v2)
        return (c - _unit_axis_cos(v1r, v2)).mean().abs() + c.mean() + 1.0 / (((t - other) ** 2).mean() + 1e-8)
    sim = lam * (reg(tp, pos, neg) + reg(tn, neg, pos))
    pp, nn_ = (pos - tp).norm() / norm_p, (neg - tn).norm() / norm_n
    sf = 1 + 4 * (1 - torch.exp(-(pp - nn_).abs() / 0.05))
    wp, wn = pp * sf / (pp * sf + nn_ * sf), nn_ * sf / (pp * sf + nn_ * sf)
    wr = torch.minimum((pp + nn_) / 2, torch.tensor(0.95, dtype=pp.dtype))
    cur = wp * pp + wn * nn_
    recon = ((pos - tp) ** 2).mean() + ((neg - tn) ** 2).mean()
    return cur + (1 - wr) * sim, recon, cur


def loop_ids(cfg):
    """Token ids of the empty, the positive and the negative prompt of the loop test: BOS, a few words, EOS to the end."""
    L, eos = cfg.max_position_embeddings, cfg.eos_token_id
    rows = []
    for words in ([], [17, 230, 401], [512, 77, 640, 3]):
        r = [eos - 1] + words
        rows.append(torch.tensor([r + [eos] * (L - len(r))]))
    return rows


def loop_ref(sd, cfg, lora0, names, scale, steps=8, lr=0.5, lam=0.1, which="last_layer_out"):
    """The two-sided loop in float64: SGD, clip_grad_value_(1.0), gradients never zeroed (as the reference), targets from the
    un-adapted tower.  lora0: {target: (down, up)} initial values.  Returns [(reconstruction, curriculum)] per step."""
    neu_ids, pos_ids, neg_ids = loop_ids(cfg)
    fwd = lambda ids, lora=None, m=None: tower_forward(sd, ids, cfg.num_attention_heads, cfg.hidden_act, lora, m, scale)[which]
    with torch.no_grad():
        neu, pos, neg = fwd(neu_ids), fwd(pos_ids), fwd(neg_ids)
    leaves = {n: (lora0[n][0].clone().requires_grad_(True), lora0[n][1].clone().requires_grad_(True)) for n in names}
    params = [t for n in names for t in leaves[n]]
    opt = torch.optim.SGD(params, lr=lr)
    out, norm_p, norm_n = [], None, None
    for i in range(steps):
        h = fwd(neu_ids.expand(2, -1), leaves, [1.0, -1.0])
        tp, tn = h[0:1], h[1:2]
        if i == 0:
            norm_p, norm_n = (pos - tp.detach()).norm(), (neg - tn.detach()).norm()
        total, recon, cur = loss_ref(tp, tn, pos, neg, neu, norm_p, norm_n, lam)
        total.backward()
        torch.nn.utils.clip_grad_value_(params, 1.0)
        opt.step()
        out.append((float(recon.detach()), float(cur.detach())))
    return out


def lora_from_network(network):
    """{engine target: (down, up)} float64 and the targets in flat-buffer order, from a sliders_conceptmod_amd LoRANetwork."""
    mods = sorted(network.unet_loras, key=lambda l: l.off_down)
    return ({l.target_path: (l.lora_down.weight.detach().double().clone(), l.lora_up.weight.detach().double().clone()) for l in mods},
            [l.target_path for l in mods])
