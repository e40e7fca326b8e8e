"""Float64 references for the native T5 encoder (csrc/t5.hip, csrc/engine_t5.hip, the BIAS form of attn_fwd_kernel): a
restatement of transformers' T5EncoderModel in plain torch (no transformers module inside), the bucket function, the
per-kernel references with first-order error bounds and rounding emulations in the manner of norm_refs.py and
attention_refs.py, and the mutated references that show what each bar can see.  Torch only, no GPU import.

ROUNDING SITES of the kernels, u = 2^-11 (fp16) or 2^-8 (bf16), U32 = 2^-24:
  rmsnorm_rows     sum of squares, mean, rsqrt, x * r, * w in fp32; ONE 16-bit rounding at the store.
                   E = u|y| + (L / 2 + 6) U32 |y| + eta + FLOOR, L = the depth of the fp32 sum (rms_sum_depth): the sum's
                   relative error L U32 reaches r = rsqrt(.) halved; v_rsq, two products and the eps add are the 6.
  gated_gelu_tanh  gelu_tanh(g) * v in fp32 (one v_exp whose argument, up to 12 in magnitude, carries 2 U32 relative error of
                   its own, a division, four products), ONE rounding.  E = u|y| + 32 U32 |y| + eta + FLOOR.
  t5_bias_table    a gather with a widening conversion: exact.
  attention        attention_refs' F1 and F2 on the BIASED scores s = q.k scale + table[k - q + L - 1]; the bias is added
                   in fp32 (one more fp32 rounding of s, left to SLACK like the other fp32 roundings there).  The bound is
                   attention_refs.bounds on the biased P.
The assertion is elementwise |got - ref| <= SLACK E (+ attention_refs.TINY for the attention)."""
import math
from dataclasses import dataclass

import torch

import attention_refs as A
from norm_refs import FLOOR, SLACK, U32, sub_eta, unit_roundoff, worst  # noqa: F401  (re-exported for the tests)


# ---------------------------------------------------------------------------------------------------------------
# configuration and seeded weights of the test models
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class Cfg:
    vocab_size: int = 128
    d_model: int = 128
    d_kv: int = 64
    num_heads: int = 3
    d_ff: int = 256
    num_layers: int = 2
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "gated-gelu"


def test_cfg():
    return Cfg()


LENGTHS = (3, 77, 130, 256)
BATCH = 2


def seeded_state(cfg, seed=0):
    """The transformers state dict (`shared.weight` once; float32): norm weights 1 + 0.2 N, bias table 1.5 N, q and k
    1.2 N / sqrt(fan_in), other matrices N / sqrt(fan_in), embedding N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    d, inner, ff = cfg.d_model, cfg.num_heads * cfg.d_kv, cfg.d_ff
    sd = {"shared.weight": rn(cfg.vocab_size, d)}
    for i in range(cfg.num_layers):
        b = f"encoder.block.{i}.layer."
        sd[b + "0.SelfAttention.q.weight"] = rn(inner, d) * (1.2 / d ** 0.5)
        sd[b + "0.SelfAttention.k.weight"] = rn(inner, d) * (1.2 / d ** 0.5)
        sd[b + "0.SelfAttention.v.weight"] = rn(inner, d) / d ** 0.5
        sd[b + "0.SelfAttention.o.weight"] = rn(d, inner) / inner ** 0.5
        if i == 0:
            sd[b + "0.SelfAttention.relative_attention_bias.weight"] = 1.5 * rn(cfg.relative_attention_num_buckets, cfg.num_heads)
        sd[b + "0.layer_norm.weight"] = 1.0 + 0.2 * rn(d)
        sd[b + "1.DenseReluDense.wi_0.weight"] = rn(ff, d) / d ** 0.5
        sd[b + "1.DenseReluDense.wi_1.weight"] = rn(ff, d) / d ** 0.5
        sd[b + "1.DenseReluDense.wo.weight"] = rn(d, ff) / ff ** 0.5
        sd[b + "1.layer_norm.weight"] = 1.0 + 0.2 * rn(d)
    sd["encoder.final_layer_norm.weight"] = 1.0 + 0.2 * rn(d)
    return sd


def rounded_state(sd, dt):
    """The weights the engine is given: rounded to dt once (the float64 reference runs on these same values)."""
    return {k: v.to(dt) for k, v in sd.items()}


def seeded_ids(cfg, n, L, seed=1):
    return torch.randint(0, cfg.vocab_size, (n, L), generator=torch.Generator().manual_seed(seed + L))


def hf_config(cfg):
    import transformers
    return transformers.T5Config(vocab_size=cfg.vocab_size, d_model=cfg.d_model, d_kv=cfg.d_kv, d_ff=cfg.d_ff,
                                 num_layers=cfg.num_layers, num_heads=cfg.num_heads,
                                 relative_attention_num_buckets=cfg.relative_attention_num_buckets,
                                 relative_attention_max_distance=cfg.relative_attention_max_distance,
                                 layer_norm_epsilon=cfg.layer_norm_epsilon, feed_forward_proj=cfg.feed_forward_proj,
                                 dropout_rate=0.0, use_cache=False, is_encoder_decoder=False)


def hf_model(cfg, sd, dtype):
    """transformers.T5EncoderModel with the state sd, in `dtype` on the CPU."""
    import transformers
    m = transformers.T5EncoderModel(hf_config(cfg)).eval()
    full = {k: v.float() for k, v in sd.items()}
    full["encoder.embed_tokens.weight"] = full["shared.weight"]
    m.load_state_dict(full)
    return m.to(dtype)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def twin_bar(cfg, sd, ids, ref):
    """The project's twin bar: 2 x the relative L2 distance of transformers' bf16 run (on the bf16-rounded weights the
    engine gets) from the float64 reference."""
    with torch.no_grad():
        twin = hf_model(cfg, sd, torch.bfloat16)(ids)[0]
    return 2.0 * rel_l2(twin, ref)


# ---------------------------------------------------------------------------------------------------------------
# the bucket function and the encoder, float64
# ---------------------------------------------------------------------------------------------------------------
def bucket(rel, num_buckets, max_distance):
    """transformers' T5Attention._relative_position_bucket(bidirectional=True) for one offset rel = key - query, in float64."""
    nb = num_buckets // 2
    b = nb if rel > 0 else 0
    a = abs(rel)
    max_exact = nb // 2
    if a < max_exact:
        return b + a
    large = max_exact + int(math.log(a / max_exact) / math.log(max_distance / max_exact) * (nb - max_exact))
    return b + min(large, nb - 1)


def buckets(num_buckets, max_distance, L):
    """The bucket of every offset -(L - 1) .. L - 1, as smi_t5_relative_buckets lays them out."""
    return [bucket(o - (L - 1), num_buckets, max_distance) for o in range(2 * L - 1)]


def bias_table(weight, num_buckets, max_distance, L, fault=None):
    """[H, 2 L - 1] in weight's dtype widened to float64: table[h, o] = weight[bucket(o - (L - 1)), h].  Faults: 'transposed'
    (the weight read as [H, num_buckets]), 'off_by_one' (offset o reads o + 1's bucket)."""
    w = weight.double()
    idx = buckets(num_buckets, max_distance, L)
    if fault == "off_by_one":
        idx = idx[1:] + idx[-1:]
    H = w.shape[1]
    if fault == "transposed":
        flat = w.reshape(-1)
        return torch.stack([torch.stack([flat[h * w.shape[0] + b] for b in idx]) for h in range(H)])
    return w[torch.tensor(idx)].t().contiguous()


def expand_table(table, L):
    """[H, L, L]: bias[h, q, k] = table[h, k - q + L - 1] (the reference may build it; no kernel does)."""
    q = torch.arange(L)[:, None]
    k = torch.arange(L)[None, :]
    return table[:, k - q + L - 1]


def gelu_tanh(x):
    """0.5 x (1 + tanh(u)), u = sqrt(2 / pi) (x + 0.044715 x^3), written as x sigmoid(2 u): the same function without the
    cancellation of 1 + tanh(u) at large negative x (in float64 it is 0 below u = -19, where the true value is x e^(2u))."""
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def rms(x, w, eps, fault=None, hf_variance=False):
    if fault == "mean_subtracted":
        x = x - x.mean(-1, keepdim=True)
    if hf_variance:  # transformers' T5LayerNorm: the variance and its rsqrt in fp32 whatever the model's dtype
        return w * (x * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps))
    ms = (x * x).mean(-1, keepdim=True)
    r = 1.0 / (ms.sqrt() + eps) if fault == "eps_outside" else torch.rsqrt(ms + eps)
    y = x * r
    return y if fault == "weight_dropped" else y * w


ENGINE_MUTATIONS = ("bias_dropped", "bias_mirrored", "scale_eighth", "halves_swapped", "final_weight_ignored",
                    "max_distance_64", "mean_subtracted", "block1_zero_table")


def forward64(cfg, sd, ids, mut=None, hf_variance=False):
    """The encoder in float64 on the weights as given (widened): last hidden state [n, L, d_model].  One mutation at most.
    hf_variance: the one place where transformers' `.double()` model is not float64 -- T5LayerNorm forms the variance and
    its rsqrt in fp32 -- is restated as it is there, so that the two can be compared to float64 rounding."""
    W = lambda k: sd[k].double()
    n, L = ids.shape
    H, dk, eps = cfg.num_heads, cfg.d_kv, cfg.layer_norm_epsilon
    nfault = "mean_subtracted" if mut == "mean_subtracted" else None
    h = W("shared.weight")[ids]
    md = 64 if mut == "max_distance_64" else cfg.relative_attention_max_distance
    table = bias_table(W("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"),
                       cfg.relative_attention_num_buckets, md, L)
    bias = expand_table(table, L)
    if mut == "bias_mirrored":
        bias = bias.transpose(1, 2)
    if mut == "bias_dropped":
        bias = torch.zeros_like(bias)
    for i in range(cfg.num_layers):
        b = f"encoder.block.{i}.layer."
        x = rms(h, W(b + "0.layer_norm.weight"), eps, nfault, hf_variance)
        q, k, v = (torch.einsum("nld,ed->nle", x, W(b + f"0.SelfAttention.{c}.weight")).reshape(n, L, H, dk) for c in "qkv")
        s = torch.einsum("nqhd,nkhd->nhqk", q, k) * (0.125 if mut == "scale_eighth" else 1.0)
        s = s + (torch.zeros_like(bias) if (mut == "block1_zero_table" and i == 1) else bias)[None]
        o = torch.einsum("nhqk,nkhd->nqhd", torch.softmax(s, dim=-1), v).reshape(n, L, H * dk)
        h = h + torch.einsum("nle,de->nld", o, W(b + "0.SelfAttention.o.weight"))
        x = rms(h, W(b + "1.layer_norm.weight"), eps, nfault, hf_variance)
        g = torch.einsum("nld,fd->nlf", x, W(b + "1.DenseReluDense.wi_0.weight"))
        u = torch.einsum("nld,fd->nlf", x, W(b + "1.DenseReluDense.wi_1.weight"))
        if mut == "halves_swapped":
            g, u = u, g
        f = (gelu_erf(g) if mut == "erf_gelu" else gelu_tanh(g)) * u
        h = h + torch.einsum("nlf,df->nld", f, W(b + "1.DenseReluDense.wo.weight"))
    fw = W("encoder.final_layer_norm.weight")
    return rms(h, fw, eps, "weight_dropped" if mut == "final_weight_ignored" else nfault, hf_variance)


# ---------------------------------------------------------------------------------------------------------------
# kernels: references, bounds, emulations, mutants
# ---------------------------------------------------------------------------------------------------------------
RMS_CASES = [(M, C) for C in (64, 2048, 2056, 4096, 8192) for M in (1, 3, 130)]
RMS_MUTANTS = ("mean_subtracted", "eps_outside", "weight_dropped")


def rms_sum_depth(C):
    """Depth of the fp32 sum of squares: 8 elements per vector and ceil(C8 / lanes) vectors per lane in sequence, then the
    tree over 64 lanes (6) and, in the four-wave form, over the waves (2)."""
    lanes = 64 if C <= 2048 else 256
    return 8 * -(-(C // 8) // lanes) + 8


def rms_inputs(M, C, dt, seed=0):
    """Rows cycle through |x| of order 1, 1e-3 (mean of squares ~ eps: where eps inside or outside the root differ) and 60;
    in bf16 the last row reaches 3e4, as the residual stream of t5-v1.1-xxl does.  w = 1 + 0.2 N."""
    g = torch.Generator().manual_seed(seed + 7 * M + C)
    mag = torch.tensor([1.0, 1e-3, 60.0])[torch.arange(M) % 3][:, None]
    x = torch.randn(M, C, generator=g) * mag + 0.3 * mag  # (a mean, so that subtracting it shows)
    if dt == torch.bfloat16:
        x[-1] = x[-1] / x[-1].abs().max() * 3.0e4
    w = 1.0 + 0.2 * torch.randn(C, generator=g)
    return x.to(dt), w.to(dt)


def rms_ref(x, w, eps, fault=None):
    return rms(x.double(), w.double(), eps, fault)


def rms_bound(ref, C, dt):
    return unit_roundoff(dt) * ref.abs() + (rms_sum_depth(C) / 2 + 6) * U32 * ref.abs() + sub_eta(dt) + FLOOR


def rms_emulate(x, w, eps, dt):
    """fp32 arithmetic in the kernel's order of operations (not of its sum), one rounding to dt."""
    xf, wf = x.float(), w.float()
    r = torch.rsqrt((xf * xf).sum(-1, keepdim=True) * (1.0 / x.shape[-1]) + eps)
    return (wf * (xf * r)).to(dt)


GG_CASES = [(M, F) for F in (128, 264) for M in (3, 130)]
GG_MUTANTS = ("erf_gelu", "halves_swapped")


def gg_inputs(M, F, dt, seed=0):
    """proj [M, 2 F] = gate | value.  A quarter of the gates lie in [-4, -1], where tanh- and erf-GELU differ by up to a
    tenth of the value: the only region where a 16-bit rounding bar tells them apart."""
    g = torch.Generator().manual_seed(seed + M + F)
    gate = 2.0 * torch.randn(M, F, generator=g)
    gate[:, ::4] = -1.0 - 3.0 * torch.rand(M, (F + 3) // 4, generator=g)
    val = 1.5 * torch.randn(M, F, generator=g)
    return torch.cat([gate, val], dim=1).to(dt)


def gg_ref(proj, fault=None):
    F = proj.shape[1] // 2
    g, v = proj[:, :F].double(), proj[:, F:].double()
    if fault == "halves_swapped":
        g, v = v, g
    return (gelu_erf(g) if fault == "erf_gelu" else gelu_tanh(g)) * v


def gg_bound(ref, dt):
    return unit_roundoff(dt) * ref.abs() + 32 * U32 * ref.abs() + sub_eta(dt) + FLOOR


def gg_emulate(proj, dt):
    F = proj.shape[1] // 2
    g, v = proj[:, :F].float(), proj[:, F:].float()
    u2 = 1.5957691216057308 * g * (0.044715 * g * g + 1.0)
    return (g / (1.0 + torch.exp(-u2)) * v).to(dt)


TABLE_CASES = [(H, L) for H in (1, 3, 64) for L in (1, 3, 130, 512)]
TABLE_MUTANTS = ("transposed", "off_by_one")

ATTN_B, ATTN_H, ATTN_D = 2, 3, 64
ATTN_LENGTHS = (1, 3, 64, 77, 128, 130, 256)
ATTN_LONG = (1, 1, 512)  # (B, H, L): once
ATTN_MUTANTS = ("bias_after_max", "bias_mirrored", "scale_eighth")
BIG_BIAS = 100.0


def attn_inputs(B, H, L, dt, seed=0):
    """q, k, v [B, L, H, 64] of the dtype and a table f32 [H, 2 L - 1] of 1.5 N entries -- with one entry of head 0, the
    offset key = query + 1, at BIG_BIAS: a kernel that took its tile maximum from unbiased scores would form exp(100)."""
    g = torch.Generator().manual_seed(seed + 13 * L + H)
    q, k, v = (torch.randn(B, L, H, ATTN_D, generator=g) * s for s in (0.35, 0.35, 1.0))
    table = 1.5 * torch.randn(H, 2 * L - 1, generator=g)
    if L > 1:
        table[0, L] = BIG_BIAS
    return q.to(dt), k.to(dt), v.to(dt), table.float()


def attn_bias_ref(q, k, v, table, scale, fault=None, dt=None):
    """{O, P, lse} in float64.  Faults: 'bias_mirrored' (query - key), 'scale_eighth', and 'bias_after_max' -- the rounding
    emulation (needs dt) with the probabilities formed against the maximum of the UNBIASED scores, as a kernel would that
    added the bias after its tile maximum."""
    q, k, v = q.double(), k.double(), v.double()
    L = q.shape[1]
    bias = expand_table(table.double(), L)
    if fault == "bias_mirrored":
        bias = bias.transpose(1, 2)
    s0 = torch.einsum("bqhd,bkhd->bhqk", q, k) * (scale / 8 if fault == "scale_eighth" else scale)
    s = s0 + bias[None]
    if fault == "bias_after_max":
        m = s0.max(dim=-1, keepdim=True).values
        pu = A.rnd16(torch.exp(s - m), dt)
        l = pu.sum(-1)
        return {"O": A.rnd16(torch.einsum("bhqk,bkhd->bqhd", pu, v) / l.permute(0, 2, 1)[..., None], dt)}
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    return {"O": torch.einsum("bhqk,bkhd->bqhd", p, v), "P": p, "lse": lse}


def attn_bias_bound(ref, q, k, v, scale, dt):
    return A.bounds(ref, q, k, v, None, scale, dt)["O"]


def attn_bias_emulate(q, k, v, table, scale, dt):
    """Float64 arithmetic with the roundings F1 and F2 of attention_refs on the biased scores."""
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale + expand_table(table.double(), q.shape[1])[None]
    m = s.max(dim=-1, keepdim=True).values
    pu = A.rnd16(torch.exp(s - m), dt)
    l = pu.sum(-1)
    return A.rnd16(torch.einsum("bhqk,bkhd->bqhd", pu, v) / l.permute(0, 2, 1)[..., None], dt)
