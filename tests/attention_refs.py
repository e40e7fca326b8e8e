"""Float64 references, operand layouts, first-order error bounds, a rounding emulation, a restatement of the dispatcher and
mutated references for the attention kernels of csrc/attention.hip.  Torch only, no GPU import: every function works on
whatever device its inputs live on, so test_attention_refs_cpu.py runs it here and test_attention_kernels_gpu.py may form
the float64 reference on the device.

Tensors are [B, N, H, D] (token-major, head h in columns h*D .. h*D+D of a row, as the kernels see them); score-shaped
tensors are [B, H, Nq, Nk]; row statistics (lse, delta) are [B, H, Nq].

ROUNDING SITES of the kernels (read from csrc/attention.hip), u = 2^-11 (fp16) or 2^-8 (bf16):
  forward   (attn_fwd_kernel, attn_xs_fwd_kernel)
    F1  p = exp2(s*sl - m*sl) is converted to 16 bits (pack8) before the P.V MFMA; the row sum l (Sum4::add8) adds those
        SAME rounded values, in both kernels
    F2  O = o * (1 / l) is converted to 16 bits by the store
  backward  (attn_bwd_dq_body, attn_xs_bwd_dq_kernel, attn_bwd_dkv_body, attn_delta_kernel)
    B1  delta = sum_d dO * O is formed from the 16-bit O the forward stored (every delta site: dQ prologue, OWN_DELTA of
        the fused launch, attn_delta_kernel), fp32 accumulation
    B2  P = exp2((s - lse/scale) * sl) is converted to 16 bits before the P^T.dO MFMA (dV)
    B3  dS = P * (dP - delta), P in fp32, is converted to 16 bits before the dS.K (dQ) and dS^T.Q (dK) MFMAs
    B4  dQ, dK (times scale, in fp32) and dV are converted to 16 bits by the store
  SUB every one of these roundings is relative (u|x|) only in the normal range: below 2^-14 an fp16 rounding is absolute,
      eta = 2^-25 (half the subnormal spacing); bf16 has the fp32 exponent range, eta = 0.  It matters for P and dS, of
      which a row of 200 keys at logit deviation 3 holds many elements below 6e-5, when few queries (Nq = 1) or few keys
      feed a sum: dV[k] = P[0, k] dO[0] with P = 1e-6 is off by eta |dO|, 60 u |dV|.
  Not modelled (SLACK is for these): fp32 accumulation order of the MFMAs and of l, the approximation error of exp2 / __logf /
  the reciprocal, the fp32 rounding of s*sl - m*sl and of lse itself.
  lse: the bf16 forward kernels form it from a second, fp32 sum of the unrounded probabilities (O keeps the sum of the rounded
  ones); the fp16 kernels take log of the rounded sum, a relative 2^-11 at most.  The emulation uses the rounded sum in both.

BOUNDS, first order in u, one tensor per output (`bounds`):
    E_O  = u (P|V| + |O|) + u|O| + eta Pmax (sum_k|V| + Nk|O|)    F1 in the numerator, F1 in the row sum (relative u on
                                          l), F2; SUB: p = exp(s - m) is off by eta, and 1 / l = Pmax, the largest P of the row
    e_dl = u sum_d |dO||O|                B1
    E_dS = u|dS| + P e_dl + eta           B3, B1 through dS = P (dP - delta), SUB
    E_dQ = scale E_dS |K|   + u|dQ|       B4
    E_dK = scale E_dS^T |Q| + u|dK|       B4
    E_dV = u P^T|dO| + u|dV| + eta sum_q|dO|                      B2, B4, SUB
The assertion is elementwise |got - ref| <= SLACK * E + TINY.  TINY = 2^-24, the spacing of fp16 subnormals: below 2^-14 a
16-bit rounding is absolute, not relative; against outputs of order 0.1 .. 1000 it is nothing."""
from dataclasses import dataclass

import torch

SLACK = 2.0
TINY = 2.0 ** -24
NAN16 = 0x7FFF  # a NaN bit pattern in fp16 and in bf16
XS_KEYS = 96

# kernel families of smi_attn_ran.family (include/smi.h SMI_ATTN_*)
FWD, XS_FWD, BWD_FUSED, DQ, XS_DQ, DKV, DK_DV, DELTA = 1, 2, 3, 4, 5, 6, 7, 8
FAMILY_NAMES = {FWD: "tiled fwd", XS_FWD: "xs fwd", BWD_FUSED: "fused bwd", DQ: "tiled dQ", XS_DQ: "xs dQ",
                DKV: "dK+dV in one", DK_DV: "dK, dV as two", DELTA: "delta kernel"}


def unit_roundoff(dt):
    return 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8


def sub_eta(dt):
    """Absolute error of a rounding below the normal range (SUB of the module docstring)."""
    return 2.0 ** -25 if dt == torch.float16 else 0.0


def rnd16(x, dt):
    """x rounded to the 16-bit type, back in float64."""
    return x.to(dt).double()


# ---------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------
def _attn64(q, k, v, scale, d_o=None, fault=None):
    """The float64 attention forward and backward of [B, N, H, D] inputs (any float dtype; used as they are, in float64),
    with at most one deliberate fault (see MUTATIONS).  Returns a dict."""
    q, k, v = q.double(), k.double(), v.double()
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    kk, vv = k, v
    if fault == "drop_last_key":
        kk, vv = k[:, :-1], v[:, :-1]
    elif fault == "v_next_head":
        vv = torch.roll(v, -1, dims=2)
    elif fault == "k_sample0":
        kk = k[:1].expand_as(k)
    elif fault == "pad_key_counted":
        z = torch.zeros_like(k[:, :1])
        kk, vv = torch.cat([k, z], 1), torch.cat([v, z], 1)
    qs, ks = q, kk
    if fault == "ragged_d":
        d16 = 16 * (D // 16)
        qs, ks = q[..., :d16], kk[..., :d16]
    s = torch.einsum("bqhd,bkhd->bhqk", qs, ks) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhqk,bkhd->bqhd", p, vv)
    out = {"O": o, "lse": lse, "P": p}
    if fault == "last_q_unwritten":
        out["O"] = o.clone()
        out["O"][:, -1] = float("nan")
    if d_o is None:
        return out
    g = d_o.double()
    pb = p
    if fault == "lse_shift":  # the backward recomputes P from the lse it is given
        pb = torch.exp(s - torch.roll(lse, -1, dims=-1)[..., None])
    dp = torch.einsum("bqhd,bkhd->bhqk", g, vv)
    delta = torch.einsum("bqhd,bqhd->bhq", g, o)
    ds = pb * (dp if fault == "no_delta" else dp - delta[..., None])
    dq = torch.einsum("bhqk,bkhd->bqhd", ds, kk) * scale
    dk = torch.einsum("bhqk,bqhd->bkhd", ds, q) * (1.0 if fault == "dk_no_scale" else scale)
    dv = torch.einsum("bhqk,bqhd->bkhd", pb, g)
    if fault in ("drop_last_key", "pad_key_counted"):  # gradients of the keys that exist
        zk = torch.zeros_like(k[:, :1])
        dk = torch.cat([dk, zk], 1) if fault == "drop_last_key" else dk[:, :Nk]
        dv = torch.cat([dv, zk], 1) if fault == "drop_last_key" else dv[:, :Nk]
    if fault == "dq_last4_zero":
        dq = dq.clone()
        dq[..., -4:] = 0.0
    if fault == "last_q_unwritten":
        dq = dq.clone()
        dq[:, -1] = float("nan")
    if fault == "dk_dv_swapped":
        dk, dv = dv, dk
    out.update({"dP": dp, "delta": delta, "dS": ds, "dQ": dq, "dK": dk, "dV": dv})
    return out


def attn_ref64(q, k, v, scale, d_o=None):
    """O, lse (and dQ, dK, dV with d_o) in float64 on the given (16-bit-rounded) inputs, plus P, dP, delta, dS."""
    return _attn64(q, k, v, scale, d_o)


# name -> (outputs it changes, predicate on the case that says where it applies).  With a single key the softmax is the
# constant 1, dS = 0 and dQ = dK = 0 exactly: a fault that only rescales or clears dQ / dK, or that changes K or the logits,
# changes nothing there.
MUTATIONS = {
    "drop_last_key": (("O", "dQ", "dK", "dV"), lambda c: c.Nk > 1),
    "lse_shift": (("dQ", "dK", "dV"), lambda c: c.Nq > 1),
    "no_delta": (("dQ", "dK"), lambda c: True),
    "dk_no_scale": (("dK",), lambda c: c.Nk > 1),
    "v_next_head": (("O", "dQ", "dK", "dV"), lambda c: c.H > 1),
    "k_sample0": (("O", "dQ", "dK", "dV"), lambda c: c.B > 1 and c.Nk > 1),
    "ragged_d": (("O", "dQ", "dK", "dV"), lambda c: c.D % 16 != 0 and c.Nk > 1),
    "dq_last4_zero": (("dQ",), lambda c: c.Nk > 1),
    "last_q_unwritten": (("O", "dQ"), lambda c: True),
    "dk_dv_swapped": (("dK", "dV"), lambda c: True),
    # on random logits a padded key changes less than one rounding; claimed where every logit is strongly negative
    "pad_key_counted": (("O",), lambda c: c.kind == "neglse"),
}


def mutated_ref(name, q, k, v, scale, d_o):
    return _attn64(q, k, v, scale, d_o, fault=name)


# ---------------------------------------------------------------------------------------------------------------
# bounds and emulation
# ---------------------------------------------------------------------------------------------------------------
def bounds(ref, q, k, v, d_o, scale, dt):
    """The error-bound tensors of the module docstring from a float64 reference (attn_ref64 output)."""
    u, eta = unit_roundoff(dt), sub_eta(dt)
    q, k, v = q.double().abs(), k.double().abs(), v.double().abs()
    p, o = ref["P"], ref["O"].abs()
    pmax = p.max(dim=-1).values.permute(0, 2, 1)[..., None]  # [B, Nq, H, 1]
    e = {"O": u * (torch.einsum("bhqk,bkhd->bqhd", p, v) + o) + u * o +
              eta * pmax * (v.sum(1, keepdim=True) + k.shape[1] * o)}
    if d_o is None:
        return e
    g = d_o.double().abs()
    e_dl = u * torch.einsum("bqhd,bqhd->bhq", g, o)
    e_ds = u * ref["dS"].abs() + p * e_dl[..., None] + eta
    e["dQ"] = scale * torch.einsum("bhqk,bkhd->bqhd", e_ds, k) + u * ref["dQ"].abs()
    e["dK"] = scale * torch.einsum("bhqk,bqhd->bkhd", e_ds, q) + u * ref["dK"].abs()
    e["dV"] = u * torch.einsum("bhqk,bqhd->bkhd", p, g) + u * ref["dV"].abs() + eta * g.sum(1, keepdim=True)
    return e


def bwd_inputs(ref, dt):
    """What the backward is given: the float64 O rounded to the dtype and the float64 lse rounded to fp32."""
    return ref["O"].to(dt), ref["lse"].float()


def emulate(q, k, v, d_o, scale, dt):
    """Float64 arithmetic with exactly the roundings F1, F2, B1 .. B4 of the module docstring and nothing else; the backward
    on bwd_inputs() of the float64 reference, as the GPU test runs it."""
    q, k, v, g = q.double(), k.double(), v.double(), d_o.double()
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * scale
    m = s.max(dim=-1, keepdim=True).values
    pu = rnd16(torch.exp(s - m), dt)                                  # F1
    l = pu.sum(-1)
    o = rnd16(torch.einsum("bhqk,bkhd->bqhd", pu, v) / l.permute(0, 2, 1)[..., None], dt)  # F2
    out = {"O": o, "lse": m[..., 0] + torch.log(l)}
    ref = attn_ref64(q, k, v, scale)
    o16, lse32 = bwd_inputs(ref, dt)
    pb = torch.exp(s - lse32.double()[..., None])
    delta = torch.einsum("bqhd,bqhd->bhq", g, o16.double())          # B1
    dp = torch.einsum("bqhd,bkhd->bhqk", g, v)
    ds = rnd16(pb * (dp - delta[..., None]), dt)                      # B3
    out["dQ"] = rnd16(torch.einsum("bhqk,bkhd->bqhd", ds, k) * scale, dt)   # B4
    out["dK"] = rnd16(torch.einsum("bhqk,bqhd->bkhd", ds, q) * scale, dt)
    out["dV"] = rnd16(torch.einsum("bhqk,bqhd->bkhd", rnd16(pb, dt), g), dt)  # B2, B4
    return out


def ratio(got, ref, e):
    """max |got - ref| / E over the elements (TINY taken off the error first); inf where got is not finite."""
    return worst(got, ref, e)[0]


def worst(got, ref, e):
    """(ratio, index) of the worst element, for messages."""
    err = (got.double() - ref).abs()
    r = (err - TINY).clamp_min(0.0) / e
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    i = int(r.argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return float(r.max()), tuple(reversed(idx))


# ---------------------------------------------------------------------------------------------------------------
# cases, inputs, layouts
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    D: int
    Nq: int
    Nk: int
    B: int = 2
    H: int = 3
    layout: str = "dense"
    kind: str = "rand"   # rand | spike | neglse

    @property
    def scale(self):
        return self.D ** -0.5

    def tag(self):
        return f"D{self.D}_q{self.Nq}_k{self.Nk}_b{self.B}h{self.H}_{self.layout}_{self.kind}"


LAYOUTS = ("dense", "self", "cross", "ext", "alldiff")


def make_inputs(case, dt, seed=0, device="cpu"):
    """q, k, v, d_o as [B, N, H, D] tensors of dtype dt.
    rand:   q = 3 N(0,1), k = N(0,1) (logits of standard deviation ~3), v = 0.5 + N(0,1), d_o = N(0,1)
    spike:  rand inputs scaled to unit logits, with one late key (index Nk - 7: the last key tile, past key 64 from Nk = 77
            on) set to 6 q[0, 5, 0]: the running maximum of query 5 jumps there, after every earlier tile
    neglse: q = 5 sqrt(D) u + 0.3 N, k = -6 u + N for one unit direction u per (batch, head): every logit ~ -30 +- 5,
            lse < -10; d_o = 512 N (as after a loss scale)"""
    c = case
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda n: torch.randn(c.B, n, c.H, c.D, generator=g)
    if c.kind == "neglse":
        u = torch.randn(c.B, 1, c.H, c.D, generator=g)
        u = u / u.norm(dim=-1, keepdim=True)
        q, k, v, d_o = 5.0 * c.D ** 0.5 * u + 0.3 * r(c.Nq), -6.0 * u + r(c.Nk), r(c.Nk), 512.0 * r(c.Nq)
    elif c.kind == "spike":
        q, k, v, d_o = r(c.Nq), r(c.Nk), r(c.Nk), r(c.Nq)
        k[0, c.Nk - 7, 0] = 6.0 * q[0, 5, 0].to(dt).float()
    else:
        q, k, v, d_o = 3.0 * r(c.Nq), r(c.Nk), 0.5 + r(c.Nk), r(c.Nq)
    return tuple(t.to(dt).to(device) for t in (q, k, v, d_o))


OPERANDS = ("q", "k", "v", "o", "do", "dq", "dk", "dv")
DESTS = ("o", "dq", "dk", "dv")


def layout_of(case):
    """operand -> (buffer name, element offset of [0, 0, 0, 0], leading dimension) and buffer name -> (rows, columns).
    Rows of an operand are b * N + n with ITS N (Nq for q, o, do, dq; Nk for the others)."""
    c = case
    C = c.H * c.D
    rq, rk = c.B * c.Nq, c.B * c.Nk
    if c.layout == "dense":
        bufs = {n: (rq if n in ("q", "o", "do", "dq") else rk, C) for n in OPERANDS}
        ops = {n: (n, 0, C) for n in OPERANDS}
    elif c.layout == "self":  # q|k|v column blocks of one [rows, 3C] tensor, the gradients of another
        rows = max(rq, rk)
        bufs = {"qkv": (rows, 3 * C), "dqkv": (rows, 3 * C), "o": (rq, C), "do": (rq, C)}
        ops = {"q": ("qkv", 0, 3 * C), "k": ("qkv", C, 3 * C), "v": ("qkv", 2 * C, 3 * C), "o": ("o", 0, C), "do": ("do", 0, C),
               "dq": ("dqkv", 0, 3 * C), "dk": ("dqkv", C, 3 * C), "dv": ("dqkv", 2 * C, 3 * C)}
    elif c.layout == "cross":
        bufs = {"q": (rq, C), "kv": (rk, 2 * C), "o": (rq, C), "do": (rq, C), "dq": (rq, C), "dkv": (rk, 2 * C)}
        ops = {"q": ("q", 0, C), "k": ("kv", 0, 2 * C), "v": ("kv", C, 2 * C), "o": ("o", 0, C), "do": ("do", 0, C),
               "dq": ("dq", 0, C), "dk": ("dkv", 0, 2 * C), "dv": ("dkv", C, 2 * C)}
    elif c.layout == "ext":   # k|v at a column offset inside a wider tensor, dK|dV in the same columns of its gradient
        ld, col = 6 * C + 8, 2 * C + 8
        bufs = {"q": (rq, C), "owner": (rk, ld), "o": (rq, C), "do": (rq, C), "dq": (rq, C), "downer": (rk, ld)}
        ops = {"q": ("q", 0, C), "k": ("owner", col, ld), "v": ("owner", col + C, ld), "o": ("o", 0, C), "do": ("do", 0, C),
               "dq": ("dq", 0, C), "dk": ("downer", col, ld), "dv": ("downer", col + C, ld)}
    elif c.layout == "alldiff":  # eight different leading dimensions, all multiples of 8
        ld = {n: C + 8 * (i + 1) for i, n in enumerate(OPERANDS)}
        bufs = {n: (rq if n in ("q", "o", "do", "dq") else rk, ld[n]) for n in OPERANDS}
        ops = {n: (n, 0, ld[n]) for n in OPERANDS}
    else:
        raise ValueError(c.layout)
    return ops, bufs


def op_view(case, flat, op, off, ld):
    """The [B, N, H, D] view of an operand inside its flat buffer."""
    c = case
    n = c.Nq if op in ("q", "o", "do", "dq") else c.Nk
    return torch.as_strided(flat, (c.B, n, c.H, c.D), (n * ld, ld, c.D, 1), off)


def build_case(case, dt, seed=0, device="cpu"):
    """Flat buffers (dtype dt, EVERY element the NaN pattern 0x7FFF until an input is copied in: gaps of source buffers are
    NaN too, so a read of a neighbour's columns shows), element offsets and leading dimensions.  Returns a dict:
      q, k, v, do   the dense [B, N, H, D] inputs          ops   operand -> (buffer, offset, ld)
      bufs          buffer name -> flat tensor             shape buffer name -> (rows, columns)"""
    ops, shape = layout_of(case)
    q, k, v, d_o = make_inputs(case, dt, seed, device)
    bufs = {n: torch.full((r * c,), NAN16, dtype=torch.int16, device=device).view(dt) for n, (r, c) in shape.items()}
    built = {"case": case, "dt": dt, "q": q, "k": k, "v": v, "do": d_o, "ops": ops, "bufs": bufs, "shape": shape}
    for n, t in (("q", q), ("k", k), ("v", v), ("do", d_o)):
        put(built, n, t)
    return built


def put(built, op, t):
    b, off, ld = built["ops"][op]
    op_view(built["case"], built["bufs"][b], op, off, ld).copy_(t)


def get(built, op):
    b, off, ld = built["ops"][op]
    return op_view(built["case"], built["bufs"][b], op, off, ld)


def owned_mask(built, buffer, written):
    """Bool mask over the flat `buffer`: the elements the kernels may write when the operands `written` are outputs -- rows
    < N, the D columns of each of the H heads."""
    flat = built["bufs"][buffer]
    m = torch.zeros(flat.numel(), dtype=torch.bool, device=flat.device)
    for op in written:
        b, off, ld = built["ops"][op]
        if b == buffer:
            op_view(built["case"], m, op, off, ld).fill_(True)
    return m


def untouched(built, buffer, written):
    """Number of elements of `buffer` outside owned_mask that no longer hold the NaN pattern."""
    flat = built["bufs"][buffer]
    keep = ~owned_mask(built, buffer, written)
    return int((flat.view(torch.int16)[keep] != NAN16).sum())


# ---------------------------------------------------------------------------------------------------------------
# the dispatcher, restated
# ---------------------------------------------------------------------------------------------------------------
def xs_chain(Nq, B, H):
    """xs_grid_x: query blocks per workgroup of the single-pass kernels."""
    nqb = -(-Nq // 128)
    chain = 1
    while chain < 4 and nqb % (2 * chain) == 0 and B * H * (nqb // (2 * chain)) >= 1280:
        chain *= 2
    return chain


def expected_path(D, Nq, Nk, B, H, grads, sel=(-1, -1)):
    """What fwd_t / bwd_t launch.  grads: "fwd", or a subset of {"q", "kv"} as a string like "q+kv", "q", "kv".
    sel = (xs, fused), -1 / 1 = on (no environment variable set), 0 = off.
    Returns {"dp", "form", "families": [...], "chain"}."""
    dp = 32 if D <= 32 else 64 if D <= 64 else 96 if D <= 96 else 160
    nsd, ns, alt = -(-D // 16), dp // 16, {64: 3, 96: 5}.get(dp, 0)
    form = 1 if nsd == ns else 2 if alt and nsd == alt else 0
    xs_on, fused_on = sel[0] != 0, sel[1] != 0
    nqb = -(-Nq // 128)
    xs = Nk <= XS_KEYS and xs_on and form != 0
    if grads == "fwd":
        return {"dp": dp, "form": form, "families": [XS_FWD if xs else FWD], "chain": xs_chain(Nq, B, H) if xs else 0}
    want_q, want_kv = "q" in grads.split("+"), "kv" in grads.split("+")
    fam, chain = [], 0
    if not want_q:
        fam.append(DELTA)
    if dp <= 64 and fused_on and want_q and want_kv and form != 0 and Nk > XS_KEYS and nqb * H * B <= 1024:
        return {"dp": dp, "form": form, "families": fam + [BWD_FUSED], "chain": 0}
    if want_q:
        fam.append(XS_DQ if xs else DQ)
        chain = xs_chain(Nq, B, H) if xs else 0
    if want_kv:
        fam.append(DKV if dp <= 96 else DK_DV)
    return {"dp": dp, "form": form, "families": fam, "chain": chain}


# ---------------------------------------------------------------------------------------------------------------
# case tables (shared by the CPU and the GPU test)
# ---------------------------------------------------------------------------------------------------------------
WIDTHS = [Case(D, 130, Nk) for D in range(8, 161, 8) for Nk in (77, 100)]
SELECT_FUSED = [Case(D, 200, 200) for D in (32, 40, 64)]          # x fused in {0, 1}
SELECT_XS = [Case(D, 200, 77) for D in (40, 64)]                  # x xs in {0, 1}
SUBSETS = [Case(D, 130, Nk) for D in (16, 40, 64, 80, 136, 160) for Nk in (77, 200)]  # x {q+kv, q, kv}
KEY_EDGES = ([Case(64, 96, Nk) for Nk in (1, 8, 31, 32, 33, 63, 64, 65, 80, 81, 95, 96, 97, 127, 128, 129, 193)] +
             [Case(40, 96, Nk) for Nk in (77, 80, 81, 96, 97)])    # x xs in {0, 1}
QUERY_EDGES = [Case(64, Nq, Nk) for Nq in (1, 31, 33, 127, 128, 129, 257) for Nk in (77, 130)]
WG_ORDER = [Case(64, 200, 200, B=3, H=5), Case(64, 200, 77, B=3, H=5), Case(64, 300, 200, B=1, H=1), Case(64, 300, 77, B=1, H=1)]
CHAINED = [Case(64, 8192 - 56, 77, B=2, H=20), Case(40, 16384 - 56, 77, B=2, H=20)]
LAYOUT_CASES = [Case(D, 200, Nk, layout=lay) for lay in LAYOUTS for D in (40, 64) for Nk in (77, 200)]
SPIKED = [Case(64, 256, 77, B=1, H=1, kind="spike"), Case(64, 256, 256, B=1, H=1, kind="spike")]
NEGLSE = [Case(64, 192, 77, kind="neglse"), Case(40, 128, 77, kind="neglse"), Case(64, 64, 130, kind="neglse")]


def cpu_cases():
    """Every case small enough for a float64 reference on the CPU (all but CHAINED: 40 heads x 16328 queries, the same
    code at a size that only changes the grid), without repeats."""
    seen, out = set(), []
    for c in WIDTHS + SELECT_FUSED + SELECT_XS + SUBSETS + KEY_EDGES + QUERY_EDGES + WG_ORDER + LAYOUT_CASES + SPIKED + NEGLSE:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out
