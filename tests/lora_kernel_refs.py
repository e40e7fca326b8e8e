"""Float64 references, seeded inputs and derived tolerances for the LoRA / DoRA gradient kernels of csrc/lora.hip
(not collected by pytest; imported by test_lora_kernels_gpu.py and test_lora_kernel_refs_cpu.py).

Every reference is written from the formula of the operation, in plain torch float64 on CPU tensors, and takes the SAME
16-bit-rounded inputs the kernel gets.  The input builders live here too, so that the CPU file can prove on the very
inputs of the GPU file that a wrong kernel cannot pass: mutated references fall outside each tolerance by at least 10x,
and the float64 reference rounded to the kernel's output format falls inside it.

Unit roundoffs: U32 = 2^-24 (fp32), U16[dt] = 2^-11 (fp16) / 2^-8 (bf16).  EPS[dt] = 2 * U16[dt] is the storage tolerance
of test_kernels_gpu.py."""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}
GUARD = 64  # floats of guard region on either side of an output


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------
# grouped weight-gradient reduction
# ---------------------------------------------------------------------------------------------------------------
def wgrad_ref(X, P, dW0, alpha, r, seg_cols=0, row_scale=None, rows_per_sample=1):
    """dW[q][k] = dW0[q][k] + alpha * sum_m (P[m][seg * r + q] * row_scale[m // rows_per_sample]) * X[m][k], seg = k // seg_cols.
    X [M, K] (any dtype), P [M, >= nseg * r], dW0 [r, K]; float64 [r, K].  Only the rows given exist: for the tail form pass the
    rows from m_begin on (and the row scales of their samples)."""
    Xd, Pd = X.double(), P.double()
    M, K = Xd.shape
    if row_scale is not None:
        Pd = Pd * row_scale.double()[torch.arange(M) // rows_per_sample][:, None]
    seg = seg_cols if seg_cols else K
    out = dW0.double().clone()
    for s in range(K // seg):
        out[:, s * seg:(s + 1) * seg] += alpha * (Pd[:, s * r:(s + 1) * r].t() @ Xd[:, s * seg:(s + 1) * seg])
    return out


def wgrad_abs(X, P, dW0, alpha, r, seg_cols=0, row_scale=None, rows_per_sample=1):
    """|alpha| * |P * row_scale|^T |X| + |dW0|: the magnitude the forward-error bound of the sum scales with."""
    rs = None if row_scale is None else row_scale.abs()
    return wgrad_ref(X.double().abs(), P.double().abs(), dW0.double().abs(), abs(alpha), r, seg_cols, rs, rows_per_sample)


def conv_tap_rows(img, tap, Hout, Wout, stride, ups):
    """The rows the down-filter gradient of a 3x3 / pad-1 conv pairs with output pixels: row (n, oy, ox) = the input pixel
    under tap (ky, kx) = (tap // 3, tap % 3), i.e. (oy * stride + ky - 1, ox * stride + kx - 1) of the conv's input -- which is
    `img` [Nb, Hin, Win, K], or its nearest-neighbour 2x upsampling when `ups` -- and zero outside it."""
    Nb, Hin, Win, K = img.shape
    H, W = (2 * Hin, 2 * Win) if ups else (Hin, Win)
    ky, kx = tap // 3, tap % 3
    out = torch.zeros(Nb * Hout * Wout, K, dtype=img.dtype)
    for n in range(Nb):
        for oy in range(Hout):
            for ox in range(Wout):
                iy, ix = oy * stride + ky - 1, ox * stride + kx - 1
                if 0 <= iy < H and 0 <= ix < W:
                    out[(n * Hout + oy) * Wout + ox] = img[n, iy // 2, ix // 2] if ups else img[n, iy, ix]
    return out


@dataclass
class WJob:
    """One job of a table.  M counts the rows of all samples; rows below m_begin do not exist (tail form)."""
    M: int
    K: int
    r: int
    seg_cols: int = 0
    rps: int = 0            # rows per sample (0: M)
    ldp: int = 0            # 0: nseg * r
    ldx: int = 0            # 0: K
    layout: str = "rk"      # "rk": dW [r, K] (so_r = K, so_k = 1); "kr": dW [K, r] (so_r = 1, so_k = r)
    scaled: bool = False    # per-sample row scales
    alpha: float = 0.5
    m_begin: int = 0


def _int_tensor(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def build_wjob(spec: WJob, dt, seed, exact=True):
    """CPU tensors of one job: X [M_live, ldx] (dt), P [M_live, ldp] fp32, rs [samples_live] fp32 or None, dW0 / ref flat fp32
    (GUARD | r * K | GUARD; ref is the float64 result cast to fp32, the guards as in dW0), abs_ (float64, [r, K] layout order of
    the flat buffer) for the random-data bound.  exact: integer data whose every partial sum is exact in fp32."""
    g = gen(seed)
    nseg = spec.K // spec.seg_cols if spec.seg_cols else 1
    ldp, ldx = spec.ldp or nseg * spec.r, spec.ldx or spec.K
    rps = spec.rps or spec.M
    ml = spec.M - spec.m_begin
    if exact:
        X = _int_tensor((ml, ldx), -8, 8, g).to(dt)
        P = _int_tensor((ml, ldp), -4, 4, g)
        dW0 = _int_tensor((spec.r, spec.K), -5, 5, g)
        rs = 2.0 ** torch.randint(-2, 3, ((ml + rps - 1) // rps,), generator=g).float() if spec.scaled else None
    else:
        X = torch.randn(ml, ldx, generator=g).to(dt)
        P = torch.randn(ml, ldp, generator=g)
        dW0 = torch.randn(spec.r, spec.K, generator=g)
        rs = torch.rand((ml + rps - 1) // rps, generator=g) + 0.5 if spec.scaled else None
    args = (X[:, :spec.K], P, dW0, spec.alpha, spec.r, spec.seg_cols, rs, rps)
    ref, abs_ = wgrad_ref(*args), wgrad_abs(*args)
    if spec.layout == "kr":
        dW0, ref, abs_ = dW0.t().contiguous(), ref.t().contiguous(), abs_.t().contiguous()
    guard = torch.full((GUARD,), -777.0)
    flat0 = torch.cat([guard, dW0.reshape(-1), guard])
    flat_ref = torch.cat([guard, ref.float().reshape(-1), guard])
    return {"spec": spec, "X": X, "P": P, "rs": rs, "dW0": flat0, "ref": flat_ref, "ref64": ref.reshape(-1),
            "abs": abs_.reshape(-1), "ldp": ldp, "ldx": ldx, "rps": rps}


def exact_headroom(job):
    """Largest |partial sum| any summation order can meet, in units of the smallest spacing the data can produce (all values
    are integer multiples of alpha * min(row scale), itself a power of two <= 1).  Below 2^24 every fp32 sum is exact."""
    unit = abs(job["spec"].alpha) * (float(job["rs"].min()) if job["rs"] is not None else 1.0)
    assert unit <= 1.0 and math.frexp(unit)[0] == 0.5
    return float(job["abs"].max()) / unit


def wgrad_random_bound(job):
    """Forward-error bound of an fp32 sum of M products in any order, plus the scaling by alpha and the accumulation onto
    dW0: |got - ref| <= (M + 2) * 2^-24 * (|alpha| |P|^T |X| + |dW0|), elementwise (flat, the job's layout)."""
    return (job["spec"].M + 2) * U32 * job["abs"]


# the tables of the exact-data cases (shared by the GPU test and the CPU headroom check): name -> list of jobs
WGRAD_EXACT = {
    "mixed_classes": [WJob(300, 72, 16, layout="rk"), WJob(154, 64, 3, layout="kr"), WJob(77, 24, 32, layout="rk"),
                      WJob(200, 136, 8, layout="kr"), WJob(130, 320, 4, layout="rk")],
    "fused_r4_staged": [WJob(154, 192, 4, seg_cols=64, ldp=16)],
    "fused_r8_staged": [WJob(154, 192, 8, seg_cols=64, ldp=32)],
    "fused_r16_unstaged": [WJob(154, 192, 16, seg_cols=64, ldp=56)],
    "fused_straddle_960": [WJob(154, 960, 4, seg_cols=320, ldp=16), WJob(100, 960, 16, seg_cols=320, ldp=48)],
    "row_scale": [WJob(154, 64, 4, rps=77, ldp=12, ldx=72, scaled=True), WJob(154, 64, 8, rps=77, ldp=16, ldx=80, scaled=True),
                  WJob(154, 192, 16, seg_cols=64, rps=77, ldp=56, ldx=200, scaled=True)],
    "geometry": [WJob(100, 24, 4), WJob(100, 72, 8), WJob(100, 64, 3), WJob(70, 2176, 4), WJob(1, 64, 16),
                 WJob(2047, 64, 4, rps=23, scaled=True), WJob(2048, 64, 8, rps=512, scaled=True)],
}
# tail form: (M, m_begin, rps, r, K, seg_cols, ldp)
WGRAD_TAIL = [(154, 77, 77, 4, 64, 0, 0), (154, 77, 77, 16, 192, 64, 56), (2048 + 80, 1067, 1067, 8, 72, 0, 0),
              (2048 + 80, 1067, 97, 4, 192, 64, 12)]
WGRAD_RANDOM = [WJob(600, 320, r, seg_cols=160, rps=200, scaled=True, alpha=0.375) for r in (3, 8, 16, 32)]
# conv_tap: (stride, ups, m_begin in images); input 6 x 10, two images
CONV_CASES = [(1, 0, 0), (2, 0, 0), (1, 1, 0), (1, 0, 1), (2, 0, 1)]
CONV_NB, CONV_HIN, CONV_WIN, CONV_K, CONV_R = 2, 6, 10, 24, 4


def conv_out_hw(stride, ups):
    H, W = (2 * CONV_HIN, 2 * CONV_WIN) if ups else (CONV_HIN, CONV_WIN)
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def build_conv_case(dt, stride, ups, skip_imgs, seed=11):
    """The nine tap jobs of one 3x3 down filter: img [Nb_live, Hin, Win, K] (dt), P = dxa [M_live, ldp] fp32 with row scales,
    the filter gradient [r][K][3][3] flat fp32 with guards (tap t at +t, so_r = 9 K, so_k = 9).  Exact integer data."""
    g = gen(seed)
    Hout, Wout = conv_out_hw(stride, ups)
    live = CONV_NB - skip_imgs
    rps = Hout * Wout
    ldp = CONV_R + 4
    img = _int_tensor((live, CONV_HIN, CONV_WIN, CONV_K), -8, 8, g).to(dt)
    P = _int_tensor((live * rps, ldp), -4, 4, g)
    rs = 2.0 ** torch.randint(-2, 3, (live,), generator=g).float()
    dW0 = _int_tensor((CONV_R, CONV_K, 9), -5, 5, g)
    ref, abs_ = dW0.double().clone(), dW0.double().abs()
    for t in range(9):
        rows = conv_tap_rows(img, t, Hout, Wout, stride, ups)
        ref[:, :, t] = wgrad_ref(rows, P, dW0[:, :, t], 0.5, CONV_R, 0, rs, rps)
        abs_[:, :, t] = wgrad_abs(rows, P, dW0[:, :, t], 0.5, CONV_R, 0, rs, rps)
    guard = torch.full((GUARD,), -777.0)
    return {"img": img, "P": P, "rs": rs, "ldp": ldp, "rps": rps, "Hout": Hout, "Wout": Wout,
            "M": CONV_NB * rps, "m_begin": skip_imgs * rps, "alpha": 0.5,
            "dW0": torch.cat([guard, dW0.reshape(-1), guard]), "ref": torch.cat([guard, ref.float().reshape(-1), guard]),
            "abs": abs_.reshape(-1), "unit": 0.5 * float(rs.min())}


def conv_filter_grad_autograd(img, P, rs, rps, r, stride, ups, alpha):
    """The same filter gradient from torch.autograd through F.conv2d in float64: [r][K][3][3]."""
    Nb, Hin, Win, K = img.shape
    x = img.double().permute(0, 3, 1, 2)
    if ups:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    w = torch.zeros(r, K, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, stride=stride, padding=1)  # [Nb, r, Hout, Wout]
    Hout, Wout = y.shape[2:]
    dy = (P.double()[:, :r] * rs.double()[torch.arange(P.shape[0]) // rps][:, None]).view(Nb, Hout, Wout, r).permute(0, 3, 1, 2)
    (gw,) = torch.autograd.grad(y, w, alpha * dy)
    return gw


# ---------------------------------------------------------------------------------------------------------------
# 16-bit shadow operands
# ---------------------------------------------------------------------------------------------------------------
# (r, nseg, K, cs, rows_pad, conv)
LORA_PREP_SITES = [(4, 3, 64, 40, 16, 0), (16, 1, 72, 42, 16, 0), (3, 1, 24, 32, 16, 1), (8, 1, 16, 24, 32, 2)]


def lora_prep_ref(down, up, r, nseg, K, cs, rows_pad, conv, dt):
    """down: lora_down of the site, [nseg * r, K] (Linear) or [r, K, 3, 3] (conv, nseg = 1); up [nseg, cs, r].  Returns the 16-bit
    operands: downT [rows_pad, K or 9 K] (conv: (tap, channel) order), upT [rows_pad, nseg * cs] block diagonal
    (upT[s r + q][s cs + n] = up[s][n][q]), and for a conv site the gradient filter gw [K][9][64] with
    gw[c][tt][q] = down[q][c][t], t = 8 - tt (conv = 1) or tt (conv = 2), else None.  Pure data movement plus one rounding."""
    kd = 9 * K if conv else K
    dT = torch.zeros(rows_pad, kd)
    dT[:nseg * r] = down.reshape(r, K, 9).permute(0, 2, 1).reshape(r, 9 * K) if conv else down.reshape(nseg * r, K)
    uT = torch.zeros(rows_pad, nseg * cs)
    for s in range(nseg):
        uT[s * r:(s + 1) * r, s * cs:(s + 1) * cs] = up[s].t()
    gw = None
    if conv:
        gw = torch.zeros(K, 9, 64)
        d9 = down.reshape(r, K, 9)
        for tt in range(9):
            gw[:, tt, :r] = d9[:, :, 8 - tt if conv == 1 else tt].t()
        gw = gw.to(dt)
    return dT.to(dt), uT.to(dt), gw


# ---------------------------------------------------------------------------------------------------------------
# transposes
# ---------------------------------------------------------------------------------------------------------------
def transpose_scaled_ref(src, M, C, Mp, f, rps, dt):
    """dst [C, Mp] (dt): dst[c][m] = (src[m][c] as fp32 * f[m // rps]) rounded to dt for m < M, zero for M <= m < Mp."""
    v = src[:M, :C].float()
    if f is not None:
        v = v * f[torch.arange(M) // rps][:, None]
    out = torch.zeros(C, Mp, dtype=dt)
    out[:, :M] = v.to(dt).t()
    return out


# ---------------------------------------------------------------------------------------------------------------
# DoRA
# ---------------------------------------------------------------------------------------------------------------
@dataclass
class DSite:
    r: int
    nseg: int
    K: int
    cs: int
    scale: float = 0.5


DORA_FWD_TABLES = {
    "mixed_3_8_4": [DSite(3, 3, 64, 40, 0.25), DSite(8, 1, 72, 42, 0.5), DSite(4, 3, 264, 100, 1.0)],
    "rank16": [DSite(16, 3, 72, 42, 0.5)],
    "rank32": [DSite(32, 1, 264, 40, 0.25)],
}
DORA_TRANSPOSE_TABLE = [DSite(4, 3, 64, 64, 0.5), DSite(8, 1, 72, 40, 0.5), DSite(3, 1, 328, 100, 0.5)]
DORA_GRAD_SITES = [DSite(3, 1, 72, 40), DSite(4, 3, 264, 100), DSite(8, 3, 72, 40), DSite(16, 1, 320, 100),
                   DSite(32, 3, 264, 40)]
DORA_MULT = 1.5


def build_dora_table(sites, dt, seed=5, w_scale=8.0):
    """Flat fp32 parameter buffers as dora.py lays them out (every lora_down, then every lora_up, then every dora_scale), here
    with gaps between the sites so that offsets are non-trivial: down_flat / up_flat, per site W (dt) and the offsets.  `up` is
    a tenth of W (0.05 against 0.5 in the engine tests), so that dW is not pure cancellation noise; dora_scale is the column norm
    of W perturbed by 10 %.  Everything is 16 times the engine tests' magnitudes: dW then stays clear of the fp16 subnormals,
    whose fixed spacing no relative bound covers (test_lora_kernel_refs_cpu.py checks that the rounded reference passes)."""
    g = gen(seed)
    down_parts, up_parts, out = [torch.full((12,), 333.0)], [torch.full((7,), 333.0)], []
    nd, nu = 12, 7
    for s in sites:
        W = (torch.randn(s.nseg * s.cs, s.K, generator=g) * w_scale).to(dt)
        down = torch.randn(s.nseg, s.r, s.K, generator=g) * s.K ** -0.5
        up = torch.randn(s.nseg, s.cs, s.r, generator=g) * 0.1 * w_scale
        gsc = W.float().view(s.nseg, s.cs, s.K).norm(dim=1) * (1 + 0.1 * torch.randn(s.nseg, s.K, generator=g))
        e = {"site": s, "W": W, "down": down, "up": up, "g": gsc, "off_down": nd}
        down_parts += [down.reshape(-1), torch.full((20,), 333.0)]  # 20: keeps off_down a multiple of 4 floats
        nd += down.numel() + 20
        e["off_up"] = nu
        up_parts += [up.reshape(-1), torch.full((5,), 333.0)]
        nu += up.numel() + 5
        out.append(e)
    for e in out:
        e["off_dora"] = nu
        up_parts += [e["g"].reshape(-1), torch.full((3,), 333.0)]
        nu += e["g"].numel() + 3
    return torch.cat(down_parts), torch.cat(up_parts), out


def dora_forward_ref(W, down, up, g, lscale, n=None):
    """V = W + up down per segment, n = ||V|| per column (over the cs rows of the segment), dW = lscale * (V g / n - W).
    W [nseg * cs, K], down [nseg, r, K], up [nseg, cs, r], g [nseg, K]; float64: (V [nseg, cs, K], n [nseg, K], dW [nseg * cs, K]).
    `n` given: the norms the delta is formed with (the delta kernel reads the stored fp32 norms)."""
    nseg, cs, _ = up.shape
    Wd = W.double().view(nseg, cs, -1)
    V = Wd + up.double() @ down.double()
    nn_ = V.norm(dim=1)
    nu = nn_ if n is None else n.double()
    dW = lscale * (V * (g.double() / nu)[:, None, :] - Wd)
    return V, nn_, dW.reshape(nseg * cs, -1)


def cnorm_bound(site):
    """Relative: cs squares summed in fp32 in any order (cs), each of a V built by r multiply-adds on W (r), the square, the
    square root (halves the relative error; counted whole) and the LDS combine: (cs + r + 4) * 2^-24."""
    return (site.cs + site.r + 4) * U32


def dora_dw_bound(V, n, W, g, lscale, r, dt, ref):
    """|got - ref| <= EPS[dt] |ref| + c 2^-24 lscale (|V g / n| + |W|), c = r + 4: r multiply-adds build V, one division g / n,
    one product, one subtraction, one scaling by lscale; then one rounding to the 16-bit output."""
    nseg, cs, K = V.shape
    mag = (V.abs() * (g.double().abs() / n.double())[:, None, :]).reshape(nseg * cs, K) + W.double().abs()
    return EPS[dt] * ref.abs() + (r + 4) * U32 * abs(lscale) * mag


def dora_grads_ref(W, down, up, g, G, alpha, detach=True, use_gn=True):
    """Gradients of alpha * <G, V g / n - W> with respect to down, up and g by autograd in float64; n = ||V||_col is DETACHED
    (dora.py; the oracle's DoRAModuleRef).  detach=False / use_gn=False are the mutants the CPU file needs."""
    nseg, cs, _ = up.shape
    d = down.double().clone().requires_grad_(True)
    u = up.double().clone().requires_grad_(True)
    gg = g.double().clone().requires_grad_(True)
    Wd = W.double().view(nseg, cs, -1)
    V = Wd + u @ d
    n = V.norm(dim=1)
    if detach:
        n = n.detach()
    fac = gg / n if use_gn else gg
    dW = V * fac[:, None, :] - Wd
    loss = alpha * (G.double().view(nseg, cs, -1) * dW).sum()
    return torch.autograd.grad(loss, (d, u, gg))


def dora_grads_bound(W, down, up, g, G, alpha, pre_down, pre_up, pre_g):
    """Elementwise bounds for (d_down, d_up, d_g).  With u = 2^-24, n the exact norm and nb = cnorm_bound the relative error of
    the fp32 norm the kernels read (carried in: every output is linear in 1 / n):

      d_g[k]      = alpha / n * sum_o G V       cs terms, each with a V of r multiply-adds, the product, alpha, 1 / n, +=:
                    (cs + r + 6) u * |alpha| / n * sum_o |G| (|W| + |up| |down|)  +  nb * the same sum  +  u |out|
      d_down[q,k] = alpha g / n * sum_o up G    cs terms, g / n, two scalings, +=:
                    (cs + 6) u * |alpha g / n| * sum_o |up| |G|                   +  nb * the same      +  u |out|
      d_up[o,q]   = alpha sum_k G (g / n) down  K terms of two products each, alpha, +=:
                    (K + 6) u * |alpha| sum_k |G| |g / n| |down|                  +  nb * the same      +  u |out|

    `out` = pre-filled value + gradient (the kernels accumulate); pre_* are the pre-fills."""
    nseg, cs, r = up.shape
    K = down.shape[2]
    Wd, Gd = W.double().view(nseg, cs, K).abs(), G.double().view(nseg, cs, K).abs()
    ua, da, ga = up.double().abs(), down.double().abs(), g.double().abs()
    V = W.double().view(nseg, cs, K) + up.double() @ down.double()
    n = V.norm(dim=1)
    nb = (cs + r + 4) * U32
    a = abs(alpha)
    rd, ru, rg = dora_grads_ref(W, down, up, g, G, alpha)
    s_g = a / n * (Gd * (Wd + ua @ da)).sum(dim=1)                       # [nseg, K]
    s_d = a * (ga / n)[:, None, :] * (ua.transpose(1, 2) @ Gd)           # [nseg, r, K]
    s_u = a * (Gd * (ga / n)[:, None, :]) @ da.transpose(1, 2)           # [nseg, cs, r]
    b_g = ((cs + r + 6) * U32 + nb) * s_g + U32 * (pre_g.double() + rg).abs()
    b_d = ((cs + 6) * U32 + nb) * s_d + U32 * (pre_down.double() + rd).abs()
    b_u = ((K + 6) * U32 + nb) * s_u + U32 * (pre_up.double() + ru).abs()
    return b_d, b_u, b_g


# ---------------------------------------------------------------------------------------------------------------
# adapted Linear, batched-pass form
# ---------------------------------------------------------------------------------------------------------------
GEMM_ROWS_CASES = [  # (N, lora_seg, r)
    (192, 64, 3), (192, 64, 4), (960, 320, 8), (960, 320, 4), (320, 0, 3), (320, 0, 8)]
GEMM_ROWS_M, GEMM_ROWS_K, GEMM_ROWS_SCALE = 154, 64, 0.5
GEMM_ROWS_ROW0 = (0, 77, 154)


def build_gemm_rows(N, seg, r, dt, seed=21):
    """A [M, K], W [N, K], bias [N], res [M, N] in dt; xa [M, r * nseg] and up [N, r] fp32.  `up` is O(1) so that the delta is
    as large as the frozen product: a delta on the wrong rows or from the wrong segment is far outside the tolerance."""
    g = gen(seed)
    M, K = GEMM_ROWS_M, GEMM_ROWS_K
    nseg = N // seg if seg else 1
    return {"a": torch.randn(M, K, generator=g).to(dt), "w": (torch.randn(N, K, generator=g) * K ** -0.5).to(dt),
            "bias": torch.randn(N, generator=g).to(dt), "res": torch.randn(M, N, generator=g).to(dt),
            "xa": torch.randn(M, r * nseg, generator=g), "up": torch.randn(N, r, generator=g)}


def gemm_rows_ref(a, w, bias, res, xa, up, r, scale, row0, seg):
    """C[m][n] = a w^T + bias + res, and for rows m >= row0: + scale * sum_q xa[m - row0][(n // seg) * r + q] * up[n][q]."""
    M, N = a.shape[0], w.shape[0]
    out = a.double() @ w.double().t() + bias.double() + res.double()
    seg = seg or N
    for s in range(N // seg):
        cols = slice(s * seg, (s + 1) * seg)
        out[row0:, cols] += scale * (xa.double()[:M - row0, s * r:(s + 1) * r] @ up.double()[cols].t())
    return out


def close_ratio(a, b, dt, mult=4.0):
    """test_kernels_gpu.close as a number: the larger of (max err / allowed) and (rel-norm / allowed); <= 1 passes."""
    a, b = a.double(), b.double()
    tol = EPS[dt] * mult
    err, ref = (a - b).abs().max().item(), b.abs().max().item()
    rel = ((a - b).norm() / (b.norm() + 1e-30)).item()
    return max(err / (tol * (ref + 1e-6)), rel / tol)


# ---------------------------------------------------------------------------------------------------------------
# loss scales
# ---------------------------------------------------------------------------------------------------------------
GRAD_TARGET = 16.0


def build_grad_scale_input(per=1000, seed=31):
    """Samples whose maxima spread over many binades; an all-zero sample; a maximum in the last element; maxima that are an
    exact power of two, just above and just below one (the edges of the (target / 2, target] window)."""
    g = gen(seed)
    up1 = lambda v: float(torch.nextafter(torch.tensor(v), torch.tensor(1e30)))  # noqa: E731  (one fp32 ulp above v)
    maxima = [3.7e-9, 0.0, 5.1e-4, 1.0, 0.13, 777.0, 2.0 ** -7, up1(2.0 ** 5), float(torch.nextafter(torch.tensor(2.0 ** -3), torch.tensor(0.0))),
              9.3e5, 16.0, 8.0, up1(2.0 ** -4), up1(2.0 ** -12)]
    x = torch.rand(len(maxima), per, generator=g) * 2 - 1
    x = x / x.abs().amax(dim=1, keepdim=True) * 0.9
    x = x * torch.tensor(maxima)[:, None]
    for j, m in enumerate(maxima):
        pos = per - 1 if j == 2 else (j * 37) % (per - 1)
        x[j, pos] = -m if j % 2 else m
    return x.float(), maxima


def ratio_to_bound(got, ref, bound):
    """max |got - ref| / bound (0 / 0 counts as 0)."""
    d = (got.double() - ref.double()).abs()
    b = bound.double()
    q = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(q.max())
