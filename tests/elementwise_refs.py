"""Float64 references, per-element bounds and mutated references for the small kernels of csrc/elementwise.hip (and
conv3x3_small of csrc/gemm.hip) that only whole-engine runs reached: pool2x2_sum, colsum, timestep_embed, softmax_rows,
chan_mix, conv3x3_small, nchw_to_nhwc and nchw_to_nhwc_scaled.  Torch only, no GPU import.

Every bound is written from the kernel's rounding sites: u = 2^-11 (fp16) / 2^-8 (bf16) the storage rounding, eta = 2^-25
its absolute form below fp16's normal range, U32 = 2^-24 one fp32 rounding; a sequential fp32 sum of n terms is off by at
most (n - 1) U32 sum|terms|.  The GPU tests assert |got - ref| <= SLACK E, SLACK = 2 (second-order terms, fused multiply-adds);
test_elementwise_refs_cpu.py holds the rounded float64 result to 1.0 E and every mutant outside SLACK E."""
import math

import torch

from norm_refs import FLOOR, SLACK, U32, Guarded, sub_eta, unit_roundoff, worst  # noqa: F401

COLSUM_RS = 16


def _store(ref, dt):
    """The storage rounding of a 16-bit output (nothing for an fp32 one)."""
    if dt == torch.float32:
        return U32 * ref.abs()
    return unit_roundoff(dt) * ref.abs() + sub_eta(dt)


# ---- pool2x2_sum: dx[n, h, w, c] = sum of the 2 x 2 block of du [n, 2h, 2w, c] ------------------------------------
def pool_ref(du, fault=None):
    d = du.double()
    n, H2, W2, C = d.shape
    taps = [d[:, a::2, b::2] for a in (0, 1) for b in (0, 1)]
    if fault == "wrong_tap":  # (a, b) = (1, 1) reads (1, 0) again
        taps[3] = taps[2]
    if fault == "tail_dropped":  # the last 8 channels of a pixel left out
        out = sum(taps)
        out[..., -8:] = float("nan")
        return out, sum(t.abs() for t in taps)
    return sum(taps), sum(t.abs() for t in taps)


def pool_bound(ref, mag, dt):
    return _store(ref, dt) + 3 * U32 * mag + FLOOR  # three fp32 additions, one store


# ---- colsum: out[n, c] = mul * sum_hw x[n, hw, c] -------------------------------------------------------------------
def colsum_ref(x, mul, fault=None):
    d = x.double()
    if fault == "tail_dropped":
        d = d[:, :-1]
    return d.sum(dim=1) * mul, d.abs().sum(dim=1) * abs(mul)


def colsum_bound(ref, mag, HW, dt):
    rows = (HW + COLSUM_RS - 1) // COLSUM_RS
    L = (rows + 7) // 8 + 8 + COLSUM_RS + 1  # a row lane's rows, the 8 lanes, the 16 slices, times mul
    return _store(ref, dt) + L * U32 * mag + FLOOR


# ---- timestep_embed: out[r, :] = cos(t f_k) | sin(t f_k), f_k = exp(-ln(10000) k / half) ------------------------------
def timestep_ref(vals, dim, fault=None):
    half = dim // 2
    k = torch.arange(half, dtype=torch.float64, device=vals.device)
    arg = -math.log(10000.0) * k / half
    a = vals.double()[:, None] * torch.exp(arg)[None]
    first, second = (torch.sin(a), torch.cos(a)) if fault == "sin_first" else (torch.cos(a), torch.sin(a))
    return torch.cat([first, second], dim=1), torch.cat([a, a], dim=1), torch.cat([arg, arg])[None]


def timestep_bound(ref, a, arg, dt):
    # the fp32 argument: the constant, c k and / half are rounded (3 U32 |arg| on the exponent, so relative on f), expf (2 ulp),
    # t f (U32): d a = |t f| (3 |arg| + 5) U32, and |d cos| , |d sin| <= d a; cosf / sinf themselves 2 ulp
    return _store(ref, dt) + a.abs() * (3 * arg.abs() + 5) * U32 + 4 * U32 + FLOOR


# ---- softmax_rows: P[r, :] = softmax(scale * S[r, :]) on fp32 scores --------------------------------------------------
def softmax_ref(S, scale, fault=None):
    s = S.double() * scale
    if fault == "tail_dropped":  # the last column left out of the sum
        p = torch.exp(s - s.max(dim=1, keepdim=True).values)
        return p / p[:, :-1].sum(dim=1, keepdim=True), s
    if fault == "max_times_scale":  # max(S) * scale, the minimum for a negative scale: exp overflows in fp32
        m = S.double().max(dim=1, keepdim=True).values * scale
        e = torch.exp((s - m).clamp_max(88.73))  # fp32 exp saturates to inf above that
        e = torch.where(s - m > 88.72, torch.full_like(e, float("inf")), e)
        return e / e.sum(dim=1, keepdim=True), s
    return torch.softmax(s, dim=1), s


def softmax_bound(ref, s, dt):
    cols = s.shape[1]
    m = s.max(dim=1, keepdim=True).values
    x = s - m
    L = (cols + 255) // 256 + 6 + 3  # a thread's columns, the wave, the four waves
    # s scale and the subtraction (U32 (|s| + |m|) absolute on the exponent), __expf (|x| U32 from x log2(e), 1 ulp), the sum, 1 / sum,
    # the product
    rel = U32 * (2 * (s.abs() + m.abs()) + x.abs() + 4 + L + 3)
    return _store(ref, dt) + ref * rel + FLOOR


# ---- chan_mix: y[m, j] = b[j] + sum_i x[m, i] W[j, i], fp32 in and out ------------------------------------------------
def chan_mix_ref(x, W, b, fault=None):
    xd, Wd, bd = x.double(), W.double(), b.double()
    if fault == "tail_dropped":
        xd, Wd = xd[:, :-1], Wd[:, :-1]
    return bd + xd @ Wd.t(), bd.abs() + xd.abs() @ Wd.abs().t()


def chan_mix_bound(ref, mag, C):
    return (C + 1) * U32 * mag + FLOOR  # C multiply-adds onto the bias, the result kept in fp32


# ---- conv3x3_small: stride 1, pad 1; in [n, H, W, Cin], w [Cout][9 Cin] tap-major, out [n, H, W, Cout] -------------------
def conv_ref(x, w, bias, fault=None):
    xd, wd = x.double(), w.double()
    n, H, W, Cin = xd.shape
    Cout = wd.shape[0]
    w4 = wd.reshape(Cout, 3, 3, Cin)
    if fault == "wrong_tap":
        w4 = w4.flip(2)  # kx mirrored
    xp = torch.zeros(n, H + 2, W + 2, Cin, dtype=torch.float64, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = xd
    if fault == "no_pad_zero":  # the border repeats the edge pixel instead of reading zero
        xp = torch.nn.functional.pad(xd.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    out = torch.zeros(n, H, W, Cout, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + H, kx:kx + W]
            out += torch.einsum("nhwc,oc->nhwo", patch, w4[:, ky, kx])
            mag += torch.einsum("nhwc,oc->nhwo", patch.abs(), w4[:, ky, kx].abs())
    if bias is not None:
        out, mag = out + bias.double(), mag + bias.double().abs()
    return out, mag


def conv_bound(ref, mag, Cin, out_dt):
    return _store(ref, out_dt) + (9 * Cin + 1) * U32 * mag + FLOOR  # 9 Cin multiply-adds in sequence, + bias


def conv_grad_pack(w):
    """The gradient filter of w [Cout][9 Cin]: wg [Cin][9 Cout], wg[ci][t'][co] = w[co][8 - t'][ci] (taps flipped)."""
    Cout = w.shape[0]
    Cin = w.shape[1] // 9
    return w.reshape(Cout, 9, Cin).flip(1).permute(2, 1, 0).reshape(Cin, 9 * Cout).contiguous()


def conv_dx_ref(dy, w):
    """d(in) of out = conv(in, w), by autograd in float64."""
    n, H, W, Cout = dy.shape
    Cin = w.shape[1] // 9
    x = torch.zeros(n, Cin, H, W, dtype=torch.float64, device=dy.device, requires_grad=True)
    wt = w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, wt, padding=1)
    (g,) = torch.autograd.grad(y, x, dy.double().permute(0, 3, 1, 2))
    return g.permute(0, 2, 3, 1)


# ---- nchw_to_nhwc(_scaled): dst[n, hw, c] = src[n, c, hw] * scale (* scale_dev[n]), columns >= C zero ------------------
def nchw_ref(src, Cpad, scale, scale_dev=None, fault=None):
    d = src.double()  # [n, C, HW]
    n, C, HW = d.shape
    sc = torch.full((n,), float(scale), dtype=torch.float64, device=src.device)
    if scale_dev is not None:
        sc = sc * (scale_dev.double()[:1].expand(n) if fault == "scale_sample0" else scale_dev.double())
    out = torch.zeros(n, HW, Cpad, dtype=torch.float64, device=src.device)
    out[:, :, :C] = d.permute(0, 2, 1) * sc[:, None, None]
    if fault == "pad_not_zero":
        out[:, :, C:] = out[:, :, :1]
    return out


def nchw_bound(ref, dt):
    return _store(ref, dt) + U32 * ref.abs() + FLOOR  # one fp32 product, one store (the tests want the pad columns exactly 0)


# ---------------------------------------------------------------------------------------------------------------
# cases and inputs of the GPU tests (made on the CPU from a seed: both test files see the same bits)
# ---------------------------------------------------------------------------------------------------------------
def _rn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


POOL_CASES = [(H, W, C) for H in (1, 3) for W in (1, 3) for C in (8, 24)]
COLSUM_CASES = [(HW, C) for HW in (1, 15, 17, 4096) for C in (8, 264)]
TIMESTEP_CASES = [256, 320]
TIMESTEP_VALUES = [0.0, 0.5, 999.0]
SOFTMAX_CASES = [(1, 0.125), (255, 0.125), (257, 0.125), (4096, 0.044), (257, -0.5)]  # (cols, scale); the last: a negative scale
CHAN_MIX_CASES = [(4, 1), (4, 300), (16, 257), (16, 1000)]  # (C, M): M never a multiple of 256
CONV_CASES = [(H, W, cin, cout) for H in (1, 2, 5) for W in (1, 2, 5) for cin, cout in ((4, 24), (24, 4))]
NCHW_CASES = [(4, 8, 5), (4, 8, 64), (8, 8, 7)]  # (C, Cpad, HW)


def pool_inputs(H, W, C, dt):
    return _rn(11 + H * 7 + W * 3 + C, 2, 2 * H, 2 * W, C).to(dt)


def colsum_inputs(HW, C, dt):
    return (_rn(21 + HW + C, 2, HW, C) + 0.25).to(dt)


def softmax_inputs(cols, scale):
    """fp32 scores [5, cols]; row 1 ends in a dominant element.  scale > 0: scaled scores of deviation 3; scale < 0: of deviation
    40, so that exp(s scale - max(S) scale) -- the kernel before its maximum was taken of the scaled scores -- overflows."""
    dev = 3.0 if scale > 0 else 40.0
    S = _rn(31 + cols, 5, cols, scale=dev / abs(scale))
    if scale > 0:
        S[1, cols - 1] = S[1].max() + 12.0 / scale
    else:
        S[1, cols - 1] = S[1].min() - 30.0 / abs(scale)
    return S.float()


def chan_mix_inputs(C, M, dt):
    return _rn(41 + C + M, M, C).float(), _rn(42 + C, C, C, scale=0.5).to(dt), _rn(43 + C, C).to(dt)


def conv_inputs(H, W, cin, cout, dt):
    return (_rn(51 + H * 5 + W + cin, 2, H, W, cin).to(dt), _rn(52 + cin, cout, 9 * cin, scale=0.2).to(dt), _rn(53 + cout, cout).to(dt))


def nchw_inputs(C, HW, src_dt):
    return _rn(61 + C + HW, 3, C, HW).to(src_dt), torch.tensor([0.5, 3.0, 1024.0])
