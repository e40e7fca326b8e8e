"""Float64 references, per-element error bounds, an fp32 emulation, a restatement of the dispatcher, guarded buffers,
mutated references and the case lists for GroupNorm / LayerNorm of csrc/norm.hip.  Torch only, no GPU import: every function
works on the device of its inputs, so test_norm_refs_cpu.py runs it here and test_norm_kernels_gpu.py forms the float64
reference on the device.

Tensors are token-major: GroupNorm x [nb, HW, C] with G groups of cpg = C / G adjacent channels, LayerNorm x [M, C].

WHAT THE KERNELS COMPUTE (read from csrc/norm.hip), all arithmetic fp32, inputs and outputs 16 bit:
  GroupNorm forward   mean, rstd = (var + eps)^-1/2 per (n, g);  a = rstd gamma, b = beta - mean a per (n, c);
                      z = x a + b;  y = silu?(z), one storage rounding
  GroupNorm backward  z as above from the saved a, b;  dz = dy silu'(z);  S1 = sum dz gamma, S2 = sum dz (z - beta) per (n, g);
                      c2 = -rstd^2 S2 / cnt, c3 = -rstd S1 / cnt - c2 mean;  dx = a dz + c2 x + c3 (+ add), one storage rounding
  LayerNorm forward   y = (x - mean) rstd gamma + beta;  backward  xh = (x - mean) rstd, dg = dy gamma,
                      dx = rstd (dg - mean(dg) - xh mean(dg xh)) (+ add)

BOUNDS.  u = 2^-11 (fp16) / 2^-8 (bf16) is the storage rounding, eta = 2^-25 its absolute form below fp16's normal range,
U32 = 2^-24 one fp32 rounding, S = 2^-14 the bar of the saved statistics (below).  E is first order; the GPU tests assert
|got - ref| <= SLACK E with SLACK = 2 for what E leaves out (second-order terms, fused multiply-adds, u |got| against u |ref|);
the CPU tests hold the fp32 emulation of a correct kernel and the rounded float64 result to 1.0 E and every mutant outside 2 E.
Terms of E_y (gn_bounds / ln_bounds, one comment per term there):
    u |y| + eta                       the store
    2 U32 (|x a| + |mean a| + |z|)    the fp32 affine: the products x a and mean a are rounded once each and the two
                                      additions at their size -- this is the cancellation term, 2^-16 |gamma| at |mean| / std = 256
    S |gamma| (|xh| + 1)              what the statistics bar allows: d xh = xh d rstd / rstd + rstd d mean
    |silu'(z)| (both of the above), U32 (|z| + 4) |y|   SiLU: the exponent product z log2(e) (|z| U32 relative on exp), v_exp
                                      (1 ulp = 2 U32), 1 + e and the division (U32 each)
Terms of E_dx:
    u |dx| + eta                      the store
    |a| e_dz                          e_dz = |dy| (e_silu' + |silu''(z)| e_z), e_z = the two z terms above
    rstd (e_m1 + |xh| e_m2)           the sums: e_m = L U32 mean|terms| + the terms' own error; L = the longest chain of fp32
                                      additions any element passes (rows of a thread, the 8-lane LDS merge, fold, slot walk: gn_sum_depth)
    2 U32 (|a dz| + |c2 x| + |c2 mean| + |rstd m1| + |add|)   the final fp32 expression; c2 x + c3 cancels like the forward affine
    S (|dx - add| + rstd |m2| (|xh| + 1) + rstd |xh| mean(|gamma dz| (|xh| + 1)))   the statistics bar through rstd and xh
FLOOR = 2^-100 is added to every bound: below fp32's normal range (silu(-100) = -3.7e-42) the intrinsics and bf16 flush to 0.

STATISTICS BAR, the same for both types (mean_rstd is fp32) and independent of E:
    |rstd / rstd64 - 1| <= 2^-14   and   |mean - mean64| rstd64 <= 2^-14      wherever |mean64| rstd64 <= 256
1/8 of an fp16 storage rounding.  What fp32 can reach there: the stored mean alone is rounded by 2^-25 |mean|, 2^-17 std at
ratio 256, 1/8 of the bar; a variance from centred sums is good to about (chain length) 2^-24, far inside."""
import math
from dataclasses import dataclass

import torch

SLACK = 2.0
U32 = 2.0 ** -24
STAT_BAR = 2.0 ** -14
STAT_DOMAIN = 256.0
FLOOR = 2.0 ** -100
GN_MAX_SLOTS = 64
LN_MAXV = 4
# smi_norm_ran.form (include/smi.h SMI_NORM_*)
GN_ONE, GN_TWO, GN_FOLD, LN = 1, 2, 3, 4
FORM_NAMES = {GN_ONE: "one launch", GN_TWO: "two launches", GN_FOLD: "two launches + fold", LN: "layernorm"}


def unit_roundoff(dt):
    return 2.0 ** -11 if dt == torch.float16 else 2.0 ** -8


def sub_eta(dt):
    return 2.0 ** -25 if dt == torch.float16 else 0.0


# ---------------------------------------------------------------------------------------------------------------
# the dispatcher of csrc/norm.hip, restated (the GPU tests assert it equals gn_last_ran())
# ---------------------------------------------------------------------------------------------------------------
def gn_rows_per_chunk(HW):
    if HW > 16384:
        return 256
    r = (HW + 63) // 64
    return 16 if r < 16 else (r + 15) // 16 * 16


def gn_num_chunks(HW):
    rpc = gn_rows_per_chunk(HW)
    return (HW + rpc - 1) // rpc


def gn_fold_per(HW):
    """Chunks per slot of the fold (0: no fold)."""
    n = gn_num_chunks(HW)
    return (n + GN_MAX_SLOTS - 1) // GN_MAX_SLOTS if n > GN_MAX_SLOTS else 0


def gn_partial_floats(nb, HW, G):
    n = gn_num_chunks(HW)
    return nb * (n + (GN_MAX_SLOTS if n > GN_MAX_SLOTS else 0)) * G * 2


def gn_scratch_floats(nb, HW, C, G):
    """smi_op_groupnorm(_ex): a [nb, C] | b [nb, C] | mean_rstd [nb, G, 2] | partials."""
    return 2 * nb * C + nb * G * 2 + gn_partial_floats(nb, HW, G)


def gn_geom(C):
    cols8 = C // 8
    return cols8, (cols8 + 255) // 256, (1 if cols8 >= 256 else 256 // cols8)  # cols8, ncol, rpar


def gn_lds_ok(C):
    return gn_geom(C)[2] * C * 8 <= 65536


def gn_fused_ok(HW, C, G, sel=-1, max_hw=256, max_bytes=98304):
    """sel as set_gn_select: -1 the tuned limits (their defaults here), 0 never, 1 wherever the shape rules hold."""
    cpg = C // G
    sl = HW * cpg * 2
    if sel == 0:
        return False
    tuned = sel == 1 or (HW <= max_hw and sl <= max_bytes)
    return tuned and cpg % 2 == 0 and 2 <= cpg <= 256 and sl + 16 + (8 + 2 * cpg) * 4 <= 160 * 1024


def gn_expected_ran(HW, C, G, sel=-1, what="fwd"):
    """(form, chunks, slots) of a forward ("fwd"), a statistics-only ("stats") or a backward ("bwd") launch."""
    if what == "fwd" and gn_fused_ok(HW, C, G, sel):
        return (GN_ONE, 0, 0)
    n = gn_num_chunks(HW)
    return (GN_FOLD, n, GN_MAX_SLOTS) if n > GN_MAX_SLOTS else (GN_TWO, n, n)


def ln_nv(C):
    return min(LN_MAXV, (C // 8 + 63) // 64)


def ln_rows(M, bwd):
    return 2 if (not bwd and M >= 16384) else 1


def ln_expected_ran(M, C, bwd):
    return (LN, ln_nv(C), ln_rows(M, bwd))


def gn_sum_depth(HW, C, G):
    """L: the longest chain of fp32 additions between an element and its group sum in the two-launch backward."""
    _, _, rpar = gn_geom(C)
    rpc = gn_rows_per_chunk(HW)
    n = gn_num_chunks(HW)
    per = gn_fold_per(HW)
    slots = min(n, GN_MAX_SLOTS)
    return (rpc + rpar - 1) // rpar + (rpar * ((C // G + 7) // 8) + 3) + per + ((slots + 7) // 8 + 3)


def ln_sum_depth(C):
    return ln_nv(C) * 8 + 6


# ---------------------------------------------------------------------------------------------------------------
# SiLU in float64
# ---------------------------------------------------------------------------------------------------------------
def _sig(z):
    return torch.sigmoid(z)


def silu(z):
    return z * _sig(z)


def dsilu(z):
    s = _sig(z)
    return s * (1 + z * (1 - s))


def d2silu(z):
    s = _sig(z)
    return s * (1 - s) * (2 + z * (1 - 2 * s))


# ---------------------------------------------------------------------------------------------------------------
# float64 references (with at most one deliberate fault: MUTANTS)
# ---------------------------------------------------------------------------------------------------------------
def _grp(t, G):
    """[nb, HW, C] -> [nb, HW, G, cpg]"""
    nb, HW, C = t.shape
    return t.reshape(nb, HW, G, C // G)


def _gmean(t, G):
    """Mean over the (HW, cpg) slice of each group, broadcast back to [nb, 1, C]."""
    nb, HW, C = t.shape
    m = _grp(t, G).mean(dim=(1, 3))  # [nb, G]
    return m.repeat_interleave(C // G, dim=1)[:, None, :]


def gn_stats64(x, G, eps, fault=None):
    """mean, rstd [nb, G] in float64."""
    nb, HW, C = x.shape
    cpg = C // G
    xg = _grp(x.double(), G)
    cnt = float(HW * cpg)
    if fault in ("drop_last_row", "dup_row"):
        # the sums miss (count twice) one row while the count stays: the one-pass form of the faulty kernel
        s, q = xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))
        row = HW - 1 if fault == "drop_last_row" else gn_rows_per_chunk(HW)
        sign = -1.0 if fault == "drop_last_row" else 1.0
        s = s + sign * xg[:, row].sum(dim=2)
        q = q + sign * (xg[:, row] ** 2).sum(dim=2)
        mean = s / cnt
        var = (q / cnt - mean * mean).clamp_min(0)
    else:
        mean = xg.mean(dim=(1, 3))
        m2 = ((xg - mean[:, None, :, None]) ** 2).sum(dim=(1, 3))
        var = m2 / (cnt - 1 if fault == "cnt_minus_1" else cnt)
    rstd = (var + (0.0 if fault == "no_eps" else eps)) ** -0.5
    return mean, rstd


def gn_ref(x, gamma, beta, G, eps, silu_on, dy=None, add=None, n0=0, fault=None, stats=None):
    """GroupNorm forward on x [nb, HW, C] and, with dy, the backward on samples [n0, nb) (dy, add, dx: [nb - n0, HW, C]).
    `stats` = (mean, rstd) [nb, G] replaces the float64 statistics (the emulation's one-pass mutant)."""
    nb, HW, C = x.shape
    cpg = C // G
    xd, ga, be = x.double(), gamma.double(), beta.double()
    mean, rstd = stats if stats is not None else gn_stats64(x, G, eps, fault)
    gi = torch.arange(C, device=x.device) // cpg
    if fault == "group_slip":  # the group of the 8-channel vector's first channel
        gi = (torch.arange(C, device=x.device) // 8 * 8) // cpg
    mean_c, rstd_c = mean[:, gi], rstd[:, gi]  # [nb, C]
    a = rstd_c * ga
    b = be - mean_c * a
    z = xd * a[:, None] + b[:, None]
    out = {"mean": mean, "rstd": rstd, "a": a, "b": b, "z": z, "y": silu(z) if silu_on else z,
           "xh": (xd - mean_c[:, None]) * rstd_c[:, None], "mean_c": mean_c, "rstd_c": rstd_c}
    if dy is None:
        return out
    sl = slice(n0, nb)
    src = slice(0, nb - n0) if fault == "stats_sample0" else sl  # the statistics the backward reads
    a_b, b_b, mu_b, r_b = a[src], b[src], mean_c[src], rstd_c[src]
    xb = xd[sl]
    zb = xb * a_b[:, None] + b_b[:, None]
    g = dy.double()
    dz = g * dsilu(xb if fault == "silu_at_x" else zb) if silu_on else g
    cnt = float(HW * cpg)
    s1 = _gmean(dz * ga, G) * cnt
    s2 = _gmean(dz * (zb if fault == "z_no_beta" else zb - be), G) * cnt
    if fault == "no_s2":
        s2 = torch.zeros_like(s2)
    c2 = -r_b[:, None] ** 2 * s2 / cnt
    c3 = (0.0 if fault == "no_c3" else -r_b[:, None] * s1 / cnt) - c2 * mu_b[:, None]
    dx = a_b[:, None] * dz + c2 * xb + c3
    ad = add.double() if add is not None else None
    if ad is not None and fault != "add_ignored":
        dx = dx + (2 * ad if fault == "add_twice" else ad)
    out.update(dx=dx, dz=dz, zb=zb, m1=s1 / cnt, m2=s2 / cnt)
    return out


def ln_ref(x, gamma, beta, eps, dy=None, add=None, row0=0, fault=None):
    M, C = x.shape
    xd, ga, be = x.double(), gamma.double(), beta.double()
    mean = xd.mean(dim=1)
    var = ((xd - mean[:, None]) ** 2).sum(dim=1)
    if fault == "pad_lanes":  # the zero lanes of the last vector counted: each adds (0 - mean)^2
        var = var + (ln_nv(C) * 512 - C) * mean * mean
    rstd = (var / C + eps) ** -0.5
    xh = (xd - mean[:, None]) * rstd[:, None]
    y = xh * ga + be
    if fault == "last_row_unwritten":
        y = y.clone()
        y[M - 1] = float("nan")
    out = {"mean": mean, "rstd": rstd, "xh": xh, "y": y}
    if dy is None:
        return out
    dg = dy.double() * ga
    xb, rb = xh[row0:], rstd[row0:, None]
    s1, s2 = dg.mean(dim=1, keepdim=True), (dg * xb).mean(dim=1, keepdim=True)
    dx = rb * (dg - s1 - xb * s2)
    if add is not None:
        dx = dx + add.double()
    out.update(dx=dx, dg=dg, s1=s1, s2=s2)
    return out


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def _z_err(xd, a, mean_c, z, gamma, xh):
    aff = 2 * U32 * ((xd * a[:, None]).abs() + (mean_c * a).abs()[:, None] + z.abs())  # x a, mean a rounded once; 2 additions
    stat = STAT_BAR * gamma.abs() * (xh.abs() + 1)                                      # d xh = xh S + S
    return aff + stat


def gn_bounds(ref, x, gamma, beta, G, silu_on, dt, dy=None, add=None, n0=0):
    """E_y [nb, HW, C] and, with dy, E_dx [nb - n0, HW, C] from a fault-free gn_ref."""
    u, eta = unit_roundoff(dt), sub_eta(dt)
    nb, HW, C = x.shape
    xd, ga = x.double(), gamma.double()
    z, y = ref["z"], ref["y"]
    e_z = _z_err(xd, ref["a"], ref["mean_c"], z, ga, ref["xh"])
    if silu_on:
        e_y = dsilu(z).abs() * e_z + U32 * (z.abs() + 4) * y.abs()  # z's error through silu'; exp argument, v_exp, 1 + e, divide
    else:
        e_y = e_z
    E_y = u * y.abs() + eta + e_y + FLOOR  # the store
    if dy is None:
        return E_y, None
    sl = slice(n0, nb)
    a, r, mu = ref["a"][sl][:, None], ref["rstd_c"][sl][:, None], ref["mean_c"][sl][:, None]
    xb, xh, zb, dz = xd[sl], ref["xh"][sl], ref["zb"], ref["dz"]
    g = dy.double()
    L = gn_sum_depth(HW, C, G)
    if silu_on:
        s = _sig(zb)
        e_ds = U32 * (zb.abs() + 8) * s * ((1 + zb * (1 - s)).abs() + zb.abs())  # s (|z| + 4 roundings), then 1 - s, z (1 - s), 1 + ., s .
        e_dz = g.abs() * (e_ds + d2silu(zb).abs() * e_z[sl])
    else:
        e_dz = torch.zeros_like(dz)
    gdz = ga * dz
    e_m1 = L * U32 * _gmean(gdz.abs(), G) + _gmean(ga.abs() * e_dz, G)
    e_m2 = (L * U32 * _gmean((gdz * xh).abs(), G) + _gmean((ga * xh).abs() * e_dz, G) + _gmean(dz.abs() * e_z[sl], G))
    c2 = r * r * ref["m2"]
    ad = add.double().abs() if add is not None else 0.0
    dxn = ref["dx"] - (add.double() if add is not None else 0.0)
    E_dx = (u * ref["dx"].abs() + eta                                                          # the store
            + a.abs() * e_dz                                                                   # dz into a dz
            + r * (e_m1 + xh.abs() * e_m2)                                                     # the two sums
            + 2 * U32 * ((a * dz).abs() + (c2 * xb).abs() + (c2 * mu).abs() + (r * ref["m1"]).abs() + ad)  # a dz + c2 x + c3 + add
            + STAT_BAR * (dxn.abs() + r * ref["m2"].abs() * (xh.abs() + 1)                     # the statistics bar
                          + r * xh.abs() * _gmean(gdz.abs() * (xh.abs() + 1), G))
            + FLOOR)
    return E_y, E_dx


def ln_bounds(ref, x, gamma, beta, dt, dy=None, add=None, row0=0):
    u, eta = unit_roundoff(dt), sub_eta(dt)
    M, C = x.shape
    ga = gamma.double()
    xh, y = ref["xh"], ref["y"]
    E_y = (u * y.abs() + eta                                   # the store
           + 3 * U32 * ((xh * ga).abs() + y.abs())             # x - mean, times rstd, times gamma; + beta
           + STAT_BAR * ga.abs() * (xh.abs() + 1) + FLOOR)     # the statistics bar
    if dy is None:
        return E_y, None
    L = ln_sum_depth(C)
    r, xb, dg = ref["rstd"][row0:, None], xh[row0:], ref["dg"]
    ad = add.double().abs() if add is not None else 0.0
    dxn = ref["dx"] - (add.double() if add is not None else 0.0)
    mabs = lambda t: t.abs().mean(dim=1, keepdim=True)
    e_xh = 2 * U32 * xb.abs()                                   # xh itself: x - mean, times rstd
    E_dx = (u * ref["dx"].abs() + eta                                                                      # the store
            + r * ((L + 1) * U32 * (mabs(dg) + xb.abs() * mabs(dg * xb)) + xb.abs() * mabs(dg * e_xh))                  # the sums
            + 3 * U32 * r * (dg.abs() + ref["s1"].abs() + (xb * ref["s2"]).abs()) + r * ref["s2"].abs() * e_xh + U32 * ad
            + STAT_BAR * (dxn.abs() + r * ref["s2"].abs() * (xb.abs() + 1) + r * xb.abs() * mabs(dg * (xb.abs() + 1)))
            + FLOOR)
    return E_y, E_dx


def worst(got, ref, E):
    """max |got - ref| / E; a NaN or inf anywhere in got counts as infinitely wrong."""
    g = got.double()
    if not torch.isfinite(g).all():
        return float("inf")
    return float(((g - ref).abs() / E).max())


def stat_worst(mean, rstd, ref, in_domain_only=True):
    """(worst |rstd / rstd64 - 1|, worst |mean - mean64| rstd64) over the groups (rows) inside the domain, in units of the bar."""
    m64, r64 = ref["mean"], ref["rstd"]
    dom = (m64.abs() * r64 <= STAT_DOMAIN) if in_domain_only else torch.ones_like(m64, dtype=torch.bool)
    if not bool(dom.any()):
        return 0.0, 0.0
    er = (rstd.double() / r64 - 1).abs()[dom]
    em = ((mean.double() - m64).abs() * r64)[dom]
    if not (torch.isfinite(er).all() and torch.isfinite(em).all()):
        return float("inf"), float("inf")
    return float(er.max()) / STAT_BAR, float(em.max()) / STAT_BAR


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulation of a correct kernel (two-pass statistics), and of the one-pass statistics the kernels used to compute
# ---------------------------------------------------------------------------------------------------------------
def gn_stats32(x, G, eps, one_pass):
    nb, HW, C = x.shape
    xg = _grp(x.float(), G)
    cnt = torch.tensor(float(HW * (C // G)), dtype=torch.float32, device=x.device)
    if one_pass:  # var = sumsq / cnt - mean * mean, as every GroupNorm form had it
        mean = xg.sum(dim=(1, 3)) / cnt
        var = ((xg * xg).sum(dim=(1, 3)) / cnt - mean * mean).clamp_min(0)
    else:  # the mean from sums shifted by the slice's first element (a raw fp32 sum of 10^4 values costs the mean 2^-21 of
        # its size: at |mean| / std = 128 already the whole bar), then the centred second pass
        k = xg[:, :1, :, :1]
        mean = k[:, 0, :, 0] + (xg - k).sum(dim=(1, 3)) / cnt
        var = ((xg - mean[:, None, :, None]) ** 2).sum(dim=(1, 3)) / cnt
    return mean, torch.rsqrt(var + eps)


def gn_emulate(x, gamma, beta, G, eps, silu_on, dt, dy=None, add=None, one_pass=False):
    """Every operation in fp32 in the kernels' order, outputs rounded to dt.  Returns y, mean, rstd, dx."""
    nb, HW, C = x.shape
    cpg = C // G
    f = torch.float32
    xf, ga, be = x.to(f), gamma.to(f), beta.to(f)
    mean, rstd = gn_stats32(x, G, eps, one_pass)
    mc, rc = mean.repeat_interleave(cpg, 1), rstd.repeat_interleave(cpg, 1)
    a = rc * ga
    b = be - mc * a
    z = xf * a[:, None] + b[:, None]
    sig = lambda t: 1 / (1 + torch.exp(-t))
    y = (z * sig(z) if silu_on else z).to(dt)
    if dy is None:
        return y, mean, rstd, None
    dz = dy.to(f)
    if silu_on:
        s = sig(z)
        dz = dz * (s * (1 + z * (1 - s)))
    cnt = float(HW * cpg)
    gsum = lambda t: _grp(t, G).sum(dim=(1, 3)).repeat_interleave(cpg, 1)[:, None]
    s1, s2 = gsum(dz * ga), gsum(dz * (z - be))
    c2 = -rc[:, None] * rc[:, None] * s2 / cnt
    c3 = -rc[:, None] * s1 / cnt - c2 * mc[:, None]
    dx = a[:, None] * dz + c2 * xf + c3
    if add is not None:
        dx = dx + add.to(f)
    return y, mean, rstd, dx.to(dt)


def ln_emulate(x, gamma, beta, eps, dt, dy=None, add=None):
    f = torch.float32
    xf, ga, be = x.to(f), gamma.to(f), beta.to(f)
    C = x.shape[1]
    mean = xf[:, 0] + (xf - xf[:, :1]).sum(dim=1) / C  # shifted by the row's first element, as the kernel
    rstd = torch.rsqrt(((xf - mean[:, None]) ** 2).sum(dim=1) / C + eps)
    xh = (xf - mean[:, None]) * rstd[:, None]
    y = (xh * ga + be).to(dt)
    if dy is None:
        return y, mean, rstd, None
    dg = dy.to(f) * ga
    s1, s2 = dg.sum(dim=1, keepdim=True) / C, (dg * xh).sum(dim=1, keepdim=True) / C
    dx = rstd[:, None] * (dg - s1 - xh * s2)
    if add is not None:
        dx = dx + add.to(f)
    return y, mean, rstd, dx.to(dt)


# ---------------------------------------------------------------------------------------------------------------
# guarded output buffers: NaN prefill, NaN guard rows on both sides
# ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """A [rows, width] output of dtype dt (16 bit or fp32) inside a buffer with `g` guard rows on each side, all NaN."""

    def __init__(self, rows, width, dt, device, g=2):
        self.full = torch.full((rows + 2 * g, width), float("nan"), dtype=dt, device=device)
        self.g, self.rows = g, rows
        self.view = self.full[g:g + rows]

    def guards_intact(self):
        return bool(torch.isnan(self.full[:self.g]).all() and torch.isnan(self.full[self.g + self.rows:]).all())

    def untouched(self):
        return bool(torch.isnan(self.full).all())


# ---------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests, and their inputs (made on the CPU from a seed, so both test files see the same bits)
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GnCase:
    name: str
    HW: int
    C: int
    G: int
    nb: int = 3
    data: str = "geom"  # see gn_inputs
    arg: float = 0.0
    silu: int = 1
    eps: float = 1e-5


EPS = 1e-5

# geometry: every (C, G) pair at a small ragged HW, every HW at C = 64 (fold with per = 3 included)
GN_GEOMETRY = (
    [GnCase(f"c{C}g{G}", 100, C, G) for C, G in [(24, 8), (64, 32), (128, 64), (320, 32), (1920, 32), (2048, 32), (2560, 32),
                                                 (64, 1)]]
    + [GnCase(f"hw{HW}", HW, 64, 8) for HW in [1, 15, 16, 17, 100, 256, 257, 1024, 1025]]
    + [GnCase(f"hw{HW}", HW, 64, 8, nb=3) for HW in [16384, 16385, 256 * 129 + 5]]
    + [GnCase("c24g8hw17", 17, 24, 8), GnCase("c320g32hw257", 257, 320, 32)])
_NUM_SHAPES = [(256, 320, 32), (1024, 320, 32), (4096, 128, 32)]
_NUM_DATA = ([("offset", r) for r in (0.0, 8.0, 32.0, 128.0, 256.0)]
             + [("std001", 0.0), ("const", 0.0), ("var_eps", 0.0), ("big", 0.0), ("lossscale", 0.0), ("silu_sat", 0.0)])


def _outlier_rows(HW):
    rpc = gn_rows_per_chunk(HW)
    return sorted({min(HW - 1, rpc - 1), min(HW - 1, rpc), HW - 1})


GN_NUMERICS = ([GnCase(f"{d}{int(a) if a else ''}_{HW}x{C}", HW, C, G, nb=2, data=d, arg=a)
                for HW, C, G in _NUM_SHAPES for d, a in _NUM_DATA]
               + [GnCase(f"outlier{r}_{HW}x{C}", HW, C, G, nb=2, data="outlier", arg=float(r))
                  for HW, C, G in _NUM_SHAPES for r in _outlier_rows(HW)])
GN_CASES = {c.name: c for c in GN_GEOMETRY + GN_NUMERICS}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_inputs(case: GnCase, dt):
    """x, gamma, beta, dy, add as CPU tensors of dtype dt (dy, add for all nb samples; a sub-range backward slices them)."""
    nb, HW, C, G = case.nb, case.HW, case.C, case.G
    cpg = C // G
    g = _gen(1000 + HW * 7 + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    base = rn(nb, HW, G, cpg)
    gm = (ru(nb, 1, G, 1) * 4 - 2)   # a mean and a std of its own for every (sample, group)
    gs = (ru(nb, 1, G, 1) * 1.5 + 0.5)
    gamma = 1 + 0.25 * rn(C)
    beta = 0.25 * rn(C)
    dy = rn(nb, HW, C)
    add = rn(nb, HW, C)
    d = case.data
    if d in ("geom", "lossscale", "silu_sat", "outlier", "const"):
        x = gm + gs * base
    elif d == "offset":  # |mean| / std = arg at std 1, the sign alternating over the groups; the 16-bit rounding only widens std
        sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).double().view(1, 1, G, 1)
        x = sign * case.arg * (0.97 - 0.02 * ru(nb, 1, G, 1)) + base
    elif d == "std001":
        x = 1.0 + 0.01 * base
    elif d == "var_eps":
        x = math.sqrt(EPS) * base
    elif d == "big":  # |x| up to 3e4 and beyond: the sums of squares must hold 1e13
        x = (1.2e4 * base).clamp(-6.0e4, 6.0e4)
    else:
        raise ValueError(d)
    if d == "const":
        x[:, :, 0, :] = 0.5
    if d == "outlier":
        x[:, int(case.arg)] = 40.0
    if d == "lossscale":  # std >= 1 and |dy| <= 5 * 2^11, so that the true dx (about |gamma| |dy| rstd) stays inside fp16
        x = gm + (gs + 0.5) * base
        dy = dy * 2.0 ** -4 * 2.0 ** 15
    if d == "silu_sat":  # z near +20, -20 and -100 in the first three groups
        for gi, b0 in ((0, 20.0), (1, -20.0), (2, -100.0)):
            gamma[gi * cpg:(gi + 1) * cpg] = 0.05
            beta[gi * cpg:(gi + 1) * cpg] = b0
    x = x.reshape(nb, HW, C)
    return {k: v.to(dt) for k, v in dict(x=x, gamma=gamma, beta=beta, dy=dy, add=add).items()}


@dataclass(frozen=True)
class LnCase:
    name: str
    M: int
    C: int
    ratio: float = 0.0
    bwd: bool = True


LN_CASES_LIST = ([LnCase(f"c{C}m{M}", M, C) for C in (8, 504, 512, 520, 1280, 2040, 2048) for M in (1, 3, 5, 77)]
                 + [LnCase(f"c{C}m{M}", M, C) for C in (64, 1024, 1280, 2048) for M in (16384, 16385)]
                 + [LnCase(f"ratio{int(r)}_c{C}", 5, C, ratio=r) for C in (520, 2048) for r in (8.0, 32.0, 128.0, 256.0)])
LN_CASES = {c.name: c for c in LN_CASES_LIST}


def ln_inputs(case: LnCase, dt):
    M, C = case.M, case.C
    g = _gen(2000 + M * 3 + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    if case.ratio:
        sign = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double().view(M, 1)
        x = sign * case.ratio * (0.94 - 0.02 * ru(M, 1)) + rn(M, C)
    else:
        x = (ru(M, 1) * 4 - 2) + (ru(M, 1) * 1.5 + 0.5) * rn(M, C)
    d = dict(x=x, gamma=1 + 0.25 * rn(C), beta=0.25 * rn(C), dy=rn(M, C), add=rn(M, C))
    return {k: v.to(dt) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------
# mutants: the fault, the case of the GPU tests that catches it, and where it shows
# ---------------------------------------------------------------------------------------------------------------
GN_MUTANTS = {  # fault -> case name
    "cnt_minus_1": "c24g8hw17",       # 51 elements per group: rstd moves by 1 %
    "no_eps": "var_eps_256x320",      # variance = eps: rstd off by sqrt 2
    "group_slip": "c24g8",            # cpg = 3: channels 3..7 of every vector read a neighbour's statistics
    "drop_last_row": "hw257",         # the ragged last chunk is one row
    "dup_row": "hw257",
    "silu_at_x": "c320g32",
    "no_c3": "c320g32",
    "no_s2": "c320g32",
    "z_no_beta": "c320g32",
    "add_ignored": "c320g32",
    "add_twice": "c320g32",
    "stats_sample0": "c320g32",       # bwd_n0 = 1
    "one_pass": "offset256_1024x320",  # the arithmetic every GroupNorm form had: var = sumsq / cnt - mean^2 in fp32
}
LN_MUTANTS = {
    "pad_lanes": "c520m5",            # 504 pad elements next to 520 real ones
    "last_row_unwritten": "c64m16385",  # odd M under R = 2
}


def gn_mutant_outputs(fault, case: GnCase, inp, dt):
    """What a kernel with the fault would return, rounded as the kernel stores it: dict y, mean, rstd, dx (+ n0)."""
    n0 = 1 if fault == "stats_sample0" else 0
    dy, add = inp["dy"][n0:], inp["add"][n0:]
    if fault == "one_pass":
        y, mean, rstd, dx = gn_emulate(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, case.silu, dt, dy, add, one_pass=True)
        return dict(y=y, mean=mean, rstd=rstd, dx=dx, n0=0)
    m = gn_ref(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, case.silu, dy, add, n0=n0, fault=fault)
    return dict(y=m["y"].to(dt), mean=m["mean"].float(), rstd=m["rstd"].float(), dx=m["dx"].to(dt), n0=n0)


def gn_judge(case: GnCase, inp, dt, got, n0=0):
    """Worst ratios of a set of outputs against the fault-free reference: y / E_y, dx / E_dx, rstd and mean over the bar."""
    dy, add = inp["dy"][n0:], inp["add"][n0:]
    ref = gn_ref(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, case.silu, dy, add, n0=n0)
    E_y, E_dx = gn_bounds(ref, inp["x"], inp["gamma"], inp["beta"], case.G, case.silu, dt, dy, add, n0=n0)
    sr, sm = stat_worst(got["mean"], got["rstd"], ref)
    if case.data == "const":
        # the constant group (rstd = eps^-1/2 multiplies fp32 noise the float64 reference does not have): y within E, dx finite
        E_dx = E_dx.clone()
        E_dx[:, :, :case.C // case.G] = float("inf")
    return dict(y=worst(got["y"], ref["y"], E_y), dx=worst(got["dx"], ref["dx"], E_dx), rstd=sr, mean=sm)
