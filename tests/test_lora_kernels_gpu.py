"""The LoRA / DoRA gradient kernels of csrc/lora.hip one by one on a real MI355X, each through its C-ABI test entry point
(include/smi.h `smi_op_*`: the launchers the engine calls), against the float64 references of tests/lora_kernel_refs.py on
the same 16-bit-rounded inputs.

Tolerances are either none (integer data whose sums are exact in fp32 in any order, or pure data movement: torch.equal) or
derived from term counts and unit roundoffs in the docstrings of lora_kernel_refs.py; test_lora_kernel_refs_cpu.py proves
on the same inputs that mutated references fall outside them and the rounded float64 reference inside."""
import ctypes as C
import math

import pytest
import torch

import lora_kernel_refs as KR
from lora_kernel_refs import WJob

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def A(t):
    return None if t is None else t.data_ptr()


def chk(lib, rc):
    assert rc == 0, lib.smi_last_error().decode()


def dcode(dt):
    return 0 if dt == torch.float16 else 1


def cu(t):
    return None if t is None else t.cuda()


def nan_filled(shape, dt):
    """A destination whose every element is a NaN bit pattern (0x7fff in fp16 and bf16)."""
    return torch.full(shape, 0x7FFF, dtype=torch.int16, device="cuda").view(dt)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------
# grouped reduction
# ---------------------------------------------------------------------------------------------------------------
def run_wgrad_table(lib, dt, entries):
    """entries: dicts with the device tensors and fields of one job each (X, P, rs, dW = flat output with guards, base = offset
    of element (0, 0) in it, so_r, so_k, and the scalar fields).  One call of the grouped reduction."""
    from sliders_conceptmod_amd._native import WgradJobC
    n = len(entries)
    arr = (WgradJobC * n)()
    for j, e in zip(arr, entries):
        j.X, j.P, j.row_scale = A(e["X"]), A(e["P"]), A(e.get("rs"))
        j.dW = e["dW"].data_ptr() + 4 * e["base"]
        j.ldx, j.ldp, j.so_r, j.so_k = e["ldx"], e["ldp"], e["so_r"], e["so_k"]
        j.M, j.K, j.r, j.seg_cols, j.rows_per_sample = e["M"], e["K"], e["r"], e.get("seg_cols", 0), e["rps"]
        j.alpha, j.m_begin, j.conv_tap = e["alpha"], e.get("m_begin", 0), e.get("conv_tap", -1)
        j.Hin, j.Win, j.Hout, j.Wout = e.get("Hin", 0), e.get("Win", 0), e.get("Hout", 0), e.get("Wout", 0)
        j.conv_stride, j.conv_ups = e.get("conv_stride", 0), e.get("conv_ups", 0)
    need = C.c_size_t(0)
    chk(lib, lib.smi_op_lora_wgrad_jobs_floats(arr, n, C.byref(need)))
    scratch = torch.empty(need.value, device="cuda")
    chk(lib, lib.smi_op_lora_wgrad_jobs(dcode(dt), arr, n, P(scratch), need.value, None))
    torch.cuda.synchronize()
    return arr, need.value


def entry_of(job):
    """A built job (lora_kernel_refs.build_wjob) on the device."""
    s = job["spec"]
    rk = s.layout == "rk"
    return {"X": cu(job["X"]), "P": cu(job["P"]), "rs": cu(job["rs"]), "dW": cu(job["dW0"]), "base": KR.GUARD,
            "ldx": job["ldx"], "ldp": job["ldp"], "so_r": s.K if rk else 1, "so_k": 1 if rk else s.r,
            "M": s.M, "K": s.K, "r": s.r, "seg_cols": s.seg_cols, "rps": job["rps"], "alpha": s.alpha, "m_begin": s.m_begin}


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sorted(KR.WGRAD_EXACT))
def test_wgrad_grouped_exact(lib, dt, name):
    """One table per case, integer data (|X| <= 8, |P| <= 4, power-of-two row scales and alpha, integer dW pre-fill): every
    partial sum is exact in fp32 whatever the order, so the result -- guards included -- EQUALS the float64 reference.
    mixed_classes: ranks 16, 3, 32, 8, 4 unsorted, both output layouts (the sort, wg0 / fb0, the per-class table base and the
    binary searches); fused_*: P staged in LDS (pw <= 12 / 32) and read from memory (pw = 48), segments inside one column block;
    row_scale: a sample boundary inside a 64-row workgroup, ldp > r, ldx > K; geometry: every column-block width rule of
    wgrad_job_plan, a single row, and the rows-per-workgroup switch at M = 2048."""
    jobs = [KR.build_wjob(s, dt, seed=100 + i) for i, s in enumerate(KR.WGRAD_EXACT[name])]
    entries = [entry_of(j) for j in jobs]
    run_wgrad_table(lib, dt, entries)
    for i, (j, e) in enumerate(zip(jobs, entries)):
        got = e["dW"].cpu()
        bad = (got != j["ref"]).nonzero().flatten()
        assert bad.numel() == 0, (f"{name} job {i} {j['spec']}: {bad.numel()} of {got.numel()} elements differ, first at flat "
                                  f"{bad[:8].tolist()} (guard = {KR.GUARD}): got {got[bad[:8]].tolist()} want {j['ref'][bad[:8]].tolist()}")


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,m_begin,rps,r,K,seg,ldp", KR.WGRAD_TAIL)
def test_wgrad_tail_form(lib, dt, M, m_begin, rps, r, K, seg, ldp):
    """m_begin > 0 (the backward over the live samples only): rows below m_begin do not exist, the geometry is that of the full
    job, split0 = m_begin // rows_per_wg workgroups are not launched and the first launched one is partly skipped (m_begin is
    no multiple of 64 / 256).  Integer data: equal to the float64 reference of the live rows, and bit-equal to the full job run
    with zero rows in front."""
    job = KR.build_wjob(WJob(M, K, r, seg_cols=seg, rps=rps, ldp=ldp, scaled=True, m_begin=m_begin), dt, seed=7)
    tail = entry_of(job)
    full = dict(tail)
    full["X"] = torch.cat([torch.zeros(m_begin, job["ldx"], dtype=dt), job["X"]]).cuda()
    full["P"] = torch.cat([torch.zeros(m_begin, job["ldp"]), job["P"]]).cuda()
    full["rs"] = torch.cat([torch.ones(m_begin // rps), job["rs"]]).cuda()
    full["dW"], full["m_begin"] = cu(job["dW0"]), 0
    run_wgrad_table(lib, dt, [tail])
    run_wgrad_table(lib, dt, [full])
    assert torch.equal(tail["dW"].cpu(), job["ref"]), "tail job differs from the float64 reference of the live rows"
    assert torch.equal(tail["dW"].view(torch.int32), full["dW"].view(torch.int32)), "tail != full job with zero rows in front"


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("stride,ups,skip", KR.CONV_CASES)
def test_wgrad_conv_taps(lib, dt, stride, ups, skip):
    """conv_tap >= 0: the nine tap jobs of a 3x3 / pad-1 down filter in one table, two non-square 6 x 10 images, stride 1, stride
    2 (3 x 5 outputs) and the nearest-2x upsampled input (12 x 20 outputs), and with the first image skipped (m_begin at the
    image boundary).  Integer data: the filter gradient [r][K][3][3] equals the float64 reference built by explicit index
    arithmetic; a wrong tap, stride or border is an exact mismatch."""
    c = KR.build_conv_case(dt, stride, ups, skip)
    img, Pm, rs, dW = cu(c["img"]), cu(c["P"]), cu(c["rs"]), cu(c["dW0"])
    entries = [{"X": img, "P": Pm, "rs": rs, "dW": dW, "base": KR.GUARD + t, "ldx": KR.CONV_K, "ldp": c["ldp"],
                "so_r": 9 * KR.CONV_K, "so_k": 9, "M": c["M"], "K": KR.CONV_K, "r": KR.CONV_R, "rps": c["rps"],
                "alpha": c["alpha"], "m_begin": c["m_begin"], "conv_tap": t, "Hin": KR.CONV_HIN, "Win": KR.CONV_WIN,
                "Hout": c["Hout"], "Wout": c["Wout"], "conv_stride": stride, "conv_ups": ups} for t in range(9)]
    run_wgrad_table(lib, dt, entries)
    got = dW.cpu()
    bad = (got != c["ref"]).nonzero().flatten() - KR.GUARD
    assert bad.numel() == 0, f"{bad.numel()} elements differ; (q, k, tap) of the first: {[(int(b) // (9 * KR.CONV_K), int(b) // 9 % KR.CONV_K, int(b) % 9) for b in bad[:8]]}"


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("spec", KR.WGRAD_RANDOM, ids=lambda s: f"r{s.r}")
def test_wgrad_random_data(lib, dt, spec):
    """Random data, one job per accumulator class (M = 600, K = 320, two fused segments, three samples with row scales) against
    float64 with the forward-error bound of an fp32 sum in any order: |got - ref| <= (M + 2) 2^-24 (|alpha| |P rs|^T |X| + |dW0|)
    elementwise -- derived, not measured."""
    job = KR.build_wjob(spec, dt, seed=40 + spec.r, exact=False)
    e = entry_of(job)
    run_wgrad_table(lib, dt, [e])
    got = e["dW"].cpu()
    assert torch.equal(got[:KR.GUARD], job["dW0"][:KR.GUARD]) and torch.equal(got[-KR.GUARD:], job["dW0"][-KR.GUARD:])
    ratio = KR.ratio_to_bound(got[KR.GUARD:-KR.GUARD], job["ref64"], KR.wgrad_random_bound(job))
    print(f"wgrad random r={spec.r} {dt}: max error / bound = {ratio:.3e}")
    assert ratio <= 1.0


def test_wgrad_jobs_rejects_small_scratch(lib):
    job = KR.build_wjob(WJob(100, 64, 4), torch.float16, seed=1)
    e = entry_of(job)
    from sliders_conceptmod_amd._native import WgradJobC
    arr = (WgradJobC * 1)()
    j = arr[0]
    j.X, j.P, j.dW = A(e["X"]), A(e["P"]), e["dW"].data_ptr() + 4 * KR.GUARD
    j.ldx, j.ldp, j.so_r, j.so_k, j.M, j.K, j.r, j.rows_per_sample, j.alpha, j.conv_tap = 64, 4, 64, 1, 100, 64, 4, 100, 0.5, -1
    need = C.c_size_t(0)
    chk(lib, lib.smi_op_lora_wgrad_jobs_floats(arr, 1, C.byref(need)))
    scratch = torch.empty(need.value, device="cuda")
    assert lib.smi_op_lora_wgrad_jobs(0, arr, 1, P(scratch), need.value - 1, None) != 0
    assert b"scratch" in lib.smi_last_error()
    assert torch.equal(e["dW"].cpu(), job["dW0"])  # nothing ran


# ---------------------------------------------------------------------------------------------------------------
# 16-bit shadow operands
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
def test_lora_prep_shadow_operands(lib, dt):
    """The fp32 -> 16-bit shadow operands of four sites in one launch: a fused Linear (three segments: block-diagonal upT), a
    rank-16 Linear, and two 3x3 conv sites (flipped and plain gradient-filter taps).  Data movement and one rounding: every
    region of the NaN-pre-filled shadow buffer is bit-equal to the reference, and everything between the regions stays NaN."""
    from sliders_conceptmod_amd._native import LoraPrepSiteC
    g = KR.gen(13)
    sites = KR.LORA_PREP_SITES
    arr = (LoraPrepSiteC * len(sites))()
    downs, ups, want = [torch.full((8,), 333.0)], [torch.full((5,), 333.0)], []
    nd, nu, ns = 8, 5, KR.GUARD
    for c, (r, nseg, K, cs, rp, conv) in zip(arr, sites):
        down = torch.randn(r, K, 3, 3, generator=g) if conv else torch.randn(nseg * r, K, generator=g)
        up = torch.randn(nseg, cs, r, generator=g)
        c.off_down, c.off_up, c.r, c.nseg, c.K, c.cs, c.rows_pad, c.conv = nd, nu, r, nseg, K, cs, rp, conv
        downs += [down.reshape(-1), torch.full((3,), 333.0)]
        ups += [up.reshape(-1), torch.full((7,), 333.0)]
        nd, nu = nd + down.numel() + 3, nu + up.numel() + 7
        parts = KR.lora_prep_ref(down, up, r, nseg, K, cs, rp, conv, dt)
        offs = []
        for p in parts:
            offs.append(ns)
            ns += (p.numel() if p is not None else 0) + KR.GUARD
        c.dst_down, c.dst_up, c.dst_gw = offs
        want.append(list(zip(offs, parts)))
    shadow = nan_filled((ns,), dt)
    ddown, dup = torch.cat(downs).cuda(), torch.cat(ups).cuda()
    table = torch.empty(len(sites) * C.sizeof(LoraPrepSiteC), dtype=torch.uint8, device="cuda")
    chk(lib, lib.smi_op_lora_prep(dcode(dt), arr, len(sites), P(ddown), P(dup), P(shadow), P(table), None))
    torch.cuda.synchronize()
    got = bits(shadow.cpu())
    expect = torch.full((ns,), 0x7FFF, dtype=torch.int16)
    for regions in want:
        for off, p in regions:
            if p is not None:
                expect[off:off + p.numel()] = bits(p.reshape(-1))
    bad = (got != expect).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} shadow elements differ, first at {bad[:8].tolist()}; regions {[[o for o, _ in r] for r in want]}"


# ---------------------------------------------------------------------------------------------------------------
# transposes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("C_,lds", [(320, 320), (320, 328), (72, 72), (72, 96), (100, 100), (100, 104)])
@pytest.mark.parametrize("with_f", [True, False])
def test_transpose_scaled(lib, dt, C_, lds, with_f):
    """dst[c][m] = src[m][c] * f[m // 77] for m < M = 154, zero for 154 <= m < Mp = 192 -- data movement and one fp32 product:
    bit-equal to (src.float() * f).to(dt) transposed and zero-padded.  The destination starts as NaN patterns, so unwritten and
    wrongly zeroed elements both show.  C % 8 == 0 with an aligned source takes the 16-byte kernel; the same data two elements
    further on (misaligned) and C = 100 take the element-wise kernel; where both apply they must agree bit for bit."""
    M, Mp, rps = 154, 192, 77
    g = KR.gen(3)
    src = torch.randn(M, lds, generator=g).to(dt)
    f = torch.tensor([0.37, 1.9]) if with_f else None
    ref = KR.transpose_scaled_ref(src, M, C_, Mp, f, rps, dt)
    dsrc, df = src.cuda(), cu(f)
    outs = []
    if C_ % 8 == 0:  # vector path
        dst = nan_filled((C_, Mp), dt)
        assert dsrc.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        chk(lib, lib.smi_op_transpose_scaled(dcode(dt), P(dsrc), lds, P(dst), M, C_, Mp, P(df), rps, None))
        outs.append(dst)
    # element-wise path: the same matrix at a source address that is not a multiple of 16 bytes
    buf = torch.zeros(M * lds + 8, dtype=dt, device="cuda")
    buf[2:2 + M * lds] = dsrc.reshape(-1)
    dst2 = nan_filled((C_, Mp), dt)
    assert (buf.data_ptr() + 4) % 16 != 0
    chk(lib, lib.smi_op_transpose_scaled(dcode(dt), C.c_void_p(buf.data_ptr() + 4), lds, P(dst2), M, C_, Mp, P(df), rps, None))
    outs.append(dst2)
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(bits(o.cpu()), bits(ref))
    assert torch.equal(bits(outs[0]), bits(outs[-1]))


def run_dora_prep(lib, dt, sites, mult, seed=5):
    """smi_op_dora_prep on a table: returns (down_flat, up_flat, entries) with per site the device outputs dW / dWt / cnorm (each
    inside a guarded buffer, dW and dWt pre-filled with NaN patterns) and the filled smi_dora_site."""
    from sliders_conceptmod_amd._native import DoraSiteC
    down, up, ents = KR.build_dora_table(sites, dt, seed)
    ddown, dup = down.cuda(), up.cuda()
    arr = (DoraSiteC * len(ents))()
    for c, e in zip(arr, ents):
        s = e["site"]
        rows = s.nseg * s.cs
        e["dWbuf"], e["dWtbuf"] = nan_filled((rows * s.K + 2 * KR.GUARD,), dt), nan_filled((rows * s.K + 2 * KR.GUARD,), dt)
        e["cnbuf"] = torch.full((s.nseg * s.K + 2 * KR.GUARD,), -777.0, device="cuda")
        e["dW"] = e["dWbuf"][KR.GUARD:KR.GUARD + rows * s.K].view(rows, s.K)
        e["dWt"] = e["dWtbuf"][KR.GUARD:KR.GUARD + rows * s.K].view(s.K, rows)
        e["cnorm"] = e["cnbuf"][KR.GUARD:KR.GUARD + s.nseg * s.K].view(s.nseg, s.K)
        e["Wd"] = e["W"].cuda()
        c.W, c.dW, c.dWt, c.cnorm = A(e["Wd"]), e["dW"].data_ptr(), e["dWt"].data_ptr(), e["cnorm"].data_ptr()
        c.off_down, c.off_up, c.off_dora = e["off_down"], e["off_up"], e["off_dora"]
        c.r, c.nseg, c.K, c.cs, c.scale = s.r, s.nseg, s.K, s.cs, s.scale
    table_dev = torch.empty(len(ents) * C.sizeof(DoraSiteC), dtype=torch.uint8, device="cuda")
    chk(lib, lib.smi_op_dora_prep(dcode(dt), arr, len(ents), P(ddown), P(dup), mult, P(table_dev), None))
    torch.cuda.synchronize()
    for c, e in zip(arr, ents):
        e["c"] = c
    assert torch.equal(ddown.cpu(), down) and torch.equal(dup.cpu(), up)  # parameters are read only
    return ddown, dup, ents, arr


def guards_intact(buf, fill_bits=None, fill=None):
    lo, hi = buf[:KR.GUARD].cpu(), buf[-KR.GUARD:].cpu()
    if fill_bits is not None:
        return bool((bits(lo) == fill_bits).all() and (bits(hi) == fill_bits).all())
    return bool((lo == fill).all() and (hi == fill).all())


@pytest.mark.parametrize("dt", DT)
def test_dora_transpose_is_exact(lib, dt):
    """dWt of every site in one launch: three sites of different sizes (192 x 64, 40 x 72, 100 x 328: the smaller ones leave the
    shared grid early, tiles are partial in both directions); dWt, pre-filled with NaN patterns, is bit for bit dW transposed."""
    _, _, ents, _ = run_dora_prep(lib, dt, KR.DORA_TRANSPOSE_TABLE, 1.0)
    for e in ents:
        assert not torch.isnan(e["dW"].float()).any()
        assert torch.equal(bits(e["dWt"].cpu()), bits(e["dW"].t().cpu())), e["site"]
        assert guards_intact(e["dWtbuf"], fill_bits=0x7FFF) and guards_intact(e["dWbuf"], fill_bits=0x7FFF)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sorted(KR.DORA_FWD_TABLES))
def test_dora_forward(lib, dt, name):
    """Column norms and delta weights of a site table in one call: ranks {3, 8, 4} together (rank class 8, the smaller ranks
    behind the q < r guards), ranks 16 and 32 alone; nseg 1 and 3, K = 264 (a partial second 256-column block), cs = 40 / 42 /
    100, non-zero offsets into flat parameter buffers, mult = 1.5.
    cnorm against float64: relative (cs + r + 4) 2^-24 (lora_kernel_refs.cnorm_bound).
    dW against float64 formed with the norms the delta kernel reads (its stored fp32 cnorm, just checked):
    |got - ref| <= EPS[dt] |ref| + (r + 4) 2^-24 lscale (|V g / n| + |W|) (lora_kernel_refs.dora_dw_bound)."""
    _, _, ents, _ = run_dora_prep(lib, dt, KR.DORA_FWD_TABLES[name], KR.DORA_MULT)
    for e in ents:
        s = e["site"]
        lscale = KR.DORA_MULT * s.scale
        V, n, _ = KR.dora_forward_ref(e["W"], e["down"], e["up"], e["g"], lscale)
        cn = e["cnorm"].cpu()
        rn = KR.ratio_to_bound(cn, n, KR.cnorm_bound(s) * n)
        _, _, dW = KR.dora_forward_ref(e["W"], e["down"], e["up"], e["g"], lscale, n=cn)
        got = e["dW"].cpu()
        rd = KR.ratio_to_bound(got, dW, KR.dora_dw_bound(V, cn, e["W"], e["g"], lscale, s.r, dt, dW))
        print(f"dora fwd {name} {s} {dt}: cnorm error / bound {rn:.3e}, dW error / bound {rd:.3e}")
        assert rn <= 1.0, f"cnorm of {s}"
        assert not torch.isnan(got.float()).any() and rd <= 1.0, f"dW of {s}"
        assert guards_intact(e["dWbuf"], fill_bits=0x7FFF) and guards_intact(e["cnbuf"], fill=-777.0)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("site", KR.DORA_GRAD_SITES, ids=lambda s: f"r{s.r}_seg{s.nseg}_K{s.K}_cs{s.cs}")
@pytest.mark.parametrize("with_alpha_dev", [False, True])
def test_dora_grads(lib, dt, site, with_alpha_dev):
    """d(down), d(up) and d(dora_scale) of one site from a random fp32 G, accumulated onto pre-filled flat buffers, against
    float64 autograd with the column norm detached.  cs = 40 leaves some of the 64 row slices of the column sums empty; K = 264 is
    a partial 256-column block.  Tolerance: lora_kernel_refs.dora_grads_bound -- the fp32 summation bound over the number of
    terms (cs for the column sums, K for the row sums) against the corresponding absolute sums, plus the relative error
    (cs + r + 4) 2^-24 of the stored norm the kernels divide by; derivation in its docstring."""
    ddown, dup, ents, arr = run_dora_prep(lib, dt, [site], 1.0, seed=9 + site.r)
    e = ents[0]
    g = KR.gen(77)
    G = torch.randn(site.nseg * site.cs, site.K, generator=g)
    pre_d = torch.randn(ddown.numel(), generator=g)
    pre_u = torch.randn(dup.numel(), generator=g)
    alpha, adev = 0.75, (torch.tensor([0.5]) if with_alpha_dev else None)
    d_down, d_up, dG, dadev = pre_d.cuda(), pre_u.cuda(), G.cuda(), cu(adev)
    need = C.c_size_t(0)
    chk(lib, lib.smi_op_dora_grads_floats(C.byref(arr[0]), C.byref(need)))
    scratch = torch.empty(need.value, device="cuda")
    chk(lib, lib.smi_op_dora_grads(dcode(dt), C.byref(arr[0]), P(dG), P(ddown), P(dup), P(d_down), P(d_up), alpha, P(dadev),
                                   P(scratch), need.value, None))
    torch.cuda.synchronize()
    a_eff = alpha * (0.5 if with_alpha_dev else 1.0)
    rd, ru, rg = KR.dora_grads_ref(e["W"], e["down"], e["up"], e["g"], G, a_eff)
    nd, nu, ng = rd.numel(), ru.numel(), rg.numel()
    sl_d = slice(e["off_down"], e["off_down"] + nd)
    sl_u = slice(e["off_up"], e["off_up"] + nu)
    sl_g = slice(e["off_dora"], e["off_dora"] + ng)
    bd, bu, bg = KR.dora_grads_bound(e["W"], e["down"], e["up"], e["g"], G, a_eff, pre_d[sl_d].view_as(rd),
                                     pre_u[sl_u].view_as(ru), pre_u[sl_g].view_as(rg))
    gd, gu = d_down.cpu(), d_up.cpu()
    ratios = {"d_down": KR.ratio_to_bound(gd[sl_d].view_as(rd), pre_d[sl_d].view_as(rd).double() + rd, bd),
              "d_up": KR.ratio_to_bound(gu[sl_u].view_as(ru), pre_u[sl_u].view_as(ru).double() + ru, bu),
              "d_dora_scale": KR.ratio_to_bound(gu[sl_g].view_as(rg), pre_u[sl_g].view_as(rg).double() + rg, bg)}
    print(f"dora grads {site} {dt} alpha_dev={with_alpha_dev}: error / bound {ratios}")
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # everything outside the site's three regions is untouched
    keep_d = torch.ones(gd.numel(), dtype=torch.bool)
    keep_d[sl_d] = False
    keep_u = torch.ones(gu.numel(), dtype=torch.bool)
    keep_u[sl_u] = False
    keep_u[sl_g] = False
    assert torch.equal(gd[keep_d], pre_d[keep_d]) and torch.equal(gu[keep_u], pre_u[keep_u])


# ---------------------------------------------------------------------------------------------------------------
# adapted Linear, batched-pass form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,seg,r", KR.GEMM_ROWS_CASES)
def test_gemm_rows(lib, dt, N, seg, r):
    """smi_op_gemm_rows with bias and residual against float64: M = 154 with lora_row0 in {0, 77, 154} (all, half, none of the rows
    adapted), fused segments whose boundaries fall inside a 128-column tile (64 of 192, 320 of 960) and unfused N = 320.
    close(mult=4) as test_gemm_full_epilogue, on the whole output and on the first adapted row alone; the rows below lora_row0
    are bit-equal to a call without LoRA."""
    from test_kernels_gpu import close
    d = KR.build_gemm_rows(N, seg, r, dt)
    M, K, s = KR.GEMM_ROWS_M, KR.GEMM_ROWS_K, KR.GEMM_ROWS_SCALE
    a, w, bias, res, up = (d[k].cuda() for k in ("a", "w", "bias", "res", "up"))
    plain = torch.empty(M, N, device="cuda", dtype=dt)
    chk(lib, lib.smi_op_gemm_rows(dcode(dt), P(a), P(w), P(plain), M, N, K, P(bias), P(res), None, None, 0, 0.0, 0, 0, None))
    for row0 in KR.GEMM_ROWS_ROW0:
        xa = d["xa"][:max(M - row0, 1)].contiguous().cuda()
        c = torch.full((M, N), float("nan"), device="cuda", dtype=dt)
        chk(lib, lib.smi_op_gemm_rows(dcode(dt), P(a), P(w), P(c), M, N, K, P(bias), P(res), P(xa), P(up), r, s, row0, seg, None))
        ref = KR.gemm_rows_ref(d["a"], d["w"], d["bias"], d["res"], d["xa"], d["up"], r, s, row0, seg)
        got = c.cpu()
        close(got, ref.float(), dt, what=f"gemm_rows row0={row0}")
        if row0 < M:
            close(got[row0:row0 + 1], ref[row0:row0 + 1].float(), dt, what=f"first adapted row {row0}")
        assert torch.equal(bits(got[:row0]), bits(plain[:row0].cpu())), f"rows below lora_row0={row0} differ from the plain GEMM"


# ---------------------------------------------------------------------------------------------------------------
# loss scales and row multipliers
# ---------------------------------------------------------------------------------------------------------------
def test_grad_scale_and_scale_min(lib):
    """Per-sample loss scales: every scale is an exact power of two with max * scale in (target / 2, target] (target 16; an
    all-zero sample gets 1), the inverse slot holds its exact reciprocal, and scale_min's outputs -- the minimum, its reciprocal,
    min / scale_j -- are exact (all powers of two).  Maxima over 50 binades, one in the last element of its sample, and at, just
    above and just below a power of two."""
    x, _ = KR.build_grad_scale_input()
    n, per = x.shape
    inv_off = 16
    out = torch.full((inv_off + n + 3,), -777.0, device="cuda")
    mn = torch.full((n + 2 + 3,), -777.0, device="cuda")
    dx = x.cuda()
    chk(lib, lib.smi_op_grad_scale(P(dx), n, per, P(out), inv_off, P(mn), None))
    torch.cuda.synchronize()
    out, mn = out.cpu().double(), mn.cpu().double()
    amax = x.double().abs().amax(dim=1)
    for j in range(n):
        s = out[j].item()
        assert s > 0 and math.frexp(s)[0] == 0.5, f"sample {j}: scale {s} is no power of two"
        if amax[j] == 0:
            assert s == 1.0
        else:
            assert KR.GRAD_TARGET / 2 < amax[j].item() * s <= KR.GRAD_TARGET, f"sample {j}: max {amax[j].item()!r} * scale {s} outside (8, 16]"
        assert out[inv_off + j].item() == 1.0 / s
    assert (out[n:inv_off] == -777.0).all() and (out[inv_off + n:] == -777.0).all()
    smin = out[:n].min().item()
    assert mn[0].item() == smin and mn[1].item() == 1.0 / smin
    assert torch.equal(mn[2:2 + n], smin / out[:n]) and (mn[2 + n:] == -777.0).all()


def test_row_scale_f32(lib):
    """x[m, :N] *= row_mul[m // rows_per_mul] with ld > N: bit-equal to the fp32 product, the padding columns untouched."""
    M, N, ld, rpm = 154, 12, 20, 77
    g = KR.gen(2)
    x = torch.randn(M, ld, generator=g)
    mul = torch.tensor([0.37, -1.9])
    dx, dmul = x.cuda(), mul.cuda()
    chk(lib, lib.smi_op_row_scale_f32(P(dx), ld, M, N, P(dmul), rpm, None))
    ref = x.clone()
    ref[:, :N] = x[:, :N] * mul[torch.arange(M) // rpm][:, None]
    assert torch.equal(dx.cpu(), ref)
