"""CPU proof that tests/test_lora_kernels_gpu.py can fail (no GPU needed).  On the very inputs of the GPU file:

* every toleranced comparison rejects mutated references -- one row dropped, two segments swapped, one tap shifted by a pixel,
  the norm not detached, g / n replaced by g, the row scale of the neighbouring sample -- by at least 10x its tolerance, and
  accepts the float64 reference rounded the way the kernel stores its output;
* the integer data of the exact comparisons keeps every partial sum below 2^24 (what makes torch.equal legitimate);
* the references themselves agree with independent statements of the same maths: torch.autograd through F.conv2d for the
  conv-tap gather, the oracle's DoRAModuleRef for DoRA."""
import pytest
import torch

import lora_kernel_refs as KR
from lora_kernel_refs import WJob

DT = [torch.float16, torch.bfloat16]
FAR = 10.0  # a mutant must miss the tolerance by this factor


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
def test_exact_cases_stay_below_2_pow_24(dt):
    jobs = [KR.build_wjob(s, dt, seed=100 + i) for name in KR.WGRAD_EXACT for i, s in enumerate(KR.WGRAD_EXACT[name])]
    jobs += [KR.build_wjob(WJob(M, K, r, seg_cols=seg, rps=rps, ldp=ldp, scaled=True, m_begin=mb), dt, seed=7)
             for (M, mb, rps, r, K, seg, ldp) in KR.WGRAD_TAIL]
    for j in jobs:
        assert KR.exact_headroom(j) < 2 ** 24, j["spec"]
        assert torch.equal(j["ref"][KR.GUARD:-KR.GUARD].double(), j["ref64"])  # the fp32 cast of the reference loses nothing
    for stride, ups, skip in KR.CONV_CASES:
        c = KR.build_conv_case(dt, stride, ups, skip)
        assert float(c["abs"].max()) / c["unit"] < 2 ** 24


@pytest.mark.parametrize("stride,ups", [(1, 0), (2, 0), (1, 1)])
def test_conv_tap_reference_matches_conv2d_autograd(stride, ups):
    """The explicit (n, oy, ox) -> input pixel arithmetic against the weight gradient of F.conv2d (pad 1) in float64; and a tap
    shifted by one pixel is not it."""
    c = KR.build_conv_case(torch.bfloat16, stride, ups, 0)
    n = KR.CONV_R * KR.CONV_K * 9
    mine = (c["ref"][KR.GUARD:KR.GUARD + n] - c["dW0"][KR.GUARD:KR.GUARD + n]).double().view(KR.CONV_R, KR.CONV_K, 3, 3)
    auto = KR.conv_filter_grad_autograd(c["img"], c["P"], c["rs"], c["rps"], KR.CONV_R, stride, ups, c["alpha"])
    assert torch.equal(mine, auto)  # integer data: exact in float64 either way
    assert (c["Hout"], c["Wout"]) == {(1, 0): (6, 10), (2, 0): (3, 5), (1, 1): (12, 20)}[(stride, ups)]
    shifted = auto.roll(1, dims=3)  # every tap one pixel to the right
    assert (mine != shifted).float().mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------
def _wgrad_mutants(job):
    s = job["spec"]
    X, Pm, rs = job["X"][:, :s.K], job["P"], job["rs"]
    dW0 = job["dW0"][KR.GUARD:-KR.GUARD].view(s.r, s.K)
    base = dict(alpha=s.alpha, r=s.r, seg_cols=s.seg_cols, row_scale=rs, rows_per_sample=job["rps"])
    keep = torch.ones(X.shape[0], dtype=torch.bool)
    keep[job["rps"] + 3] = False  # a row of the second sample (the scales are applied first: the later rows keep theirs)
    Ps = Pm * rs[torch.arange(X.shape[0]) // job["rps"]][:, None]
    out = {"row dropped": KR.wgrad_ref(X[keep], Ps[keep], dW0, s.alpha, s.r, s.seg_cols)}
    nseg = s.K // s.seg_cols
    perm = list(range(nseg))
    perm[0], perm[1] = 1, 0
    Pswap = torch.cat([Pm[:, p * s.r:(p + 1) * s.r] for p in perm], dim=1)
    out["segments swapped"] = KR.wgrad_ref(X, Pswap, dW0, **base)
    out["neighbour's row scale"] = KR.wgrad_ref(X, Pm, dW0, **{**base, "row_scale": rs.roll(1)})
    out["dW0 not accumulated"] = KR.wgrad_ref(X, Pm, torch.zeros_like(dW0), **base)
    return out


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("spec", KR.WGRAD_RANDOM, ids=lambda s: f"r{s.r}")
def test_wgrad_random_tolerance_separates(dt, spec):
    job = KR.build_wjob(spec, dt, seed=40 + spec.r, exact=False)
    bound = KR.wgrad_random_bound(job)
    assert KR.ratio_to_bound(job["ref64"].float(), job["ref64"], bound) <= 1.0  # the stored (fp32) reference is inside
    for what, mut in _wgrad_mutants(job).items():
        ratio = KR.ratio_to_bound(mut.reshape(-1), job["ref64"], bound)
        assert ratio >= FAR, f"{what}: only {ratio:.2f} x the tolerance"


# ---------------------------------------------------------------------------------------------------------------
def _swap_segments(t):
    t = t.clone()
    t[[0, 1]] = t[[1, 0]]
    return t


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("name", sorted(KR.DORA_FWD_TABLES))
def test_dora_forward_tolerance_separates(dt, name):
    _, _, ents = KR.build_dora_table(KR.DORA_FWD_TABLES[name], dt)
    for e in ents:
        s = e["site"]
        lscale = KR.DORA_MULT * s.scale
        W, down, up, g = e["W"], e["down"], e["up"], e["g"]
        V, n, dW = KR.dora_forward_ref(W, down, up, g, lscale)
        nb = KR.cnorm_bound(s) * n
        db = KR.dora_dw_bound(V, n, W, g, lscale, s.r, dt, dW)
        # cap: the float64 reference in the kernel's storage formats
        assert KR.ratio_to_bound(n.float(), n, nb) <= 1.0
        assert KR.ratio_to_bound(dW.to(dt), dW, db) <= 1.0, f"{s}: the rounded reference itself misses the tolerance"
        # mutants
        Wv = W.view(s.nseg, s.cs, s.K)
        keep = [o for o in range(s.cs) if o != 5]
        _, n_drop, _ = KR.dora_forward_ref(Wv[:, keep].reshape(-1, s.K), down, up[:, keep], g, lscale)
        mut_n = {"row dropped": n_drop}
        _, _, dW_g = KR.dora_forward_ref(W, down, up, g, lscale, n=torch.ones_like(n))
        mut_d = {"g / n replaced by g": dW_g,
                 "lscale without mult": KR.dora_forward_ref(W, down, up, g, s.scale)[2],
                 "rank r - 1": KR.dora_forward_ref(W, down[:, :-1], up[:, :, :-1], g, lscale)[2]}
        if s.nseg > 1:
            Vs, n_s, dW_s = KR.dora_forward_ref(W, _swap_segments(down), up, g, lscale)
            mut_n["segments swapped (down)"] = n_s
            mut_d["segments swapped (down)"] = dW_s
            mut_d["segments swapped (dora_scale)"] = KR.dora_forward_ref(W, down, up, _swap_segments(g), lscale)[2]
        for what, m in mut_n.items():
            ratio = KR.ratio_to_bound(m, n, nb)
            assert ratio >= FAR, f"cnorm {s} {what}: only {ratio:.2f} x the tolerance"
        for what, m in mut_d.items():
            ratio = KR.ratio_to_bound(m, dW, db)
            assert ratio >= FAR, f"dW {s} {what}: only {ratio:.2f} x the tolerance"


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("site", KR.DORA_GRAD_SITES, ids=lambda s: f"r{s.r}_seg{s.nseg}_K{s.K}_cs{s.cs}")
def test_dora_grads_tolerance_separates(dt, site):
    down_flat, up_flat, ents = KR.build_dora_table([site], dt, seed=9 + site.r)
    e = ents[0]
    W, down, up, g = e["W"], e["down"], e["up"], e["g"]
    gg = KR.gen(77)
    G = torch.randn(site.nseg * site.cs, site.K, generator=gg)
    pre_d = torch.randn(down_flat.numel(), generator=gg)
    pre_u = torch.randn(up_flat.numel(), generator=gg)
    alpha = 0.75
    ref = KR.dora_grads_ref(W, down, up, g, G, alpha)
    pres = (pre_d[e["off_down"]:e["off_down"] + ref[0].numel()].view_as(ref[0]),
            pre_u[e["off_up"]:e["off_up"] + ref[1].numel()].view_as(ref[1]),
            pre_u[e["off_dora"]:e["off_dora"] + ref[2].numel()].view_as(ref[2]))
    bounds = KR.dora_grads_bound(W, down, up, g, G, alpha, *pres)
    want = [p.double() + r for p, r in zip(pres, ref)]
    for w, b in zip(want, bounds):  # cap: the fp32 storage of the reference
        assert KR.ratio_to_bound(w.float(), w, b) <= 1.0

    def worst(mut):  # the output that shows the mutant best
        return max(KR.ratio_to_bound(p.double() + m, w, b) for p, m, w, b in zip(pres, mut, want, bounds))

    Gv = G.view(site.nseg, site.cs, site.K).clone()
    Gv[:, 5] = 0  # a dropped row contributes nothing
    mutants = {"n not detached": KR.dora_grads_ref(W, down, up, g, G, alpha, detach=False),
               "g / n replaced by g": KR.dora_grads_ref(W, down, up, g, G, alpha, use_gn=False),
               "row dropped": KR.dora_grads_ref(W, down, up, g, Gv.view_as(G), alpha),
               "not accumulated": [r - p.double() for p, r in zip(pres, ref)],
               "alpha_dev ignored": KR.dora_grads_ref(W, down, up, g, G, alpha * 0.5)}
    if site.nseg > 1:
        sw = KR.dora_grads_ref(W, _swap_segments(down), up, g, G, alpha)
        mutants["segments swapped (down)"] = sw
        Gs = _swap_segments(G.view(site.nseg, site.cs, site.K)).reshape_as(G)
        mutants["segments swapped (G)"] = KR.dora_grads_ref(W, down, up, g, Gs, alpha)
    for what, m in mutants.items():
        ratio = worst(m)
        assert ratio >= FAR, f"{site} {what}: only {ratio:.2f} x the tolerance"


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("N,seg,r", KR.GEMM_ROWS_CASES)
def test_gemm_rows_tolerance_separates(dt, N, seg, r):
    d = KR.build_gemm_rows(N, seg, r, dt)
    M, s = KR.GEMM_ROWS_M, KR.GEMM_ROWS_SCALE
    args = (d["a"], d["w"], d["bias"], d["res"])
    for row0 in KR.GEMM_ROWS_ROW0:
        ref = KR.gemm_rows_ref(*args, d["xa"], d["up"], r, s, row0, seg)
        assert KR.close_ratio(ref.to(dt), ref.float(), dt) <= 1.0  # cap: the stored reference passes close(mult=4)
        if row0 == M:
            continue
        mut = {"xa row of the neighbour": KR.gemm_rows_ref(*args, d["xa"].roll(1, dims=0), d["up"], r, s, row0, seg),
               "no delta": KR.gemm_rows_ref(*args, d["xa"], d["up"], r, 0.0, row0, seg)}
        if seg:
            nseg = N // seg
            xs = d["xa"].view(M, nseg, r)[:, [1, 0] + list(range(2, nseg))].reshape(M, nseg * r)
            mut["segments swapped"] = KR.gemm_rows_ref(*args, xs, d["up"], r, s, row0, seg)
        if row0 > 0:
            mut["all rows adapted"] = KR.gemm_rows_ref(*args, d["xa"], d["up"], r, s, 0, seg)
        for what, m in mut.items():
            ratio = KR.close_ratio(m, ref, dt)
            assert ratio >= FAR, f"row0={row0} {what}: only {ratio:.2f} x the tolerance"
        # the single-row comparison of the first adapted row catches an off-by-one in lora_row0
        off = KR.gemm_rows_ref(*args, d["xa"], d["up"], r, s, row0 + 1, seg)
        ratio = KR.close_ratio(off[row0:row0 + 1], ref[row0:row0 + 1], dt)
        assert ratio >= FAR, f"row0={row0} delta one row late: only {ratio:.2f} x the tolerance"


# ---------------------------------------------------------------------------------------------------------------
def test_dora_reference_matches_oracle_module():
    """dora_forward_ref / dora_grads_ref against oracle.slider_ref.DoRAModuleRef on one small Linear, in float64."""
    from oracle import slider_ref as R
    torch.manual_seed(0)
    lin = torch.nn.Linear(16, 12, bias=True).double()
    mod = R.DoRAModuleRef("t", lin, multiplier=1.5, lora_dim=4, alpha=2).double()
    mod.apply_to()
    with torch.no_grad():
        mod.lora_up.weight.copy_(torch.randn(12, 4, dtype=torch.float64) * 0.05)
        mod.dora_scale.mul_(1 + 0.1 * torch.randn(1, 16, dtype=torch.float64))
    x = torch.randn(7, 16, dtype=torch.float64)
    gy = torch.randn(7, 12, dtype=torch.float64)
    (lin.forward(x) * gy).sum().backward()  # lin.forward is the adapted forward after apply_to
    lscale = mod.scale * mod.multiplier
    W, down, up, g = lin.weight.detach(), mod.lora_down.weight.detach()[None], mod.lora_up.weight.detach()[None], mod.dora_scale.detach()
    G = gy.t() @ x  # d(loss) / d(dW) up to lscale
    rd, ru, rg = KR.dora_grads_ref(W, down, up, g, G, lscale)
    torch.testing.assert_close(rd[0], mod.lora_down.weight.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ru[0], mod.lora_up.weight.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(rg, mod.dora_scale.grad, rtol=1e-12, atol=1e-14)
    _, n, dW = KR.dora_forward_ref(W, down, up, g, lscale)
    y_ref = x @ W.t() + lin.bias.detach() + x @ dW.t()
    torch.testing.assert_close(y_ref, lin.forward(x).detach(), rtol=1e-12, atol=1e-14)
    # not detaching the norm is a different gradient: the reference would notice
    md = KR.dora_grads_ref(W, down, up, g, G, lscale, detach=False)[0]
    assert (md - rd).abs().max() > 1e-3 * rd.abs().max()


def test_grad_scale_inputs_cover_the_edges():
    x, maxima = KR.build_grad_scale_input()
    amax = x.abs().amax(dim=1)
    assert torch.equal(amax, torch.tensor(maxima).float())
    assert amax[1] == 0 and x[2].abs().argmax() == x.shape[1] - 1
    import math
    exps = [math.frexp(float(a))[1] for a in amax if a > 0]
    assert max(exps) - min(exps) >= 40  # many binades
    mant = [math.frexp(float(a))[0] for a in amax if a > 0]
    assert 0.5 in mant and min(m for m in mant if m > 0.5) == 0.5 + 2.0 ** -24 and max(mant) == 1 - 2.0 ** -24
