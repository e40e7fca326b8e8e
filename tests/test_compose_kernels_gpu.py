"""The kernels of slider composition one by one, through their C entry points: smi_lora_stack against the plain-torch layout
of tests/compose_refs.py, the column-multiplier form of the skinny product against the plain form times the table, and the
separate column-scaling launch.  Everything is bitwise unless a tolerance is written at the assert: the stack kernel copies and
does ONE fp32 multiply, the column form does ONE fp32 multiply after the fixed-order reduction."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import compose_refs as CR

from sliders_conceptmod_amd import _native

DT = [torch.float16, torch.bfloat16]
SENTINEL = 7.25


def P(t):
    return _native.ptr(t)


def run_stack(sites):
    """sites: [(row_len, n_out, [(r_k, down_k or None, up_k or None, coef_k)], lead_down, lead_up)] with CPU tensors; lead_*:
    floats of padding in front of the site's stacked matrices (moves their alignment).  Returns [(down, up)] per site as
    the kernel wrote them into sentinel-filled buffers, after checking that the sentinels around them are intact."""
    keep, jobs_py, outs = [], [], []
    for row_len, n_out, blocks, lead_d, lead_u in sites:
        R = sum(b[0] for b in blocks)
        dst_d = torch.full((lead_d + R * row_len + 8,), SENTINEL, device="cuda")
        dst_u = torch.full((lead_u + n_out * R + 8,), SENTINEL, device="cuda")
        outs.append((dst_d, dst_u, lead_d, lead_u, R, row_len, n_out))
        c0 = 0
        for r, d, u, coef in blocks:
            sd = su = None
            if d is not None:
                sd, su = d.float().contiguous().cuda(), u.float().contiguous().cuda()
                keep += [sd, su]
            jobs_py.append((sd, su, dst_d, dst_u, lead_d, lead_u, row_len, r, c0, R, n_out, coef))
            c0 += r
    jobs = (_native.LoraStackJobC * len(jobs_py))()
    for j, (sd, su, dd, du, ld_, lu_, row_len, r, c0, R, n_out, coef) in zip(jobs, jobs_py):
        j.src_down = None if sd is None else sd.data_ptr()
        j.src_up = None if su is None else su.data_ptr()
        j.dst_down, j.dst_up = dd.data_ptr() + 4 * ld_, du.data_ptr() + 4 * lu_
        j.row_len, j.r, j.c0, j.R, j.n_out, j.coef = row_len, r, c0, R, n_out, coef
    jobs_dev = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    _native.check(_native.lib().smi_lora_stack(jobs, len(jobs), P(jobs_dev), None), "smi_lora_stack")
    torch.cuda.synchronize()
    got = []
    for dst_d, dst_u, lead_d, lead_u, R, row_len, n_out in outs:
        d = dst_d[lead_d:lead_d + R * row_len].view(R, row_len).cpu()
        u = dst_u[lead_u:lead_u + n_out * R].view(n_out, R).cpu()
        # nothing outside the site's matrices is touched
        assert (dst_d[:lead_d] == SENTINEL).all() and (dst_d[lead_d + R * row_len:] == SENTINEL).all()
        assert (dst_u[:lead_u] == SENTINEL).all() and (dst_u[lead_u + n_out * R:] == SENTINEL).all()
        got.append((d, u))
    return got


def blocks_of(g, row_len, n_out, spec):
    """spec: [(rank, present, coef)] -> blocks with random fp32 operands."""
    out = []
    for r, present, coef in spec:
        if present:
            out.append((r, torch.randn(r, row_len, generator=g), torch.randn(n_out, r, generator=g), coef))
        else:
            out.append((r, None, None, coef))
    return out


STACK_CASES = {
    # ranks (4, 8): every access 16 bytes wide
    "ranks_4_8": [(64, 128, [(4, True, 0.25), (8, True, 0.5)], 0, 0)],
    # ranks (4, 4, 4), the middle slider absent at the second site: its block must be WRITTEN as zeros over the sentinel
    "ranks_4_4_4_middle_absent": [(64, 64, [(4, True, 0.25), (4, True, 1.0), (4, True, -0.75)], 0, 0),
                                  (128, 64, [(4, True, 0.25), (4, False, 1.0), (4, True, -0.75)], 0, 0)],
    # 3x3 conv sites (rows of Cin * 9 floats) with ranks clamped to 3: odd ranks, odd column offsets, R = 7: the scalar paths
    "conv_clamped_rank_3": [(3 * 9, 3, [(3, True, 1.0 / 3.0), (3, False, 2.0), (1, True, 4.0)], 0, 0),
                            (64 * 9, 96, [(3, True, 1.0 / 3.0), (4, True, 0.7)], 0, 0)],
    # offsets that are no multiple of 16 bytes: the scalar path for both matrices although every rank is a multiple of 4
    "misaligned_offsets": [(64, 128, [(4, True, 0.3), (8, True, -1.1)], 1, 3),
                           (40, 24, [(4, False, 0.3), (8, True, -1.1)], 2, 1)],
}


@pytest.mark.parametrize("case", list(STACK_CASES))
def test_lora_stack_matches_reference_bitwise(case):
    g = torch.Generator().manual_seed(11)
    sites = [(row_len, n_out, blocks_of(g, row_len, n_out, spec), ld_, lu_)
             for row_len, n_out, spec, ld_, lu_ in STACK_CASES[case]]
    got = run_stack(sites)
    for (row_len, n_out, blocks, _ld, _lu), (d, u) in zip(sites, got):
        ranks = [b[0] for b in blocks]
        coefs = [float(torch.tensor(b[3], dtype=torch.float32)) for b in blocks]
        want_d, want_u = CR.stack_site_reference([b[1] for b in blocks], [b[2] for b in blocks], ranks, coefs, row_len, n_out)
        assert torch.equal(d, want_d), f"{case}: stacked lora_down"
        assert torch.equal(u, want_u), f"{case}: stacked lora_up"
        assert not (d == SENTINEL).any() and not (u == SENTINEL).any()
        c = 0
        for r, dn, _up, _coef in blocks:
            if dn is None:
                assert not d[c:c + r].any() and not u[:, c:c + r].any(), "an absent slider's block must be written as zeros"
            c += r


def test_lora_stack_refuses_bad_jobs():
    jobs = (_native.LoraStackJobC * 1)()
    dst = torch.zeros(64, device="cuda")
    j = jobs[0]
    j.dst_down, j.dst_up, j.row_len, j.r, j.c0, j.R, j.n_out, j.coef = dst.data_ptr(), dst.data_ptr(), 4, 4, 2, 4, 4, 1.0
    dev = torch.empty(C.sizeof(jobs), dtype=torch.uint8, device="cuda")
    with pytest.raises(_native.SmiError, match="lora_stack"):  # columns [2, 6) of a rank-4 stack
        _native.check(_native.lib().smi_lora_stack(jobs, 1, P(dev), None), "smi_lora_stack")
    assert not dst.any()


def rnd(*shape, dt, scale=1.0, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dt)


def dcode(dt):
    return _native.DTYPE_CODE[dt]


# (M, K, R, rows_per_mul, period)
SKINNY_CASES = [
    (40, 128, 16, 20, 12),    # a sample boundary inside a 16-row workgroup, a partial last workgroup, period < R
    (7, 384, 32, 7, 8),       # three fused segments of 8 + padding columns; the generic k-step instantiation
    (64, 640, 16, 32, 16),    # the 5-step instantiation
    (64, 1280, 32, 16, 24),   # the 10-step instantiation; period 24: the second fragment wraps inside a lane's four columns
]


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("M,K,R,rpm,period", SKINNY_CASES)
def test_lora_skinny_cols_is_plain_product_times_table(dt, M, K, R, rpm, period):
    lib = _native.lib()
    x, s = rnd(M, K, dt=dt, seed=1), rnd(R, K, dt=dt, scale=K ** -0.5, seed=2)
    n_samp = (M + rpm - 1) // rpm
    ld_mul = period + 3  # a row stride larger than the period
    table = torch.randn(n_samp, ld_mul, generator=torch.Generator().manual_seed(5)).cuda()
    plain = torch.full((M, R), 9.0, device="cuda")
    _native.check(lib.smi_op_lora_skinny(dcode(dt), P(x), P(s), P(plain), M, R, K, None), "smi_op_lora_skinny")
    # the plain form is what it was: fp32 accumulate and output (tests/test_kernels_gpu.py::test_lora_skinny_product)
    torch.testing.assert_close(plain, x.float() @ s.float().t(), rtol=2e-5, atol=2e-5)
    out = torch.full((M, R), 9.0, device="cuda")
    _native.check(lib.smi_op_lora_skinny_cols(dcode(dt), P(x), P(s), P(out), M, R, K, P(table), ld_mul, period, rpm, None),
                  "smi_op_lora_skinny_cols")
    want = CR.col_mul_reference(plain, table[:, :period], rpm, period)
    assert torch.equal(out, want)
    assert (out != plain).any()
    out2 = torch.empty_like(out)
    _native.check(lib.smi_op_lora_skinny_cols(dcode(dt), P(x), P(s), P(out2), M, R, K, P(table), ld_mul, period, rpm, None),
                  "smi_op_lora_skinny_cols")
    assert torch.equal(out, out2)
    # a table of ones is the plain form; a zero row switches a sample off exactly
    ones = torch.ones_like(table)
    ones[0] = 0.0
    _native.check(lib.smi_op_lora_skinny_cols(dcode(dt), P(x), P(s), P(out2), M, R, K, P(ones), ld_mul, period, rpm, None),
                  "smi_op_lora_skinny_cols")
    assert torch.equal(out2[min(rpm, M):], plain[min(rpm, M):]) and not out2[:rpm].any()


def test_lora_skinny_cols_refuses_unsupported_shapes():
    lib = _native.lib()
    x, s = rnd(8, 320, dt=torch.float16), rnd(16, 320, dt=torch.float16)  # K % 128 != 0: GEMM + col_scale in the engine
    out, table = torch.zeros(8, 16, device="cuda"), torch.ones(1, 16, device="cuda")
    with pytest.raises(_native.SmiError, match="unsupported layout"):
        _native.check(lib.smi_op_lora_skinny_cols(0, P(x), P(s), P(out), 8, 16, 320, P(table), 16, 16, 8, None), "cols")
    with pytest.raises(_native.SmiError, match="bad table"):
        _native.check(lib.smi_op_lora_skinny_cols(0, P(x), P(s), P(out), 8, 16, 320, P(table), 16, 0, 8, None), "cols")


def test_col_scale_f32_matches_torch_bitwise():
    lib = _native.lib()
    M, N, ld, period, rpm = 70, 48, 48, 12, 35
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, ld, generator=g).cuda()
    table = torch.randn(2, period, generator=g).cuda()
    want = CR.col_mul_reference(x, table, rpm, period)
    got = x.clone()
    _native.check(lib.smi_op_col_scale_f32(P(got), ld, M, N, P(table), period, period, rpm, None), "smi_op_col_scale_f32")
    assert torch.equal(got, want)
    # a row stride wider than the scaled columns: the tail of every row stays
    wide = torch.randn(M, 56, generator=g).cuda()
    got = wide.clone()
    _native.check(lib.smi_op_col_scale_f32(P(got), 56, M, N, P(table), period, period, rpm, None), "smi_op_col_scale_f32")
    assert torch.equal(got[:, :N], CR.col_mul_reference(wide[:, :N], table, rpm, period))
    assert torch.equal(got[:, N:], wide[:, N:])
