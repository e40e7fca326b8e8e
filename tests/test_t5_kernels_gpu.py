"""The T5 encoder's kernels (csrc/t5.hip and the BIAS form of attn_fwd_kernel), one launch at a time on a real MI355X through
their thin C entries (include/smi.h smi_op_rmsnorm, smi_op_gated_gelu_tanh, smi_op_t5_bias_table, smi_op_attention_bias_fwd),
against the float64 references of tests/t5_refs.py: every element within SLACK * E, bit-exact where no arithmetic happens;
outputs NaN-prefilled with NaN guard rows on both sides that must stay untouched.  The largest ratio to the bound is printed
per case."""
import ctypes as C

import pytest
import torch

import attention_refs as A
import t5_refs as R
from norm_refs import Guarded

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


def done(lib, rc):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, session stopped: {e}", returncode=3)
    m = lib.smi_last_error()
    assert rc == 0, m.decode() if m else "?"


def code(dt):
    return 0 if dt == torch.float16 else 1


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def within(got, ref, E, what):
    r = R.worst(got.cpu(), ref, E)
    print(f"{what}: {r:.3f} E")
    assert r <= R.SLACK, f"{what}: {r:.3f} E"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,C_", R.RMS_CASES, ids=[f"m{m}c{c}" for m, c in R.RMS_CASES])
def test_rmsnorm(lib, dt, M, C_):
    x, w = R.rms_inputs(M, C_, dt)
    ref = R.rms_ref(x, w, 1e-6)
    out = Guarded(M, C_, dt, "cuda")
    xg, wg = x.cuda(), w.cuda()
    done(lib, lib.smi_op_rmsnorm(code(dt), P(xg), P(wg), P(out.view), M, C_, 1e-6, None))
    within(out.view, ref, R.rms_bound(ref, C_, dt), f"rmsnorm M={M} C={C_}")
    assert out.guards_intact()


def test_rmsnorm_refusals(lib):
    x = torch.zeros(2, 8200, dtype=torch.bfloat16, device="cuda")
    for c in (12, 8200):
        assert lib.smi_op_rmsnorm(1, P(x), P(x), P(x), 2, c, 1e-6, None) != 0
        assert b"rmsnorm" in lib.smi_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,F", R.GG_CASES, ids=[f"m{m}f{f}" for m, f in R.GG_CASES])
def test_gated_gelu_tanh(lib, dt, M, F):
    proj = R.gg_inputs(M, F, dt)
    assert ((proj[:, :F] <= -1) & (proj[:, :F] >= -4)).float().mean() > 0.2  # the region that tells tanh from erf
    ref = R.gg_ref(proj)
    pg = proj.cuda()
    out = Guarded(M, F, dt, "cuda")
    done(lib, lib.smi_op_gated_gelu_tanh(code(dt), P(pg), P(out.view), M, F, None))
    within(out.view, ref, R.gg_bound(ref, dt), f"gated_gelu_tanh M={M} F={F}")
    assert out.guards_intact()
    # the gate half's GELU is smi_op_act kind 2 to the bit: a value half of ones
    ones = torch.cat([proj[:, :F], torch.ones(M, F, dtype=dt)], dim=1).cuda()
    a = Guarded(M, F, dt, "cuda")
    done(lib, lib.smi_op_gated_gelu_tanh(code(dt), P(ones), P(a.view), M, F, None))
    gate = proj[:, :F].contiguous().cuda()
    b = Guarded(M, F, dt, "cuda")
    done(lib, lib.smi_op_act(code(dt), P(gate), P(b.view), None, None, M * F, 2, None))
    assert torch.equal(a.view, b.view) and a.guards_intact() and b.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("H,L", R.TABLE_CASES, ids=[f"h{h}l{l}" for h, l in R.TABLE_CASES])
def test_t5_bias_table(lib, dt, H, L):
    from sliders_conceptmod_amd import _native
    nb, md = 32, 128
    w = (1.5 * torch.randn(nb, H, generator=torch.Generator().manual_seed(H + L))).to(dt)
    bk = _native.t5_relative_buckets(nb, md, L)
    assert bk == R.buckets(nb, md, L)
    out = Guarded(H, 2 * L - 1, torch.float32, "cuda")
    wg, bg = w.cuda(), torch.tensor(bk, dtype=torch.int32).cuda()
    done(lib, lib.smi_op_t5_bias_table(code(dt), P(wg), P(bg), P(out.view), H, L, nb, None))
    assert torch.equal(out.view.cpu().double(), R.bias_table(w, nb, md, L)) and out.guards_intact()


def run_attention(lib, dt, B, H, L, scale, q, k, v, table):
    """q | k | v as column blocks of one [B L, 3 H D] tensor; the output inside guard rows and with guard columns (ldo wider
    than H D); the table with no slack after its H (2 L - 1) floats, between two NaN regions of the same allocation."""
    D = R.ATTN_D
    qkv = torch.cat([t.reshape(B * L, H * D) for t in (q, k, v)], dim=1).cuda()
    ldo = H * D + 8
    out = Guarded(B * L, ldo, dt, "cuda")
    n_tab, pad = H * (2 * L - 1), 64
    buf = torch.full((pad + n_tab + pad,), float("nan"), dtype=torch.float32, device="cuda")
    buf[pad:pad + n_tab] = table.reshape(-1).cuda()
    tab = buf[pad:pad + n_tab]
    lse = torch.full((B * H * L + 4,), float("nan"), dtype=torch.float32, device="cuda")
    esz = 2
    base = qkv.data_ptr()
    rc = lib.smi_op_attention_bias_fwd(code(dt), C.c_void_p(base), C.c_void_p(base + H * D * esz),
                                       C.c_void_p(base + 2 * H * D * esz), P(out.view), P(lse[2:]), P(tab), 2 * L - 1, B, H, L, D,
                                       3 * H * D, 3 * H * D, 3 * H * D, ldo, scale, None)
    done(lib, rc)
    assert out.guards_intact() and torch.isnan(out.view[:, H * D:]).all(), "guard rows or columns were written"
    assert torch.isnan(lse[:2]).all() and torch.isnan(lse[-2:]).all()
    assert torch.isnan(buf[:pad]).all() and torch.isnan(buf[pad + n_tab:]).all()
    o = out.view[:, :H * D]
    assert not torch.isnan(o).any(), "a NaN of the table's guard regions reached the output"
    return o.reshape(B, L, H, D), lse[2:2 + B * H * L].reshape(B, H, L), qkv


ATTN_CASES = [(R.ATTN_B, R.ATTN_H, L) for L in R.ATTN_LENGTHS] + [R.ATTN_LONG]


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("B,H,L", ATTN_CASES, ids=[f"b{b}h{h}l{l}" for b, h, l in ATTN_CASES])
def test_attention_bias(lib, dt, B, H, L):
    q, k, v, table = R.attn_inputs(B, H, L, dt)
    scale = 1.0
    ref = R.attn_bias_ref(q, k, v, table, scale)
    o, lse, _ = run_attention(lib, dt, B, H, L, scale, q, k, v, table)
    E = R.attn_bias_bound(ref, q, k, v, scale, dt)
    r, at = A.worst(o.cpu(), ref["O"], E)
    print(f"attention_bias L={L}: {r:.3f} E at {at}")
    assert r <= A.SLACK
    err = float((lse.cpu().double() - ref["lse"]).abs().max())
    print(f"attention_bias L={L}: lse off by {err:.3g}")
    assert err <= 2e-3  # the absolute bar test_attention_kernels_gpu.py holds every forward's lse to


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("L", (3, 77, 130))
@pytest.mark.parametrize("scale", (1.0, 0.125))
def test_zero_table_is_plain_attention(lib, dt, L, scale):
    """A zero table gives the bits of smi_op_attention_ex_fwd with the tiled forward pinned (sel_xs = 0) at the same scale
    (1: T5's; 1/8: a power of two, so that scaling the scores before or inside the exponent's argument rounds alike)."""
    from sliders_conceptmod_amd import _native
    B, H, D = R.ATTN_B, R.ATTN_H, R.ATTN_D
    q, k, v, table = R.attn_inputs(B, H, L, dt)
    o, lse, qkv = run_attention(lib, dt, B, H, L, scale, q, k, v, torch.zeros_like(table))
    out = Guarded(B * L, H * D, dt, "cuda")
    lse2 = torch.empty(B * H * L, dtype=torch.float32, device="cuda")
    a = _native.AttnArgsC()
    base = qkv.data_ptr()
    a.q, a.k, a.v = base, base + H * D * 2, base + 2 * H * D * 2
    a.o, a.lse = out.view.data_ptr(), lse2.data_ptr()
    a.ldq = a.ldk = a.ldv = 3 * H * D
    a.ldo = H * D
    a.dtype, a.b, a.h, a.nq, a.nk, a.d = code(dt), B, H, L, L, D
    a.scale, a.causal, a.sel_xs, a.sel_fused = scale, 0, 0, -1
    ran = _native.AttnRanC()
    done(lib, lib.smi_op_attention_ex_fwd(C.byref(a), C.byref(ran)))
    assert ran.family[0] == A.FWD
    assert torch.equal(o.reshape(B * L, H * D), out.view) and torch.equal(lse.reshape(-1), lse2)


def test_attention_bias_refusals(lib):
    t = torch.zeros(64, 3 * 64, dtype=torch.bfloat16, device="cuda")
    tab = torch.zeros(4096 * 2, dtype=torch.float32, device="cuda")
    ld = 3 * 64
    call = lambda n, d, ldt, table=tab: lib.smi_op_attention_bias_fwd(1, P(t), P(t), P(t), P(t), None, P(table), ldt, 1, 1, n, d,
                                                                      ld, ld, ld, ld, 1.0, None)
    assert call(8, 32, 15) != 0 and b"head_dim 64" in lib.smi_last_error()
    assert call(4096, 64, 8191) != 0 and b"exceeds" in lib.smi_last_error()
    assert call(8, 64, 14) != 0 and b"2 L - 1" in lib.smi_last_error()
    assert call(8, 64, 15, None) != 0 and b"table is NULL" in lib.smi_last_error()
    torch.cuda.synchronize()
