"""The backward kernels of the T5 tower, one launch at a time on a real MI355X through their thin C entries (include/smi.h
smi_op_attention_bias_bwd, smi_op_rmsnorm_bwd, smi_op_gated_gelu_tanh_bwd), against the float64 references of
tests/t5_bwd_refs.py: every element within SLACK * E, bit-exact where another entry computes the same expression; outputs
NaN-prefilled with NaN guard rows (and, where the leading dimension is wider than the operand, guard columns) that must stay
untouched; the bias table between two NaN regions with no slack.  The largest ratio to the bound is printed per case."""
import ctypes as C
import functools

import pytest
import torch

import attention_refs as A
import t5_bwd_refs as B
from norm_refs import Guarded

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
NAN16 = A.NAN16


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
    r = B.worst(got.cpu(), ref, E)
    print(f"{what}: {r:.3f} E")
    assert r <= B.SLACK, f"{what}: {r:.3f} E"


# ---------------------------------------------------------------------------------------------------------------
# attention backward with the bias table
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attn_case(B_, H, L, dt, zero_table=False, scale=1.0):
    """Inputs, the float64 reference and its bounds, formed once per shape and shared (nothing below writes to them)."""
    q, k, v, table, d_o = B.attn_bwd_inputs(B_, H, L, dt)
    if zero_table:
        table = torch.zeros_like(table)
    ref = B.attn_bias_bwd_ref(q, k, v, table, d_o, scale)
    o16, lse32 = A.bwd_inputs(ref, dt)
    E = B.attn_bias_bwd_bounds(ref, q, k, v, d_o, scale, dt)
    return {"q": q, "k": k, "v": v, "table": table, "do": d_o, "o": o16, "lse": lse32, "ref": ref, "E": E}


def nan16(rows, cols, dt):
    return torch.full((rows * cols,), NAN16, dtype=torch.int16, device="cuda").view(dt).view(rows, cols)


class AttnRun:
    """One call of smi_op_attention_bias_bwd (or, table None, of smi_op_attention_ex_bwd) on a case.
    layout 'packed': q, k, v, o, dO, dQ, dK, dV each [B L, H D].
    layout 'fused':  q | k | v column blocks of one [B L, 3 H D] tensor, dQ | dK | dV of another; o and dO at a leading
                     dimension of H D + 8 (NaN in the extra columns).
    Gradients live between NaN guard rows; a gradient that is not asked for stays NaN everywhere."""

    def __init__(self, lib, case, dt, B_, H, L, layout, grads, fused, scale=1.0, biased=True, xs=-1):
        from sliders_conceptmod_amd import _native
        D, HD, rows, G = B.ATTN_D, H * B.ATTN_D, B_ * L, 2
        want_q, want_kv = "q" in grads.split("+"), "kv" in grads.split("+")
        flat = lambda t: t.reshape(rows, HD).cuda()
        if layout == "fused":
            self.src = torch.cat([flat(case[n]) for n in ("q", "k", "v")], dim=1)
            ld, offs = 3 * HD, (0, HD, 2 * HD)
            ldo = HD + 8
            self.grad = nan16(rows + 2 * G, 3 * HD, dt)
            gptr = [self.grad[G:, o:] for o in offs]
            qkv = [self.src[:, o:] for o in offs]
        else:
            self.src = [flat(case[n]) for n in ("q", "k", "v")]
            ld, ldo = HD, HD
            self.grad = [nan16(rows + 2 * G, HD, dt) for _ in range(3)]
            gptr = [g[G:] for g in self.grad]
            qkv = self.src
        self.o, self.do = nan16(rows, ldo, dt), nan16(rows, ldo, dt)
        self.o[:, :HD] = flat(case["o"])
        self.do[:, :HD] = flat(case["do"])
        n_tab, pad = H * (2 * L - 1), 64
        self.tab_buf = torch.full((pad + n_tab + pad,), float("nan"), dtype=torch.float32, device="cuda")
        self.tab_buf[pad:pad + n_tab] = case["table"].reshape(-1).cuda()
        self.lse = case["lse"].reshape(-1).cuda()
        self.delta = torch.full((B_ * H * L + 4,), float("nan"), dtype=torch.float32, device="cuda")
        a = _native.AttnArgsC()
        a.q, a.k, a.v = (t.data_ptr() for t in qkv)
        a.o, a.lse, a.d_o, a.delta = self.o.data_ptr(), self.lse.data_ptr(), self.do.data_ptr(), self.delta[2:].data_ptr()
        a.dq = gptr[0].data_ptr() if want_q else None
        a.dk = gptr[1].data_ptr() if want_kv else None
        a.dv = gptr[2].data_ptr() if want_kv else None
        a.ldq = a.ldk = a.ldv = a.lddq = a.lddk = a.lddv = ld
        a.ldo = a.lddo = ldo
        a.dtype, a.b, a.h, a.nq, a.nk, a.d = code(dt), B_, H, L, L, D
        a.scale, a.causal, a.sel_xs, a.sel_fused = scale, 0, xs, fused
        ran = _native.AttnRanC()
        if biased:
            rc = lib.smi_op_attention_bias_bwd(C.byref(a), P(self.tab_buf[pad:]), 2 * L - 1, C.byref(ran))
        else:
            rc = lib.smi_op_attention_ex_bwd(C.byref(a), C.byref(ran))
        done(lib, rc)
        self.families = list(ran.family[:ran.n_launches])
        assert torch.isnan(self.tab_buf[:pad]).all() and torch.isnan(self.tab_buf[pad + n_tab:]).all()
        assert torch.isnan(self.delta[:2]).all() and torch.isnan(self.delta[-2:]).all()
        # guard rows, and every gradient that was not asked for, still hold the NaN pattern
        bits = lambda t: t.contiguous().view(torch.int16)
        self.out = {}
        for i, (n, want) in enumerate((("dQ", want_q), ("dK", want_kv), ("dV", want_kv))):
            full = self.grad[:, i * HD:(i + 1) * HD] if layout == "fused" else self.grad[i]
            assert (bits(full[:G]) == NAN16).all() and (bits(full[G + rows:]) == NAN16).all(), f"{n}: guard rows written"
            body = full[G:G + rows]
            if want:
                assert not torch.isnan(body).any(), f"{n}: a NaN (of the table's guards, or of a padded row) reached the gradient"
                self.out[n] = body.reshape(B_, L, H, D)
            else:
                assert (bits(body) == NAN16).all(), f"{n} was written though not asked for"


MODES = (("q+kv", 1), ("q+kv", 0), ("q", -1), ("kv", -1))  # (gradient subset, sel_fused): every form bwd_bias can pick


def check_attention(lib, dt, B_, H, L, layout):
    case = attn_case(B_, H, L, dt)
    for grads, fused in MODES:
        run = AttnRun(lib, case, dt, B_, H, L, layout, grads, fused)
        assert run.families == B.expected_bias_path(L, B_, H, grads, fused), (grads, fused, run.families)
        for n, got in run.out.items():
            r, at = A.worst(got.cpu(), case["ref"][n], case["E"][n])
            print(f"attention_bias_bwd L={L} {layout} {grads} {[A.FAMILY_NAMES[f] for f in run.families]} {n}: {r:.3f} E at {at}")
            assert r <= A.SLACK, (grads, fused, n, r, at)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("layout", ("packed", "fused"))
@pytest.mark.parametrize("L", B.ATTN_BWD_LENGTHS)
def test_attention_bias_bwd(lib, dt, layout, L):
    check_attention(lib, dt, B.ATTN_B, B.ATTN_H, L, layout)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_attention_bias_bwd_long(lib, dt):
    check_attention(lib, dt, *B.ATTN_LONG, "fused")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("L", (3, 77, 130))
@pytest.mark.parametrize("scale", (1.0, 0.125))
def test_zero_table_is_plain_attention_bwd(lib, dt, L, scale):
    """A zero table gives the bits of smi_op_attention_ex_bwd with the same form pinned (the single-pass kernels off): the
    two tiled launches at every length, the one-launch form where the bias-free dispatcher offers it (more than 96 keys)."""
    B_, H = B.ATTN_B, B.ATTN_H
    case = attn_case(B_, H, L, dt, True, scale)
    for grads, fused in MODES:
        if fused == 1 and L <= A.XS_KEYS:
            continue
        got = AttnRun(lib, case, dt, B_, H, L, "fused", grads, fused, scale)
        plain = AttnRun(lib, case, dt, B_, H, L, "fused", grads, fused, scale, biased=False, xs=0)
        assert got.families == plain.families, (grads, fused, got.families, plain.families)
        for n in got.out:
            assert torch.equal(got.out[n], plain.out[n]), (grads, fused, n)


def test_attention_bias_bwd_refusals(lib):
    from sliders_conceptmod_amd import _native
    t = torch.zeros(64, 3 * 64, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(4096 * 2, dtype=torch.float32, device="cuda")
    a = _native.AttnArgsC()
    a.q = a.k = a.v = a.o = a.d_o = a.dq = a.dk = a.dv = t.data_ptr()
    a.lse = a.delta = f.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = 3 * 64
    a.dtype, a.b, a.h, a.nq, a.nk, a.d, a.scale, a.causal, a.sel_xs, a.sel_fused = 1, 1, 1, 8, 8, 64, 1.0, 0, -1, -1
    ran = _native.AttnRanC()
    call = lambda ld, table=f: lib.smi_op_attention_bias_bwd(C.byref(a), P(table), ld, C.byref(ran))
    assert call(15, None) != 0 and b"table is NULL" in lib.smi_last_error()
    assert call(14) != 0 and b"2 L - 1" in lib.smi_last_error() and ran.n_launches == 0
    a.d = 32
    assert call(15) != 0 and b"head_dim 64" in lib.smi_last_error()
    a.d, a.causal = 64, 1
    assert call(15) != 0 and b"no causal mask" in lib.smi_last_error()
    a.causal, a.nq, a.nk = 0, 4096, 4096
    assert call(8191) != 0 and b"exceeds" in lib.smi_last_error()
    a.nq = a.nk = 8
    a.dv = None
    a.dq = None  # the dK / dV-only form: refused before its delta launch is queued
    assert call(15) != 0 and b"dK and dV must both be given" in lib.smi_last_error() and ran.n_launches == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# rmsnorm_rows_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,C_", B.RMS_CASES, ids=[f"m{m}c{c}" for m, c in B.RMS_CASES])
def test_rmsnorm_bwd(lib, dt, M, C_):
    x, w, dy, add = B.rms_bwd_inputs(M, C_, dt)
    if dt == torch.bfloat16:
        assert float(x[-1].abs().max()) >= 2.9e4  # the row of magnitude 3e4
    xg, wg, dyg, addg = x.cuda(), w.cuda(), dy.cuda(), add.cuda()
    for a, ag in ((None, None), (add, addg)):
        ref = B.rms_bwd_ref(x, w, dy, a)
        out = Guarded(M, C_, dt, "cuda")
        done(lib, lib.smi_op_rmsnorm_bwd(code(dt), P(xg), P(dyg), P(wg), P(ag), P(out.view), M, C_, B.RMS_EPS, None))
        within(out.view, ref, B.rms_bwd_bound(x, w, dy, a, ref, C_, dt), f"rmsnorm_bwd M={M} C={C_} add={a is not None}")
        assert out.guards_intact()
    # add may be the output itself: the same bits
    inplace = Guarded(M, C_, dt, "cuda")
    inplace.view.copy_(addg)
    done(lib, lib.smi_op_rmsnorm_bwd(code(dt), P(xg), P(dyg), P(wg), P(inplace.view), P(inplace.view), M, C_, B.RMS_EPS, None))
    assert torch.equal(inplace.view, out.view) and inplace.guards_intact()


def test_rmsnorm_bwd_refusals(lib):
    x = torch.zeros(2, 8200, dtype=torch.bfloat16, device="cuda")
    for c in (12, 8200):
        assert lib.smi_op_rmsnorm_bwd(1, P(x), P(x), P(x), None, P(x), 2, c, 1e-6, None) != 0
        assert b"rmsnorm_bwd" in lib.smi_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# gated_gelu_tanh_bwd
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,F", B.GG_CASES, ids=[f"m{m}f{f}" for m, f in B.GG_CASES])
def test_gated_gelu_tanh_bwd(lib, dt, M, F):
    proj, dout = B.gg_bwd_inputs(M, F, dt)
    ref = B.gg_bwd_ref(proj, dout)
    pg, dg = proj.cuda(), dout.cuda()
    out = Guarded(M, 2 * F, dt, "cuda")
    done(lib, lib.smi_op_gated_gelu_tanh_bwd(code(dt), P(pg), P(dg), P(out.view), M, F, None))
    within(out.view, ref, B.gg_bwd_bound(proj, dout, ref, dt), f"gated_gelu_tanh_bwd M={M} F={F}")
    assert out.guards_intact()
    # with up = 1 the gate half is smi_op_act's backward, kind 2, to the bit
    ones = torch.cat([proj[:, :F], torch.ones(M, F, dtype=dt)], dim=1).cuda()
    a = Guarded(M, 2 * F, dt, "cuda")
    done(lib, lib.smi_op_gated_gelu_tanh_bwd(code(dt), P(ones), P(dg), P(a.view), M, F, None))
    gate = proj[:, :F].contiguous().cuda()
    b = Guarded(M, F, dt, "cuda")
    done(lib, lib.smi_op_act(code(dt), P(gate), None, P(dg), P(b.view), M * F, 2, None))
    assert torch.equal(a.view[:, :F], b.view) and a.guards_intact() and b.guards_intact()


def test_gated_gelu_tanh_bwd_refusals(lib):
    x = torch.zeros(2, 64, dtype=torch.bfloat16, device="cuda")
    assert lib.smi_op_gated_gelu_tanh_bwd(1, P(x), P(x), P(x), 2, 12, None) != 0
    assert b"gated_gelu_tanh_bwd" in lib.smi_last_error()
    torch.cuda.synchronize()
