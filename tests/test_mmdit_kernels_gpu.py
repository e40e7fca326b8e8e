"""The kernels of csrc/mmdit.hip and tanh-GELU (launch_act kind 2), one launch at a time on a real MI355X through their thin
C entries (include/smi.h smi_op_adaln_modulate ... smi_op_sd3_unpatchify), against the float64 references of
tests/mmdit_refs.py: every element within SLACK * E, bit-exact where no arithmetic happens; outputs NaN-prefilled with NaN
guard rows on both sides that must stay untouched.  The largest ratio to the bound is printed per case."""
import ctypes as C

import pytest
import torch

import mmdit_refs as R
from norm_refs import Guarded, stat_worst

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


def rn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def within(got, ref, E, what):
    r = R.worst(got.cpu(), ref, E)
    print(f"{what}: {r:.3f} E")
    assert r <= R.SLACK, f"{what}: {r:.3f} E"


CS = (64, 128, 200, 1536, 2048)
RPS = (1, 5, 333)


def mod_inputs(C_, dt, seed):
    """mod [3, ldm] wider than 3 C with the chunks at non-zero offsets that are multiples of 8; values of order 0.1 to 1."""
    ldm = 3 * C_ + 40
    return rn(seed, 3, ldm, scale=0.5).to(dt), ldm, (8, C_ + 16, 2 * C_ + 32)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rps", RPS)
@pytest.mark.parametrize("C_", CS)
def test_adaln_modulate(lib, dt, C_, rps):
    M = 3 * rps
    # rows cycle through |mean| / std = 0, 8, 256: the statistics must survive the cancellation
    off = torch.tensor([0.0, 8.0, 256.0])[torch.arange(M) % 3][:, None] * 0.25
    x = (rn(100 + C_ + rps, M, C_, scale=0.25) + off).to(dt)
    mod, ldm, (o_gate, o_scale, o_shift) = mod_inputs(C_, dt, 200 + C_)
    xg, mg = x.cuda(), mod.cuda()  # (named: a device operand must outlive its launch)
    out = Guarded(M, C_, dt, "cuda")
    st = Guarded(M, 2, torch.float32, "cuda", g=8)
    done(lib, lib.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(out.view), P(st.view), M, C_, rps, ldm,
                                        o_scale, o_shift, 1e-6, None))
    ref = R.adaln_ref(x, mod, rps, o_scale, o_shift, 1e-6)
    within(out.view, ref["y"], R.adaln_bound(ref, dt), f"adaln_modulate C={C_} rps={rps}")
    assert out.guards_intact() and st.guards_intact()
    er, em = stat_worst(st.view[:, 0].cpu(), st.view[:, 1].cpu(), ref)
    print(f"  statistics: rstd {er:.3f}, mean {em:.3f} of the bar")
    assert er <= 1.0 and em <= 1.0
    # without mean_rstd: the same bits
    out2 = Guarded(M, C_, dt, "cuda")
    done(lib, lib.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(out2.view), None, M, C_, rps, ldm, o_scale,
                                        o_shift, 1e-6, None))
    assert torch.equal(out.view, out2.view)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rps", RPS)
@pytest.mark.parametrize("C_", CS)
def test_gate_residual(lib, dt, C_, rps):
    M = 3 * rps
    h, f = rn(300 + C_ + rps, M, C_).to(dt), rn(301 + C_ + rps, M, C_).to(dt)
    mod, ldm, (o_gate, _s, _t) = mod_inputs(C_, dt, 400 + C_)
    ref, mag = R.gate_ref(h, f, mod, rps, o_gate)
    hg, fg, mg = h.cuda(), f.cuda(), mod.cuda()
    E = R.gate_bound(ref, mag, dt)
    out = Guarded(M, C_, dt, "cuda")
    done(lib, lib.smi_op_gate_residual(code(dt), P(hg), P(fg), P(mg), P(out.view), M, C_, rps, ldm, o_gate,
                                       None))
    within(out.view, ref, E, f"gate_residual C={C_} rps={rps}")
    assert out.guards_intact()
    # y aliasing h: the same bits
    inplace = Guarded(M, C_, dt, "cuda")
    inplace.view.copy_(h)
    done(lib, lib.smi_op_gate_residual(code(dt), P(inplace.view), P(fg), P(mg), P(inplace.view), M, C_, rps, ldm,
                                       o_gate, None))
    assert torch.equal(inplace.view, out.view) and inplace.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("Nx,Nc", [(12, 5), (64, 13), (1, 1)])
def test_joint_pack_split(lib, dt, Nx, Nc):
    n, W = 3, 24
    a, b = rn(500 + Nx, n * Nx, W).to(dt).cuda(), rn(501 + Nc, n * Nc, W).to(dt).cuda()
    j = Guarded(n * (Nx + Nc), W, dt, "cuda")
    done(lib, lib.smi_op_joint_rows_pack(code(dt), P(a), P(b), P(j.view), n, Nx, Nc, W, None))
    want = torch.cat([a.reshape(n, Nx, W), b.reshape(n, Nc, W)], dim=1).reshape(-1, W)
    assert torch.equal(j.view, want) and j.guards_intact()
    a2, b2 = Guarded(n * Nx, W, dt, "cuda"), Guarded(n * Nc, W, dt, "cuda")
    done(lib, lib.smi_op_joint_rows_split(code(dt), P(j.view), P(a2.view), P(b2.view), n, Nx, Nc, W, None))
    assert torch.equal(a2.view, a) and torch.equal(b2.view, b) and a2.guards_intact() and b2.guards_intact()
    a3 = Guarded(n * Nx, W, dt, "cuda")  # the context stream dropped
    done(lib, lib.smi_op_joint_rows_split(code(dt), P(j.view), P(a3.view), None, n, Nx, Nc, W, None))
    assert torch.equal(a3.view, a) and a3.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("S", [6, 4])  # a 3 x 4 grid under a 6 x 6 table (offsets 1 and 1) and a 4 x 4 one (0 and 0)
def test_patchify_add_pos_unpatchify(lib, dt, S):
    n, Cin, H, W, p, d = 2, 16, 6, 8, 2, 72
    gh, gw = H // p, W // p
    lat = rn(600, n, Cin, H, W).float()
    latg = lat.cuda()
    pm = Guarded(n * gh * gw, Cin * p * p, dt, "cuda")
    done(lib, lib.smi_op_sd3_patchify(code(dt), P(latg), P(pm.view), n, Cin, H, W, p, None))
    want = R.patchify(lat, p).reshape(-1, Cin * p * p).to(dt)  # one rounding of an fp32 value: exact in the reference too
    assert torch.equal(pm.view.cpu(), want) and pm.guards_intact()

    x, pos = rn(601, n * gh * gw, d).to(dt), rn(602 + S, S * S, d, scale=0.5).to(dt)
    win = R.pos_window(pos.double(), S, gh, gw)
    assert (S - gh) // 2 == (1 if S == 6 else 0) and (S - gw) // 2 == (1 if S == 6 else 0)
    xg, pg = x.cuda(), pos.cuda()
    ref = x.double().reshape(n, gh * gw, d) + win[None]
    mag = x.double().abs().reshape(n, gh * gw, d) + win.abs()[None]
    out = Guarded(n * gh * gw, d, dt, "cuda")
    done(lib, lib.smi_op_sd3_add_pos(code(dt), P(xg), P(pg), P(out.view), n, gh, gw, d, S, None))
    within(out.view, ref.reshape(-1, d), R.add_pos_bound(ref, mag, dt).reshape(-1, d), f"sd3_add_pos S={S}")
    assert out.guards_intact()

    Cout = 16
    rows = rn(603, n * gh * gw, p * p * Cout).to(dt)
    rg = rows.cuda()
    img = Guarded(n * Cout * H, W, torch.float32, "cuda")
    done(lib, lib.smi_op_sd3_unpatchify(code(dt), P(rg), P(img.view), n, Cout, gh, gw, p, None))
    want = R.unpatchify(rows.float(), n, Cout, gh, gw, p)
    assert torch.equal(img.view.cpu().reshape(n, Cout, H, W), want) and img.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gelu_tanh(lib, dt):
    x = torch.cat([rn(700, 4096, scale=2.0), torch.linspace(-12, 12, 4096, dtype=torch.float64)]).to(dt)
    out = Guarded(1, x.numel(), dt, "cuda")
    xg = x.cuda()
    done(lib, lib.smi_op_act(code(dt), P(xg), P(out.view), None, None, x.numel(), 2, None))
    ref = R.gelu_tanh(x.double())
    within(out.view[0], ref, R.gelu_tanh_bound(x, ref, dt), "act kind 2 (tanh-GELU)")
    assert out.guards_intact()
    # the erf form is another function: it leaves the bound
    assert R.worst(R.gelu_erf(x.double()).to(dt), ref, R.gelu_tanh_bound(x, ref, dt)) > R.SLACK
