"""The backward kernels of the MMDiT ops -- adaln_modulate_bwd, gate_residual_bwd (csrc/mmdit.hip) and the tanh-GELU backward
(launch_act_bwd kind 2) -- one launch at a time on a real MI355X through their thin C entries, against the float64 references
of tests/mmdit_bwd_refs.py: every element within SLACK * E; outputs NaN-prefilled with NaN guard rows on both sides that
must stay untouched.  Pack and split are each other's backward: packed, then split, the bits return.  The largest ratio to the
bound is printed per case."""
import ctypes as C

import pytest
import torch

import mmdit_bwd_refs as B
import mmdit_refs as R
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


def rn(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def within(got, ref, E, what):
    r = R.worst(got.cpu(), ref, E)
    print(f"{what}: {r:.3f} E")
    assert r <= R.SLACK, f"{what}: {r:.3f} E"


def mod_inputs(C_, dt, seed):
    """mod [3, ldm] wider than 3 C with the chunks at non-zero offsets that are multiples of 8; values of order 0.1 to 1."""
    ldm = 3 * C_ + 40
    return rn(seed, 3, ldm, scale=0.5).to(dt), ldm, (8, C_ + 16, 2 * C_ + 32)


# m = 7 rows: a partial last workgroup (4 rows each); rows_per_sample 3 or 4: the sample changes inside a workgroup
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rps", (3, 4))
@pytest.mark.parametrize("C_", (64, 128, 1536, 2048))
def test_adaln_modulate_bwd(lib, dt, C_, rps):
    M = 7
    # rows cycle through |mean| / std = 0, 4, 16
    off = torch.tensor([0.0, 4.0, 16.0])[torch.arange(M) % 3][:, None] * 0.25
    x = (rn(100 + C_ + rps, M, C_, scale=0.25) + off).to(dt)
    dy = rn(101 + C_ + rps, M, C_).to(dt)
    add = rn(102 + C_ + rps, M, C_).to(dt)
    mod, ldm, (_g, o_scale, o_shift) = mod_inputs(C_, dt, 200 + C_)
    xg, dyg, mg, ag = x.cuda(), dy.cuda(), mod.cuda(), add.cuda()  # (named: a device operand must outlive its launch)
    y = torch.empty(M, C_, dtype=dt, device="cuda")
    st = torch.empty(M, 2, dtype=torch.float32, device="cuda")
    done(lib, lib.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(y), P(st), M, C_, rps, ldm, o_scale, o_shift, 1e-6, None))

    def launch(add_t, dx_t):
        done(lib, lib.smi_op_adaln_modulate_bwd(code(dt), P(xg), P(dyg), P(mg), P(st), P(add_t), P(dx_t), M, C_, rps, ldm,
                                                o_scale, None))

    plain = Guarded(M, C_, dt, "cuda")
    launch(None, plain.view)
    ref = B.adaln_bwd_ref(x, dy, mod, rps, o_scale, 1e-6)
    within(plain.view, ref["dx"], B.adaln_bwd_bound(ref, dt), f"adaln_modulate_bwd C={C_} rps={rps}")
    assert plain.guards_intact()
    summed = Guarded(M, C_, dt, "cuda")
    launch(ag, summed.view)
    ref_a = B.adaln_bwd_ref(x, dy, mod, rps, o_scale, 1e-6, add=add)
    within(summed.view, ref_a["dx"], B.adaln_bwd_bound(ref_a, dt), f"adaln_modulate_bwd C={C_} rps={rps} + add")
    assert summed.guards_intact()
    inplace = Guarded(M, C_, dt, "cuda")  # add aliasing dx: the same bits
    inplace.view.copy_(add)
    launch(inplace.view, inplace.view)
    assert torch.equal(inplace.view, summed.view) and inplace.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("M,C_,rps", [(7, 64, 3), (5, 1536, 2)])
def test_gate_residual_bwd(lib, dt, M, C_, rps):
    dy = rn(300 + C_, M, C_).to(dt)
    mod, ldm, (o_gate, _s, _t) = mod_inputs(C_, dt, 400 + C_)
    assert o_gate != 0
    dyg, mg = dy.cuda(), mod.cuda()
    out = Guarded(M, C_, dt, "cuda")
    done(lib, lib.smi_op_gate_residual_bwd(code(dt), P(dyg), P(mg), P(out.view), M, C_, rps, ldm, o_gate, None))
    ref = B.gate_bwd_ref(dy, mod, rps, o_gate)
    within(out.view, ref, B.gate_bwd_bound(ref, dt), f"gate_residual_bwd {M} x {C_}")
    assert out.guards_intact()


def _act_x(n):
    """n values over [-12, 12] that hold +-0, +-6 and +-12 exactly where n allows."""
    special = torch.tensor([0.0, -0.0, 6.0, -6.0, 12.0, -12.0, -0.75], dtype=torch.float64)
    if n <= special.numel():
        return special[:n] if n > 1 else torch.tensor([-12.0], dtype=torch.float64)
    return torch.cat([special, torch.linspace(-12, 12, n - special.numel(), dtype=torch.float64)])


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("n", (1, 7, 8, 4099))
def test_gelu_tanh_bwd(lib, dt, n):
    x = _act_x(n).to(dt)
    dy = rn(700 + n, n).to(dt)
    xg, dyg = x.cuda(), dy.cuda()
    out = Guarded(1, n, dt, "cuda", g=8)  # (8 guard rows of n elements: the view stays 16-byte aligned for every n)
    done(lib, lib.smi_op_act(code(dt), P(xg), None, P(dyg), P(out.view), n, 2, None))
    ref = B.gelu_tanh_bwd_ref(x, dy)
    within(out.view[0], ref, B.gelu_tanh_bwd_bound(x, dy, dt), f"act kind 2 backward n={n}")
    assert out.guards_intact()
    assert torch.isfinite(out.view).all()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gelu_tanh_forward_bits_are_the_frozen_ones(lib, dt):
    """The forward of kind 2 through the entry that now also takes dy: alone and together with a backward, the same bits, and
    those within the forward's bound."""
    x = torch.cat([rn(701, 4096, scale=2.0), torch.linspace(-12, 12, 4096, dtype=torch.float64)]).to(dt)
    dy = rn(702, x.numel()).to(dt)
    xg, dyg = x.cuda(), dy.cuda()
    y0 = Guarded(1, x.numel(), dt, "cuda")
    done(lib, lib.smi_op_act(code(dt), P(xg), P(y0.view), None, None, x.numel(), 2, None))
    y1, dx = Guarded(1, x.numel(), dt, "cuda"), Guarded(1, x.numel(), dt, "cuda")
    done(lib, lib.smi_op_act(code(dt), P(xg), P(y1.view), P(dyg), P(dx.view), x.numel(), 2, None))
    assert torch.equal(y0.view, y1.view) and y1.guards_intact() and dx.guards_intact()
    ref = R.gelu_tanh(x.double())
    within(y0.view[0], ref, R.gelu_tanh_bound(x, ref, dt), "act kind 2 forward")
    within(dx.view[0], B.gelu_tanh_bwd_ref(x, dy), B.gelu_tanh_bwd_bound(x, dy, dt), "act kind 2 backward, same call")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("Nx,Nc", [(12, 5), (64, 13)])
def test_pack_then_split_returns_the_bits(lib, dt, Nx, Nc):
    """The backward of a split is a pack and the reverse; the last block's split, which drops the context rows, has a pack
    whose b rows are zero."""
    n, W = 3, 24
    a, b = rn(500 + Nx, n * Nx, W).to(dt).cuda(), rn(501 + Nc, n * Nc, W).to(dt).cuda()
    j = Guarded(n * (Nx + Nc), W, dt, "cuda")
    done(lib, lib.smi_op_joint_rows_pack(code(dt), P(a), P(b), P(j.view), n, Nx, Nc, W, None))
    a2, b2 = Guarded(n * Nx, W, dt, "cuda"), Guarded(n * Nc, W, dt, "cuda")
    done(lib, lib.smi_op_joint_rows_split(code(dt), P(j.view), P(a2.view), P(b2.view), n, Nx, Nc, W, None))
    assert torch.equal(a2.view, a) and torch.equal(b2.view, b) and a2.guards_intact() and b2.guards_intact()
    z = torch.zeros_like(b)
    jz = Guarded(n * (Nx + Nc), W, dt, "cuda")
    done(lib, lib.smi_op_joint_rows_pack(code(dt), P(a), P(z), P(jz.view), n, Nx, Nc, W, None))
    rows = jz.view.reshape(n, Nx + Nc, W)
    assert torch.equal(rows[:, :Nx].reshape(-1, W), a) and not rows[:, Nx:].any() and jz.guards_intact()
