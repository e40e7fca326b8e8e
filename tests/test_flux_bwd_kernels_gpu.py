"""The backward kernels the Flux trainer adds -- qk_norm_rope_bwd, gelu_tanh_cols_bwd, flux_unpack_bwd (csrc/flux.hip) and
adaln_modulate_bwd at Flux's width (csrc/mmdit.hip) -- one launch at a time on a real MI355X through their thin C entries,
against the float64 references of tests/flux_bwd_refs.py: every element within SLACK * E, bit-exact where no arithmetic
happens; outputs NaN-prefilled with NaN guard rows on both sides that must stay untouched.  The largest ratio to the bound is
printed per case."""
import ctypes as C
import os

import pytest
import torch

import flux_bwd_refs as B
import flux_refs as F
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


HEADS = [(2, 64, (16, 24, 24)), (3, 128, (16, 56, 56)), (1, 160, (32, 64, 64)), (2, 16, (4, 6, 6))]
# (tokens, offset, L): a stream's rows at the head of the joint sequence, in its middle up to the end, the whole sequence
TOKENS = [(5, 0, 17), (12, 5, 17), (17, 0, 17)]


def table_for(L, axes, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 64, (L, 3), generator=g)
    ids[:, 0] = 0
    ids[L - 1, 1] = ids[L - 1, 2] = 63
    cos, sin = F.rope_table(ids, axes, f32=True)
    return torch.cat([cos, sin], dim=1).float(), cos, sin


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("tokens,off,L", TOKENS)
@pytest.mark.parametrize("H,D,axes", HEADS, ids=[f"h{h}x{d}" for h, d, _ in HEADS])
def test_qk_norm_rope_bwd(lib, dt, H, D, axes, tokens, off, L):
    n = 2
    ld = 3 * H * D
    lds, ldd, ldx = ld + 8, ld + 16, ld  # three row strides; the source and the joint gradient sit inside wider rows
    # tokens cycle through |x| of order 1, 1e-3 (mean of squares ~ eps) and 60 (fp16's range in the squares' sum)
    mag = torch.tensor([1.0, 1e-3, 60.0])[torch.arange(tokens) % 3][None, :, None, None, None]
    x = (rn(10 + H + tokens, n, tokens, 3, H, D) * mag).to(dt)
    dj = rn(40 + D + tokens, n, L, 3, H, D).to(dt)  # the whole joint gradient: rows outside the stream's must not be read
    wq, wk = ((0.5 + torch.rand(D, generator=torch.Generator().manual_seed(s), dtype=torch.float64)).to(dt) for s in (11, 12))
    tab, cos, sin = table_for(L, axes, 20 + D)
    ref = B.qk_norm_rope_bwd_ref(x, dj[:, off:off + tokens], wq, wk, cos[off:off + tokens], sin[off:off + tokens])
    xg = torch.zeros(n * tokens, lds, dtype=dt, device="cuda")
    xg[:, :ld] = x.reshape(n * tokens, ld).cuda()
    dg = torch.full((n * L, ldd), float("nan"), dtype=dt, device="cuda")
    dg[:, :ld] = dj.reshape(n * L, ld).cuda()
    wqg, wkg, tg = wq.cuda(), wk.cuda(), tab.cuda()
    out = Guarded(n * tokens, ldx, dt, "cuda")
    done(lib, lib.smi_op_qk_norm_rope_bwd(code(dt), P(dg), ldd, P(xg), lds, P(out.view), ldx, P(wqg), P(wkg), P(tg), n, tokens, L,
                                          off, H, D, 1e-6, None))
    got = out.view.reshape(n, tokens, 3, H, D)
    within(got.reshape(-1, ld), ref["dx"].reshape(-1, ld), B.qk_norm_rope_bwd_bound(ref, dt).reshape(-1, ld),
           f"qk_norm_rope_bwd H={H} D={D} tokens={tokens} off={off}")
    assert torch.equal(got[:, :, 2].cpu(), dj[:, off:off + tokens, 2]), "dv is a copy"
    assert out.guards_intact()
    # one sample alone: the bits it has in the batch
    one = Guarded(tokens, ldx, dt, "cuda")
    done(lib, lib.smi_op_qk_norm_rope_bwd(code(dt), P(dg[L:]), ldd, P(xg[tokens:]), lds, P(one.view), ldx, P(wqg), P(wkg), P(tg),
                                          1, tokens, L, off, H, D, 1e-6, None))
    assert torch.equal(one.view, out.view[tokens:]) and one.guards_intact()


def test_qk_norm_rope_bwd_refusals(lib):
    t = torch.zeros(64, 3 * 24, dtype=torch.float16, device="cuda")
    o = torch.zeros(64, 3 * 24, dtype=torch.float16, device="cuda")
    w = torch.ones(24, dtype=torch.float16, device="cuda")
    tab = torch.zeros(64, 24, device="cuda")
    assert lib.smi_op_qk_norm_rope_bwd(0, P(t), 72, P(t), 72, P(o), 72, P(w), P(w), P(tab), 1, 64, 64, 0, 1, 24, 1e-6, None) != 0
    assert b"multiple of 16" in lib.smi_last_error()
    t2 = torch.zeros(8, 96, dtype=torch.float16, device="cuda")
    o2 = torch.zeros(8, 96, dtype=torch.float16, device="cuda")
    assert lib.smi_op_qk_norm_rope_bwd(0, P(t2), 96, P(t2), 96, P(o2), 96, P(w), P(w), P(tab), 1, 8, 8, 1, 1, 32, 1e-6, None) != 0
    assert b"outside the joint sequence" in lib.smi_last_error()
    assert lib.smi_op_qk_norm_rope_bwd(0, P(t2), 96, P(o2), 96, P(t2), 96, P(w), P(w), P(tab), 1, 8, 8, 0, 1, 32, 1e-6, None) != 0
    assert b"alias" in lib.smi_last_error()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gelu_tanh_cols_bwd(lib, dt):
    """The strided tanh-GELU backward: x inside rows of 80, dy inside rows of 96, dx dense (64); inputs hold +-0, +-6, +-12 and
    -0.75 (where act' cancels); the bits of launch_act_bwd kind 2 on dense copies."""
    M, Cc, ldx, ldy = 37, 64, 80, 96
    special = torch.tensor([0.0, -0.0, 6.0, -6.0, 12.0, -12.0, -0.75], dtype=torch.float64)
    x = torch.cat([special, torch.linspace(-12, 12, 249, dtype=torch.float64), rn(800, M * Cc - 256, scale=2.0)]).reshape(M, Cc).to(dt)
    dy = rn(801, M, Cc).to(dt)
    xw = torch.full((M, ldx), float("nan"), dtype=dt, device="cuda")
    dw = torch.full((M, ldy), float("nan"), dtype=dt, device="cuda")
    xw[:, 8:8 + Cc] = x.cuda()
    dw[:, 16:16 + Cc] = dy.cuda()
    out = Guarded(M, Cc, dt, "cuda")
    done(lib, lib.smi_op_gelu_tanh_cols_bwd(code(dt), P(xw[:, 8:]), ldx, P(dw[:, 16:]), ldy, P(out.view), Cc, M, Cc, None))
    within(out.view, B.gelu_tanh_bwd_ref(x, dy), B.gelu_tanh_bwd_bound(x, dy, dt), "gelu_tanh_cols_bwd")
    assert out.guards_intact() and torch.isfinite(out.view).all()
    xd, dd = x.cuda(), dy.cuda()
    dense = Guarded(M, Cc, dt, "cuda")
    done(lib, lib.smi_op_act(code(dt), P(xd), None, P(dd), P(dense.view), M * Cc, 2, None))
    assert torch.equal(dense.view, out.view), "not the bits of launch_act_bwd kind 2"
    # a strided destination: the other columns stay untouched
    wide = Guarded(M, ldx, dt, "cuda")
    done(lib, lib.smi_op_gelu_tanh_cols_bwd(code(dt), P(xw[:, 8:]), ldx, P(dw[:, 16:]), ldy, P(wide.view[:, 8:]), ldx, M, Cc, None))
    assert torch.equal(wide.view[:, 8:8 + Cc], out.view)
    assert torch.isnan(wide.view[:, :8]).all() and torch.isnan(wide.view[:, 8 + Cc:]).all() and wide.guards_intact()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("gh,gw", [(4, 3), (1, 1)])
def test_flux_unpack_bwd(lib, dt, gh, gw):
    n, Cc = 3, 16
    scales = [4.0, 0.5, 1024.0]
    d_out = rn(900 + gh, n, Cc, 2 * gh, 2 * gw).float()
    dg, sg = d_out.cuda(), torch.tensor(scales, device="cuda")
    rows = Guarded(n * gh * gw, Cc * 4, dt, "cuda")
    done(lib, lib.smi_op_flux_unpack_bwd(code(dt), P(dg), P(rows.view), n, Cc, gh, gw, 2, P(sg), None))
    ref = B.flux_unpack_bwd_ref(d_out, scales)
    within(rows.view, ref, B.flux_unpack_bwd_bound(ref, dt), f"flux_unpack_bwd {gh} x {gw}")
    assert torch.equal(rows.view.cpu(), ref.to(dt)) and rows.guards_intact()
    # the inverse of flux_unpack: unpacking the rows gives scale x d_out, rounded once
    img = Guarded(n * Cc * 2 * gh, 2 * gw, torch.float32, "cuda")
    done(lib, lib.smi_op_flux_unpack(code(dt), P(rows.view), P(img.view), n, Cc, gh, gw, 2, None))
    want = (d_out.double() * torch.tensor(scales, dtype=torch.float64)[:, None, None, None]).to(dt).float()
    assert torch.equal(img.view.cpu().reshape(n, Cc, 2 * gh, 2 * gw), want) and img.guards_intact()


def _adaln_case(C_, rps, dt, M=7):
    off = torch.tensor([0.0, 4.0, 16.0])[torch.arange(M) % 3][:, None] * 0.25
    x = (rn(100 + C_ + rps, M, C_, scale=0.25) + off).to(dt)
    dy = rn(101 + C_ + rps, M, C_).to(dt)
    add = rn(102 + C_ + rps, M, C_).to(dt)
    ldm = 3 * C_ + 40
    mod = rn(200 + C_, 3, ldm, scale=0.5).to(dt)
    return x, dy, add, mod, ldm, C_ + 16, 2 * C_ + 32


# m = 7 rows: a partial last workgroup (4 rows each); rows_per_sample 3: ragged, the sample changes inside a workgroup
@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("C_", (2560, 3072))
def test_adaln_modulate_bwd_flux_width(lib, dt, C_):
    M, rps = 7, 3
    x, dy, add, mod, ldm, o_scale, o_shift = _adaln_case(C_, rps, dt)
    xg, dyg, mg, ag = x.cuda(), dy.cuda(), mod.cuda(), add.cuda()
    y = torch.empty(M, C_, dtype=dt, device="cuda")
    st = torch.empty(M, 2, dtype=torch.float32, device="cuda")
    done(lib, lib.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(y), P(st), M, C_, rps, ldm, o_scale, o_shift, 1e-6, None))

    def launch(add_t, dx_t):
        done(lib, lib.smi_op_adaln_modulate_bwd(code(dt), P(xg), P(dyg), P(mg), P(st), P(add_t), P(dx_t), M, C_, rps, ldm,
                                                o_scale, None))

    plain = Guarded(M, C_, dt, "cuda")
    launch(None, plain.view)
    ref = B.adaln_bwd_ref(x, dy, mod, rps, o_scale, 1e-6)
    within(plain.view, ref["dx"], B.adaln_bwd_bound(ref, dt), f"adaln_modulate_bwd C={C_}")
    assert plain.guards_intact()
    summed = Guarded(M, C_, dt, "cuda")
    launch(ag, summed.view)
    ref_a = B.adaln_bwd_ref(x, dy, mod, rps, o_scale, 1e-6, add=add)
    within(summed.view, ref_a["dx"], B.adaln_bwd_bound(ref_a, dt), f"adaln_modulate_bwd C={C_} + add")
    assert summed.guards_intact()
    inplace = Guarded(M, C_, dt, "cuda")  # add aliasing dx: the same bits
    inplace.view.copy_(add)
    launch(inplace.view, inplace.view)
    assert torch.equal(inplace.view, summed.view) and inplace.guards_intact()


def test_adaln_modulate_bwd_refuses_wider(lib):
    x = torch.zeros(1, 3080, dtype=torch.float16, device="cuda")
    st = torch.zeros(1, 2, device="cuda")
    assert lib.smi_op_adaln_modulate_bwd(0, P(x), P(x), P(x), P(st), None, P(x), 1, 3080, 1, 3080, 0, None) != 0
    assert b"3072" in lib.smi_last_error()


PARENT_LIB_ENV = "SMI_PARENT_LIB"


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_adaln_modulate_bwd_2048_keeps_the_parent_bits(lib, dt):
    """C = 2048 runs the instantiation it always did: the bits of a build of the parent commit, loaded next to this tree's
    library from SMI_PARENT_LIB (a bare ctypes handle with the two symbols' signatures set).  Skipped where the variable is
    not set, as the forward's test is."""
    parent_path = os.environ.get(PARENT_LIB_ENV)
    if not parent_path:
        pytest.skip(f"{PARENT_LIB_ENV} does not name a build of the parent commit")
    from sliders_conceptmod_amd import _native
    parent = C.CDLL(parent_path)
    for sym in ("smi_op_adaln_modulate", "smi_op_adaln_modulate_bwd"):
        getattr(parent, sym).restype, getattr(parent, sym).argtypes = _native._SIGS[sym]
    C_, M, rps = 2048, 7, 3
    x, dy, add, mod, ldm, o_scale, o_shift = _adaln_case(C_, rps, dt)
    xg, dyg, mg, ag = x.cuda(), dy.cuda(), mod.cuda(), add.cuda()
    outs = []
    for which in (lib, parent):
        y = torch.empty(M, C_, dtype=dt, device="cuda")
        st = torch.empty(M, 2, dtype=torch.float32, device="cuda")
        rc = which.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(y), P(st), M, C_, rps, ldm, o_scale, o_shift, 1e-6, None)
        done(lib, 0)
        assert rc == 0
        plain, summed = Guarded(M, C_, dt, "cuda"), Guarded(M, C_, dt, "cuda")
        for add_t, dx in ((None, plain), (ag, summed)):
            rc = which.smi_op_adaln_modulate_bwd(code(dt), P(xg), P(dyg), P(mg), P(st), P(add_t), P(dx.view), M, C_, rps, ldm,
                                                 o_scale, None)
            done(lib, 0)
            assert rc == 0 and dx.guards_intact()
        outs.append((plain, summed))
    assert torch.equal(outs[0][0].view, outs[1][0].view), "C = 2048 changed its bits against the parent build"
    assert torch.equal(outs[0][1].view, outs[1][1].view), "C = 2048 (+ add) changed its bits against the parent build"
