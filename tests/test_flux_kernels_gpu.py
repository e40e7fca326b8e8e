"""The kernels of csrc/flux.hip and the wider rows of adaln_modulate, one launch at a time on a real MI355X through their thin
C entries (include/smi.h smi_op_qk_norm_rope, smi_op_gelu_tanh_cols, smi_op_flux_unpack, smi_op_adaln_modulate), against the
float64 references of tests/flux_refs.py and tests/mmdit_refs.py: every element within SLACK * E, bit-exact where no
arithmetic happens; outputs NaN-prefilled with NaN guard rows on both sides that must stay untouched.  The largest ratio to
the bound is printed per case."""
import ctypes as C
import os

import pytest
import torch

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


HEADS = [(2, 64, (16, 24, 24)), (3, 128, (16, 56, 56)), (1, 160, (32, 64, 64))]
TOKENS = [(1, 0), (13, 5), (70, 13)]


def table_for(L, off, axes, seed):
    """fp32 table [L, D] = cos | sin for L joint rows with ids in [0, 63]; row `off` sits at (row, column) = (63, 63)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 64, (L, 3), generator=g)
    ids[:, 0] = 0
    ids[off, 1] = ids[off, 2] = 63
    cos, sin = F.rope_table(ids, axes, f32=True)
    return torch.cat([cos, sin], dim=1).float(), cos, sin


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("tokens,off", TOKENS)
@pytest.mark.parametrize("H,D,axes", HEADS, ids=[f"h{h}x{d}" for h, d, _ in HEADS])
def test_qk_norm_rope(lib, dt, H, D, axes, tokens, off):
    n, L = 2, off + tokens + 3  # three rows of every sample after the stream's: they must stay untouched too
    ld = 3 * H * D
    # tokens cycle through |x| of order 1, 1e-3 (mean of squares ~ eps) and 60 (fp16's range in the squares' sum)
    mag = torch.tensor([1.0, 1e-3, 60.0])[torch.arange(tokens) % 3][None, :, None, None, None]
    x = (rn(10 + H + tokens, n, tokens, 3, H, D) * mag).to(dt)
    wq, wk = ((0.5 + torch.rand(D, generator=torch.Generator().manual_seed(s), dtype=torch.float64)).to(dt) for s in (11, 12))
    tab, cos, sin = table_for(L, off, axes, 20 + D)
    ref, rmag = F.qk_norm_rope_ref(x, wq, wk, cos[off:off + tokens], sin[off:off + tokens])
    xg, wqg, wkg, tg = x.reshape(n * tokens, ld).cuda(), wq.cuda(), wk.cuda(), tab.cuda()
    out = Guarded(n * L, ld, dt, "cuda")
    done(lib, lib.smi_op_qk_norm_rope(code(dt), P(xg), ld, P(out.view), ld, P(wqg), P(wkg), P(tg), n, tokens, L, off, H, D, 1e-6,
                                      None))
    got = out.view.reshape(n, L, 3, H, D)
    mine = got[:, off:off + tokens]
    within(mine.reshape(-1, ld), ref.reshape(-1, ld), F.qk_norm_rope_bound(ref, rmag, dt).reshape(-1, ld),
           f"qk_norm_rope H={H} D={D} tokens={tokens} off={off}")
    assert torch.equal(mine[:, :, 2].cpu(), x[:, :, 2]), "v is a copy"
    rest = torch.ones(L, dtype=torch.bool)
    rest[off:off + tokens] = False
    assert torch.isnan(got[:, rest]).all() and out.guards_intact(), "rows of the other stream were written"
    if off == 0:
        return
    # in place over a whole joint sequence == out of place, bit for bit (and v untouched)
    xj = (rn(30 + H, n, L, 3, H, D)).to(dt)
    tj = tab.cuda()
    a = Guarded(n * L, ld, dt, "cuda")
    xjg = xj.reshape(n * L, ld).cuda()
    done(lib, lib.smi_op_qk_norm_rope(code(dt), P(xjg), ld, P(a.view), ld, P(wqg), P(wkg), P(tj), n, L, L, 0, H, D, 1e-6, None))
    b = Guarded(n * L, ld, dt, "cuda")
    b.view.copy_(xjg)
    done(lib, lib.smi_op_qk_norm_rope(code(dt), P(b.view), ld, P(b.view), ld, P(wqg), P(wkg), P(tj), n, L, L, 0, H, D, 1e-6, None))
    assert torch.equal(a.view, b.view) and a.guards_intact() and b.guards_intact()


def test_qk_norm_rope_refusals(lib):
    t = torch.zeros(64, 3 * 24, dtype=torch.float16, device="cuda")
    w = torch.ones(24, dtype=torch.float16, device="cuda")
    tab = torch.zeros(64, 24, device="cuda")
    assert lib.smi_op_qk_norm_rope(0, P(t), 72, P(t), 72, P(w), P(w), P(tab), 1, 64, 64, 0, 1, 24, 1e-6, None) != 0
    assert b"multiple of 16" in lib.smi_last_error()
    t2 = torch.zeros(8, 96, dtype=torch.float16, device="cuda")
    assert lib.smi_op_qk_norm_rope(0, P(t2), 96, P(t), 96, P(w), P(w), P(tab), 1, 8, 8, 1, 1, 32, 1e-6, None) != 0
    assert b"outside the joint sequence" in lib.smi_last_error()


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rps", (1, 5))
@pytest.mark.parametrize("C_", (2048, 2056, 3072))
def test_adaln_modulate_wide_rows(lib, dt, C_, rps):
    """Rows wider than 2048 columns (Flux: d = 3072) under the bound of the narrower ones, and 2048 itself (whose bits
    against a build of the parent commit are the next test's)."""
    M = 3 * rps
    off = torch.tensor([0.0, 8.0, 256.0])[torch.arange(M) % 3][:, None] * 0.25
    x = (rn(100 + C_ + rps, M, C_, scale=0.25) + off).to(dt)
    ldm = 3 * C_ + 40
    mod = rn(200 + C_, 3, ldm, scale=0.5).to(dt)
    o_scale, o_shift = C_ + 16, 2 * C_ + 32
    xg, mg = x.cuda(), mod.cuda()
    out = Guarded(M, C_, dt, "cuda")
    st = Guarded(M, 2, torch.float32, "cuda", g=8)
    done(lib, lib.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(out.view), P(st.view), M, C_, rps, ldm, o_scale, o_shift, 1e-6,
                                        None))
    ref = R.adaln_ref(x, mod, rps, o_scale, o_shift, 1e-6)
    within(out.view, ref["y"], R.adaln_bound(ref, dt), f"adaln_modulate C={C_} rps={rps}")
    assert out.guards_intact() and st.guards_intact()


PARENT_LIB_ENV = "SMI_PARENT_LIB"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("rps", (1, 5))
def test_adaln_modulate_2048_keeps_the_parent_bits(lib, dt, rps):
    """C = 2048 runs the instantiation it always did: the bits of a build of the parent commit, loaded next to this tree's
    library from SMI_PARENT_LIB (a bare ctypes handle with the one symbol's signature set: a parent build lacks the Flux
    symbols, so it cannot be the package's own library, which SMI_LIB would make it).  Skipped where the variable is not set."""
    parent_path = os.environ.get(PARENT_LIB_ENV)
    if not parent_path:
        pytest.skip(f"{PARENT_LIB_ENV} does not name a build of the parent commit")
    from sliders_conceptmod_amd import _native
    parent = C.CDLL(parent_path)
    parent.smi_op_adaln_modulate.restype, parent.smi_op_adaln_modulate.argtypes = _native._SIGS["smi_op_adaln_modulate"]
    C_, M = 2048, 3 * rps
    off = torch.tensor([0.0, 8.0, 256.0])[torch.arange(M) % 3][:, None] * 0.25
    xg = (rn(100 + C_ + rps, M, C_, scale=0.25) + off).to(dt).cuda()
    ldm = 3 * C_ + 40
    mg = rn(200 + C_, 3, ldm, scale=0.5).to(dt).cuda()
    outs = []
    for which in (lib, parent):
        out, st = Guarded(M, C_, dt, "cuda"), Guarded(M, 2, torch.float32, "cuda", g=8)
        rc = which.smi_op_adaln_modulate(code(dt), P(xg), P(mg), P(out.view), P(st.view), M, C_, rps, ldm, C_ + 16, 2 * C_ + 32,
                                         1e-6, None)
        done(lib, 0)
        assert rc == 0 and out.guards_intact() and st.guards_intact()
        outs.append((out, st))
    assert torch.equal(outs[0][0].view, outs[1][0].view), "C = 2048 changed its bits against the parent build"
    assert torch.equal(outs[0][1].view, outs[1][1].view), "the saved statistics changed their bits"


def test_adaln_modulate_refuses_wider(lib):
    x = torch.zeros(1, 3080, dtype=torch.float16, device="cuda")
    assert lib.smi_op_adaln_modulate(0, P(x), P(x), P(x), None, 1, 3080, 1, 3080, 0, 0, 1e-6, None) != 0
    assert b"3072" in lib.smi_last_error()


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_pack_and_unpack_order(lib, dt):
    """The patch matrix is the pipeline's _pack_latents and flux_unpack its _unpack_latents, bit for bit (an odd grid: 3 x 5)."""
    n, Cc, H, W = 2, 16, 6, 10
    lat = rn(600, n, Cc, H, W).float()
    latg = lat.cuda()
    pm = Guarded(n * (H // 2) * (W // 2), Cc * 4, dt, "cuda")
    done(lib, lib.smi_op_sd3_patchify(code(dt), P(latg), P(pm.view), n, Cc, H, W, 2, None))
    want = lat.view(n, Cc, H // 2, 2, W // 2, 2).permute(0, 2, 4, 1, 3, 5).reshape(-1, Cc * 4).to(dt)
    assert torch.equal(pm.view.cpu(), want) and pm.guards_intact()
    rows = rn(601, n * (H // 2) * (W // 2), Cc * 4).to(dt)
    rg = rows.cuda()
    img = Guarded(n * Cc * H, W, torch.float32, "cuda")
    done(lib, lib.smi_op_flux_unpack(code(dt), P(rg), P(img.view), n, Cc, H // 2, W // 2, 2, None))
    want = rows.float().view(n, H // 2, W // 2, Cc, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(n, Cc, H, W)
    assert torch.equal(img.view.cpu().reshape(n, Cc, H, W), want) and img.guards_intact()
    sd3 = R.unpatchify(rows.float(), n, Cc, H // 2, W // 2, 2)  # SD3's (py, px, c) is another image
    assert not torch.equal(sd3, want)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_gelu_tanh_cols(lib, dt):
    """tanh-GELU on a column block of a wider matrix, in place: the bits of launch_act kind 2, the other columns untouched."""
    M, Cc, ld, c0 = 7, 40, 72, 16
    x = torch.cat([rn(700, M * Cc - 64, scale=2.0), torch.linspace(-12, 12, 64, dtype=torch.float64)]).reshape(M, Cc).to(dt)
    dense = Guarded(M, Cc, dt, "cuda")
    xg = x.cuda()
    done(lib, lib.smi_op_act(code(dt), P(xg), P(dense.view), None, None, x.numel(), 2, None))
    ref = R.gelu_tanh(x.double())
    within(dense.view, ref, R.gelu_tanh_bound(x, ref, dt), "act kind 2")
    wide = Guarded(M, ld, dt, "cuda")
    wide.view[:, c0:c0 + Cc] = xg
    blk = wide.view[:, c0:c0 + Cc]
    done(lib, lib.smi_op_gelu_tanh_cols(code(dt), P(blk), ld, P(blk), ld, M, Cc, None))
    assert torch.equal(blk, dense.view)
    assert torch.isnan(wide.view[:, :c0]).all() and torch.isnan(wide.view[:, c0 + Cc:]).all() and wide.guards_intact()
