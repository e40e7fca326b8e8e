"""The small kernels that only whole-engine runs reached, one launch at a time on a real MI355X through their thin C entries
(include/smi.h smi_op_pool2x2_sum ... smi_op_nchw_to_nhwc_scaled), against the float64 references of
tests/elementwise_refs.py: every element within SLACK * E, outputs NaN-prefilled with NaN guard rows on both sides that must
stay untouched.  test_elementwise_refs_cpu.py shows on the same inputs that a tail dropped, a wrong tap or a missing pad zero
leaves SLACK * E."""
import ctypes as C

import pytest
import torch

import elementwise_refs as R

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
    return C.c_void_p(t.data_ptr())


def within(out, ref, E, what):
    r = R.worst(out.view, ref.reshape(out.view.shape), E.reshape(out.view.shape))
    print(f"{what}: {r:.3f} E")
    assert r <= R.SLACK, f"{what}: {r:.3f} E"
    assert out.guards_intact(), f"{what}: a guard row was written"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("H,W,Cc", R.POOL_CASES)
def test_pool2x2_sum(lib, dt, H, W, Cc):
    du = R.pool_inputs(H, W, Cc, dt).cuda()
    out = R.Guarded(2 * H * W, Cc, dt, "cuda")
    done(lib, lib.smi_op_pool2x2_sum(code(dt), P(du), P(out.view), 2, H, W, Cc, None))
    ref, mag = R.pool_ref(du)
    within(out, ref, R.pool_bound(ref, mag, dt), f"pool2x2_sum {H}x{W}x{Cc}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("HW,Cc", R.COLSUM_CASES)
def test_colsum(lib, dt, HW, Cc):
    x = R.colsum_inputs(HW, Cc, dt).cuda()
    n = C.c_size_t()
    assert lib.smi_op_colsum_floats(2, Cc, C.byref(n)) == 0 and n.value == 2 * R.COLSUM_RS * Cc
    outs = []
    for _ in range(2):
        out = R.Guarded(2, Cc, dt, "cuda")
        scr = R.Guarded(n.value, 1, torch.float32, "cuda", g=64)
        done(lib, lib.smi_op_colsum(code(dt), P(x), P(out.view), P(scr.view), 2, HW, Cc, 0.375, None))
        ref, mag = R.colsum_ref(x, 0.375)
        within(out, ref, R.colsum_bound(ref, mag, HW, dt), f"colsum {HW}x{Cc}")
        assert scr.guards_intact()
        outs.append(out.view.clone())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), "colsum differs on repeat"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("dim", R.TIMESTEP_CASES)
def test_timestep_embed(lib, dt, dim):
    vals = torch.tensor(R.TIMESTEP_VALUES, device="cuda")
    out = R.Guarded(len(R.TIMESTEP_VALUES), dim, dt, "cuda")
    done(lib, lib.smi_op_timestep_embed(code(dt), P(vals), P(out.view), len(R.TIMESTEP_VALUES), dim, None))
    ref, a, arg = R.timestep_ref(vals, dim)
    within(out, ref, R.timestep_bound(ref, a, arg, dt), f"timestep_embed {dim}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("cols,scale", R.SOFTMAX_CASES)
def test_softmax_rows(lib, dt, cols, scale):
    S = R.softmax_inputs(cols, scale).cuda()
    out = R.Guarded(S.shape[0], cols, dt, "cuda")
    done(lib, lib.smi_op_softmax_rows(code(dt), P(S), P(out.view), S.shape[0], cols, scale, None))
    ref, s = R.softmax_ref(S, scale)
    E = R.softmax_bound(ref, s, dt)
    within(out, ref, E, f"softmax_rows {cols} scale {scale}")
    row_err = (out.view.double().sum(dim=1) - 1).abs()
    assert bool((row_err <= R.SLACK * E.sum(dim=1)).all()), f"row sums off by {float(row_err.max()):.3e}"


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("Cc,M", R.CHAN_MIX_CASES)
def test_chan_mix(lib, dt, Cc, M):
    x, W, b = (t.cuda() for t in R.chan_mix_inputs(Cc, M, dt))
    out = R.Guarded(M, Cc, torch.float32, "cuda")
    done(lib, lib.smi_op_chan_mix(code(dt), P(x), P(W), P(b), P(out.view), M, Cc, None))
    ref, mag = R.chan_mix_ref(x, W, b)
    within(out, ref, R.chan_mix_bound(ref, mag, Cc), f"chan_mix {M}x{Cc}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("H,W,cin,cout", R.CONV_CASES)
def test_conv3x3_small(lib, dt, H, W, cin, cout):
    """conv_in (4 -> C) and conv_out (C -> 4) forms, 16-bit and fp32 output, and the gradient use: the same kernel on dy with the
    flipped, transposed filter gives d(in)."""
    x, w, bias = (t.cuda() for t in R.conv_inputs(H, W, cin, cout, dt))
    ref, mag = R.conv_ref(x, w, bias)
    for odt in (dt, torch.float32):
        out = R.Guarded(2 * H * W, cout, odt, "cuda")
        done(lib, lib.smi_op_conv3x3_small(code(dt), P(x), P(w), P(bias), P(out.view), int(odt == torch.float32), 2, H, W, cin, cout, None))
        within(out, ref, R.conv_bound(ref, mag, cin, odt), f"conv3x3_small {H}x{W} {cin}->{cout} {odt}")
    dy = R._rn(7 + H + W, 2, H, W, cout).to(dt).cuda()
    wg = R.conv_grad_pack(w)
    gref, gmag = R.conv_ref(dy, wg, None)
    assert torch.allclose(gref, R.conv_dx_ref(dy, w), rtol=1e-12, atol=1e-12)
    out = R.Guarded(2 * H * W, cin, dt, "cuda")
    done(lib, lib.smi_op_conv3x3_small(code(dt), P(dy), P(wg), None, P(out.view), 0, 2, H, W, cout, cin, None))
    within(out, gref, R.conv_bound(gref, gmag, cout, dt), f"conv3x3_small gradient {H}x{W} {cout}->{cin}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("Cc,Cpad,HW", R.NCHW_CASES)
def test_nchw_to_nhwc(lib, dt, Cc, Cpad, HW):
    for src_dt in (dt, torch.float32):
        src, sc = R.nchw_inputs(Cc, HW, src_dt)
        src, sc = src.cuda(), sc.cuda()
        out = R.Guarded(3 * HW, Cpad, dt, "cuda")
        done(lib, lib.smi_op_nchw_to_nhwc(code(dt), P(src), int(src_dt == torch.float32), P(out.view), 3, Cc, HW, Cpad, 0.18215, None))
        ref = R.nchw_ref(src, Cpad, 0.18215)
        within(out, ref, R.nchw_bound(ref, dt), f"nchw_to_nhwc {Cc}->{Cpad} x {HW} from {src_dt}")
        assert bool((out.view.reshape(3, HW, Cpad)[:, :, Cc:] == 0).all()), "pad columns not zero"
    src, sc = R.nchw_inputs(Cc, HW, torch.float32)
    src, sc = src.cuda(), sc.cuda()
    out = R.Guarded(3 * HW, Cpad, dt, "cuda")
    done(lib, lib.smi_op_nchw_to_nhwc_scaled(code(dt), P(src), P(out.view), 3, Cc, HW, Cpad, P(sc), None))
    ref = R.nchw_ref(src, Cpad, 1.0, sc)
    within(out, ref, R.nchw_bound(ref, dt), f"nchw_to_nhwc_scaled {Cc}->{Cpad} x {HW}")
    assert bool((out.view.reshape(3, HW, Cpad)[:, :, Cc:] == 0).all()), "pad columns not zero"
