"""CPU checks of tests/elementwise_refs.py: on the GPU tests' own inputs the float64 result rounded to the output type stays
inside 1.0 E, and every mutant (a tail dropped, a wrong tap, a missing pad zero, ...) leaves SLACK E."""
import pytest
import torch

import elementwise_refs as R

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def inside(ref, E, dt):
    assert R.worst(ref.to(dt), ref, E) <= 1.0


def outside(mut, ref, E, dt, what):
    assert R.worst(mut.to(dt), ref, E) > R.SLACK, f"{what} passes"


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_pool(dt):
    for H, W, C in R.POOL_CASES:
        du = R.pool_inputs(H, W, C, dt)
        ref, mag = R.pool_ref(du)
        E = R.pool_bound(ref, mag, dt)
        inside(ref, E, dt)
        for f in ("wrong_tap", "tail_dropped"):
            outside(R.pool_ref(du, f)[0], ref, E, dt, f"pool {f} {H}x{W}x{C}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_colsum(dt):
    for HW, C in R.COLSUM_CASES:
        x = R.colsum_inputs(HW, C, dt)
        ref, mag = R.colsum_ref(x, 0.375)
        E = R.colsum_bound(ref, mag, HW, dt)
        inside(ref, E, dt)
        if HW in (15, 17):  # the row whose loss shows: the last row of a ragged slice
            outside(R.colsum_ref(x, 0.375, "tail_dropped")[0], ref, E, dt, f"colsum tail {HW}x{C}")


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_timestep(dt):
    vals = torch.tensor(R.TIMESTEP_VALUES)
    for dim in R.TIMESTEP_CASES:
        ref, a, arg = R.timestep_ref(vals, dim)
        E = R.timestep_bound(ref, a, arg, dt)
        inside(ref, E, dt)
        outside(R.timestep_ref(vals, dim, "sin_first")[0], ref, E, dt, f"timestep sin first {dim}")
        # the fp32 argument error is in the bound: at t = 999 the first frequencies carry 999 * 5 * 2^-24 = 3e-4
        assert float((a.abs() * (3 * arg.abs() + 5) * R.U32).max()) > 2e-4


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_softmax(dt):
    for cols, scale in R.SOFTMAX_CASES:
        S = R.softmax_inputs(cols, scale)
        ref, s = R.softmax_ref(S, scale)
        E = R.softmax_bound(ref, s, dt)
        inside(ref, E, dt)
        assert float(ref[1, cols - 1]) > 0.9 or cols == 1  # the dominant late element
        if cols > 1:
            outside(R.softmax_ref(S, scale, "tail_dropped")[0], ref, E, dt, f"softmax tail {cols}")
        if scale < 0:
            outside(R.softmax_ref(S, scale, "max_times_scale")[0], ref, E, dt, "softmax max(S) * scale")


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_chan_mix(dt):
    for C, M in R.CHAN_MIX_CASES:
        x, W, b = R.chan_mix_inputs(C, M, dt)
        ref, mag = R.chan_mix_ref(x, W, b)
        E = R.chan_mix_bound(ref, mag, C)
        assert R.worst(ref.float(), ref, E) <= 1.0
        assert R.worst(R.chan_mix_ref(x, W, b, "tail_dropped")[0].float(), ref, E) > R.SLACK


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_conv(dt):
    for H, W, cin, cout in R.CONV_CASES:
        x, w, bias = R.conv_inputs(H, W, cin, cout, dt)
        ref, mag = R.conv_ref(x, w, bias)
        for odt in (dt, torch.float32):
            E = R.conv_bound(ref, mag, cin, odt)
            inside(ref, E, odt)
            if W > 1:
                outside(R.conv_ref(x, w, bias, "wrong_tap")[0], ref, E, odt, f"conv wrong tap {H}x{W}")
            if H > 1 or W > 1:  # (a 1 x 1 image replicated is the image itself in every tap: caught from 2 pixels on)
                outside(R.conv_ref(x, w, bias, "no_pad_zero")[0], ref, E, odt, f"conv pad {H}x{W}")
        # the gradient filter: conv(dy, flipped and transposed w) is d(in)
        dy = R._rn(7 + H + W, 2, H, W, cout).to(dt)
        g, _ = R.conv_ref(dy, R.conv_grad_pack(w), None)
        assert torch.allclose(g, R.conv_dx_ref(dy, w), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dt", DT, ids=IDS)
def test_nchw(dt):
    for C, Cpad, HW in R.NCHW_CASES:
        for src_dt in (dt, torch.float32):
            src, sc = R.nchw_inputs(C, HW, src_dt)
            for sdev in (None, sc):
                ref = R.nchw_ref(src, Cpad, 0.18215, sdev)
                E = R.nchw_bound(ref, dt)
                inside(ref, E, dt)
                if Cpad > C:
                    outside(R.nchw_ref(src, Cpad, 0.18215, sdev, "pad_not_zero"), ref, E, dt, "nchw pad")
                if sdev is not None:
                    outside(R.nchw_ref(src, Cpad, 0.18215, sdev, "scale_sample0"), ref, E, dt, "nchw scale of sample 0")
