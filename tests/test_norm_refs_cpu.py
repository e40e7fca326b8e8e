"""CPU checks of tests/norm_refs.py itself: the restated dispatcher against a table, the bounds E against an fp32 emulation of
a correct kernel and against the rounded float64 result (both within 1.0 E, the statistics within the bar), and every mutant
outside 2 E (or twice the statistics bar) on a named case of the GPU tests' own inputs."""
import pytest
import torch

import norm_refs as R

DT = [torch.float16, torch.bfloat16]


def test_dispatcher_table():
    #        HW      rows/chunk chunks fold-per
    table = [(1, 16, 1, 0), (15, 16, 1, 0), (16, 16, 1, 0), (17, 16, 2, 0), (100, 16, 7, 0), (256, 16, 16, 0),
             (257, 16, 17, 0), (1024, 16, 64, 0), (1025, 32, 33, 0), (4096, 64, 64, 0), (16384, 256, 64, 0),
             (16385, 256, 65, 2), (256 * 129 + 5, 256, 130, 3), (1024 * 1024, 256, 4096, 64)]
    for HW, rpc, n, per in table:
        assert (R.gn_rows_per_chunk(HW), R.gn_num_chunks(HW), R.gn_fold_per(HW)) == (rpc, n, per), HW
    assert R.gn_expected_ran(16385, 64, 8) == (R.GN_FOLD, 65, 64)
    assert R.gn_expected_ran(1025, 64, 8) == (R.GN_TWO, 33, 33)
    assert R.gn_partial_floats(2, 16385, 32) == 2 * (65 + 64) * 32 * 2
    assert R.gn_partial_floats(2, 1024, 32) == 2 * 64 * 32 * 2
    # the one-launch form: HW <= 256, even group width <= 256, slice <= 96 KB
    fused = [((256, 320, 32), True), ((257, 320, 32), False), ((100, 24, 8), False), ((100, 64, 1), True),
             ((100, 2048, 32), True), ((256, 2560, 32), True), ((100, 64, 32), True), ((1, 64, 8), True),
             ((256, 8192, 16), False)]
    for (HW, C, G), ok in fused:
        assert R.gn_fused_ok(HW, C, G) is ok, (HW, C, G)
        assert R.gn_fused_ok(HW, C, G, sel=0) is False
    assert R.gn_fused_ok(1024, 320, 32, sel=1) and not R.gn_fused_ok(1024, 24, 8, sel=1)
    assert not R.gn_fused_ok(16384, 320, 32, sel=1)  # 320 KB slice: past LDS whatever the selection
    assert R.gn_expected_ran(256, 320, 32) == (R.GN_ONE, 0, 0) and R.gn_expected_ran(256, 320, 32, what="bwd") == (R.GN_TWO, 16, 16)
    assert [R.gn_geom(C) for C in (24, 320, 2048, 2560)] == [(3, 1, 85), (40, 1, 6), (256, 1, 1), (320, 2, 1)]
    assert R.gn_lds_ok(8192) and not R.gn_lds_ok(8200)
    assert [R.ln_nv(C) for C in (8, 504, 512, 520, 1024, 1280, 1536, 2040, 2048)] == [1, 1, 1, 2, 2, 3, 3, 4, 4]
    assert R.ln_expected_ran(16384, 1280, False) == (R.LN, 3, 2) and R.ln_expected_ran(16384, 1280, True) == (R.LN, 3, 1)
    assert R.ln_expected_ran(16383, 64, False) == (R.LN, 1, 1)


def test_case_lists_cover_the_issue():
    names = set(R.GN_CASES)
    assert len(names) == len(R.GN_GEOMETRY) + len(R.GN_NUMERICS)  # no two cases share a name
    assert {c.HW for c in R.GN_GEOMETRY} >= {1, 15, 16, 17, 100, 256, 257, 1024, 1025, 16384, 16385, 256 * 129 + 5}
    assert {(c.C, c.G) for c in R.GN_GEOMETRY} >= {(24, 8), (64, 8), (128, 64), (320, 32), (1920, 32), (2048, 32), (2560, 32),
                                                   (64, 1), (64, 32)}
    for m, c in list(R.GN_MUTANTS.items()):
        assert c in R.GN_CASES, (m, c)
    for m, c in R.LN_MUTANTS.items():
        assert c in R.LN_CASES, (m, c)


# the cases the emulation runs here: every numerics case of the two smaller shapes, the small geometry, one fold
_EMU = [c.name for c in R.GN_NUMERICS if c.HW <= 1024] + [c.name for c in R.GN_GEOMETRY if c.HW <= 1025] + ["hw16385"]


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_groupnorm_emulation_and_rounded_reference_within_E(dt):
    worst = {}
    for name in _EMU:
        case = R.GN_CASES[name]
        inp = R.gn_inputs(case, dt)
        y, mean, rstd, dx = R.gn_emulate(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, case.silu, dt, inp["dy"], inp["add"])
        j = R.gn_judge(case, inp, dt, dict(y=y, mean=mean, rstd=rstd, dx=dx))
        ref = R.gn_ref(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, case.silu, inp["dy"], inp["add"])
        k = R.gn_judge(case, inp, dt, dict(y=ref["y"].to(dt), mean=ref["mean"].float(), rstd=ref["rstd"].float(), dx=ref["dx"].to(dt)))
        for tag, res in (("emulation", j), ("rounded float64", k)):
            for key, v in res.items():
                assert v <= 1.0, f"{name} {tag}: {key} at {v:.3f} of its bound"
                worst[(tag, key)] = max(worst.get((tag, key), 0.0), v)
    print("groupnorm", dt, {f"{t} {k}": round(v, 3) for (t, k), v in worst.items()})


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_layernorm_emulation_and_rounded_reference_within_E(dt):
    for case in R.LN_CASES_LIST:
        if case.M > 77:
            continue
        inp = R.ln_inputs(case, dt)
        ref = R.ln_ref(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["dy"], inp["add"])
        E_y, E_dx = R.ln_bounds(ref, inp["x"], inp["gamma"], inp["beta"], dt, inp["dy"], inp["add"])
        y, mean, rstd, dx = R.ln_emulate(inp["x"], inp["gamma"], inp["beta"], R.EPS, dt, inp["dy"], inp["add"])
        for tag, (yy, mm, rr, dd) in (("emulation", (y, mean, rstd, dx)),
                                      ("rounded float64", (ref["y"].to(dt), ref["mean"].float(), ref["rstd"].float(), ref["dx"].to(dt)))):
            sr, sm = R.stat_worst(mm, rr, ref)
            res = dict(y=R.worst(yy, ref["y"], E_y), dx=R.worst(dd, ref["dx"], E_dx), rstd=sr, mean=sm)
            for key, v in res.items():
                assert v <= 1.0, f"{case.name} {tag}: {key} at {v:.3f} of its bound"


@pytest.mark.parametrize("fault", sorted(R.GN_MUTANTS))
@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_groupnorm_mutant_is_caught(fault, dt):
    case = R.GN_CASES[R.GN_MUTANTS[fault]]
    inp = R.gn_inputs(case, dt)
    got = R.gn_mutant_outputs(fault, case, inp, dt)
    res = R.gn_judge(case, inp, dt, got, n0=got["n0"])
    assert max(res.values()) > R.SLACK, f"{fault} passes on {case.name}: {res}"


@pytest.mark.parametrize("fault", sorted(R.LN_MUTANTS))
@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
def test_layernorm_mutant_is_caught(fault, dt):
    case = R.LN_CASES[R.LN_MUTANTS[fault]]
    inp = R.ln_inputs(case, dt)
    ref = R.ln_ref(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["dy"], inp["add"])
    E_y, E_dx = R.ln_bounds(ref, inp["x"], inp["gamma"], inp["beta"], dt, inp["dy"], inp["add"])
    m = R.ln_ref(inp["x"], inp["gamma"], inp["beta"], R.EPS, inp["dy"], inp["add"], fault=fault)
    sr, sm = R.stat_worst(m["mean"].float(), m["rstd"].float(), ref)
    res = dict(y=R.worst(m["y"].to(dt), ref["y"], E_y), dx=R.worst(m["dx"].to(dt), ref["dx"], E_dx), rstd=sr, mean=sm)
    assert max(res.values()) > R.SLACK, f"{fault} passes on {case.name}: {res}"


def test_one_pass_statistics_lose_the_bar_from_ratio_32_up():
    """The arithmetic every GroupNorm form had (var = sumsq / cnt - mean^2 in fp32) against the bar, by offset."""
    out = {}
    for r in (0, 8, 32, 128, 256):
        case = R.GN_CASES[f"offset{r if r else ''}_1024x320"]
        inp = R.gn_inputs(case, torch.float16)
        ref = R.gn_ref(inp["x"], inp["gamma"], inp["beta"], case.G, case.eps, 0)
        one = R.stat_worst(*R.gn_stats32(inp["x"], case.G, case.eps, True), ref)
        two = R.stat_worst(*R.gn_stats32(inp["x"], case.G, case.eps, False), ref)
        out[r] = (one, two)
        assert max(two) <= 1.0, (r, two)
    print("one-pass | two-pass statistics error over the bar, by |mean| / std:", out)
    assert max(out[256][0]) > R.SLACK and max(out[128][0]) > R.SLACK and max(out[0][0]) <= 1.0


def test_guarded_buffer():
    b = R.Guarded(3, 8, torch.float16, "cpu")
    assert b.untouched() and b.guards_intact()
    b.view.fill_(1.0)
    assert b.guards_intact() and not b.untouched()
    b.full[0, 0] = 0.0
    assert not b.guards_intact()
