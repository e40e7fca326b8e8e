"""CPU proof that tests/test_conv_gather_gpu.py can fail (no GPU needed), on the very inputs of the GPU file:

* the two references of tests/conv_gather_refs.py -- torch's float64 convolution and the index rule of csrc/kernels.h as a
  patch matrix -- agree exactly on the integer data and to 1e-12 on the random data, for every case and both types;
* the integer data is what the exactness argument needs: every reference value a multiple of 1/2 that fp32 holds exactly,
  below 2^15;
* every mutant of the index rule (MUTANT_CASES: which error, on which cases) changes at least one element of
  reference.to(dt) on the integer data, in both types and in every case it is listed for; on the random data it misses
  `close` as well, except where EXACT_ONLY states that only the exact comparison sees it;
* the expectation table (expected_tile) gives the coverage the GPU file relies on: every mutant is caught on every kernel
  generation that has the gather it breaks, every tile that takes convs runs un-replaced on a plain case, every gemm2 tile
  and v1 on each of the stride-2, pad-0, transposed and up-sampled gathers, the 8-phase and the persistent kernels on the
  cases written for them."""
import pytest
import torch

import conv_gather_refs as CR

DT = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
BY = {c.name: c for c in CR.ALL}

FWD = [c.name for c in CR.ALL if c.mode != "t"]
T = [c.name for c in CR.ALL if c.mode == "t"]
# which cases each mutant must be caught on
MUTANT_CASES = {
    # (t_odd, t_wide: no valid tap of an odd map's gradient passes the parity test and lies past the border)
    "no_mask": FWD + ["t_even", "t_splitk"],
    "origin": FWD,
    "swap_kykx": [c.name for c in CR.ALL if c.name != "plain_1x1"],  # (1 x 1: only the centre tap is inside)
    "pad0_as_pad1": ["s2_pad0", "s2_pad0_wide"],
    "t_no_parity": T,
    "t_round_up": T,
    "ups_halve_first": ["ups_ragged", "ups_rows_a", "ups_rows_b"],
    "img_from_in": [c.name for c in CR.ALL if c.mode != "plain"],
    "rowvec_shift": ["plain_ragged", "plain_whole_c128", "plain_splitk"],
    "row0_shift": ["plain_ragged", "plain_whole_c128"],
    "drop_c0": ["plain_ragged", "plain_whole_c128", "s2_splitk", "plain_splitk", "t_splitk"],
}
# (mutant, case, type) where the random data would pass `close` although the mutant is wrong, so that only torch.equal on the
# integer data catches it.  Empty: at these map sizes every mutant touches enough of the output to miss `close` as well.
EXACT_ONLY = set()

GENERATIONS = {"v1": ["v1"], "gemm2": ["128", "256", "64w", "160", "160w", "deep", "64x160"], "gemm3": ["8ph"], "gemm4": ["5ph"]}
MODE_GENERATIONS = {"plain": ("v1", "gemm2", "gemm3", "gemm4"), "ups": ("v1", "gemm2", "gemm4"), "s2": ("v1", "gemm2"),
                    "s2_pad0": ("v1", "gemm2"), "t": ("v1", "gemm2")}


def stored(case, t, dt):
    return t.float() if case.out_f32 else t.to(dt)


def native(case, tile):
    return CR.expected_tile(case, tile) == CR.TILES[tile]


def test_the_mutant_table_names_every_mutant_and_known_cases():
    assert set(MUTANT_CASES) == set(CR.MUTANTS)
    for names in MUTANT_CASES.values():
        assert names and set(names) <= set(BY)
    assert all(m in MUTANT_CASES and c in MUTANT_CASES[m] for m, c, _ in EXACT_ONLY)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", CR.ALL, ids=[c.name for c in CR.ALL])
def test_the_two_references_agree(case, dt):
    d = CR.build(case, dt, "int")
    assert torch.equal(d["ref"], CR.gather_reference(case, d))
    d = CR.build(case, dt, "randn")
    err = (d["ref"] - CR.gather_reference(case, d)).abs().max().item()
    assert err <= 1e-12 * d["ref"].abs().max().item(), err


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", CR.ALL, ids=[c.name for c in CR.ALL])
def test_integer_data_is_exact_in_fp32_and_below_fp16_overflow(case, dt):
    d = CR.build(case, dt, "int")
    ref = d["ref"]
    assert ref.abs().max().item() < 2 ** 15
    assert torch.equal(ref.float().double(), ref) and torch.equal((2 * ref).round(), 2 * ref)
    for k in ("x", "w", "bias", "res", "rowvec", "xa", "up"):  # the inputs are the integers drawn, in either type
        if d[k] is not None:
            assert torch.equal(d[k].double().round(), d[k].double()), k
    # the worst partial sum: every |product| at its bound, every epilogue term at its own
    bound = case.K * 2 * 8 + 4 * (case.bias + case.res + bool(case.rows_per_vec)) + case.scale * case.r * 2 * 4
    assert bound < 2 ** 15 and ref.abs().max().item() <= bound


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("mutant", CR.MUTANTS)
def test_every_mutant_is_caught(mutant, dt):
    for name in MUTANT_CASES[mutant]:
        case = BY[name]
        d = CR.build(case, dt, "int")
        got = stored(case, CR.gather_reference(case, d, mutant), dt)
        assert not torch.equal(got, stored(case, d["ref"], dt)), (mutant, name, "integer data unchanged")
        d = CR.build(case, dt, "randn")
        e, r = CR.bar(stored(case, CR.gather_reference(case, d, mutant), dt), d["ref"], dt)
        passes_close = max(e, r) <= 1.0
        assert passes_close == ((mutant, name, IDS[DT.index(dt)]) in EXACT_ONLY), (mutant, name, e, r)


@pytest.mark.parametrize("dt", DT, ids=IDS)
@pytest.mark.parametrize("case", CR.ALL, ids=[c.name for c in CR.ALL])
def test_the_rounded_reference_passes_close(case, dt):
    d = CR.build(case, dt, "randn")
    e, r = CR.bar(stored(case, d["ref"], dt), d["ref"], dt)
    assert max(e, r) <= 0.25, (case.name, e, r)  # half an ulp against a bar of 4 eps


def test_every_mutant_is_caught_on_every_generation_that_has_its_gather():
    for mutant, names in MUTANT_CASES.items():
        for mode in {BY[n].mode for n in names}:
            cases = [BY[n] for n in names if BY[n].mode == mode]
            for gen in MODE_GENERATIONS[mode]:
                assert any(native(c, t) for c in cases for t in GENERATIONS[gen]), (mutant, mode, gen)


def test_coverage_of_the_expected_tile_table():
    # every tile that takes convs runs un-replaced on a plain case; the two-wave 64 x 128 tile takes none and is always
    # replaced by the four-wave 128 x 128 tile, whose code no name of TILES asks for
    for tile in CR.TILES:
        if tile == "64":
            assert all(CR.expected_tile(c, tile) == CR.T128x128_4WAVES for c in CR.ALL)
        else:
            assert any(native(c, tile) for c in CR.PLAIN), tile
    # every gemm2 tile that takes convs, and v1, on each of the other gathers
    for mode in ("s2", "s2_pad0", "t", "ups"):
        cases = [c for c in CR.ALL if c.mode == mode]
        for tile in GENERATIONS["gemm2"] + GENERATIONS["v1"]:
            assert any(native(c, tile) for c in cases), (mode, tile)
        assert not any(native(c, "8ph") for c in cases)
        assert mode == "ups" or not any(native(c, "5ph") for c in cases)
    for name in ("plain_ragged", "plain_whole", "plain_whole_c128", "plain_handover", "plain_handover_ragged"):
        assert native(BY[name], "8ph"), name
    for name in ("plain_whole", "plain_whole_c128", "plain_handover", "plain_handover_ragged", "ups_rows_a", "ups_rows_b"):
        assert native(BY[name], "5ph"), name
    assert not native(BY["plain_ragged"], "5ph") and not native(BY["ups_ragged"], "5ph")
    # what stands in is the eight-wave 128 x 128 tile at every size of this file but the hand-over cases', which need none
    for c in CR.ALL:
        if not c.name.startswith("plain_handover"):
            assert CR.heuristic(c) == CR.TILES["128"], c.name
    for name in ("plain_handover", "plain_handover_ragged"):
        assert all(native(BY[name], t) for t in CR.TILES if t != "64")
        # more 256 x 320 tiles than a persistent grid of one workgroup per CU (256 on the MI355X) starts
        assert (BY[name].M // 256) * (BY[name].N // 320) > 256
    # N == 4: gemm2's 128-wide tiles and v1 only
    n4 = BY["conv_out_n4"]
    assert {t for t in CR.TILES if native(n4, t)} == {"128", "256", "64w", "v1"}
    # forced split-K: 18 K-tiles, so three slices start mid-tap and four are uneven
    for c in CR.SPLITK_CASES:
        assert c.K // 64 == 18 and c.ksplit == (2, 3, 4) and all(native(c, t) for t in CR.SPLITK_TILES)


def test_pad0_is_tested_on_even_maps_only():
    for c in CR.ALL:
        if c.mode == "s2_pad0":
            assert c.H % 2 == 0 and c.W % 2 == 0
