"""CPU proof that tests/test_gemm_epilogue_gpu.py can fail (no GPU needed).  On the very inputs of the GPU file, for every
case and both 16-bit types:

* the float64 reference rounded the way the kernel stores its output (once, to the 16-bit type; fp32 for the fp32 cases)
  passes bar (a) -- `close(mult=4)` of tests/test_kernels_gpu.py -- with room to spare;
* every single-term mutation of the reference that the case has the term for misses that bar by at least FAR = 10 times:
  bias dropped, row vector dropped, the rows_per_vec boundary one row early, the delta also on row row0 - 1, two segments'
  xa columns swapped, the dX operand read untransposed, residual dropped;
* the expectation table of tile fallbacks says what the issue of record says: every tile native on the whole-tile cases,
  the 160-column eight-wave / deep / 64-row tiles and the persistent kernel falling back on the tails, only gemm2's
  128-wide tiles and v1 native at N == 4."""
import pytest
import torch

import gemm_epilogue_refs as GR

DT = [torch.float16, torch.bfloat16]
FAR = 10.0  # a mutant must miss the bar by this factor (measured: the closest is the one-row mutants at bf16, ~12x)
ALL = GR.CASES + [GR.SPLITK]


def mutants(case, d):
    out = {}
    if case.bias:
        out["bias dropped"] = GR.reference(case, d, drop=("bias",))
    if case.res:
        out["residual dropped"] = GR.reference(case, d, drop=("res",))
    if case.rows_per_vec:
        out["row vector dropped"] = GR.reference(case, d, drop=("rowvec",))
        out["row-vector boundary one row early"] = GR.reference(case, d, rowvec_shift=1)
    if case.form:
        out["delta dropped"] = GR.reference(case, d, drop=("delta",))
    if case.form == "fwd" and case.row0 > 0:
        out["delta on row row0 - 1"] = GR.reference(case, d, row_shift=1)
    if case.form == "fwd" and case.seg:
        out["segments' xa swapped"] = GR.reference(case, d, swap_segments=True)
    if case.form == "dx":
        out["dX operand untransposed"] = GR.reference(case, d, untransposed=True)
    return out


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_bar_accepts_the_rounded_reference_and_rejects_every_mutant(case, dt):
    d = GR.build(case, dt)
    ref = d["ref"]
    stored = ref.float() if case.out_f32 else ref.to(dt)
    e, r = GR.bar(stored, ref, dt)
    assert max(e, r) <= 0.25, (case.name, "rounded reference", e, r)  # half an ulp against a bar of 4 eps
    muts = mutants(case, d)
    assert muts
    for name, m in muts.items():
        e, r = GR.bar(m.float() if case.out_f32 else m.to(dt), ref, dt)
        assert max(e, r) >= FAR, (case.name, name, e, r)


def test_every_term_and_mutation_is_exercised():
    seen = set()
    for case in ALL:
        seen |= set(mutants(case, GR.build(case, torch.float16)))
    assert seen == {"bias dropped", "residual dropped", "row vector dropped", "row-vector boundary one row early",
                    "delta dropped", "delta on row row0 - 1", "segments' xa swapped", "dX operand untransposed"}


def test_expected_tile_table():
    by = {c.name: c for c in ALL}
    for name in ("whole", "batched", "dx", "r3", "r16", "r32", "f32"):
        for tile, code in GR.TILES.items():
            assert GR.expected_tile(by[name], tile) == code, (name, tile)
    fall = {t for t in GR.TILES if GR.expected_tile(by["tails"], t) != GR.TILES[t]}
    assert fall == {"160w", "deep", "64x160", "5ph"}  # (the four-wave 128 x 160 tile takes any N % 8 == 0: partial last tile)
    for name in ("n4", "n4_f32"):
        native = {t for t in GR.TILES if GR.expected_tile(by[name], t) == GR.TILES[t]}
        assert native == {"128", "256", "64", "64w", "v1"}
        assert GR.expected_tile(by[name], "160") == GR.T128x128_4WAVES
    # the batched case is the slider step's layout (3 frozen : 1 adapted), which the persistent kernel interleaves per tile
    assert 4 * by["batched"].row0 == 3 * by["batched"].M
