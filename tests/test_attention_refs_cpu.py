"""The yardstick of test_attention_kernels_gpu.py, checked without a GPU (tests/attention_refs.py): on every case of the GPU
test that fits a CPU float64 reference, in both dtypes,
  * the rounding emulation (exactly the modelled rounding sites) lies within 1.0 E of the float64 reference,
  * the float64 reference rounded to the dtype lies within it,
  * every mutated reference that applies to the case leaves SLACK * E somewhere in an output it changes,
so the bound the kernels are held to is neither violated by the roundings they are known to make nor wide enough to hide one
of the listed faults.  Also: the dispatcher restatement gives the documented choices, and the operand layouts do not overlap.
test_emulation_ratio_table prints the emulation's maxima per output."""
import pytest
import torch

import attention_refs as AR
from attention_refs import Case

DT = [torch.float16, torch.bfloat16]
CASES = AR.cpu_cases()
OUTS = ("O", "dQ", "dK", "dV")
_EMU_MAX = {}


@pytest.fixture(scope="module")
def refs():
    """(case, dtype) -> inputs, float64 reference, bounds: computed once, shared, never modified."""
    cache = {}

    def of(case, dt):
        key = (case, dt)
        if key not in cache:
            q, k, v, d_o = AR.make_inputs(case, dt)
            ref = AR.attn_ref64(q, k, v, case.scale, d_o)
            cache[key] = (q, k, v, d_o, ref, AR.bounds(ref, q, k, v, d_o, case.scale, dt))
        return cache[key]
    return of


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=Case.tag)
def test_emulation_and_rounded_reference_within_bound(refs, case, dt):
    q, k, v, d_o, ref, e = refs(case, dt)
    emu = AR.emulate(q, k, v, d_o, case.scale, dt)
    for n in OUTS:
        r = AR.ratio(emu[n], ref[n], e[n])
        _EMU_MAX[(n, dt)] = max(_EMU_MAX.get((n, dt), 0.0), r)
        assert r <= 1.0, f"{case.tag()} {n}: emulation at {r:.3f} E"
        r = AR.ratio(AR.rnd16(ref[n], dt), ref[n], e[n])
        assert r <= 1.0, f"{case.tag()} {n}: rounded reference at {r:.3f} E"
    assert (emu["lse"] - ref["lse"]).abs().max() < 2e-3


@pytest.mark.parametrize("dt", DT, ids=["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=Case.tag)
def test_every_applicable_mutation_leaves_the_bound(refs, case, dt):
    q, k, v, d_o, ref, e = refs(case, dt)
    for name, (outs, applies) in AR.MUTATIONS.items():
        if not applies(case):
            continue
        mut = AR.mutated_ref(name, q, k, v, case.scale, d_o)
        worst = max(AR.ratio(mut[n], ref[n], e[n]) for n in outs)
        assert worst > AR.SLACK, f"{case.tag()}: mutation {name} stays within {worst:.2f} E (SLACK {AR.SLACK})"


def test_emulation_ratio_table():
    """Runs after the parametrised test above (file order): the emulation's worst |err| / E per output and dtype."""
    for (n, dt), r in sorted(_EMU_MAX.items(), key=str):
        print(f"emulation max |err|/E  {n:3s} {str(dt):15s} {r:.3f}")
        assert r <= 1.0


def path(D, Nq=130, Nk=200, B=2, H=3, grads="fwd", sel=(-1, -1)):
    return AR.expected_path(D, Nq, Nk, B, H, grads, sel)


def test_expected_path_documented_choices():
    for D, dp, form in [(40, 64, 2), (80, 96, 2), (72, 96, 2), (48, 64, 2), (24, 32, 1), (56, 64, 1), (88, 96, 1), (152, 160, 1),
                        (16, 32, 0), (8, 32, 0), (136, 160, 0), (104, 160, 0), (64, 64, 1), (32, 32, 1), (96, 96, 1),
                        (160, 160, 1)]:
        p = path(D)
        assert (p["dp"], p["form"]) == (dp, form), (D, p)
    # Nk 96 -> the single-pass kernels, 97 -> the tiled ones; the switch and the run-time form keep them off
    assert path(64, Nk=96)["families"] == [AR.XS_FWD] and path(64, Nk=97)["families"] == [AR.FWD]
    assert path(64, Nk=96, grads="q")["families"] == [AR.XS_DQ] and path(64, Nk=97, grads="q")["families"] == [AR.DQ]
    assert path(64, Nk=77, sel=(0, -1))["families"] == [AR.FWD]
    assert path(16, Nk=77)["families"] == [AR.FWD] and path(16, Nk=77, grads="q+kv")["families"] == [AR.DQ, AR.DKV]
    assert path(64, Nk=77, grads="q+kv")["families"] == [AR.XS_DQ, AR.DKV]
    # the fused backward: all gradients, a compile-time form, depth <= 64, more than 96 keys, <= 1024 workgroups per kind
    assert path(64, grads="q+kv")["families"] == [AR.BWD_FUSED]
    assert path(64, grads="q+kv", sel=(-1, 0))["families"] == [AR.DQ, AR.DKV]
    assert path(64, grads="q")["families"] == [AR.DQ] and path(64, grads="kv")["families"] == [AR.DELTA, AR.DKV]
    assert path(80, grads="q+kv")["families"] == [AR.DQ, AR.DKV] and path(16, grads="q+kv")["families"] == [AR.DQ, AR.DKV]
    assert path(136, grads="q+kv")["families"] == [AR.DQ, AR.DK_DV] and path(160, grads="kv")["families"] == [AR.DELTA, AR.DK_DV]
    assert path(64, Nq=128 * 1024, B=1, H=1, grads="q+kv")["families"] == [AR.BWD_FUSED]
    assert path(64, Nq=128 * 1025, B=1, H=1, grads="q+kv")["families"] == [AR.DQ, AR.DKV]  # 1025 workgroups
    assert path(64, Nq=128 * 41, B=5, H=5, grads="q+kv")["families"] == [AR.DQ, AR.DKV]    # 1025 workgroups
    # chained query blocks: only once B*H*nqb/2 >= 1280, only while the block count stays divisible
    assert path(64, Nq=8192 - 56, Nk=77, B=2, H=20)["chain"] == 2
    assert path(40, Nq=16384 - 56, Nk=77, B=2, H=20)["chain"] == 4
    assert path(64, Nq=8192 - 56 - 128, Nk=77, B=2, H=20)["chain"] == 1   # 63 blocks: odd
    assert path(64, Nq=8192 - 128, Nk=77, B=2, H=19)["chain"] == 1        # 38 * 32 = 1216 < 1280
    assert path(64, Nq=200, Nk=77)["chain"] == 1 and path(64, Nq=200, Nk=200)["chain"] == 0


@pytest.mark.parametrize("layout", AR.LAYOUTS)
@pytest.mark.parametrize("Nk", [77, 200])
def test_layouts_do_not_overlap_and_masks_cover_the_operand(layout, Nk):
    case = Case(40, 200, Nk, layout=layout)
    built = AR.build_case(case, torch.float16)
    ops, shape = built["ops"], built["shape"]
    for b, flat in built["bufs"].items():
        count = torch.zeros(flat.numel(), dtype=torch.int32)
        for op, (bn, off, ld) in ops.items():
            if bn == b:
                assert ld % 8 == 0 and off % 8 == 0
                AR.op_view(case, count, op, off, ld).add_(1)
        assert int(count.max()) == 1, f"{layout}: operands overlap in {b}"
    for op in AR.OPERANDS:
        n = case.Nq if op in ("q", "o", "do", "dq") else case.Nk
        assert int(AR.owned_mask(built, ops[op][0], [op]).sum()) == case.B * n * case.H * case.D
    # inputs landed where the views say, everything else is still the NaN pattern
    for op in ("q", "k", "v", "do"):
        assert torch.equal(AR.get(built, op), built[op])
    for b in built["bufs"]:
        srcs = [op for op in ("q", "k", "v", "do") if ops[op][0] == b]
        assert AR.untouched(built, b, srcs) == 0
    if layout == "alldiff":
        assert len({ops[op][2] for op in AR.OPERANDS}) == 8
    if layout == "ext":
        assert ops["k"][2] == 6 * case.H * case.D + 8 and ops["dk"][1] == ops["k"][1] and ops["dv"][1] == ops["v"][1]


def test_leading_dimensions_that_are_no_16_byte_multiple_are_refused():
    """O moves in 16-byte pieces (the single-pass forward's row stores, every backward kernel's reads), dO and the single-pass
    dQ likewise: check_attn refuses a leading dimension that is a multiple of 4 but not of 8 on the host, before any launch
    (no GPU is touched: the pointers are never dereferenced)."""
    import ctypes as C
    from sliders_conceptmod_amd import _native, build as smi_build
    smi_build.build()
    lib = _native.lib()
    for field, bwd in [("ldo", False), ("ldq", False), ("ldo", True), ("lddo", True), ("lddq", True), ("lddk", True)]:
        a, ran = _native.AttnArgsC(), _native.AttnRanC()
        a.q = a.k = a.v = a.o = a.lse = a.d_o = a.dq = a.dk = a.dv = a.delta = 256
        a.b, a.h, a.nq, a.nk, a.d, a.scale = 1, 2, 16, 16, 40, 1.0
        a.sel_xs = a.sel_fused = -1
        for f in ("ldq", "ldk", "ldv", "ldo", "lddo", "lddq", "lddk", "lddv"):
            setattr(a, f, 80)
        setattr(a, field, 84)
        ran.n_launches = 7
        rc = (lib.smi_op_attention_ex_bwd if bwd else lib.smi_op_attention_ex_fwd)(C.byref(a), C.byref(ran))
        msg = lib.smi_last_error().decode()
        assert rc != 0 and ran.n_launches == 0, (field, rc, ran.n_launches)
        assert field in msg and "84" in msg and "multiples of 8" in msg, msg
