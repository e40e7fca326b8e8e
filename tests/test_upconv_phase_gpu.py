"""The up-sampler conv's phase form on the GPU (include/smi.h smi_op_upconv_phase: phase pack, four 2x2 phase convs, the
concat's un-shuffling copy) against the one-launch form it replaces (smi_op_conv3x3 with upsample = 1) and against float64.

Exactness: with integer-valued inputs and |w| <= 8 the sums of up to four weights are exact in fp16 and bf16 and every fp32
accumulation is exact in any order, so the two forms must agree bit for bit -- which pins the tap map, the borders and the
phase interleave.  Random data: the phase form adds one rounding of the summed filters, of the size of the output's own
rounding (CPU model: relative L2 x sqrt(2)); the bar is 2 x the old form's relative L2 and max error against the float64
reference from the same 16-bit inputs.

Every tile code of the GEMM tests is forced in turn (0 = the launcher's own choice, with and without split-K scratch); a
tile that cannot take the launch must be replaced, not fail."""
import ctypes as C

import pytest
import torch

import gemm_epilogue_refs as GR
import upconv_phase_refs as R

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
# (Nb, H, W, Cin, Cout): one pixel; ragged (105 rows per phase: a phase boundary inside a tile, were the planes one launch);
# 256 rows per phase; two samples with W != H
SHAPES = [(1, 1, 1, 64, 64), (3, 5, 7, 64, 320), (1, 16, 16, 320, 640), (2, 8, 32, 128, 320)]
CODES = [0] + sorted(GR.TILES.values())
KNOWN = set(CODES) | {GR.T128x128_4WAVES}


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def chk(lib, rc):
    assert rc == 0, lib.smi_last_error().decode()


def dcode(dt):
    return 0 if dt == torch.float16 else 1


def pack_fwd(w):  # [Cout, Cin, 3, 3] -> [Cout, 9 * Cin] in (ky, kx, ci) order
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def old_form(lib, dt, x, w, b):
    nb, H, W, cin = x.shape
    cout = w.shape[0]
    y = torch.empty(nb, 2 * H, 2 * W, cout, device="cuda", dtype=dt)
    chk(lib, lib.smi_op_conv3x3(dcode(dt), P(x), P(pack_fwd(w)), P(b), P(y), nb, H, W, cin, cout, 1, 1, 0, 2 * H, 2 * W, None))
    return y


def phase_form(lib, dt, x, w, b, code):
    nb, H, W, cin = x.shape
    cout = w.shape[0]
    wph = torch.empty(16 * cout * cin, device="cuda", dtype=dt)
    planes = torch.full((4, nb, H, W, cout), 7.0, device="cuda", dtype=dt)
    y = torch.full((nb, 2 * H, 2 * W, cout), 9.0, device="cuda", dtype=dt)
    ran = (C.c_int * 4)(-1, -1, -1, -1)
    chk(lib, lib.smi_op_upconv_phase(dcode(dt), P(x), P(w), P(b), P(wph), P(planes), P(y), nb, H, W, cin, cout, code, ran, None))
    assert all(r in KNOWN for r in ran), f"tile code {code}: ran {list(ran)}"
    return y, wph.view(4, cout, 4 * cin), planes


def every_form(lib, dt, x, w, b):
    """(label, output) of the phase form under every tile code, and under the launcher's choice with split-K scratch lent"""
    for code in CODES:
        yield f"tile {code}", phase_form(lib, dt, x, w, b, code)[0]
    ws = torch.empty(4 << 20, device="cuda", dtype=torch.float32)
    try:
        chk(lib, lib.smi_op_gemm_scratch(P(ws), ws.numel() * 4))
        yield "tile 0 + split-K scratch", phase_form(lib, dt, x, w, b, 0)[0]
    finally:
        chk(lib, lib.smi_op_gemm_scratch(None, 0))


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_is_bit_equal_on_integers(lib, dt, shape):
    nb, H, W, cin, cout = shape
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randint(-2, 3, (nb, H, W, cin), device="cuda", generator=g).to(dt)
    w = torch.randint(-8, 9, (cout, cin, 3, 3), device="cuda", generator=g).to(dt)
    b = torch.randint(-4, 5, (cout,), device="cuda", generator=g).to(dt)
    want = old_form(lib, dt, x, w, b)
    _, wph, planes = phase_form(lib, dt, x, w, b, 0)
    assert torch.equal(wph, R.phase_pack(w.float(), dt)), "phase pack"
    assert torch.equal(R.unshuffle(planes), want), "planes"
    bad = [label for label, got in every_form(lib, dt, x, w, b) if not torch.equal(got, want)]
    assert not bad, f"differs from smi_op_conv3x3(upsample=1): {bad}"


_REF = {}


def random_case(shape, dt):
    """16-bit inputs and their float64 reference, computed once per (shape, dtype) and left unchanged"""
    key = (shape, dt)
    if key not in _REF:
        nb, H, W, cin, cout = shape
        g = torch.Generator().manual_seed(11)
        x = torch.randn(nb, H, W, cin, generator=g).to(dt)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5).to(dt)
        b = torch.randn(cout, generator=g).to(dt)
        ref = R.upconv_ref(x.double().permute(0, 3, 1, 2), w.double(), b.double()).permute(0, 2, 3, 1).contiguous()
        _REF[key] = (x.cuda(), w.cuda(), b.cuda(), ref.cuda())
    return _REF[key]


def errors(y, ref):
    d = y.double() - ref
    return (d.norm() / ref.norm()).item(), d.abs().max().item()


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_error_within_twice_the_old_form(lib, dt, shape):
    x, w, b, ref = random_case(shape, dt)
    rel_old, max_old = errors(old_form(lib, dt, x, w, b), ref)
    print(f"\n{shape} {dt}: old form rel L2 {rel_old:.3e} max {max_old:.3e}")
    bad = []
    seen = []
    for label, got in every_form(lib, dt, x, w, b):
        if any(torch.equal(got, s) for s in seen):
            continue  # (the generations agree bit for bit: one figure per distinct result)
        seen.append(got)
        rel, mx = errors(got, ref)
        print(f"  phase form, {label}: rel L2 {rel:.3e} ({rel / rel_old:.2f} x) max {mx:.3e} ({mx / max_old:.2f} x)")
        if not (rel <= 2 * rel_old and mx <= 2 * max_old):
            bad.append(label)
    assert not bad, f"more than 2 x the old form's error: {bad}"
