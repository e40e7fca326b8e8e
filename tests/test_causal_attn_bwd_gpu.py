"""The causal self-attention backward (csrc/attention_causal.hip) and the activation backward through their C-ABI test
entries, against the float64 references of tests/notrigger_refs.py on the same 16-bit inputs.

Bar: relative L2 of each output against the exact reference A at most 3 e_q + 1e-4, with e_q the distance of the rounded
reference B from A (P, dS and the outputs rounded to the storage type).  tests/test_notrigger_refs_cpu.py shows that a
wrong mask, a dropped delta and a missing scale all miss that bar."""
import ctypes as C

import pytest
import torch

import notrigger_refs as R

pytestmark = pytest.mark.gpu

DT = [torch.float16, torch.bfloat16]
LENGTHS = [2, 16, 64, 65, 77]  # below a tile, exact tiles, one past a tile, the text towers' length


@pytest.fixture(scope="module")
def lib():
    from sliders_conceptmod_amd import _native
    assert torch.cuda.is_available(), "these tests need the GPU box"
    return _native.lib()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def dcode(dt):
    return 0 if dt == torch.float16 else 1


_cases = {}


def case(L, dt):
    """The inputs and both float64 references of one (length, dtype): computed once, shared, never modified."""
    if (L, dt) not in _cases:
        _cases[(L, dt)] = R.causal_attn_case(L, dt)
    return _cases[(L, dt)]


def nan_filled(shape, dt):
    return torch.full(shape, 0x7FFF, dtype=torch.int16, device="cuda").view(dt)


def run(lib, c, dt, fused, samples=None):
    """Forward then backward on the GPU.  fused: q | k | v are the column blocks of one [b L, 3 h D] tensor (leading
    dimension 3 h D) and so are dq | dk | dv, as in the engine; else everything is packed.  samples: a slice of the batch."""
    sl = slice(None) if samples is None else samples
    q, k, v, do = (c[n][sl].to(dt).cuda().contiguous() for n in ("q", "k", "v", "do"))
    b, L, h, D = q.shape
    hd = h * D
    if fused:
        qkv = torch.cat([q.reshape(b * L, hd), k.reshape(b * L, hd), v.reshape(b * L, hd)], dim=1).contiguous()
        qp, kp, vp, ld = qkv, qkv[:, hd:], qkv[:, 2 * hd:], 3 * hd
        dqkv = nan_filled((b * L, 3 * hd), dt)
        dqp, dkp, dvp = dqkv, dqkv[:, hd:], dqkv[:, 2 * hd:]
    else:
        qp, kp, vp, ld = q, k, v, hd
        dqp, dkp, dvp = (nan_filled((b * L, hd), dt) for _ in range(3))
    o = nan_filled((b, L, h, D), dt)
    lse = torch.full((b, h, L), float("nan"), device="cuda")
    rc = lib.smi_op_attention_causal_fwd(dcode(dt), P(qp), P(kp), P(vp), P(o), P(lse), b, h, L, D, ld, ld, ld, hd,
                                         c["scale"], None)
    assert rc == 0, lib.smi_last_error().decode()
    rc = lib.smi_op_attention_causal_bwd(dcode(dt), P(qp), P(kp), P(vp), P(o), P(lse), P(do), P(dqp), P(dkp), P(dvp), None,
                                         b, h, L, L, D, ld, ld, ld, hd, hd, ld, ld, ld, c["scale"], None)
    assert rc == 0, lib.smi_last_error().decode()
    torch.cuda.synchronize()
    grads = [t[:, :hd].reshape(b, L, h, D).clone() for t in (dqp, dkp, dvp)]
    return o, lse, grads


@pytest.mark.parametrize("fused", [False, True], ids=["packed", "fused3C"])
@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("L", LENGTHS)
def test_causal_backward_against_f64(lib, L, dt, fused):
    c = case(L, dt)
    o, lse, grads = run(lib, c, dt, fused)
    oA, lseA = c["A"][0], c["A"][1]
    # (the forward is attention.hip's and has its own tests: only that o and lse are what the backward should be given)
    assert R.rel(o, oA) < (2e-3 if dt == torch.float16 else 1.5e-2) and R.rel(lse, lseA) < 1e-3
    for name, got, a, b_ in zip(("dq", "dk", "dv"), grads, c["A"][2:], c["B"][2:]):
        assert torch.isfinite(got.float()).all(), name
        e_q, e = R.rel(b_, a), R.rel(got, a)
        print(f"L {L} {dt} {'fused' if fused else 'packed'} {name}: e {e:.3e}  e_q {e_q:.3e}  ratio {e / e_q:.2f}")
        assert e <= R.bar(e_q), (name, e, e_q)
    # a second run gives the same bits
    _, _, again = run(lib, c, dt, fused)
    assert all(torch.equal(a.view(torch.int16), g.view(torch.int16)) for a, g in zip(again, grads))


@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
def test_a_sample_alone_and_in_a_batch_gives_equal_bits(lib, dt):
    c = case(77, dt)
    _, _, both = run(lib, c, dt, True)
    for i in range(2):
        _, _, alone = run(lib, c, dt, True, slice(i, i + 1))
        for a, g in zip(alone, both):
            assert torch.equal(a.view(torch.int16), g[i:i + 1].view(torch.int16))


def test_refused_shapes_return_an_error(lib):
    """Outside 1 <= Nq == Nk <= 128, head_dim 64, all three gradients: an error that names the limit, never the unmasked
    kernels."""
    dt = torch.float16
    t = lambda *s: torch.zeros(s, dtype=dt, device="cuda")

    def bwd(b, h, nq, nk, d, dq=True):
        q, k, v, o, do = t(b, nq, h, d), t(b, nk, h, d), t(b, nk, h, d), t(b, nq, h, d), t(b, nq, h, d)
        g = [t(b, nq, h, d) if dq else None, t(b, nk, h, d), t(b, nk, h, d)]
        lse = torch.zeros((b, h, nq), device="cuda")
        ld = h * d
        return lib.smi_op_attention_causal_bwd(0, P(q), P(k), P(v), P(o), P(lse), P(do), P(g[0]), P(g[1]), P(g[2]), None, b, h,
                                               nq, nk, d, ld, ld, ld, ld, ld, ld, ld, ld, d ** -0.5, None)

    for args, word in (((1, 2, 129, 129, 64), "128"), ((1, 2, 77, 64, 64), "Nq == Nk"), ((1, 2, 77, 77, 32), "head_dim"),
                       ((1, 2, 77, 77, 128), "head_dim")):
        assert bwd(*args) != 0
        assert word in lib.smi_last_error().decode(), (args, lib.smi_last_error().decode())
    assert bwd(1, 2, 77, 77, 64, dq=False) != 0 and "required" in lib.smi_last_error().decode()
    assert bwd(1, 2, 128, 128, 64) == 0  # the longest sequence it takes
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", [0, 1], ids=["quick_gelu", "gelu"])
@pytest.mark.parametrize("dt", DT, ids=["fp16", "bf16"])
@pytest.mark.parametrize("n", [4096, 1003])
def test_act_backward_against_f64(lib, n, dt, kind):
    g = torch.Generator().manual_seed(7 + n)
    x, dy = R.representable((n,), g, dt, 2.0), R.representable((n,), g, dt)
    A, B = R.act_bwd(x, dy, kind), R.act_bwd(x, dy, kind, dt)
    xg, dyg = x.to(dt).cuda(), dy.to(dt).cuda()
    dx = nan_filled((n + 8,), dt)
    y = nan_filled((n,), dt) if n % 8 == 0 else None  # the forward kernel takes whole 8-packs only
    rc = lib.smi_op_act(dcode(dt), P(xg), P(y), P(dyg), P(dx), n, kind, None)
    assert rc == 0, lib.smi_last_error().decode()
    torch.cuda.synchronize()
    e_q, e = R.rel(B, A), R.rel(dx[:n], A)
    print(f"act bwd n {n} {dt} kind {kind}: e {e:.3e}  e_q {e_q:.3e}  ratio {e / e_q:.2f}")
    assert e <= R.bar(e_q)
    assert torch.isnan(dx[n:].float()).all()  # nothing written past n
    if y is not None:
        assert R.rel(y, R.act_fwd(x, kind)) < R.bar(R.rel(R.rnd(R.act_fwd(x, kind), dt), R.act_fwd(x, kind)))
