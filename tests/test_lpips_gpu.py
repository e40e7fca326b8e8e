"""The LPIPS engine against the fp64 restatement (tests/lpips_refs.py) and its three bitwise properties."""
import functools

import pytest
import torch

from tests import lpips_refs as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
CASES = [(net, dt, size) for net in R.NETS for dt in DTYPES for size in R.SIZES]
IDS = [f"{net}-{dt}-{size[0]}x{size[1]}" for net, dt, size in CASES]


@functools.lru_cache(maxsize=None)
def model(net, dt):
    from sliders_conceptmod_amd import model_util
    return model_util.load_lpips(f"synthetic://{net}").to("cuda", DTYPES[dt])


def bits(t):
    return t.detach().cpu().view(torch.int32)


@pytest.mark.parametrize("net,dt,size", CASES, ids=IDS)
def test_taps_per_layer_and_distances_against_fp64(net, dt, size):
    a, b = R.pairs_u8(size)
    ref_taps, ref_per, ref_dist = R.reference(net, size)
    bars = R.bars(net, size, DTYPES[dt])
    eng = model(net, dt)._engine(a.shape[0], *size)
    for form in ("uint8", "fp32"):
        if form == "uint8":
            dist, per, feats = eng.distance(rgb8_a=a, rgb8_b=b, want_per_layer=True, want_feats=True)
        else:
            dist, per, feats = eng.distance(img_a=R.to_input(a).float(), img_b=R.to_input(b).float(),
                                            want_per_layer=True, want_feats=True)
        dist, per = dist.cpu().double(), per.cpu().double()
        figures = []
        for t in range(5):
            got = feats[t].permute(0, 3, 1, 2)
            assert tuple(got.shape) == tuple(ref_taps[t].shape)
            figures.append((f"tap {t}", R.rel(got, ref_taps[t]), bars["taps"][t]))
            figures.append((f"per_layer {t}", R.rel(per[:, t], ref_per[:, t]), bars["per_layer"][t]))
        figures.append(("batch of distances", R.rel(dist, ref_dist), bars["batch"]))
        figures.append(("largest pair error (absolute)", (dist - ref_dist).abs().max().item(), bars["pair_abs"]))
        for what, got, bar in figures:
            print(f"{net} {dt} {size} {form}: {what}: {got:.3e} (bar {bar:.3e})")
        for what, got, bar in figures:
            assert got <= bar, (form, what, got, bar)
        assert torch.allclose(per.sum(1), dist, rtol=1e-6, atol=0)  # dist is the fp32 sum of the five terms


@pytest.mark.parametrize("net,dt,size", CASES, ids=IDS)
def test_bitwise_properties(net, dt, size):
    a, b = R.pairs_u8(size)
    n = a.shape[0]
    m = model(net, dt)
    full = bits(m.distance(a, b))
    assert torch.equal(bits(m.distance(a, b)), full)  # two runs, the same bits
    # a pair alone, and at another position of another batch
    roll = [(j + 2) % n for j in range(n)]
    rolled = bits(m.distance(a[roll], b[roll]))
    sub = [5, 0, 3, 1]
    part = bits(m.distance(a[sub], b[sub]))
    for j in range(n):
        assert torch.equal(bits(m.distance(a[j:j + 1], b[j:j + 1])), full[j:j + 1]), j
        assert rolled[roll.index(j)] == full[j], j
    for pos, j in enumerate(sub):
        assert part[pos] == full[j], j
    # the float form too: alone against the batch
    fa, fb = R.to_input(a).float().cuda(), R.to_input(b).float().cuda()
    ffull = bits(m(fa, fb))
    assert tuple(m(fa, fb).shape) == (n, 1, 1, 1)
    for j in (0, n - 1):
        assert torch.equal(bits(m(fa[j:j + 1], fb[j:j + 1])), ffull[j:j + 1]), j
    # d(a, b) == d(b, a), d(a, a) == 0.0
    assert torch.equal(bits(m.distance(b, a)), full)
    assert torch.equal(bits(m(fb, fa)), ffull)
    assert torch.equal(m.distance(a, a).cpu(), torch.zeros(n))
    assert torch.equal(m.distance(b, b).cpu(), torch.zeros(n))
    assert (m.distance(a, b) > 0).all()
    # normalize=True takes [0, 1] images
    assert torch.allclose(m((fa + 1) / 2, (fb + 1) / 2, normalize=True), m(fa, fb), rtol=1e-3, atol=1e-7)


def test_create_refuses_30x30():
    from sliders_conceptmod_amd import _native
    m = model("tiny_alex", "fp16")
    z = torch.zeros(1, 30, 30, 3, dtype=torch.uint8)
    with pytest.raises(_native.SmiError, match="smaller than 31 x 31"):
        m.distance(z, z)
    z = torch.zeros(1, 31, 31, 3, dtype=torch.uint8)
    assert m.distance(z, z).item() == 0.0


@pytest.mark.parametrize("net", R.NETS)
def test_engine_for_eight_pairs_scores_fewer(net):
    from sliders_conceptmod_amd import _native
    size = (64, 64)
    a6, b6 = R.pairs_u8(size)
    a, b = torch.cat([a6, b6[:2]]), torch.cat([b6, a6[1:3]])  # eight pairs
    m = model(net, "fp16")
    alone = torch.cat([bits(m.distance(a[j:j + 1], b[j:j + 1])) for j in range(8)])
    state = {k: v.detach() for k, v in m.state_dict().items()}
    eng = m._new_engine(state, 8, *size)
    try:
        for n in (1, 5, 8):
            dist, per, feats = eng.distance(rgb8_a=a[:n], rgb8_b=b[:n])
            assert per is None and feats is None
            assert torch.equal(bits(dist), alone[:n]), n
        with pytest.raises(_native.SmiError, match=r"outside \[1, 8\]"):
            eng.distance(rgb8_a=torch.cat([a, a[:1]]), rgb8_b=torch.cat([b, b[:1]]))
        with pytest.raises(_native.SmiError, match="exactly one form"):
            eng.distance(rgb8_a=a[:1], rgb8_b=b[:1], img_a=torch.zeros(1, 3, 64, 64), img_b=torch.zeros(1, 3, 64, 64))
    finally:
        eng.close()
