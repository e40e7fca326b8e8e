"""The d(text_embeds) bar of tests/test_pooled_grad_gpu.py can see the mistakes an engine can make: a resnet whose
time_emb_proj term is missing or counted twice (a wrong power-of-two fold of one column block of the grouped gradient is a
multiple of that), a per-sample loss scale applied wrongly.  Everything here runs on the CPU oracle
(tests/pooled_grad_refs.py); the "engine" is the oracle's own gradient with one such mistake put in."""
import pytest
import torch

from tests import pooled_grad_refs as R

N_TERMS = 17  # resnets of the SD-XL topology: 2 + 2 + 2 down, 2 mid, 3 + 3 + 3 up
BF16_VISIBLE = 15


@pytest.fixture(scope="module")
def split():
    parts, full = R.term_contributions()
    ref = R.plain_refs()
    q = {dt: R.plain_refs(dt) for dt in (torch.float16, torch.bfloat16)}
    return parts, full, ref, q


def test_storage_rounding_floor(split):
    _, full, ref, q = split
    assert torch.equal(full, ref)  # the hooks change nothing
    assert ref.shape == (R.N, R.std_inputs()[2]["text_embeds"].shape[1]) and float(ref.abs().max()) > 0
    for dt, g in q.items():
        e_q = R.rel(g, ref)
        per = [R.rel(g[s], ref[s]) for s in range(R.N)]
        print(f"{dt}: e_q {e_q:.3e} (bar {R.bar(e_q):.3e})  per sample {' '.join(f'{p:.3e}' for p in per)}")
        assert 0 < e_q < 0.1
    assert R.rel(q[torch.float16], ref) < R.rel(q[torch.bfloat16], ref)


def test_terms_sum_to_the_full_gradient(split):
    parts, full, _, _ = split
    assert len(parts) == N_TERMS
    total = sum(p.double() for p in parts.values())  # the sum itself adds no fp32 rounding
    err = R.rel(total, full)
    print(f"sum of {len(parts)} time_emb_proj terms vs full d(text_embeds): {err:.2e}")
    assert err < 1e-6


def test_a_dropped_or_doubled_term_exceeds_the_bar(split):
    parts, full, ref, q = split
    share = {b: (p.double().norm() / full.double().norm()).item() for b, p in parts.items()}
    for b, s in sorted(share.items(), key=lambda kv: kv[1]):
        print(f"{b:30s} {s:.3e}")
    bar16, barb = R.bar(R.rel(q[torch.float16], ref)), R.bar(R.rel(q[torch.bfloat16], ref))
    print(f"bar fp16 {bar16:.2e}  bf16 {barb:.2e}")
    for b, p in parts.items():
        for wrong in (full - p, full + p):  # dropped; counted twice (= its block folded with a factor 2)
            d = R.rel(wrong, full)
            assert abs(d - share[b]) < 1e-5 * share[b] + 1e-9
            assert d > bar16, f"{b}: moves d(text_embeds) by {d:.2e}, inside the fp16 bar {bar16:.2e}"
    visible = [b for b, s in share.items() if s > barb]
    blind = sorted(b for b in share if b not in visible)
    print(f"bf16 bar cannot see {blind}")
    assert len(visible) == BF16_VISIBLE and all(b.startswith("mid_block.resnets.") for b in blind)


def test_a_wrong_sample_scale_exceeds_the_bar(split):
    """Sample 1 carries 8 x the output gradient: sample 0 off by a factor of two moves the whole tensor by about 0.1 and
    that sample by 1.0 -- both outside both bars, whole tensor and per sample."""
    _, full, ref, q = split
    for dt in (torch.float16, torch.bfloat16):
        whole = R.bar(R.rel(q[dt], ref))
        for s in range(R.N):
            bar_s = R.bar(R.rel(q[dt][s], ref[s]))
            for f in (2.0, 0.5):
                wrong = full.clone()
                wrong[s] *= f
                d, ds = R.rel(wrong, full), R.rel(wrong[s], full[s])
                print(f"{dt}: sample {s} x {f}: whole {d:.3e} (bar {whole:.2e})  sample {ds:.3e} (bar {bar_s:.2e})")
                assert d > whole and ds > bar_s
