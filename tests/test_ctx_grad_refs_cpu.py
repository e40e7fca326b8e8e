"""The d_ctx bar of tests/test_ctx_grad_gpu.py can see the mistakes an engine can make: a cross-attention block whose term
is missing, a per-sample loss scale applied wrongly, a K or V half that is dropped.  Everything here runs on the CPU oracle
(tests/ctx_grad_refs.py); the "engine" is the oracle's own gradient with one such mistake put in."""
import pytest
import torch

from tests import ctx_grad_refs as R

MODELS = ["tiny_sd1x", "tiny_sdxl"]
N_BLOCKS = {"tiny_sd1x": 16, "tiny_sdxl": 28}
BF16_BLIND = {"tiny_sd1x": 1, "tiny_sdxl": 2}  # blocks whose loss the wider bf16 bar cannot see (the reference gives these)


@pytest.fixture(scope="module", params=MODELS)
def split(request):
    model = request.param
    parts, full = R.block_contributions(model)
    e_q = {dt: R.rel(R.plain_refs(model, dt), R.plain_refs(model)) for dt in (torch.float16, torch.bfloat16)}
    return model, parts, full, e_q


def test_block_terms_sum_to_the_full_gradient(split):
    model, parts, full, _ = split
    assert len(parts) == N_BLOCKS[model] and all(set(p) == {"k", "v"} for p in parts.values())
    total = sum(p["k"].double() + p["v"].double() for p in parts.values())  # the sum itself adds no fp32 rounding
    assert torch.equal(full, R.plain_refs(model))  # the hooks change nothing
    err = R.rel(total, full)
    print(f"{model}: sum of {len(parts)} block terms vs full d_ctx: {err:.2e}")
    assert err < 1.5e-7


def test_a_missing_block_exceeds_the_bar(split):
    model, parts, full, e_q = split
    share = {b: ((p["k"] + p["v"]).double().norm() / full.double().norm()).item() for b, p in parts.items()}
    for b, s in sorted(share.items(), key=lambda kv: kv[1]):
        print(f"{model}: {b:55s} {s:.3e}")
    bar16, barb = R.bar(e_q[torch.float16]), R.bar(e_q[torch.bfloat16])
    print(f"{model}: e_q fp16 {e_q[torch.float16]:.2e} (bar {bar16:.2e})  bf16 {e_q[torch.bfloat16]:.2e} (bar {barb:.2e})")
    for b, s in share.items():
        assert s > bar16, f"dropping {b} moves d_ctx by {s:.2e}, inside the fp16 bar {bar16:.2e}"
    blind = [b for b, s in share.items() if s <= barb]
    assert len(blind) <= BF16_BLIND[model], f"bf16 bar {barb:.2e} cannot see {blind}"
    first = next(iter(parts))  # named_modules order: the first cross-attention of the net (its q carries no gradient)
    print(f"{model}: first cross-attention {first}: {share[first]:.2e}")
    if model == "tiny_sd1x":  # there it carries two fifths of the gradient: an engine that skips the dQ-free backward fails
        assert share[first] > 0.3, f"{first}: {share[first]:.2e}"


def test_scale_and_half_mutations_exceed_the_bar(split):
    """One sample off by a factor of two and a dropped K or V half.  Sample 1 carries 8 x the output gradient, so a wrong
    sample 0 moves the WHOLE-tensor distance by only ~0.06: the fp16 bar sees it, the bf16 bar of the tiny SD-XL net
    (0.068) does not -- which is why the GPU test also holds every sample to the bar by itself, checked here too."""
    model, parts, full, e_q = split
    bar16, barb = R.bar(e_q[torch.float16]), R.bar(e_q[torch.bfloat16])
    qb, ref = R.plain_refs(model, torch.bfloat16), R.plain_refs(model)
    for s in range(R.N):
        bar_s = R.bar(R.rel(qb[s], ref[s]))  # the per-sample bf16 bar
        for f in (2.0, 0.5):
            wrong = full.clone()
            wrong[s] *= f
            assert R.rel(wrong, full) > bar16, f"sample {s} x {f} passes the fp16 bar"
            assert R.rel(wrong[s], full[s]) > bar_s, f"sample {s} x {f} passes its own bf16 bar {bar_s:.2e}"
    for half in ("k", "v"):
        wrong = full - sum(p[half] for p in parts.values())
        d = R.rel(wrong, full)
        print(f"{model}: without every {half} term: {d:.2e}")
        assert d > barb
