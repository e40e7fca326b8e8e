"""CLIP image tower, similarity head and joint model on the HIP engine against transformers on the CPU
(clip_vision_refs: references in fp64 / fp32, bars = 2 x transformers' own 16-bit distance from them)."""
import math

import pytest
import torch

import clip_vision_refs as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def native_vision(which, dtype, seed=3):
    import sliders_conceptmod_amd.clip as PC
    m = PC.CLIPVisionModelWithProjection(R.our_vision_config(which))
    m.load_state_dict(R.hf_vision(which, seed).state_dict(), strict=True)
    return m.to("cuda", dtype)


def native_clip(which, dtype):
    import sliders_conceptmod_amd.clip as PC
    m = PC.CLIPModel(R.our_text_config(which), R.our_vision_config(which))
    m.load_state_dict(R.hf_clip(which).state_dict(), strict=True)
    return m.to("cuda", dtype)


# ---- 1 + 2. tower against transformers, both entries -------------------------------------------------------------
CASES = [(w, d) for w in ("tiny_p8", "tiny_p14", "vit_b32") for d in DTYPES] + [("vit_l14", torch.float16)]


@pytest.mark.parametrize("which,dtype", CASES, ids=[f"{w}-{str(d).split('.')[1]}" for w, d in CASES])
def test_tower_matches_transformers(which, dtype):
    """Token counts 17 / 5 / 50 / 257 (no tile multiple), K = 192 and 3072 unpadded and 588 -> 640 padded, head_dim 16
    and 64, both activations.  bf16 cannot tell quick_gelu from gelu on these towers (test_bar_rejects_mutated_towers);
    the fp16 cases check the activation."""
    n = 1 if which == "vit_l14" else 3
    ref_emb, ref_last = R.vision_reference(which, n)
    bar_emb, bar_last = R.vision_bars(which, dtype, n)
    m = native_vision(which, dtype)
    u8 = R.images_u8(which, n)
    out = m(R.normalise(u8).cuda())
    assert out.image_embeds.shape == ref_emb.shape and out.last_hidden_state.shape == ref_last.shape
    e_emb, e_last = R.rel(out.image_embeds, ref_emb), R.rel(out.last_hidden_state, ref_last)
    print(f"{which} {dtype} pixel_values: image_embeds {e_emb:.2e} (bar {bar_emb:.2e}), last_hidden_state {e_last:.2e} "
          f"(bar {bar_last:.2e})")
    assert e_emb <= bar_emb and e_last <= bar_last, (e_emb, bar_emb, e_last, bar_last)
    # the uint8 entry normalises on the device: same bar, no bit equality with the float entry (FMA contraction)
    out8 = m.encode_rgb8(u8.cuda(), output_last_hidden_state=True)
    e8, e8_last = R.rel(out8.image_embeds, ref_emb), R.rel(out8.last_hidden_state, ref_last)
    print(f"{which} {dtype} uint8: image_embeds {e8:.2e}, last_hidden_state {e8_last:.2e}")
    assert e8 <= bar_emb and e8_last <= bar_last, (e8, bar_emb, e8_last, bar_last)
    assert m.encode_rgb8(u8.cuda()).last_hidden_state is None


def test_wrong_engine_kind_and_shapes_are_refused():
    from sliders_conceptmod_amd import _native
    m = native_vision("tiny_p8", torch.float16)
    u8 = R.images_u8("tiny_p8").cuda()
    m.encode_rgb8(u8)
    eng = next(iter(m._engines.values()))
    ids = torch.zeros((1, 77), dtype=torch.int32, device="cuda")
    out = torch.empty((1, 77, 64), dtype=torch.float16, device="cuda")
    rc = _native.lib().smi_clip_encode(eng.handle, 1, _native.ptr(ids), None, _native.ptr(out), None, None)
    assert rc != 0 and b"not a CLIP text engine" in _native.lib().smi_last_error()
    with pytest.raises(_native.SmiError, match="uint8"):
        m.encode_rgb8(u8[:, :16])
    with pytest.raises(_native.SmiError, match="exactly one"):
        eng.encode()
    clip = native_clip("tiny_p8", torch.float16)
    clip.get_text_features(R.prompt_ids("tiny_p8").cuda())
    teng = next(iter(clip.text._engines.values()))
    emb = torch.empty((3, 32), dtype=torch.float16, device="cuda")
    rc = _native.lib().smi_clip_vision_encode(teng.handle, 3, _native.ptr(u8), None, None, _native.ptr(emb))
    assert rc != 0 and b"not a CLIP vision engine" in _native.lib().smi_last_error()


# ---- 3. batch rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny_p8", "vit_b32"])
def test_an_image_encodes_to_the_same_bits_alone_or_in_a_batch(which):
    m = native_vision(which, torch.float16)
    u8 = R.images_u8(which).cuda()
    both = m.encode_rgb8(u8, output_last_hidden_state=True)
    for i in range(3):
        one = m.encode_rgb8(u8[i:i + 1], output_last_hidden_state=True)
        assert torch.equal(one.image_embeds[0], both.image_embeds[i])
        assert torch.equal(one.last_hidden_state[0], both.last_hidden_state[i])
    assert not torch.equal(both.image_embeds[0], both.image_embeds[1])


# ---- 4. similarity head ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ni,nt,dim", [(3, 2, 32), (3, 2, 40), (5, 1, 512)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_logits_against_fp64(ni, nt, dim, dtype):
    from sliders_conceptmod_amd import _native
    g = torch.Generator().manual_seed(ni * 100 + dim)
    a, b = torch.randn(ni, dim, generator=g).to(dtype), torch.randn(nt, dim, generator=g).to(dtype)
    scale = math.log(100.0)
    got = _native.clip_logits(a.cuda(), b.cuda(), scale).cpu().double()
    ad, bd = a.double(), b.double()
    want = math.exp(scale) * (ad / ad.norm(dim=1, keepdim=True)) @ (bd / bd.norm(dim=1, keepdim=True)).t()
    bound = 2 * (dim + 8) * 2.0 ** -24 * math.exp(scale)  # worst case of three fp32 reductions of `dim` terms
    err = float((got - want).abs().max())
    print(f"clip_logits {ni}x{nt}x{dim} {dtype}: max |d| {err:.2e} (bound {bound:.2e})")
    assert got.shape == (ni, nt) and err <= bound
    with pytest.raises(_native.SmiError, match="multiple of 8"):
        _native.clip_logits(a[:, :dim - 4].contiguous().cuda(), b[:, :dim - 4].contiguous().cuda(), scale)


# ---- 5. joint model --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny_p8", "vit_b32"])
def test_clip_model_end_to_end(which):
    dtype = torch.float16
    ref_ie, ref_te, ref_logits = R.clip_reference(which)
    bar_i, bar_t = R.clip_bars(which, dtype)
    m = native_clip(which, dtype)
    scale = float(m.logit_scale.detach())
    assert abs(scale - math.log(100.0)) < 1e-3
    ids = R.prompt_ids(which).cuda()          # 2 prompts of 12 and 7 tokens
    px = R.normalise(R.images_u8(which)).cuda()
    ie, te = m.get_image_features(px), m.get_text_features(ids)
    e_i, e_t = R.rel(ie, ref_ie), R.rel(te, ref_te)
    print(f"{which}: image_embeds {e_i:.2e} (bar {bar_i:.2e}), text_embeds {e_t:.2e} (bar {bar_t:.2e})")
    assert e_i <= bar_i and e_t <= bar_t
    out = m(ids, px)
    bound = 2 * math.exp(scale) * (bar_i + bar_t)  # what the two embedding bars allow for unit vectors; loose on purpose
    err = float((out.logits_per_image.cpu().double() - ref_logits.double()).abs().max())
    print(f"{which}: max |d logit| {err:.2e} (bound {bound:.2e})")
    assert out.logits_per_image.shape == (3, 2) and err <= bound
    assert torch.equal(out.logits_per_text, out.logits_per_image.t())
    unit = out.image_embeds.float().norm(dim=-1)
    assert torch.allclose(unit, torch.ones_like(unit), atol=2e-3)
    # ids of length 12 and the same ids padded to 77 with EOS: the same bits
    padded = torch.cat([ids, ids.new_full((2, 77 - ids.shape[1]), R.TEXT[which][5])], dim=1)
    assert torch.equal(m.get_text_features(padded), te)
    assert torch.equal(m(padded, px).logits_per_image, out.logits_per_image)


# ---- 6. engine lifetime ----------------------------------------------------------------------------------------
def test_load_state_dict_drops_the_engines():
    m = native_clip("tiny_p8", torch.float16)
    ids, u8 = R.prompt_ids("tiny_p8").cuda(), R.images_u8("tiny_p8").cuda()
    first = m(ids, rgb8=u8)
    old = [next(iter(t._engines.values())) for t in m.towers]
    new_state = R.seeded(R.build_uninitialised(type(R.hf_clip("tiny_p8")), R.hf_clip("tiny_p8").config), 6).state_dict()
    m.load_state_dict(new_state)
    assert all(t._engines == {} for t in m.towers) and all(e.handle is None for e in old)
    again = m(ids, rgb8=u8)
    import sliders_conceptmod_amd.clip as PC
    fresh = PC.CLIPModel(R.our_text_config("tiny_p8"), R.our_vision_config("tiny_p8"))
    fresh.load_state_dict(new_state)
    want = fresh.to("cuda", torch.float16)(ids, rgb8=u8)
    for a, w in ((again.logits_per_image, want.logits_per_image), (again.image_embeds, want.image_embeds),
                 (again.text_embeds, want.text_embeds)):
        assert torch.equal(a, w)
    assert not torch.equal(again.logits_per_image, first.logits_per_image)
    v = native_vision("tiny_p8", torch.float16)
    v.encode_rgb8(u8)
    eng = next(iter(v._engines.values()))
    v.load_state_dict(R.hf_vision("tiny_p8", 4).state_dict())
    assert v._engines == {} and eng.handle is None
    assert torch.equal(v.encode_rgb8(u8).image_embeds, native_vision("tiny_p8", torch.float16, 4).encode_rgb8(u8).image_embeds)
