"""CLIP image tower, host side: the engine's dry runs and config refusals, the host preprocessing against
`transformers.CLIPImageProcessor`, the tolerance rule of clip_vision_refs against deliberately wrong towers, and the
clip_score command's table logic with a stub scorer.  No GPU."""
import dataclasses
import math
import os

import numpy as np
import pytest
import torch

import clip_vision_refs as R


# ---- 1. dry runs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny_p8", "tiny_p14", "vit_b32", "vit_l14"])
@pytest.mark.parametrize("batch", [1, 64])
def test_workspace_bytes_dry_run(which, batch):
    from sliders_conceptmod_amd import _native
    small = _native.clip_vision_workspace_bytes(R.our_vision_config(which), torch.float16, batch)
    assert small > 0
    if batch == 64:
        assert small > _native.clip_vision_workspace_bytes(R.our_vision_config(which), torch.float16, 1)


@pytest.mark.parametrize("change,message", [
    (dict(image_size=30), "image_size 30 is not a multiple of patch_size 8"),
    (dict(hidden_size=96, num_attention_heads=4), "hidden_size 96 must be a multiple of 64 and <= 2048"),
    (dict(hidden_size=4096, num_attention_heads=64), "hidden_size 4096 must be a multiple of 64 and <= 2048"),
    (dict(num_attention_heads=16), "head_dim .* must be a multiple of 8"),
    (dict(intermediate_size=100), "intermediate_size 100 must be a multiple of 64"),
    (dict(projection_dim=20), "projection_dim 20 must be a multiple of 8"),
])
def test_config_refusals_name_the_limit(change, message):
    from sliders_conceptmod_amd import _native
    cfg = dataclasses.replace(R.our_vision_config("tiny_p8"), **change)
    with pytest.raises(_native.SmiError, match=message):
        _native.clip_vision_workspace_bytes(cfg, torch.float16, 1)


def test_new_symbols_are_exported():
    from sliders_conceptmod_amd import _native
    for s in ("smi_clip_vision_workspace_bytes", "smi_clip_vision_create", "smi_clip_vision_encode", "smi_clip_logits"):
        assert s in _native.EXPORTED_SYMBOLS and hasattr(_native.lib(), s)


def test_containers_load_transformers_state_dicts_strictly():
    import sliders_conceptmod_amd.clip as PC
    hf = R.hf_clip("tiny_p8")
    m = PC.CLIPModel(R.our_text_config("tiny_p8"), R.our_vision_config("tiny_p8"))
    m.load_state_dict(hf.state_dict(), strict=True)
    assert set(m.state_dict()) == set(hf.state_dict())
    assert abs(float(m.logit_scale.detach()) - math.log(100.0)) < 1e-6
    # each tower sees only its own keys
    assert all(k.startswith(("vision_model.", "visual_projection.")) for k in m.vision.state_dict())
    assert all(k.startswith(("text_model.", "text_projection.")) for k in m.text.state_dict())
    assert m.vision.vision_model is m.vision_model and m.text.text_model is m.text_model
    v = PC.CLIPVisionModelWithProjection(R.our_vision_config("tiny_p8"))
    v.load_state_dict(R.hf_vision("tiny_p8").state_dict(), strict=True)
    with pytest.raises(Exception, match="HIP engine"):  # no CPU forward
        v(torch.zeros(1, 3, 32, 32))


def test_pad_ids_pads_with_eos():
    import sliders_conceptmod_amd.clip as PC
    m = PC.CLIPModel(R.our_text_config("tiny_p8"), R.our_vision_config("tiny_p8"))
    ids = R.prompt_ids("tiny_p8")
    p = m.pad_ids(ids)
    assert p.shape == (2, 77) and torch.equal(p[:, :12], ids) and bool((p[:, 12:] == 999).all())


# ---- 2. host preprocessing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(96, 80), (80, 96), (64, 64), (32, 32), (100, 37), (45, 33)])
def test_preprocess_equals_clip_image_processor(w, h):
    transformers = pytest.importorskip("transformers")
    from PIL import Image
    from sliders_conceptmod_amd.clip import clip_image_preprocess
    rs = np.random.RandomState(w * 1000 + h)
    im = Image.fromarray(rs.randint(0, 256, (h, w, 3)).astype(np.uint8))
    proc = transformers.CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    px = np.asarray(proc(images=im, return_tensors="np")["pixel_values"][0], dtype=np.float64)  # [3, 32, 32]
    mean, std = np.array(proc.image_mean).reshape(3, 1, 1), np.array(proc.image_std).reshape(3, 1, 1)
    back = (px * std + mean) * 255.0
    err = float(np.abs(back - np.rint(back)).max())
    print(f"{w}x{h}: de-normalised pixel_values are {err:.1e} from integers")
    assert err < 1e-3  # float32 normalisation noise (3e-5 measured): the processor's pixels ARE uint8 values
    want = np.rint(back).astype(np.uint8).transpose(1, 2, 0)
    got = clip_image_preprocess(im, 32)
    assert got.dtype == np.uint8 and got.shape == (32, 32, 3)
    assert np.array_equal(got, want)


def test_preprocess_converts_to_rgb():
    from PIL import Image
    from sliders_conceptmod_amd.clip import clip_image_preprocess
    g = Image.fromarray(np.arange(32 * 32, dtype=np.uint8).reshape(32, 32), mode="L")
    out = clip_image_preprocess(g, 32)
    assert out.shape == (32, 32, 3) and np.array_equal(out[..., 0], out[..., 2])


# ---- 3. the tolerance rule rejects wrong towers -----------------------------------------------------------------
@pytest.mark.parametrize("which", ["tiny_p8", "tiny_p14"])
def test_bar_rejects_mutated_towers(which):
    """fp16: 2 x floor is below every mutation's distance, the activation swap (the smallest) included.  bf16: every
    mutation but the activation swap -- bf16's own rounding is as large as quick_gelu vs gelu on these towers, so the
    fp16 run is what checks the activation.  That is a limit of bf16, not of the rule."""
    pytest.importorskip("transformers")
    ref = R.vision_reference(which)[0]
    bar16, bar_bf = R.vision_bars(which, torch.float16)[0], R.vision_bars(which, torch.bfloat16)[0]
    print(f"{which}: image_embeds bar fp16 {bar16:.2e}, bf16 {bar_bf:.2e}")
    for mutation in R.MUTATIONS:
        d = R.rel(R.mutated_vision_embeds(which, mutation), ref)
        print(f"  {mutation}: {d:.2e}")
        assert d > bar16, (mutation, d, bar16)
        if mutation != "act_swapped":
            assert d > bar_bf, (mutation, d, bar_bf)
    assert R.rel(ref, ref) == 0.0


# ---- 4. command logic with a stub scorer ------------------------------------------------------------------------
def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def _sweep(tmp_path):
    root = str(tmp_path / "images")
    for folder, files in {"-1": ["3_0.png", "3_1.png", "10_0.png", "7_0.png"], "0": ["10_0.png", "3_10.png", "3_2.png"],
                          "half": ["3_0.png"], "all": ["3_0.png"]}.items():
        for f in files:
            _touch(os.path.join(root, folder, f))
    _touch(os.path.join(root, "old_scores.csv"))
    return root


def _stub(calls):
    def scorer(paths):
        calls.append(list(paths))
        return [float(os.path.basename(p).split(".")[0].replace("_", ".")) for p in paths]  # "3_10.png" -> 3.10
    return scorer


def test_score_sweep_table_logic(tmp_path):
    pd = pytest.importorskip("pandas")
    from sliders_conceptmod_amd import clip_score as CS
    root = _sweep(tmp_path)
    # the index (0, 1, 2) differs from the case numbers (10, 3, 5); case 7 is not in the CSV, case 5 has no images
    df = pd.DataFrame({"case_number": [10, 3, 5], "prompt": ["a", "b", "c"]})
    calls, lines = [], []
    out = CS.score_sweep(root, df, _stub(calls), log=lines.append)
    assert [c for c in out.columns if c.startswith("clip_")] == ["clip_-1", "clip_0", "clip_0.5"]  # sorted, no `all`
    assert len(out) == 3  # no row was added under an index label
    names = [[os.path.basename(p) for p in c] for c in calls]
    assert names[0] == ["3_0.png", "3_1.png", "10_0.png"]            # natural order, case 7 skipped
    assert names[1] == ["3_2.png", "3_10.png", "10_0.png"]           # 3_2 before 3_10
    row = {c: out[out.case_number == c].iloc[0] for c in (10, 3, 5)}
    assert row[3]["clip_-1"] == pytest.approx((3.0 + 3.1) / 2) and row[10]["clip_-1"] == pytest.approx(10.0)
    assert row[3]["clip_0"] == pytest.approx((3.2 + 3.10) / 2)
    assert row[3]["clip_0.5"] == pytest.approx(3.0) and math.isnan(row[10]["clip_0.5"])
    assert all(math.isnan(row[5][c]) for c in ("clip_-1", "clip_0", "clip_0.5"))  # a case without images
    assert sum(l.startswith("Mean CLIP score:") for l in lines) == 3


def test_score_sweep_case_bounds(tmp_path):
    pd = pytest.importorskip("pandas")
    from sliders_conceptmod_amd import clip_score as CS
    root = _sweep(tmp_path)
    df = pd.DataFrame({"case_number": [10, 3, 5]})
    out = CS.score_sweep(root, df, _stub([]), from_case=4, till_case=10, log=lambda *_: None)
    assert math.isnan(out[out.case_number == 3].iloc[0]["clip_-1"])
    assert out[out.case_number == 10].iloc[0]["clip_-1"] == pytest.approx(10.0)
    out = CS.score_sweep(root, pd.DataFrame({"case_number": [10, 3, 5]}), _stub([]), till_case=3, log=lambda *_: None)
    assert math.isnan(out[out.case_number == 10].iloc[0]["clip_-1"])
    assert out[out.case_number == 3].iloc[0]["clip_0.5"] == pytest.approx(3.0)


def test_unreadable_image_raises_naming_the_file(tmp_path):
    from sliders_conceptmod_amd import clip_score as CS
    bad = str(tmp_path / "3_0.png")
    open(bad, "wb").write(b"not a png")
    scorer = CS.ClipScorer.__new__(CS.ClipScorer)
    scorer.size, scorer.batch_size = 32, 4
    with pytest.raises(RuntimeError, match="3_0.png"):
        scorer([bad])


def test_load_clip_names():
    from sliders_conceptmod_amd import model_util
    model, tok, size = model_util.load_clip("synthetic://tiny_clip")
    assert size == 32 and float(model.logit_scale.detach()) == pytest.approx(math.log(100.0))
    ids = tok(["An old person", "an old person smiling"]).input_ids
    assert ids.shape == (2, 6) and ids[0, 0] == 998 and ids[0, 4] == 999 and torch.equal(ids[0, 1:4], ids[1, 1:4])
    with pytest.raises(ValueError, match="no network"):
        model_util.load_clip("openai/clip-vit-base-patch32")
