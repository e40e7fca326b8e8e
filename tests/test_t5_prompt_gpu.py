"""The native T5 tower where a user meets it, on a real MI355X: model_util.NativeT5Tower through encode_prompts_flux and
encode_prompts_sd3 (shapes, the cast to the pipeline's dtype, the prompt cache), `generate_images --base flux --t5_backend
native` against the `--no_t5` run, and one iteration of train_lora_flux / train_lora_sd3 on the tiny models with the flag."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T5_TOKENS, RES = 3, 64


def settings():
    from sliders_conceptmod_amd import prompt_util
    return prompt_util.PromptSettings(target="person", positive="person, very old", negative="person, very young",
                                      unconditional="", neutral="person", action="enhance", guidance_scale=2.0,
                                      resolution=RES, batch_size=1)


def test_tower_through_the_prompt_encoders():
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import model_util as MU, train_util as TU
    toks, encs, _model, _s = MU.load_models_flux("synthetic://tiny_flux", t5_backend="native")
    tower = encs[1]
    with pytest.warns(UserWarning, match="float16 requested"):
        for te in encs:
            te.to(DEV, torch.float16)  # the loop the commands run; the tower stays bf16
    assert tower.dtype == torch.bfloat16 and tower.device.type == "cuda"
    calls = []
    encode = tower.encode
    tower.encode = lambda p, n: (calls.append((p, n)), encode(p, n))[1]
    emb, pooled = TU.encode_prompts_flux(None, toks, encs, "a photo of a person", 2, 7, 64)
    assert tuple(emb.shape) == (2, 7, 64) and emb.dtype == pooled.dtype == torch.float16 and emb.device.type == "cuda"
    assert torch.isfinite(emb).all() and float(emb.float().abs().max()) > 0 and torch.equal(emb[0], emb[1])
    again, _ = TU.encode_prompts_flux(None, toks, encs, "a photo of a person", 1, 7, 64)
    other, _ = TU.encode_prompts_flux(None, toks, encs, "a photo of a dog", 1, 7, 64)
    assert calls == [("a photo of a person", 7), ("a photo of a dog", 7)], "the second call of a prompt is a cache hit"
    assert torch.equal(again[0], emb[0]) and not torch.equal(other[0], emb[0])
    with pytest.raises(ValueError, match="64 wide"):
        TU.encode_prompts_flux(None, toks, encs, "a photo of a person", 1, 7, 128)

    toks3, encs3, model3, _s = MU.load_models_sd3("synthetic://tiny_sd3", t5_backend="native")
    for te in encs3:
        te.to(DEV, torch.float16)
    jd = model3.config.joint_attention_dim
    e3, p3 = TU.encode_prompts_sd3(None, toks3, encs3, "a photo of a person", 2, 5, jd)
    e2, p2 = TU.encode_prompts_sd3(None, toks3[:2], encs3[:2], "a photo of a person", 2, 5, jd)
    assert tuple(e3.shape) == tuple(e2.shape) == (2, 77 + 5, jd) and e3.dtype == e2.dtype
    assert torch.equal(e3[:, :77], e2[:, :77]) and torch.equal(p3, p2) and not bool(e2[:, 77:].any())
    assert torch.isfinite(e3).all() and bool(e3[:, 77:].any()), "the T5 rows stand where the zero rows were"


def test_generate_images_flux_with_the_native_tower(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    import numpy as np
    from PIL import Image
    from sliders_conceptmod_amd import generate_images as G
    prompts = tmp_path / "prompts.csv"
    prompts.write_text("prompt,evaluation_seed,case_number\na photo of a person,11,0\n")
    common = ["--scales=0", "--prompts_path", str(prompts), "--pretrained_model", "synthetic://tiny_flux", "--base", "flux",
              "--image_size", "64", "--num_samples", "1", "--ddim_steps", "2", "--t5_tokens", str(T5_TOKENS)]
    G.main(common + ["--save_path", str(tmp_path / "native"), "--t5_backend", "native"])
    G.main(common + ["--save_path", str(tmp_path / "zero"), "--no_t5"])
    a, b = (tmp_path / d / "frozen" / "all" / "0_0.png" for d in ("native", "zero"))
    assert a.exists() and b.exists()
    ia, ib = (np.asarray(Image.open(p)) for p in (a, b))
    assert ia.shape == ib.shape and (ia != ib).any(), "the T5 rows reach the image"


def test_train_lora_flux_one_iteration(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import config_util, train_lora_flux as T
    cfg = config_util.load_config_from_yaml("data/config-flux.yaml")
    cfg.pretrained_model.name_or_path = "synthetic://tiny_flux"
    cfg.train.precision, cfg.save.precision = "float16", "float16"
    cfg.train.iterations, cfg.train.cfg = 1, 3.5
    cfg.save.name, cfg.save.path, cfg.save.per_steps = "t5", str(tmp_path / "models"), 100
    torch.manual_seed(1)
    with pytest.warns(UserWarning, match="float16 requested"):
        net = T.train(cfg, [settings()], torch.device(DEV), save_file=False, t5_tokens=T5_TOKENS, t5_backend="native")
    assert isinstance(net, dict) and len(net) > 0 and all(torch.isfinite(v).all() for v in net.values())


def test_train_lora_sd3_one_iteration(tmp_path):
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from sliders_conceptmod_amd import config_util, train_lora_sd3 as T
    cfg = config_util.load_config_from_yaml("data/config-sd3.yaml")
    cfg.pretrained_model.name_or_path = "synthetic://tiny_sd3"
    cfg.train.precision, cfg.save.precision = "float16", "float16"
    cfg.train.iterations, cfg.train.max_denoising_steps, cfg.train.cfg = 1, 4, 3.0
    cfg.save.name, cfg.save.path, cfg.save.per_steps = "t5", str(tmp_path / "models"), 100
    torch.manual_seed(1)
    with pytest.warns(UserWarning, match="float16 requested"):
        net = T.train(cfg, [settings()], torch.device(DEV), save_file=False, t5_tokens=T5_TOKENS, t5_backend="native")
    assert isinstance(net, dict) and len(net) > 0 and all(torch.isfinite(v).all() for v in net.values())
