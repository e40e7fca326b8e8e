"""Host side of the no-trigger text-encoder trainer, without a GPU: the LoRA network on a CLIP text tower (key names, flat
layout, RNG-order init), the loss against its float64 restatement, the command lines and their refusals, combine_loras."""
import math
import os

import pytest
import torch
import torch.nn as nn

import notrigger_refs as R


def tiny_encoder(act="quick_gelu", proj=None):
    import sliders_conceptmod_amd.clip as PC
    cfg = R.tiny_config(act, proj)
    enc = (PC.CLIPTextModelWithProjection if proj else PC.CLIPTextModel)(cfg)
    enc.load_state_dict(R.tiny_state(cfg))
    return cfg, enc


def network_on(enc, prefix="lora_te1", rank=4, seed=0):
    from sliders_conceptmod_amd.lora import CLIP_TARGET_REPLACE, LoRANetwork
    torch.manual_seed(seed)
    return LoRANetwork(enc, rank=rank, multiplier=1.0, alpha=1.0, target_replace=CLIP_TARGET_REPLACE, prefix=prefix,
                       train_method="full")


def test_key_names_are_the_references():
    """transformers-4 layout: the `text_model.` prefix is part of the module path."""
    cfg, enc = tiny_encoder()
    assert type(enc.text_model.encoder.layers[0].self_attn).__name__ == "CLIPAttention"
    net = network_on(enc)
    keys = list(net.state_dict().keys())
    assert keys[:3] == ["lora_te1_text_model_encoder_layers_0_self_attn_k_proj.alpha",
                        "lora_te1_text_model_encoder_layers_0_self_attn_k_proj.lora_down.weight",
                        "lora_te1_text_model_encoder_layers_0_self_attn_k_proj.lora_up.weight"]
    want = {f"lora_te1_text_model_encoder_layers_{i}_self_attn_{p}.{t}" for i in range(2) for p in ("k_proj", "v_proj", "q_proj", "out_proj")
            for t in ("alpha", "lora_down.weight", "lora_up.weight")}
    assert set(keys) == want
    assert all(k.startswith("lora_te2_") for k in network_on(tiny_encoder("gelu", 64)[1], prefix="lora_te2").state_dict())
    # the encoder's own state dict is untouched by the class rename
    assert "text_model.encoder.layers.1.self_attn.q_proj.weight" in enc.state_dict()


def test_flat_layout_puts_q_k_v_adjacent_in_engine_order():
    cfg, enc = tiny_encoder()
    net = network_on(enc)
    d, r = cfg.hidden_size, 4
    by = {l.target_path: l for l in net.unet_loras}
    for i in range(cfg.num_hidden_layers):
        b = f"text_model.encoder.layers.{i}.self_attn."
        q, k, v, o = (by[b + p] for p in ("q_proj", "k_proj", "v_proj", "out_proj"))
        assert (k.off_down, v.off_down, o.off_down) == (q.off_down + r * d, q.off_down + 2 * r * d, q.off_down + 3 * r * d)
        assert (k.off_up, v.off_up) == (q.off_up + d * r, q.off_up + 2 * d * r)
    offs = sorted(l.off_down for l in net.unet_loras)
    assert offs == [j * r * d for j in range(8)] and net._n_down == 8 * r * d
    # the engine accepts these sites (a host-only dry run) -- it refuses q | k | v that are not adjacent in its order
    from sliders_conceptmod_amd import _native
    assert _native.clip_lora_workspace_bytes(cfg, torch.float16, net.engine_sites(), 2) > 0
    bad = [dict(s) for s in net.engine_sites()]
    bad[0]["off_down"], bad[1]["off_down"] = bad[1]["off_down"], bad[0]["off_down"]
    with pytest.raises(_native.SmiError, match="adjacent"):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, bad, 2)


def test_unet_flat_layout_is_unchanged():
    """flat_order touches CLIP self_attn q / k / v only: a UNet network keeps the order of the walk."""
    from sliders_conceptmod_amd.lora import flat_order
    targets = [("a", "down.attn1.to_q", None), ("b", "down.attn1.to_k", None), ("c", "down.attn1.to_v", None), ("d", "down.attn1.to_out.0", None)]
    assert flat_order(targets) == [0, 1, 2, 3]
    clip = [("k", "l.0.self_attn.k_proj", None), ("v", "l.0.self_attn.v_proj", None), ("q", "l.0.self_attn.q_proj", None),
            ("o", "l.0.self_attn.out_proj", None), ("k1", "l.1.self_attn.k_proj", None), ("v1", "l.1.self_attn.v_proj", None),
            ("q1", "l.1.self_attn.q_proj", None), ("o1", "l.1.self_attn.out_proj", None)]
    assert flat_order(clip) == [2, 0, 1, 3, 6, 4, 5, 7]


def test_init_follows_the_walks_rng_order():
    """Seed-compatible with the reference: per visited child (k, v, q, out) an nn.Linear down, an nn.Linear up, then
    kaiming_uniform_(down, a=1) and zeros_(up) (lora.py:97-98, 123-124)."""
    cfg, enc = tiny_encoder()
    net = network_on(enc, seed=7)
    torch.manual_seed(7)
    d, r = cfg.hidden_size, 4
    for i in range(cfg.num_hidden_layers):
        for p in ("k_proj", "v_proj", "q_proj", "out_proj"):
            down, up = nn.Linear(d, r, bias=False), nn.Linear(r, d, bias=False)
            nn.init.kaiming_uniform_(down.weight, a=1)
            nn.init.zeros_(up.weight)
            sd = net.state_dict()
            name = f"lora_te1_text_model_encoder_layers_{i}_self_attn_{p}"
            assert torch.equal(sd[name + ".lora_down.weight"], down.weight.detach()), name
            assert float(sd[name + ".lora_up.weight"].abs().max()) == 0.0


def test_loss_equals_its_float64_restatement():
    from sliders_conceptmod_amd.notrigger import notrigger_loss
    g = torch.Generator().manual_seed(3)
    t = lambda: torch.randn((1, 77, 128), generator=g, dtype=torch.float64)
    pos, neg, neu = t(), t(), t()
    tp, tn = (neu + 0.1 * t()).requires_grad_(True), (neu + 0.1 * t()).requires_grad_(True)
    norm_p, norm_n = (pos - neu).norm(), (neg - neu).norm()
    total, logs = notrigger_loss(tp, tn, pos, neg, neu, norm_p, norm_n, 0.1)
    want, recon, cur = R.loss_ref(tp, tn, pos, neg, neu, norm_p, norm_n, 0.1)
    assert abs(total.item() - want.item()) <= 1e-12 * abs(want.item())
    assert abs(logs["reconstruction"].item() - recon.item()) <= 1e-12 and abs(logs["curriculum"].item() - cur.item()) <= 1e-12
    ga = torch.autograd.grad(total, [tp, tn])
    gb = torch.autograd.grad(want, [tp, tn])
    assert all(R.rel(a, b) < 1e-10 for a, b in zip(ga, gb))
    # the curriculum weights carry gradients (N:421-432 does not detach pperc / nperc): with w_p = w_n = 1/2 held constant
    # -- what detaching them would give here, since w_p pperc + w_n nperc = (pperc^2 + nperc^2) / (pperc + nperc) -- the
    # gradient of the curriculum term is a different one
    # (taken where pperc != nperc: at pperc = nperc the two gradients coincide)
    pp, nn_ = (pos - tp).norm() / norm_p, (neg - tn).norm() / (3 * norm_n)
    w_p, w_n = (pp / (pp + nn_)).detach(), (nn_ / (pp + nn_)).detach()
    g_detached = torch.autograd.grad(w_p * pp + w_n * nn_, [tp, tn], retain_graph=True)
    g_kept = torch.autograd.grad((pp * pp + nn_ * nn_) / (pp + nn_), [tp, tn])
    assert all(R.rel(a, b) > 1e-3 for a, b in zip(g_detached, g_kept))
    # one-sided: the plain MSE to the one target
    one, _ = notrigger_loss(tp, None, pos, None, neu, None, None, 0.1)
    assert abs(one.item() - ((pos - tp) ** 2).mean().item()) < 1e-15
    one, _ = notrigger_loss(None, tn, None, neg, neu, None, None, 0.1)
    assert abs(one.item() - ((neg - tn) ** 2).mean().item()) < 1e-15


def test_first_curriculum_loss_is_one_and_the_oracle_loop_learns():
    import json
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "notrigger_oracle.json")))
    assert gold["curriculum"][0] == 1.0 and len(gold["reconstruction"]) == gold["steps"] == 8
    assert min(gold["reconstruction"]) < 0.9 * gold["reconstruction"][0]
    # the file is what loop_ref records: its first three steps, run again here
    cfg, enc = tiny_encoder()
    net = network_on(enc, seed=gold["seed"], rank=gold["rank"])
    lora0, names = R.lora_from_network(net)
    hist = R.loop_ref({k: v.double() for k, v in R.tiny_state(cfg).items()}, cfg, lora0, names, gold["alpha"] / gold["rank"],
                      steps=3, lr=gold["lr"], lam=gold["lambda_similarity"])
    for i, (rec, cur) in enumerate(hist):
        assert abs(rec - gold["reconstruction"][i]) <= 1e-9 * rec and abs(cur - gold["curriculum"][i]) <= 1e-9, i


def test_cli_parsing_and_refusals():
    import sliders_conceptmod_amd.train_notrigger as T
    a = T.build_parser().parse_args(["--config_file", "data/config-notrigger-xl.yaml", "--alpha", "1.0", "--name", "smile",
                                     "--positive", "smiling", "happy", "--negative", "frowning", "--clip_index", "1"])
    assert (a.rank, a.model, a.peft_type, a.chosen_layer, a.positive, a.negative) == (4, "SDXL", "lora", -1, ["smiling", "happy"], ["frowning"])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--config_file", "x", "--alpha", "1", "--clip_index", "0", "--chosen_layer", "-3"])
    for model, ci, peft, word in (("FLUX.1", 0, "lora", "FLUX"), ("SD3-Medium", 0, "lora", "SD3"), ("SDXL", 2, "lora", "T5"),
                                  ("SD1", 1, "lora", "one CLIP tower"), ("SDXL", 0, "dora", "dora"), ("PonyXL", 3, "lora", "two CLIP towers")):
        with pytest.raises(ValueError, match=word):
            T.check_args(model, ci, peft)
    T.check_args("PonyXL", 1, "lora")
    T.check_args("SD1", 0, "lora")
    from sliders_conceptmod_amd import config_util
    cfg = config_util.load_config_from_yaml("data/config-notrigger-xl.yaml")
    assert cfg.train.lambda_similarity == 0.1 and cfg.network.training_method == "noxattn"
    # the towers run on the GPU only: on the CPU the trainer fails with the engine's message, not silently
    toks, encs = T.synthetic_towers("tiny_sdxl")
    assert len(encs) == 2 and encs[1].config.projection_dim == 64
    assert T.tokenize(toks[0], encs[0], "").tolist()[0][:3] == [998, 999, 999] and T.tokenize(toks[0], encs[0], "a b").shape == (1, 77)


def test_combine_loras(tmp_path):
    from safetensors.torch import load_file, save_file
    import sliders_conceptmod_amd.combine_loras as CL
    g = torch.Generator().manual_seed(1)
    def lora_file(prefix, name, n=2):
        sd = {}
        for i in range(n):
            k = f"{prefix}_block_{i}"
            sd[k + ".alpha"] = torch.tensor(1.0)
            sd[k + ".lora_down.weight"] = torch.randn((4, 8), generator=g)
            sd[k + ".lora_up.weight"] = torch.randn((8, 4), generator=g)
        save_file(sd, str(tmp_path / name))
        return sd
    u, t1, t2 = lora_file("lora_unet", "u.safetensors"), lora_file("lora_te1", "a.safetensors"), lora_file("lora_te2", "b.safetensors")
    out = tmp_path / "o.safetensors"
    CL.main([str(tmp_path / "u.safetensors"), str(tmp_path / "a.safetensors"), str(tmp_path / "b.safetensors"), str(out), "0.5", "2.0"])
    got = load_file(str(out))
    assert set(got) == set(u) | set(t1) | set(t2)
    for src, s in ((u, 0.5), (t1, 2.0), (t2, 1.0)):
        for k, v in src.items():
            assert torch.equal(got[k], s * v if "lora_down" in k else v), k
    parts = CL.split_by_prefix(got)
    assert set(parts["lora_te1_"]) == set(t1) and set(parts["lora_unet_"]) == set(u)
    # an input left out, a wrong prefix, a pickle
    CL.main(["-", str(tmp_path / "a.safetensors"), "-", str(out)])
    assert set(load_file(str(out))) == set(t1)
    with pytest.raises(ValueError, match="does not start with"):
        CL.main([str(tmp_path / "a.safetensors"), "-", "-", str(out)])
    with pytest.raises(ValueError, match="safetensors"):
        CL.main(["x.bin", "-", "-", str(out)])


def test_generate_images_text_encoder_flags():
    from sliders_conceptmod_amd import generate_images as G
    a = G.build_parser().parse_args(["--prompts_path", "p.csv", "--save_path", "o", "--te_model_name", "a.safetensors,b.safetensors",
                                     "--te_model_name", "c.safetensors"])
    assert a.model_name is None and G.parse_te_names(a.te_model_name) == ["a.safetensors", "b.safetensors", "c.safetensors"]
    assert G.parse_te_names(None) == []
    t = torch.zeros(1)
    assert G.te_tower_of({"lora_te1_x.alpha": t}, "f") == 0 and G.te_tower_of({"lora_te2_x.alpha": t}, "f") == 1
    for bad in ({"lora_te1_x.alpha": t, "lora_te2_x.alpha": t}, {"lora_unet_x.alpha": t}, {"lora_te1_x.alpha": t, "lora_unet_y.alpha": t}):
        with pytest.raises(ValueError, match="exactly one"):
            G.te_tower_of(bad, "f")
    # the stand-in tokenizer pads like CLIPTokenizer when asked to, and only then
    from sliders_conceptmod_amd.model_util import SyntheticClipTokenizer
    tok = SyntheticClipTokenizer(1000, 999)
    assert tok(["a b"], padding="max_length", max_length=77).input_ids.shape == (1, 77)
    assert tok(["a b"], padding=True).input_ids.shape == (1, 4) and tok("a b").input_ids.shape == (1, 4)


# ---- the engine's site-list refusals, through the dry run (host only) ----------------------------------------------------
@pytest.mark.parametrize("change,gist", [
    (dict(off_dora=0), r"DoRA site 'text_model\.encoder\.layers\.0\.self_attn\.q_proj'"),
    (dict(rank=0), r"rank 0 of 'text_model\.encoder\.layers\.0\.self_attn\.q_proj' outside \[1, 16\]"),
    (dict(rank=17), r"rank 17 of 'text_model\.encoder\.layers\.0\.self_attn\.q_proj' outside \[1, 16\]"),
    (dict(target="text_model.encoder.layers.0.mlp.fc1"), r"target 'text_model\.encoder\.layers\.0\.mlp\.fc1'.*self_attn\.\{q,k,v\}_proj and self_attn\.out_proj"),
], ids=["dora", "rank0", "rank17", "target"])
def test_clip_lora_plan_refuses_a_site(change, gist):
    """smi_clip_lora_workspace_bytes returns -1 with the tower's prefix, the site and the reason in the message."""
    from sliders_conceptmod_amd import _native
    cfg = R.tiny_config()
    sites, _, _ = R.flat_layout(R.site_names(cfg.num_hidden_layers), cfg.hidden_size, 4, 1.0)
    q = next(i for i, s in enumerate(sites) if s["target"].endswith("layers.0.self_attn.q_proj"))
    bad = [dict(s, **change) if i == q else s for i, s in enumerate(sites)]
    with pytest.raises(_native.SmiError, match=r"failed \(-1\): smi_clip_lora: " + gist):
        _native.clip_lora_workspace_bytes(cfg, torch.float16, bad, 2)
    assert _native.clip_lora_workspace_bytes(cfg, torch.float16, sites, 2) > 0
