"""CPU checks of model.ClipTextEncoder and the pre_norm model.VisionTransformer against transformers'
CLIPTextModelWithProjection / CLIPVisionModelWithProjection (fixtures tests/golden/clip_hf_tiny_*.safetensors,
written by tests/golden/make_golden_clip.py from `transformers` itself): the module wiring in fp32 through
the CPU restatement ops (SDPA with is_causal, torch LayerNorm), both pooling rules, the strict weight
loader, a round trip from a fresh transformers.CLIPModel, the config key, the optimizer groups, and the
unchanged state-dict keys of the default towers.  No HIP kernel runs.

Tolerance: an fp32 forward + backward of a 2-layer tower differs from the fp64 one by ~1e-6 (normalised
||got - ref|| / ||ref||; the generator prints 4e-7 / 7e-7 for HF's own fp32 run); 1e-4 leaves two orders of
margin and admits no wrong formula (removing the causal mask moves text_embeds by 0.9, gelu instead of
quick_gelu by 9e-3)."""
import types

import pytest
import torch

from clip_fixture import (EOT, EOT_POS, build_clip_model, grad_floor, nerr, state_dict, text_fixture,
                          text_outputs_and_grads, tiny_towers, vision_fixture, vision_outputs_and_grads)

TOL = 1e-4


def test_text_tower_matches_transformers_fp32_cpu():
    from oracle.cpu_model import oracle_ops
    _, extra, grads = text_fixture()
    tower = build_clip_model().text
    with oracle_ops():
        hidden, emb, got = text_outputs_and_grads(tower, "cpu")
    assert all(b.attn.last_path == "sdpa" and b.attn.causal for b in tower.blocks)
    assert hidden.shape == extra["last_hidden_state"].shape and emb.shape == extra["text_embeds"].shape
    for what, a, b in (("hidden", hidden, extra["last_hidden_state"]), ("text_embeds", emb, extra["text_embeds"])):
        e = nerr(a, b)
        print(f"{what} {e:.3e}")
        assert e < TOL, what
    for name, ref in grads.items():
        e = nerr(got[name], ref, grad_floor(name, grads))
        print(f"{name} {e:.3e}")
        assert e < TOL, name


def test_gelu_text_variant_matches_transformers_fp32_cpu():
    from oracle.cpu_model import oracle_ops
    _, extra, _ = text_fixture()
    tower = build_clip_model(act="gelu").text
    with oracle_ops(), torch.no_grad():
        hidden, emb = tower.forward_hidden(extra["tokens"]), tower(extra["tokens"])
    assert nerr(hidden, extra["gelu.last_hidden_state"]) < TOL and nerr(emb, extra["gelu.text_embeds"]) < TOL
    assert nerr(emb, extra["text_embeds"]) > 10 * TOL          # and the fixture tells the two activations apart


def test_vision_tower_matches_transformers_fp32_cpu():
    from oracle.cpu_model import oracle_ops
    _, extra, grads = vision_fixture()
    tower = build_clip_model().visual
    with oracle_ops():
        hidden, emb, got = vision_outputs_and_grads(tower, "cpu")
    assert hidden.shape == extra["last_hidden_state"].shape == (3, 17, 128)
    for what, a, b in (("hidden", hidden, extra["last_hidden_state"]), ("image_embeds", emb, extra["image_embeds"])):
        e = nerr(a, b)
        print(f"{what} {e:.3e}")
        assert e < TOL, what
    for name, ref in grads.items():
        e = nerr(got[name], ref)
        print(f"{name} {e:.3e}")
        assert e < TOL, name


def test_both_pooling_rules_pick_the_same_rows():
    from oracle.cpu_model import oracle_ops
    _, extra, _ = text_fixture()
    tokens = extra["tokens"]
    a, b = build_clip_model().text, build_clip_model(eot_token_id=EOT).text
    assert a.pool_index(tokens).tolist() == b.pool_index(tokens).tolist() == list(EOT_POS)
    with oracle_ops(), torch.no_grad():
        ea, eb = a(tokens), b(tokens)
        # the pooled-rows-only final LayerNorm: the same values as ln_final over every row, then the gather
        ref = a.text_projection(a.forward_hidden(tokens)[torch.arange(len(EOT_POS)), torch.tensor(EOT_POS)])
    assert torch.equal(ea, eb)
    assert nerr(ea, ref) < 1e-6
    t2 = tokens.clone()
    t2[3, 20] = EOT
    assert b.pool_index(t2)[3] == 8 and a.pool_index(t2)[3] == 8      # the first occurrence under both rules
    # the rules differ where they should: an end-of-text id that is not the largest moves the id rule only
    c = build_clip_model(eot_token_id=50).text
    t3 = tokens.clone()
    t3[:, 5] = 50
    assert (c.pool_index(t3) <= 5).all() and a.pool_index(t3).tolist() == list(EOT_POS)


def test_pooled_row_gather_backward():
    from mamba_clip_amd.model import _PoolRowsFn
    x = torch.randn(4, 7, 5, dtype=torch.float64, requires_grad=True)
    idx = torch.tensor([6, 0, 3, 3])
    torch.autograd.gradcheck(lambda t: _PoolRowsFn.apply(t, idx), (x,))
    assert torch.equal(_PoolRowsFn.apply(x, idx), x[torch.arange(4), idx])


def test_loader_is_strict():
    from mamba_clip_amd.model import load_hf_clip_state_dict
    sd = state_dict()
    m = tiny_towers()
    ok = dict(sd)
    ok["text_model.embeddings.position_ids"] = torch.arange(48)[None]       # ignored buffers
    ok["vision_model.embeddings.position_ids"] = torch.arange(17)[None]
    load_hf_clip_state_dict(m, ok)
    q = sd["text_model.encoder.layers.1.self_attn.q_proj.weight"]
    k = sd["vision_model.encoder.layers.0.self_attn.k_proj.bias"]
    v = sd["text_model.encoder.layers.0.self_attn.v_proj.weight"]
    assert torch.equal(m.text.blocks[1].attn.qkv.weight[:128], q) and torch.equal(m.visual.blocks[0].attn.qkv.bias[128:256], k)
    assert torch.equal(m.text.blocks[0].attn.qkv.weight[256:], v)
    assert torch.equal(m.visual.cls_token.flatten(), sd["vision_model.embeddings.class_embedding"])
    assert torch.equal(m.visual.pos_embed[0], sd["vision_model.embeddings.position_embedding.weight"])
    assert torch.equal(m.text.positional_embedding[0], sd["text_model.embeddings.position_embedding.weight"])
    assert torch.equal(m.visual.ln_pre.weight, sd["vision_model.pre_layrnorm.weight"])
    assert torch.equal(m.visual.norm.bias, sd["vision_model.post_layernorm.bias"])
    assert torch.equal(m.visual.head.weight, sd["visual_projection.weight"])
    assert torch.equal(m.logit_scale, sd["logit_scale"])
    for drop in ("text_model.encoder.layers.1.self_attn.k_proj.bias", "vision_model.pre_layrnorm.weight", "logit_scale"):
        with pytest.raises(KeyError, match="missing.*" + drop):
            load_hf_clip_state_dict(m, {k: v for k, v in sd.items() if k != drop})
    with pytest.raises(KeyError, match="unexpected.*text_model.encoder.layers.2.mlp.fc1.weight"):
        load_hf_clip_state_dict(m, dict(sd, **{"text_model.encoder.layers.2.mlp.fc1.weight": torch.zeros(1)}))
    with pytest.raises(KeyError, match="unexpected.*vision_model.embeddings.patch_embedding.bias"):
        load_hf_clip_state_dict(m, dict(sd, **{"vision_model.embeddings.patch_embedding.bias": torch.zeros(128)}))
    with pytest.raises(ValueError, match="text_model.embeddings.token_embedding.weight"):
        load_hf_clip_state_dict(m, dict(sd, **{"text_model.embeddings.token_embedding.weight": torch.zeros(97, 128)}))
    with pytest.raises(ValueError, match="self_attn.q_proj.weight"):
        load_hf_clip_state_dict(m, dict(sd, **{"vision_model.encoder.layers.0.self_attn.q_proj.weight": torch.zeros(64, 128)}))
    with pytest.raises(ValueError, match="class_embedding"):
        load_hf_clip_state_dict(m, dict(sd, **{"vision_model.embeddings.class_embedding": torch.zeros(64)}))


def test_round_trip_from_transformers_clip_model():
    """A fresh transformers.CLIPModel of the tiny configs -> state_dict -> our towers: logits_per_image."""
    from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
    from mamba_clip_amd.model import load_hf_clip_state_dict
    from oracle.cpu_model import oracle_ops
    torch.manual_seed(3)
    tc = CLIPTextConfig(vocab_size=96, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512,
                        max_position_embeddings=48, eos_token_id=EOT, bos_token_id=0, pad_token_id=0, projection_dim=64,
                        hidden_act="quick_gelu")
    vc = CLIPVisionConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512,
                          image_size=32, patch_size=8, projection_dim=64, hidden_act="quick_gelu")
    hf = CLIPModel(CLIPConfig(text_config=tc.to_dict(), vision_config=vc.to_dict(), projection_dim=64)).eval()
    ours = load_hf_clip_state_dict(tiny_towers(eot_token_id=EOT), hf.state_dict()).eval()
    tokens = text_fixture()[1]["tokens"][:3]
    pixels = vision_fixture()[1]["pixel_values"]
    with torch.no_grad():
        ref = hf(input_ids=tokens, pixel_values=pixels).logits_per_image
        with oracle_ops():
            i = torch.nn.functional.normalize(ours.visual(pixels), dim=-1)
            t = torch.nn.functional.normalize(ours.text(tokens), dim=-1)
        got = ours.logit_scale.exp() * i @ t.t()
    e = nerr(got, ref)
    print(f"logits_per_image {e:.3e}")
    assert got.shape == ref.shape == (3, 3) and e < TOL


VIT_BLOCK_KEYS = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                  "norm2.weight", "norm2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def test_default_towers_keep_their_state_dict_keys():
    from mamba_clip_amd.model import Attention, ViTBlock, VisionTransformer
    assert list(ViTBlock(64, 1).state_dict()) == VIT_BLOCK_KEYS
    with torch.device("meta"):
        vit = VisionTransformer()
    want = ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    want += [f"blocks.{i}.{k}" for i in range(12) for k in VIT_BLOCK_KEYS]
    want += ["norm.weight", "norm.bias", "head.weight"]
    assert list(vit.state_dict()) == want
    assert vit.norm.eps == vit.blocks[0].norm1.eps == 1e-6 and vit.blocks[0].act == "gelu"
    assert not vit.blocks[0].attn.causal and not Attention(64, 1).causal
    with torch.device("meta"):
        clipv = VisionTransformer(pre_norm=True, eps=1e-5, patch_bias=False, act="quick_gelu")
    assert set(clipv.state_dict()) - set(want) == {"ln_pre.weight", "ln_pre.bias"}
    assert set(want) - set(clipv.state_dict()) == {"patch_embed.proj.bias"}


def test_causal_attention_rejects_a_padding_mask():
    from mamba_clip_amd.model import Attention
    from mamba_clip_amd.ops import packed_attention
    a = Attention(64, 1, causal=True)
    with pytest.raises(ValueError, match="causal"):
        a(torch.zeros(1, 4, 64), None, torch.ones(1, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="causal"):
        packed_attention(torch.zeros(1, 4, 192), 1, key_mask=torch.zeros(1, 8, dtype=torch.int32), causal=True)
    with pytest.raises(ValueError, match="act"):
        from mamba_clip_amd.model import ViTBlock
        ViTBlock(64, 1, act="relu")


def test_config_key_optimizer_groups_and_locking():
    from mamba_clip_amd.cli import build_parser
    from mamba_clip_amd.model import MODEL_CONFIGS, ClipTextEncoder, build_clip
    from mamba_clip_amd.train import _no_decay
    assert "clip-vit_b16-hf" in MODEL_CONFIGS
    with torch.device("meta"):
        m = build_clip("clip-vit_b16-hf")
    t, v = m.text, m.visual
    assert isinstance(t, ClipTextEncoder) and m.context_length == 77 and m.vocab_size == 49408 and t.output_dim == 512
    assert t.token_embedding.weight.shape == (49408, 512) and t.positional_embedding.shape == (1, 77, 512)
    assert len(t.blocks) == 12 and t.blocks[0].attn.heads == 8 and t.blocks[0].fc1.out_features == 2048
    assert all(b.attn.causal and b.act == "quick_gelu" and b.norm1.eps == 1e-5 for b in t.blocks)
    assert t.ln_final.eps == v.ln_pre.eps == v.norm.eps == v.blocks[0].norm2.eps == 1e-5
    assert v.patch_embed.proj.bias is None and not v.blocks[0].attn.causal and v.blocks[0].act == "quick_gelu"
    # openai/clip-vit-base-patch16: 149.6 M parameters
    assert sum(p.numel() for p in m.parameters()) == 149_620_737
    assert m.side_priority == 0
    assert "clip-vit_b16-hf" in build_parser().format_help().replace("\n", "").replace(" ", "")
    # optimizer groups: gains, biases, ln_pre, the position table and the final LayerNorm undecayed; Linear
    # weights, the token table and the projections decayed
    nd = {n for n, p in m.named_parameters() if _no_decay(n, p)}
    assert {"visual.ln_pre.weight", "visual.ln_pre.bias", "text.positional_embedding", "text.ln_final.weight",
            "text.ln_final.bias", "text.blocks.3.norm1.weight", "text.blocks.3.fc1.bias", "logit_scale"} <= nd
    assert not {"text.blocks.0.attn.qkv.weight", "text.blocks.11.fc2.weight", "text.text_projection.weight",
                "text.token_embedding.weight", "visual.head.weight", "visual.patch_embed.proj.weight"} & nd
    # the existing towers' groups are what they were
    with torch.device("meta"):
        old = build_clip("biomedclip-vit_b16-pubmedbert256")
    assert not any("positional_embedding" in n for n, _ in old.named_parameters())
    # lock_text_tower: embeddings, blocks and the final norm frozen, the projection trainable
    m.lock_text_tower()
    assert {n for n, p in t.named_parameters() if p.requires_grad} == {"text_projection.weight"}
    with torch.device("meta"):
        m2 = build_clip("clip-vit_b16-hf")
    m2.lock_text_tower(unlocked_layers=1)
    tr = {n for n, p in m2.text.named_parameters() if p.requires_grad}
    assert any(n.startswith("blocks.11.") for n in tr) and not any(n.startswith("blocks.10.") for n in tr)
    assert "token_embedding.weight" not in tr and "positional_embedding" not in tr
    m2.text.set_grad_checkpointing(True)
    assert m2.text.grad_checkpointing


def test_weight_cast_scope_sees_the_new_linears():
    """ops.weight_cast_scope collects nn.Linear parameters: the text projection and the bias-free patch
    projection's siblings must be Linear modules like their counterparts in the other towers."""
    m = tiny_towers()
    lin = {n for n, mod in m.named_modules() if isinstance(mod, torch.nn.Linear)}
    assert {"text.text_projection", "text.blocks.0.attn.qkv", "text.blocks.1.fc2", "visual.head", "visual.blocks.0.fc1"} <= lin
    assert isinstance(m.visual.ln_pre, torch.nn.LayerNorm) and isinstance(m.text.ln_final, torch.nn.LayerNorm)
