"""Shared by test_clip_hf_cpu.py / test_clip_hf_gpu.py: the transformers CLIP fixtures
(tests/golden/make_golden_clip.py) joined from their split files, and the towers built from them."""
import functools
import math

import torch

from conftest import load_golden

TEXT_FILES = ("clip_hf_tiny_text.safetensors", "clip_hf_tiny_text_layer0.safetensors", "clip_hf_tiny_text_layer1.safetensors",
              "clip_hf_tiny_text_grads.safetensors", "clip_hf_tiny_text_grads_fc2.safetensors")
VISION_FILES = ("clip_hf_tiny_vision.safetensors", "clip_hf_tiny_vision_layer0.safetensors",
                "clip_hf_tiny_vision_layer1.safetensors")
TEXT_EXTRA = ("tokens", "gy", "last_hidden_state", "text_embeds", "gelu.last_hidden_state", "gelu.text_embeds",
              "bf16_err_hidden", "bf16_err_grad")
VISION_EXTRA = ("pixel_values", "gy", "last_hidden_state", "image_embeds", "bf16_err_hidden", "bf16_err_grad")
EOT, EOT_POS = 95, (39, 32, 31, 8, 1, 0)
TL = "text_model.encoder.layers."
# HF name of each stored gradient -> (parameter of the tower, row slice of it or None)
TEXT_GRAD_MAP = {
    "text_model.embeddings.token_embedding.weight": ("token_embedding.weight", None),
    "text_model.embeddings.position_embedding.weight": ("positional_embedding", None),
    TL + "0.self_attn.q_proj.weight": ("blocks.0.attn.qkv.weight", slice(0, 128)),
    TL + "0.self_attn.k_proj.bias": ("blocks.0.attn.qkv.bias", slice(128, 256)),
    TL + "0.self_attn.v_proj.weight": ("blocks.0.attn.qkv.weight", slice(256, 384)),
    TL + "1.mlp.fc2.weight": ("blocks.1.fc2.weight", None),
    "text_model.final_layer_norm.bias": ("ln_final.bias", None),
    "text_projection.weight": ("text_projection.weight", None),
}
VISION_GRAD_MAP = {
    "vision_model.embeddings.class_embedding": ("cls_token", None),
    "vision_model.embeddings.patch_embedding.weight": ("patch_embed.proj.weight", None),
    "vision_model.embeddings.position_embedding.weight": ("pos_embed", None),
    "vision_model.pre_layrnorm.weight": ("ln_pre.weight", None),
    "vision_model.encoder.layers.1.layer_norm2.bias": ("blocks.1.norm2.bias", None),
    "visual_projection.weight": ("head.weight", None),
}


def _join(files, extra_names, grad_map):
    merged = {}
    for f in files:
        merged.update(load_golden(f))
    extra = {k: merged.pop(k) for k in extra_names}
    grads = {k[5:]: merged.pop(k) for k in list(merged) if k.startswith("grad.")}
    assert set(grads) == set(grad_map)
    return merged, extra, grads


@functools.lru_cache(maxsize=None)
def text_fixture():
    """(HF state dict fp32, {tokens, gy, fp64 outputs, bf16_err_*}, {HF name: fp64 gradient}); read once, not to be modified."""
    return _join(TEXT_FILES, TEXT_EXTRA, TEXT_GRAD_MAP)


@functools.lru_cache(maxsize=None)
def vision_fixture():
    return _join(VISION_FILES, VISION_EXTRA, VISION_GRAD_MAP)


def state_dict():
    """The two fixtures' weights as one transformers.CLIPModel state dict (logit_scale at CLIP's initial value)."""
    sd = dict(text_fixture()[0])
    sd.update(vision_fixture()[0])
    sd["logit_scale"] = torch.tensor(math.log(1 / 0.07))
    return sd


def tiny_towers(act="quick_gelu", eot_token_id=None):
    """An unloaded ClipModel of the fixtures' shape."""
    from mamba_clip_amd.model import ClipModel, ClipTextEncoder, VisionTransformer
    vis = VisionTransformer(img_size=32, patch=8, width=128, layers=2, heads=2, output_dim=64, pre_norm=True, eps=1e-5,
                            patch_bias=False, act="quick_gelu")
    txt = ClipTextEncoder(vocab_size=96, context_length=48, width=128, layers=2, heads=2, output_dim=64, act=act,
                          eot_token_id=eot_token_id, mlp_dim=512)
    return ClipModel(vis, txt)


def build_clip_model(act="quick_gelu", eot_token_id=None):
    from mamba_clip_amd.model import load_hf_clip_state_dict
    return load_hf_clip_state_dict(tiny_towers(act, eot_token_id), state_dict())


def nerr(a, b, floor=0.0):
    """||a - b|| / max(||b||, floor)"""
    a, b = a.detach().double().cpu(), b.double()
    return ((a.reshape(b.shape) - b).norm() / b.norm().clamp_min(floor)).item()


def grad_floor(name, grads):
    """As make_golden_clip.grad_floor: k_proj.bias has no gradient in exact arithmetic (softmax ignores a
    constant added to every key's score), its stored value is fp64 noise; it is measured on the scale of
    the same layer's q_proj.weight gradient.  Every other gradient on its own."""
    if name.endswith("self_attn.k_proj.bias"):
        return grads[name.replace("k_proj.bias", "q_proj.weight")].norm().item()
    return 0.0


def _autocast(dtype):
    return torch.autocast("cuda", dtype=dtype, enabled=dtype is not None)


def _collect(tower, grad_map):
    params = dict(tower.named_parameters())
    got = {}
    for name, (ours, rows) in grad_map.items():
        g = params[ours].grad
        got[name] = g if rows is None else g[rows]
    return got


def text_outputs_and_grads(tower, device, autocast=None):
    """(last_hidden_state, text_embeds, stored gradients of (text_embeds * gy).sum()) of a ClipTextEncoder."""
    _, extra, _ = text_fixture()
    tower.zero_grad()
    tokens, gy = extra["tokens"].to(device), extra["gy"].float().to(device)
    with _autocast(autocast):
        with torch.no_grad():
            hidden = tower.forward_hidden(tokens)
        emb = tower(tokens)
    (emb.float() * gy).sum().backward()
    return hidden.detach(), emb.detach(), _collect(tower, TEXT_GRAD_MAP)


def vision_outputs_and_grads(tower, device, autocast=None):
    """(last_hidden_state, image_embeds, stored gradients of (image_embeds * gy).sum()) of a VisionTransformer."""
    _, extra, _ = vision_fixture()
    tower.zero_grad()
    pixels, gy = extra["pixel_values"].to(device), extra["gy"].float().to(device)
    with _autocast(autocast):
        with torch.no_grad():
            hidden = tower.forward_hidden(pixels)
        emb = tower(pixels)
    (emb.float() * gy).sum().backward()
    return hidden.detach(), emb.detach(), _collect(tower, VISION_GRAD_MAP)
