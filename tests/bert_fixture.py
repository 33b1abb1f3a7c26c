"""Shared by test_bert_hf_cpu.py / test_bert_hf_gpu.py: the transformers.BertModel fixture
(tests/golden/make_golden_bert.py) and the tower built from it."""
import functools

import torch

from conftest import load_golden

FILES = ("bert_hf_tiny.safetensors", "bert_hf_tiny_layer0.safetensors", "bert_hf_tiny_layer1.safetensors",
         "bert_hf_tiny_grads.safetensors")
EXTRA = ("ids", "gy", "last_hidden_state", "bf16_err_hidden", "bf16_err_grad")
# HF name of each stored gradient -> (parameter of HFBertTextEncoder, row slice of it or None)
GRAD_MAP = {
    "embeddings.word_embeddings.weight": ("tok.weight", None),
    "embeddings.position_embeddings.weight": ("pos.weight", None),
    "embeddings.token_type_embeddings.weight": ("tok_type.weight", None),
    "embeddings.LayerNorm.weight": ("ln.weight", None),
    "encoder.layer.0.attention.self.query.weight": ("blocks.0.attn.qkv.weight", slice(0, 128)),
    "encoder.layer.0.attention.self.key.bias": ("blocks.0.attn.qkv.bias", slice(128, 256)),
    "encoder.layer.0.attention.self.value.weight": ("blocks.0.attn.qkv.weight", slice(256, 384)),
    "encoder.layer.1.output.dense.weight": ("blocks.1.fc2.weight", None),
    "encoder.layer.1.output.LayerNorm.bias": ("blocks.1.norm2.bias", None),
}


@functools.lru_cache(maxsize=None)
def fixture():
    """(HF state dict fp32, {ids, gy, last_hidden_state, bf16_err_*}, {HF name: fp64 gradient}); read once, not to be modified."""
    merged = {}
    for f in FILES:
        merged.update(load_golden(f))
    extra = {k: merged.pop(k) for k in EXTRA}
    grads = {k[5:]: merged.pop(k) for k in list(merged) if k.startswith("grad.")}
    assert set(grads) == set(GRAD_MAP)
    return merged, extra, grads


def build_tower():
    from mamba_clip_amd.model import HFBertTextEncoder, load_hf_bert_state_dict
    sd, _, _ = fixture()
    tower = HFBertTextEncoder(vocab_size=96, context_length=40, max_positions=48, type_vocab_size=2, width=128,
                              layers=2, heads=2, output_dim=32, pad_token_id=0)
    return load_hf_bert_state_dict(tower, sd)


def nerr(a, b, floor=0.0):
    """||a - b|| / max(||b||, floor)"""
    a, b = a.detach().double().cpu(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(floor)).item()


def grad_floor(name, grads):
    """As make_golden_bert.grad_floor: key.bias has no gradient in exact arithmetic (softmax ignores a
    constant added to every key's score), its stored value is fp64 noise; it is measured on the scale
    of the same layer's query.weight gradient.  Every other gradient on its own."""
    if name.endswith("attention.self.key.bias"):
        return grads[name.replace("key.bias", "query.weight")].norm().item()
    return 0.0


def hidden_and_grads(tower, device, autocast=None):
    """last_hidden_state and the stored gradients of loss = (hidden[:, 0] * gy).sum()."""
    _, extra, grads = fixture()
    tower.zero_grad()
    ids, gy = extra["ids"].to(device), extra["gy"].float().to(device)
    if autocast is None:
        hidden = tower.forward_hidden(ids)
    else:
        with torch.autocast("cuda", dtype=autocast):
            hidden = tower.forward_hidden(ids)
    (hidden[:, 0].float() * gy).sum().backward()
    params = dict(tower.named_parameters())
    got = {}
    for name, (ours, rows) in GRAD_MAP.items():
        g = params[ours].grad
        got[name] = g if rows is None else g[rows]
    return hidden.detach(), got
