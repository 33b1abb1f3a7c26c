"""Shared by test_mamba_hf_cpu.py / test_mamba_hf_gpu.py: the transformers.MambaModel fixture
(tests/golden/make_golden_mamba.py) and the tower built from it."""
import functools

import torch

from conftest import load_golden

FILES = ("mamba_hf_tiny.safetensors", "mamba_hf_tiny_layer0.safetensors", "mamba_hf_tiny_layer1.safetensors",
         "mamba_hf_tiny_grads.safetensors")
EXTRA = ("ids", "gy", "last_hidden_state", "bf16_err_hidden", "bf16_err_grad")
LENGTHS = (40, 33, 32, 9, 8, 7, 1)


def tower_name(hf):
    """HF parameter name -> MambaTextEncoder parameter name (model.load_hf_mamba_state_dict's map)."""
    if hf == "embeddings.weight":
        return "embedding.weight"
    if hf == "norm_f.weight":
        return "norm_f"
    return hf.replace(".norm.weight", ".norm_weight")


@functools.lru_cache(maxsize=None)
def fixture():
    """(HF state dict fp32, {ids, gy, last_hidden_state, bf16_err_*}, {HF name: fp64 gradient}); read once,
    not to be modified."""
    merged = {}
    for f in FILES:
        merged.update(load_golden(f))
    extra = {k: merged.pop(k) for k in EXTRA}
    grads = {k[5:]: merged.pop(k) for k in list(merged) if k.startswith("grad.")}
    assert len(grads) == 11 and tuple((extra["ids"] != 0).sum(1).tolist()) == LENGTHS
    return merged, extra, grads


def pooled_ref():
    """HF's hidden row len_b - 1 of every caption, (7, 128) fp64."""
    _, extra, _ = fixture()
    return extra["last_hidden_state"][torch.arange(len(LENGTHS)), torch.tensor(LENGTHS) - 1]


def build_tower(pad_id=0):
    from mamba_clip_amd.model import MambaTextEncoder, load_hf_mamba_state_dict
    sd, _, _ = fixture()
    tower = MambaTextEncoder(vocab_size=96, context_length=40, d_model=128, n_layer=2, d_state=16, output_dim=32,
                             pad_id=pad_id)
    return load_hf_mamba_state_dict(tower, sd)


def nerr(a, b):
    """||a - b|| / ||b||"""
    a, b = a.detach().double().cpu(), b.double()
    return ((a - b).norm() / b.norm()).item()


def hidden_and_grads(tower, device, autocast=None, ids=None):
    """The pooled rows (forward_hidden) and the stored gradients of loss = (pooled * gy).sum()."""
    _, extra, grads = fixture()
    tower.zero_grad()
    ids = (extra["ids"] if ids is None else ids).to(device)
    gy = extra["gy"].float().to(device)
    if autocast is None:
        hidden = tower.forward_hidden(ids)
    else:
        with torch.autocast("cuda", dtype=autocast):
            hidden = tower.forward_hidden(ids)
    (hidden.float() * gy).sum().backward()
    params = dict(tower.named_parameters())
    return hidden.detach(), {name: params[tower_name(name)].grad for name in grads}
