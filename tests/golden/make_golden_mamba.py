"""Generate the fixtures that pin model.MambaTextEncoder to transformers.MambaModel.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mamba.py

Imports `transformers` (5.x) and torch only; builds the model from a config (nothing is fetched) and
runs HF's slow (pure torch) path on the CPU.

Model: MambaModel(MambaConfig(vocab_size=96, hidden_size=128, state_size=16, num_hidden_layers=2,
expand=2, conv_kernel=4, time_step_rank=8, pad_token_id=0, residual_in_fp32=True, use_cache=False)),
seed 0, the RMSNorm weights and D moved away from 1 by 0.1 randn.
Tokens (7, 40): ids in [1, 96) on lengths 40, 33, 32, 9, 8, 7, 1 -- both sides of the scan's
32-position chunk and of its 8-position sub-tile -- then pad (0).

Files (split so that each stays below the 1 MiB limit of a committed file; tests/mamba_fixture.py
joins them again):
* mamba_hf_tiny.safetensors         ids, gy (7, 128) fp64, last_hidden_state (fp64, weights upcast),
                                    embeddings.weight and norm_f.weight (fp32, HF names),
                                    bf16_err_hidden, bf16_err_grad
* mamba_hf_tiny_layer{0,1}.safetensors   the fp32 weights of layers.{0,1} under HF names
* mamba_hf_tiny_grads.safetensors   fp64 gradients ("grad." + HF name) of
                                    loss = (last_hidden_state[b, len_b - 1] * gy[b]).sum() for GRADS below
bf16_err_hidden / bf16_err_grad: ||x - ref|| / ||ref|| of the same HF model under CPU bf16 autocast
against its own fp64 result (the pooled rows; the maximum over the stored gradients): the reference's
own 16-bit error, which the GPU bf16 test scales its bound from.

The model is causal: the generator asserts that the pooled rows are bit-identical with and without
attention_mask, so the tower needs no masking inside its layers, only the right row.
"""
import copy
import os

import torch
from safetensors.torch import save_file
from transformers import MambaConfig, MambaModel

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (40, 33, 32, 9, 8, 7, 1)
T = 40
GRADS = ("embeddings.weight", "norm_f.weight", "layers.0.norm.weight", "layers.0.mixer.A_log", "layers.0.mixer.D",
         "layers.0.mixer.conv1d.weight", "layers.0.mixer.conv1d.bias", "layers.0.mixer.x_proj.weight",
         "layers.0.mixer.dt_proj.weight", "layers.0.mixer.dt_proj.bias", "layers.1.mixer.out_proj.weight")


def nerr(a, b):
    """||a - b|| / ||b||."""
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def pooled(hidden):
    return hidden[torch.arange(len(LENGTHS)), torch.tensor(LENGTHS) - 1]


def run(model, ids, gy, autocast=False, mask=True):
    model.zero_grad()
    kw = dict(attention_mask=(ids != 0).long()) if mask else {}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        hidden = model(input_ids=ids, **kw).last_hidden_state
    (pooled(hidden).to(gy.dtype) * gy).sum().backward()
    params = dict(model.named_parameters())
    return hidden.detach(), {n: params[n].grad.clone() for n in GRADS}


def main():
    torch.manual_seed(0)
    cfg = MambaConfig(vocab_size=96, hidden_size=128, state_size=16, num_hidden_layers=2, expand=2, conv_kernel=4,
                      time_step_rank=8, pad_token_id=0, residual_in_fp32=True, use_cache=False)
    model = MambaModel(cfg).eval()
    with torch.no_grad():   # non-trivial RMSNorm scales and skip weights (HF inits them to 1)
        for n, p in model.named_parameters():
            if n.endswith("norm.weight") or n.endswith("norm_f.weight") or n.endswith("mixer.D"):
                p.add_(torch.randn_like(p) * 0.1)
    g = torch.Generator().manual_seed(1)
    ids = torch.zeros(len(LENGTHS), T, dtype=torch.int64)
    for b, n in enumerate(LENGTHS):
        ids[b, :n] = torch.randint(1, 96, (n,), generator=g)
    gy = torch.randn(len(LENGTHS), 128, generator=g, dtype=torch.float64)

    sd = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items()}
    ref_model = copy.deepcopy(model).double()
    ref_hidden, ref_grads = run(ref_model, ids, gy)
    nomask_hidden, nomask_grads = run(ref_model, ids, gy, mask=False)
    assert torch.equal(pooled(nomask_hidden), pooled(ref_hidden)), "the pooled rows depend on attention_mask"
    assert all(torch.equal(nomask_grads[n], ref_grads[n]) for n in GRADS)
    print("pooled rows and stored gradients: bit-identical with and without attention_mask")
    for b, n in enumerate(LENGTHS):
        print(f"  len {n:2d}: row T-1 vs row len-1 {nerr(nomask_hidden[b, T - 1], ref_hidden[b, n - 1]):.3e}")

    bf_hidden, bf_grads = run(model, ids, gy.float(), autocast=True)
    err_hidden = nerr(pooled(bf_hidden), pooled(ref_hidden))
    for n in GRADS:
        print(f"  {n}: ||ref|| {ref_grads[n].norm().item():.3e}, bf16 err {nerr(bf_grads[n], ref_grads[n]):.3e}")
    err_grad = max(nerr(bf_grads[n], ref_grads[n]) for n in GRADS)
    print(f"bf16 autocast vs fp64: pooled rows {err_hidden:.3e}, grads {err_grad:.3e}")

    main_file = {k: v for k, v in sd.items() if not k.startswith("layers.")}
    main_file.update(ids=ids, gy=gy, last_hidden_state=ref_hidden.contiguous(),
                     bf16_err_hidden=torch.tensor(err_hidden, dtype=torch.float64),
                     bf16_err_grad=torch.tensor(err_grad, dtype=torch.float64))
    files = {"mamba_hf_tiny.safetensors": main_file,
             "mamba_hf_tiny_grads.safetensors": {"grad." + n: ref_grads[n].contiguous() for n in GRADS}}
    for i in range(cfg.num_hidden_layers):
        files[f"mamba_hf_tiny_layer{i}.safetensors"] = {k: v for k, v in sd.items() if k.startswith(f"layers.{i}.")}
    assert sum(len(f) for f in files.values()) == len(sd) + 5 + len(GRADS)
    for name, tensors in files.items():
        path = os.path.join(HERE, name)
        save_file(tensors, path, metadata={"generator": "tests/golden/make_golden_mamba.py"})
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        print(f"{name}: {len(tensors)} tensors, {size} B")


if __name__ == "__main__":
    main()
