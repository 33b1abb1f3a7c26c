"""Generate the fixtures that pin model.HFBertTextEncoder to transformers.BertModel.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bert.py

Imports `transformers` (5.x) and torch only; builds the model from a config (nothing is fetched).

Model: BertModel(BertConfig(vocab_size=96, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
intermediate_size=512, max_position_embeddings=48, type_vocab_size=2, dropouts 0, layer_norm_eps=1e-12,
pad_token_id=0), add_pooling_layer=False), seed 0 -- head dim 64, the fused attention kernel's.
Tokens (5, 40): non-pad ids in [1, 96), row lengths 40, 33, 32, 7, 1 (CLS only), the rest pad (0);
attention_mask = ids != 0.

Files (split so that each stays below the 1 MiB limit of a committed file; tests/bert_fixture.py
joins them again):
* bert_hf_tiny.safetensors        ids, gy, last_hidden_state (fp64, weights upcast), the embedding
                                  weights (fp32, HF names), bf16_err_hidden, bf16_err_grad
* bert_hf_tiny_layer{0,1}.safetensors   the fp32 weights of encoder.layer.{0,1} under HF names
* bert_hf_tiny_grads.safetensors  fp64 gradients ("grad." + HF name) of loss = (last_hidden_state[:, 0]
                                  * gy).sum() for the three embedding tables, embeddings.LayerNorm.weight,
                                  layer 0 query.weight / key.bias / value.weight, layer 1
                                  output.dense.weight / output.LayerNorm.bias
bf16_err_hidden / bf16_err_grad: ||x - ref|| / ||ref|| of the same HF model under CPU bf16 autocast
against its own fp64 result (hidden state; the maximum over the stored gradients): the reference's
own 16-bit error, which the GPU bf16 test scales its bound from.  The key.bias gradient, zero in exact
arithmetic, is normalised as grad_floor() says (tests/bert_fixture.py does the same).
"""
import copy
import os

import torch
from safetensors.torch import save_file
from transformers import BertConfig, BertModel

HERE = os.path.dirname(os.path.abspath(__file__))
LENGTHS = (40, 33, 32, 7, 1)
GRADS = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
         "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight",
         "encoder.layer.0.attention.self.query.weight", "encoder.layer.0.attention.self.key.bias",
         "encoder.layer.0.attention.self.value.weight", "encoder.layer.1.output.dense.weight",
         "encoder.layer.1.output.LayerNorm.bias")


def nerr(a, b, floor=0.0):
    """||a - b|| / max(||b||, floor)."""
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(floor)).item()


def grad_floor(name, ref_grads):
    """attention.self.key.bias has no gradient in exact arithmetic (a constant added to every key's score
    leaves the softmax unchanged): its fp64 value is rounding noise (~1e-17) and cannot normalise an error.
    Its error is normalised by the norm of the same layer's query.weight gradient instead (both are sums
    of the same dS), i.e. it must vanish on that scale; every other gradient by its own norm."""
    if name.endswith("attention.self.key.bias"):
        return ref_grads[name.replace("key.bias", "query.weight")].norm().item()
    return 0.0


def run(model, ids, gy, autocast=False):
    model.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        hidden = model(input_ids=ids, attention_mask=(ids != 0).long()).last_hidden_state
    (hidden[:, 0].to(gy.dtype) * gy).sum().backward()
    params = dict(model.named_parameters())
    return hidden.detach(), {n: params[n].grad.clone() for n in GRADS}


def main():
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=96, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                     intermediate_size=512, max_position_embeddings=48, type_vocab_size=2,
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, layer_norm_eps=1e-12,
                     pad_token_id=0, hidden_act="gelu")
    model = BertModel(cfg, add_pooling_layer=False).eval()
    with torch.no_grad():   # non-trivial LayerNorm scales / biases and Linear biases (HF inits them to 1 / 0)
        for n, p in model.named_parameters():
            if "LayerNorm.weight" in n:
                p.add_(torch.randn_like(p) * 0.1)
            elif n.endswith(".bias"):
                p.copy_(torch.randn_like(p) * 0.05)
    g = torch.Generator().manual_seed(1)
    ids = torch.zeros(len(LENGTHS), 40, dtype=torch.int64)
    for b, n in enumerate(LENGTHS):
        ids[b, :n] = torch.randint(1, 96, (n,), generator=g)
    gy = torch.randn(len(LENGTHS), 128, generator=g, dtype=torch.float64)

    sd = {k: v.detach().clone().contiguous() for k, v in model.state_dict().items()
          if not k.startswith("embeddings.position_ids")}
    ref_hidden, ref_grads = run(copy.deepcopy(model).double(), ids, gy)
    bf_hidden, bf_grads = run(model, ids, gy.float(), autocast=True)
    err_hidden = nerr(bf_hidden, ref_hidden)
    for n in GRADS:
        print(f"  {n}: ||ref|| {ref_grads[n].norm().item():.3e}, bf16 err "
              f"{nerr(bf_grads[n], ref_grads[n], grad_floor(n, ref_grads)):.3e}")
    err_grad = max(nerr(bf_grads[n], ref_grads[n], grad_floor(n, ref_grads)) for n in GRADS)

    # the mask matters: without it the CLS rows move by far more than any tolerance used on this fixture
    with torch.no_grad():
        unmasked = copy.deepcopy(model).double()(input_ids=ids).last_hidden_state
    print(f"CLS rows, masked vs unmasked: {nerr(unmasked[:, 0], ref_hidden[:, 0]):.3e}")
    print(f"bf16 autocast vs fp64: hidden {err_hidden:.3e}, grads {err_grad:.3e}")

    main_file = {k: v for k, v in sd.items() if k.startswith("embeddings.")}
    main_file.update(ids=ids, gy=gy, last_hidden_state=ref_hidden.contiguous(),
                     bf16_err_hidden=torch.tensor(err_hidden, dtype=torch.float64),
                     bf16_err_grad=torch.tensor(err_grad, dtype=torch.float64))
    files = {"bert_hf_tiny.safetensors": main_file,
             "bert_hf_tiny_grads.safetensors": {"grad." + n: ref_grads[n].contiguous() for n in GRADS}}
    for i in range(cfg.num_hidden_layers):
        files[f"bert_hf_tiny_layer{i}.safetensors"] = {k: v for k, v in sd.items()
                                                        if k.startswith(f"encoder.layer.{i}.")}
    assert sum(len(f) for f in files.values()) == len(sd) + 5 + len(GRADS)
    for name, tensors in files.items():
        path = os.path.join(HERE, name)
        save_file(tensors, path, metadata={"generator": "tests/golden/make_golden_bert.py"})
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        print(f"{name}: {len(tensors)} tensors, {size} B")


if __name__ == "__main__":
    main()
