"""Generate the fixtures that pin model.ClipTextEncoder and the pre_norm model.VisionTransformer to
transformers' CLIP towers.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_clip.py

Imports `transformers` (5.x), torch and safetensors only; builds the models from configs (nothing is
fetched).  Seed 0; LayerNorm scales and every bias are moved away from HF's 1 / 0.

Text: CLIPTextModelWithProjection(hidden 128, 2 heads of 64, 2 layers, intermediate 512, 48 positions,
vocab 96, eos_token_id 95, projection_dim 64, quick_gelu, no dropout).  Tokens (6, 40): ids in [1, 95),
the end-of-text id 95 at positions 39, 32, 31, 8, 1, 0 and 0 behind it, so argmax pooling (open_clip)
and first-eos pooling (transformers) pick the same rows.  The model is called WITHOUT attention_mask,
as open_clip calls it: causal mask only.
Second text variant: the same weights and tokens with hidden_act="gelu" (the LAION conversions), outputs only.
Vision: CLIPVisionModelWithProjection(hidden 128, 2 heads, 2 layers, intermediate 512, image 32, patch 8
= 17 tokens, projection_dim 64, quick_gelu), pixel_values (3, 3, 32, 32).

Files (each below the 1 MiB limit of a committed file; tests/clip_fixture.py joins them again):
* clip_hf_tiny_text.safetensors          tokens, gy, fp64 last_hidden_state / text_embeds, the same two of
                                         the gelu variant ("gelu." prefix), embeddings, final_layer_norm and
                                         text_projection (fp32, HF names), bf16_err_hidden, bf16_err_grad
* clip_hf_tiny_text_layer{0,1}.safetensors    the fp32 weights of text_model.encoder.layers.{0,1}
* clip_hf_tiny_text_grads{,_fc2}.safetensors  fp64 gradients ("grad." + HF name) of (text_embeds * gy).sum()
* clip_hf_tiny_vision.safetensors        pixel_values, gy, fp64 last_hidden_state / image_embeds, the
                                         non-layer weights, the fp64 gradients of (image_embeds * gy).sum(),
                                         bf16_err_hidden, bf16_err_grad
* clip_hf_tiny_vision_layer{0,1}.safetensors  the fp32 weights of vision_model.encoder.layers.{0,1}
bf16_err_hidden / bf16_err_grad: ||x - ref|| / ||ref|| of the same HF model under CPU bf16 autocast
against its own fp64 result (last_hidden_state and the embeds, the larger; the maximum over the stored
gradients): the reference's own 16-bit error, which the GPU bf16 test scales its bound from.  The k_proj
bias gradient, zero in exact arithmetic, is normalised by the q_proj weight gradient's norm (grad_floor).

The generator also checks what the fixture can tell apart: an fp64 restatement of the text transformer
written below reproduces HF to 1e-12 with the causal mask and, with the mask removed, moves the pooled
rows by at least 100 x the fp32 tolerance of the tests (1e-4); HF's own fp32 result sits far inside the
bf16 bounds.
"""
import copy
import os

import torch
import torch.nn.functional as F
from safetensors.torch import save_file
from transformers import (CLIPTextConfig, CLIPTextModelWithProjection, CLIPVisionConfig,
                          CLIPVisionModelWithProjection)

HERE = os.path.dirname(os.path.abspath(__file__))
FP32_TOL = 1e-4
EOT, EOT_POS = 95, (39, 32, 31, 8, 1, 0)
TL = "text_model.encoder.layers."
TEXT_GRADS = ("text_model.embeddings.token_embedding.weight", "text_model.embeddings.position_embedding.weight",
              TL + "0.self_attn.q_proj.weight", TL + "0.self_attn.k_proj.bias", TL + "0.self_attn.v_proj.weight",
              TL + "1.mlp.fc2.weight", "text_model.final_layer_norm.bias", "text_projection.weight")
VISION_GRADS = ("vision_model.embeddings.class_embedding", "vision_model.embeddings.patch_embedding.weight",
                "vision_model.embeddings.position_embedding.weight", "vision_model.pre_layrnorm.weight",
                "vision_model.encoder.layers.1.layer_norm2.bias", "visual_projection.weight")


def nerr(a, b, floor=0.0):
    """||a - b|| / max(||b||, floor)."""
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(floor)).item()


def grad_floor(name, ref_grads):
    """self_attn.k_proj.bias has no gradient in exact arithmetic (a constant added to every key's score
    leaves the softmax unchanged): its fp64 value is rounding noise and cannot normalise an error.  Its
    error is normalised by the norm of the same layer's q_proj.weight gradient instead; every other
    gradient by its own norm."""
    if name.endswith("self_attn.k_proj.bias"):
        return ref_grads[name.replace("k_proj.bias", "q_proj.weight")].norm().item()
    return 0.0


def perturb(model):
    with torch.no_grad():   # non-trivial LayerNorm scales / biases and Linear biases (HF inits them to 1 / 0)
        for n, p in model.named_parameters():
            if n.endswith(".weight") and any(s in n for s in ("layer_norm", "layrnorm", "layernorm")):
                p.add_(torch.randn_like(p) * 0.1)
            elif n.endswith(".bias"):
                p.copy_(torch.randn_like(p) * 0.05)


def run(model, inputs, gy, names, embeds, autocast=False):
    model.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        out = model(**inputs)
    emb = getattr(out, embeds)
    (emb.to(gy.dtype) * gy).sum().backward()
    params = dict(model.named_parameters())
    return out.last_hidden_state.detach(), emb.detach(), {n: params[n].grad.clone() for n in names}


def reference_and_errors(model, inputs, gy, names, embeds, what):
    """fp64 results of `model`, and its own bf16-autocast / fp32 errors against them."""
    d_in = {k: (v.double() if v.is_floating_point() else v) for k, v in inputs.items()}
    hid, emb, grads = run(copy.deepcopy(model).double(), d_in, gy, names, embeds)
    errs = {}
    for tag, ac in (("bf16", True), ("fp32", False)):
        h, e, g = run(model, inputs, gy.float(), names, embeds, autocast=ac)
        eh = max(nerr(h, hid), nerr(e, emb))
        eg = max(nerr(g[n], grads[n], grad_floor(n, grads)) for n in names)
        errs[tag] = (eh, eg)
        print(f"{what} {tag} vs fp64: hidden/embeds {eh:.3e}, grads {eg:.3e}")
        if ac:
            for n in names:
                print(f"    {n}: ||ref|| {grads[n].norm().item():.3e}, bf16 err "
                      f"{nerr(g[n], grads[n], grad_floor(n, grads)):.3e}")
    # the fp32 result sits far inside the bounds the bf16 test derives from the bf16 error
    assert errs["fp32"][0] < 1e-2 * errs["bf16"][0] and errs["fp32"][1] < 1e-2 * errs["bf16"][1], errs
    return hid, emb, grads, errs["bf16"]


def text_restatement(sd, tokens, cfg, causal):
    """The CLIP text transformer in plain fp64 torch from an HF state dict: (last_hidden_state, text_embeds)."""
    sd = {k: v.double() for k, v in sd.items()}
    B, T = tokens.shape
    H, C = cfg.num_attention_heads, cfg.hidden_size
    ln = lambda x, p: F.layer_norm(x, (C,), sd[p + ".weight"], sd[p + ".bias"], cfg.layer_norm_eps)  # noqa: E731
    lin = lambda x, p: F.linear(x, sd[p + ".weight"], sd.get(p + ".bias"))  # noqa: E731
    act = (lambda u: u * torch.sigmoid(1.702 * u)) if cfg.hidden_act == "quick_gelu" else F.gelu
    x = sd["text_model.embeddings.token_embedding.weight"][tokens] + sd["text_model.embeddings.position_embedding.weight"][:T]
    for i in range(cfg.num_hidden_layers):
        p = f"{TL}{i}."
        y = ln(x, p + "layer_norm1")
        q, k, v = (lin(y, p + "self_attn." + n).view(B, T, H, C // H).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        s = q @ k.transpose(-1, -2) * (C // H) ** -0.5
        if causal:
            s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
        x = x + lin((s.softmax(-1) @ v).transpose(1, 2).reshape(B, T, C), p + "self_attn.out_proj")
        x = x + lin(act(lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")), p + "mlp.fc2")
    hidden = ln(x, "text_model.final_layer_norm")
    pooled = hidden[torch.arange(B), (tokens == cfg.eos_token_id).int().argmax(-1)]
    return hidden, pooled @ sd["text_projection.weight"].t()


def save(files):
    for name, tensors in files.items():
        path = os.path.join(HERE, name)
        save_file({k: v.contiguous() for k, v in tensors.items()}, path,
                  metadata={"generator": "tests/golden/make_golden_clip.py"})
        size = os.path.getsize(path)
        assert size < 1 << 20, (name, size)
        print(f"{name}: {len(tensors)} tensors, {size} B")


def weights(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items() if not k.endswith(".position_ids")}


def main():
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    # ---------------------------------------------------------------- text
    kw = dict(vocab_size=96, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512,
              max_position_embeddings=48, eos_token_id=EOT, bos_token_id=0, pad_token_id=0, projection_dim=64,
              attention_dropout=0.0)
    cfg = CLIPTextConfig(hidden_act="quick_gelu", **kw)
    model = CLIPTextModelWithProjection(cfg).eval()
    perturb(model)
    tokens = torch.randint(1, EOT, (len(EOT_POS), 40), generator=g)
    for b, e in enumerate(EOT_POS):
        tokens[b, e] = EOT
        tokens[b, e + 1:] = 0
    assert torch.equal(tokens.argmax(-1), (tokens == EOT).int().argmax(-1))      # both pooling rules agree
    assert tuple(tokens.argmax(-1).tolist()) == EOT_POS
    gy = torch.randn(len(EOT_POS), 64, generator=g, dtype=torch.float64)
    sd = weights(model)
    hid, emb, grads, (eh, eg) = reference_and_errors(model, dict(input_ids=tokens), gy, TEXT_GRADS, "text_embeds", "text")

    rh, re = text_restatement(sd, tokens, cfg, causal=True)
    assert nerr(rh, hid) < 1e-12 and nerr(re, emb) < 1e-12, (nerr(rh, hid), nerr(re, emb))
    _, ne = text_restatement(sd, tokens, cfg, causal=False)
    moved = nerr(ne, emb)
    print(f"text_embeds, causal mask removed: {moved:.3e} (fp32 tolerance {FP32_TOL:.0e})")
    assert moved >= 100 * FP32_TOL, moved

    gmodel = CLIPTextModelWithProjection(CLIPTextConfig(hidden_act="gelu", **kw)).eval().double()
    gmodel.load_state_dict(sd)
    with torch.no_grad():
        gout = gmodel(input_ids=tokens)
    print(f"gelu variant vs quick_gelu: text_embeds {nerr(gout.text_embeds, emb):.3e}")

    main_file = {k: v for k, v in sd.items() if not k.startswith(TL)}
    main_file.update({"tokens": tokens, "gy": gy, "last_hidden_state": hid, "text_embeds": emb,
                      "gelu.last_hidden_state": gout.last_hidden_state, "gelu.text_embeds": gout.text_embeds,
                      "bf16_err_hidden": torch.tensor(eh, dtype=torch.float64),
                      "bf16_err_grad": torch.tensor(eg, dtype=torch.float64)})
    files = {"clip_hf_tiny_text.safetensors": main_file,
             "clip_hf_tiny_text_grads.safetensors": {"grad." + n: grads[n] for n in TEXT_GRADS if "fc2" not in n},
             "clip_hf_tiny_text_grads_fc2.safetensors": {"grad." + n: grads[n] for n in TEXT_GRADS if "fc2" in n}}
    for i in range(cfg.num_hidden_layers):
        files[f"clip_hf_tiny_text_layer{i}.safetensors"] = {k: v for k, v in sd.items() if k.startswith(f"{TL}{i}.")}
    assert sum(len(f) for f in files.values()) == len(sd) + 8 + len(TEXT_GRADS)
    save(files)

    # ---------------------------------------------------------------- vision
    vcfg = CLIPVisionConfig(hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=512,
                            image_size=32, patch_size=8, projection_dim=64, hidden_act="quick_gelu", attention_dropout=0.0)
    vmodel = CLIPVisionModelWithProjection(vcfg).eval()
    perturb(vmodel)
    pixels = torch.randn(3, 3, 32, 32, generator=g)
    vgy = torch.randn(3, 64, generator=g, dtype=torch.float64)
    vsd = weights(vmodel)
    vhid, vemb, vgrads, (veh, veg) = reference_and_errors(vmodel, dict(pixel_values=pixels), vgy, VISION_GRADS,
                                                          "image_embeds", "vision")
    VL = "vision_model.encoder.layers."
    vmain = {k: v for k, v in vsd.items() if not k.startswith(VL)}
    vmain.update({"pixel_values": pixels, "gy": vgy, "last_hidden_state": vhid, "image_embeds": vemb,
                  "bf16_err_hidden": torch.tensor(veh, dtype=torch.float64),
                  "bf16_err_grad": torch.tensor(veg, dtype=torch.float64)})
    vmain.update({"grad." + n: vgrads[n] for n in VISION_GRADS})
    vfiles = {"clip_hf_tiny_vision.safetensors": vmain}
    for i in range(vcfg.num_hidden_layers):
        vfiles[f"clip_hf_tiny_vision_layer{i}.safetensors"] = {k: v for k, v in vsd.items() if k.startswith(f"{VL}{i}.")}
    assert sum(len(f) for f in vfiles.values()) == len(vsd) + 6 + len(VISION_GRADS)
    save(vfiles)


if __name__ == "__main__":
    main()
