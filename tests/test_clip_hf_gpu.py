"""GPU checks of model.ClipTextEncoder and the pre_norm model.VisionTransformer against transformers' CLIP
towers (the fixtures of tests/golden/make_golden_clip.py: captions with the end-of-text token at positions
39, 32, 31, 8, 1 and 0, head dim 64; 17 image tokens).

* fp32: the causal SDPA fallback and the HIP LayerNorm / MLP kernels; outputs and stored gradients within
  1e-4 normalised of the fp64 fixtures (fp32 vs fp64 is ~1e-6; test_clip_hf_cpu.py), all three fixtures.
* bf16 autocast: the fused causal attention kernel in the text tower, the unmasked one in the vision tower.
  The bound is the reference's own 16-bit error from the fixture -- the same HF model under bf16 autocast
  against its fp64 self -- times 2 for a different rounding order and the kernel's 16-bit P / dS.
* one training step of the full-size "clip-vit_b16-hf" config with the end-of-text token at the tile edges,
  with and without activation checkpointing; patch dropout in front of ln_pre."""
import pytest
import torch

from clip_fixture import (build_clip_model, grad_floor, nerr, text_fixture, text_outputs_and_grads, vision_fixture,
                          vision_outputs_and_grads)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _paths(tower):
    return {blk.attn.last_path for blk in tower.blocks}


def _within(tag, outs, grads_got, grads_ref, tol_out, tol_grad):
    worst = 0.0
    for what, a, b in outs:
        e = nerr(a, b)
        worst = max(worst, e / tol_out)
        print(f"{tag} {what} {e:.3e} (limit {tol_out:.3e}, ratio {e / tol_out:.3f})")
    for name, ref in grads_ref.items():
        e = nerr(grads_got[name], ref, grad_floor(name, grads_ref))
        worst = max(worst, e / tol_grad)
        print(f"{tag} {name} {e:.3e} (limit {tol_grad:.3e}, ratio {e / tol_grad:.3f})")
    for what, a, b in outs:
        assert nerr(a, b) < tol_out, (tag, what)
    for name, ref in grads_ref.items():
        assert nerr(grads_got[name], ref, grad_floor(name, grads_ref)) < tol_grad, (tag, name)
    return worst


def test_fp32_matches_transformers():
    model = build_clip_model().to(DEV)
    _, extra, grads = text_fixture()
    hidden, emb, got = text_outputs_and_grads(model.text, DEV)
    assert _paths(model.text) == {"sdpa"}
    _within("fp32 text", (("hidden", hidden, extra["last_hidden_state"]), ("text_embeds", emb, extra["text_embeds"])),
            got, grads, 1e-4, 1e-4)
    _, vextra, vgrads = vision_fixture()
    hidden, emb, got = vision_outputs_and_grads(model.visual, DEV)
    assert _paths(model.visual) == {"sdpa"}
    _within("fp32 vision", (("hidden", hidden, vextra["last_hidden_state"]), ("image_embeds", emb, vextra["image_embeds"])),
            got, vgrads, 1e-4, 1e-4)
    gelu = build_clip_model(act="gelu").text.to(DEV)
    with torch.no_grad():
        hidden, emb = gelu.forward_hidden(extra["tokens"].to(DEV)), gelu(extra["tokens"].to(DEV))
    assert _paths(gelu) == {"sdpa"}
    _within("fp32 gelu text", (("hidden", hidden, extra["gelu.last_hidden_state"]), ("text_embeds", emb, extra["gelu.text_embeds"])),
            {}, {}, 1e-4, 1e-4)


def test_bf16_autocast_runs_the_causal_kernel_within_the_reference_bf16_error(monkeypatch):
    import mamba_clip_amd.model as M
    model = build_clip_model().to(DEV)
    calls, real = [], M.packed_attention

    def spy(qkv, heads, key_mask=None, causal=False):
        calls.append((qkv.shape[1], causal, key_mask is not None))
        return real(qkv, heads, key_mask, causal)
    monkeypatch.setattr(M, "packed_attention", spy)

    _, extra, grads = text_fixture()
    hidden, emb, got = text_outputs_and_grads(model.text, DEV, autocast=torch.bfloat16)
    # forward_hidden and forward: every text layer, causal, no key mask
    assert _paths(model.text) == {"fused"} and calls == [(40, True, False)] * 4
    _within("bf16 text", (("hidden", hidden, extra["last_hidden_state"]), ("text_embeds", emb, extra["text_embeds"])),
            got, grads, 2 * extra["bf16_err_hidden"].item(), 2 * extra["bf16_err_grad"].item())

    del calls[:]
    _, vextra, vgrads = vision_fixture()
    hidden, emb, got = vision_outputs_and_grads(model.visual, DEV, autocast=torch.bfloat16)
    assert _paths(model.visual) == {"fused"} and calls == [(17, False, False)] * 4
    _within("bf16 vision", (("hidden", hidden, vextra["last_hidden_state"]), ("image_embeds", emb, vextra["image_embeds"])),
            got, vgrads, 2 * vextra["bf16_err_hidden"].item(), 2 * vextra["bf16_err_grad"].item())


def test_clip_config_train_step_with_eot_at_the_tile_edges():
    from mamba_clip_amd.loss import ClipLoss
    from mamba_clip_amd.model import ClipTextEncoder, build_clip
    torch.manual_seed(0)
    model = build_clip("clip-vit_b16-hf").to(DEV)
    assert isinstance(model.text, ClipTextEncoder)
    g = torch.Generator().manual_seed(1)
    B, eot = 8, 49407
    images = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    tokens = torch.randint(1, eot, (B, 77), generator=g)
    pos = (76, 0, 1, 31, 32, 33, 50, 64)
    for b, n in enumerate(pos):
        tokens[b, n] = eot
        tokens[b, n + 1:] = 0
    tokens = tokens.to(DEV)
    assert model.text.pool_index(tokens).tolist() == list(pos)
    losses = []
    for ckpt in (False, True):
        model.set_grad_checkpointing(ckpt)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(images, tokens)
            loss = ClipLoss()(**out)["contrastive_loss"]
        loss.backward()
        torch.cuda.synchronize()
        assert _paths(model.text) == {"fused"} and _paths(model.visual) == {"fused"}
        assert torch.isfinite(loss)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        losses.append(loss.item())
    assert losses[0] == losses[1]


def test_patch_dropout_with_pre_norm():
    from mamba_clip_amd.model import build_clip
    torch.manual_seed(0)
    model = build_clip("clip-vit_b16-hf", force_patch_dropout=0.5).to(DEV).train()
    vis = model.visual
    images = torch.randn(4, 3, 224, 224, device=DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        f = vis(images)
    (f.float() ** 2).sum().backward()
    assert vis.last_keep is not None and vis.last_keep.shape == (4, 98)
    assert torch.isfinite(f).all()
    for n, p in vis.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    vis.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.isfinite(vis(images)).all()
    assert vis.last_keep is None
