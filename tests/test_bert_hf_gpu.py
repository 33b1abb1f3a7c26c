"""GPU checks of model.HFBertTextEncoder against transformers.BertModel (the fixture of
tests/golden/make_golden_bert.py: padded captions of 40, 33, 32, 7 and 1 tokens, head dim 64).

* fp32: the masked SDPA fallback and the HIP LayerNorm / MLP kernels, hidden state and stored
  gradients within 1e-4 normalised of the fp64 fixture (fp32 vs fp64 is ~1e-6; test_bert_hf_cpu.py).
* bf16 autocast: the fused masked attention kernel.  The bound is the reference's own 16-bit error
  from the fixture -- the same HF model under bf16 autocast against its fp64 self -- times 2 for a
  different rounding order and the kernel's 16-bit P / dS.
* one training step of the full-size "-hf" config with padded captions."""
import pytest
import torch

from bert_fixture import build_tower, fixture, grad_floor, hidden_and_grads, nerr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _paths(tower):
    return {blk.attn.last_path for blk in tower.blocks}


def test_fp32_matches_transformers():
    _, extra, grads = fixture()
    tower = build_tower().to(DEV)
    hidden, got = hidden_and_grads(tower, DEV)
    assert _paths(tower) == {"sdpa"}
    e = nerr(hidden, extra["last_hidden_state"])
    print(f"fp32 hidden {e:.3e}")
    assert e < 1e-4
    for name, ref in grads.items():
        e = nerr(got[name], ref, grad_floor(name, grads))
        print(f"fp32 {name} {e:.3e}")
        assert e < 1e-4, name


def test_bf16_autocast_runs_the_masked_kernel_within_the_reference_bf16_error(monkeypatch):
    import mamba_clip_amd.model as M
    _, extra, grads = fixture()
    tower = build_tower().to(DEV)
    calls, real = [], M.packed_attention

    def spy(qkv, heads, key_mask=None):
        calls.append(key_mask is not None)
        return real(qkv, heads, key_mask)
    monkeypatch.setattr(M, "packed_attention", spy)
    hidden, got = hidden_and_grads(tower, DEV, autocast=torch.bfloat16)
    assert _paths(tower) == {"fused"} and calls == [True, True]      # both layers, with the mask words
    tol_h, tol_g = 2 * extra["bf16_err_hidden"].item(), 2 * extra["bf16_err_grad"].item()
    e = nerr(hidden, extra["last_hidden_state"])
    print(f"bf16 hidden {e:.3e} (limit {tol_h:.3e})")
    assert e < tol_h
    for name, ref in grads.items():
        e = nerr(got[name], ref, grad_floor(name, grads))
        print(f"bf16 {name} {e:.3e} (limit {tol_g:.3e})")
        assert e < tol_g, name


def test_hf_config_train_step_with_padded_captions():
    from mamba_clip_amd.loss import ClipLoss
    from mamba_clip_amd.model import HFBertTextEncoder, build_clip
    torch.manual_seed(0)
    model = build_clip("biomedclip-vit_b16-pubmedbert256-hf").to(DEV)
    assert isinstance(model.text, HFBertTextEncoder)
    g = torch.Generator().manual_seed(1)
    B = 8
    images = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    tokens = torch.randint(1, 30522, (B, 256), generator=g)
    for b, n in enumerate((256, 1, 17, 32, 33, 64, 100, 200)):
        tokens[b, n:] = 0
    tokens = tokens.to(DEV)
    losses = []
    for ckpt in (False, True):
        model.set_grad_checkpointing(ckpt)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = model(images, tokens)
            loss = ClipLoss()(**out)["contrastive_loss"]
        loss.backward()
        torch.cuda.synchronize()
        assert {blk.attn.last_path for blk in model.text.blocks} == {"fused"}
        assert torch.isfinite(loss)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        losses.append(loss.item())
    assert losses[0] == losses[1]
