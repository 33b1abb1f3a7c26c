"""GPU checks of model.MambaTextEncoder(pad_id=0) against transformers.MambaModel (the fixture of
tests/golden/make_golden_mamba.py: right-padded captions of 40, 33, 32, 9, 8, 7 and 1 tokens, HF's
hidden row len - 1 of each).

* fp32: the general scan kernels, the conv / norm kernels and the last-token add + RMSNorm kernel;
  pooled rows and stored gradients within 1e-4 normalised of the fp64 fixture (fp32 vs fp64 is ~1e-6;
  test_mamba_hf_cpu.py).
* bf16 autocast: the lane-pair scan kernels.  The bound is the reference's own 16-bit error from the
  fixture -- the same HF model under bf16 autocast against its fp64 self -- times 2 for a different
  rounding order, the factor and the reasoning of test_bert_hf_gpu.py.
* 37 given tokens (the tower pads to 40 itself): the captions that fit still match.
* one training step of the full-size "-hf" config with padded captions.

Measured on an MI355X (normalised ||got - ref|| / ||ref||):
  fp32  pooled rows 5.0e-07; gradients at most 1.8e-06 (layers.0.mixer.x_proj.weight)
  bf16  pooled rows 6.7e-03 (limit 1.57e-02); gradients at most 1.46e-02 (layers.0.mixer.dt_proj.bias,
        limit 3.33e-02)
  37 given tokens, fp32: at most 5.9e-07 per caption"""
import pytest
import torch

from mamba_fixture import LENGTHS, build_tower, fixture, hidden_and_grads, nerr, pooled_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def dispatch(monkeypatch):
    from mamba_clip_amd import selective_scan_interface as ssi
    monkeypatch.setattr(ssi, "RECORD_DISPATCH", True)
    monkeypatch.setattr(ssi, "DISPATCH", [])
    return ssi.DISPATCH


def _spy_pool(monkeypatch):
    import mamba_clip_amd.model as M
    calls, real = [], M.last_token_rmsnorm

    def spy(tokens, pad_id, x, residual, weight, eps=1e-5):
        y, pos = real(tokens, pad_id, x, residual, weight, eps)
        calls.append(pos)
        return y, pos
    monkeypatch.setattr(M, "last_token_rmsnorm", spy)
    return calls


def test_fp32_matches_transformers(dispatch, monkeypatch):
    from mamba_clip_amd import _lib
    _, _, grads = fixture()
    calls = _spy_pool(monkeypatch)
    tower = build_tower().to(DEV)
    hidden, got = hidden_and_grads(tower, DEV)
    assert len(calls) == 1 and calls[0].tolist() == [n - 1 for n in LENGTHS]
    assert sorted(dispatch) == [("bwd", _lib.MC_SCAN_KERNEL_GENERIC)] * 2 + [("fwd", _lib.MC_SCAN_KERNEL_GENERIC)] * 2
    assert hidden.shape == (7, 128) and hidden.dtype == torch.float32
    e = nerr(hidden, pooled_ref())
    print(f"fp32 pooled rows {e:.3e}")
    assert e < 1e-4
    for name, ref in grads.items():
        e = nerr(got[name], ref)
        print(f"fp32 {name} {e:.3e}")
        assert e < 1e-4, name
    assert not tower.embedding.weight.grad[0].any()


def test_bf16_autocast_runs_the_pair_kernels_within_the_reference_bf16_error(dispatch, monkeypatch):
    from mamba_clip_amd import _lib
    _, extra, grads = fixture()
    calls = _spy_pool(monkeypatch)
    tower = build_tower().to(DEV)
    hidden, got = hidden_and_grads(tower, DEV, autocast=torch.bfloat16)
    assert len(calls) == 1 and calls[0].tolist() == [n - 1 for n in LENGTHS]
    assert sorted(dispatch) == [("bwd", _lib.MC_SCAN_KERNEL_PAIR)] * 2 + [("fwd", _lib.MC_SCAN_KERNEL_PAIR)] * 2
    tol_h, tol_g = 2 * extra["bf16_err_hidden"].item(), 2 * extra["bf16_err_grad"].item()
    e = nerr(hidden, pooled_ref())
    print(f"bf16 pooled rows {e:.3e} (limit {tol_h:.3e})")
    assert e < tol_h
    for name, ref in grads.items():
        e = nerr(got[name], ref)
        print(f"bf16 {name} {e:.3e} (limit {tol_g:.3e})")
        assert e < tol_g, name


def test_37_given_tokens_are_padded_to_40_by_the_tower():
    _, extra, _ = fixture()
    tower = build_tower().to(DEV)
    with torch.no_grad():
        hidden = tower.forward_hidden(extra["ids"][:, :37].to(DEV))
    ref = pooled_ref()
    fit = [b for b, n in enumerate(LENGTHS) if n <= 37]
    assert len(fit) == 6
    for b in fit:
        e = nerr(hidden[b], ref[b])
        print(f"len {LENGTHS[b]}: {e:.3e}")
        assert e < 1e-4, LENGTHS[b]


def test_hf_config_train_step_with_padded_captions():
    from mamba_clip_amd.loss import ClipLoss
    from mamba_clip_amd.model import MambaTextEncoder, build_clip
    torch.manual_seed(0)
    model = build_clip("vit_b16-mamba130m-hf").to(DEV)
    assert isinstance(model.text, MambaTextEncoder) and model.text.pad_id == 0
    g = torch.Generator().manual_seed(1)
    B = 8
    images = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    tokens = torch.randint(1, 50280, (B, 77), generator=g)
    for b, n in enumerate((77, 1, 8, 9, 32, 33, 40, 64)):
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
        assert torch.isfinite(loss)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
        # pad positions receive no gradient in a causal tower pooled inside each caption
        assert not model.text.embedding.weight.grad[0].any()
        losses.append(loss.item())
    assert losses[0] == losses[1]
