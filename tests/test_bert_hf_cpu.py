"""CPU checks of model.HFBertTextEncoder against transformers.BertModel (fixture
tests/golden/bert_hf_tiny*.safetensors, written by tests/golden/make_golden_bert.py from
`transformers` itself): the module wiring in fp32 through the CPU restatement ops, the strict weight
loader, lock_text_tower, the config key and the key-mask packing.  No HIP kernel runs.

Tolerance: an fp32 forward + backward of a 2-layer encoder differs from the fp64 one by ~1e-6
(normalised ||got - ref|| / ||ref||); 1e-4 leaves two orders of margin and admits no wrong formula
(dropping the padding mask alone moves the CLS rows by 3e-2)."""
import pytest
import torch

from bert_fixture import build_tower, fixture, grad_floor, hidden_and_grads, nerr

TOL = 1e-4


def test_tower_matches_transformers_fp32_cpu():
    from oracle.cpu_model import oracle_ops
    _, extra, grads = fixture()
    tower = build_tower()
    with oracle_ops():
        hidden, got = hidden_and_grads(tower, "cpu")
    assert hidden.shape == extra["last_hidden_state"].shape
    e = nerr(hidden, extra["last_hidden_state"])
    print(f"hidden {e:.3e}")
    assert e < TOL
    for name, ref in grads.items():
        e = nerr(got[name], ref, grad_floor(name, grads))
        print(f"{name} {e:.3e}")
        assert e < TOL, name
    # the padded rows are rows of last_hidden_state too, and the CLS-only caption attends to itself alone
    assert nerr(hidden[4], extra["last_hidden_state"][4]) < TOL


def test_forward_projects_the_cls_row():
    from oracle.cpu_model import oracle_ops
    _, extra, _ = fixture()
    tower = build_tower()
    with oracle_ops(), torch.no_grad():
        out = tower(extra["ids"])
        ref = tower.proj(tower.forward_hidden(extra["ids"])[:, 0])
    assert out.shape == (5, 32) and torch.equal(out, ref)
    assert not any(p.bias is not None for p in tower.proj if isinstance(p, torch.nn.Linear))


def test_loader_is_strict():
    from mamba_clip_amd.model import load_hf_bert_state_dict
    sd, _, _ = fixture()
    tower = build_tower()
    # ignored: the pooler and the position_ids buffer; a "bert." prefix is stripped
    ok = {"bert." + k: v for k, v in sd.items()}
    ok["bert.pooler.dense.weight"] = torch.zeros(128, 128)
    ok["bert.embeddings.position_ids"] = torch.arange(48)[None]
    load_hf_bert_state_dict(tower, ok)
    tower.load_hf_bert_state_dict(sd)
    q = sd["encoder.layer.1.attention.self.query.weight"]
    k = sd["encoder.layer.1.attention.self.key.bias"]
    assert torch.equal(tower.blocks[1].attn.qkv.weight[:128], q) and torch.equal(tower.blocks[1].attn.qkv.bias[128:256], k)
    missing = {k: v for k, v in sd.items() if k != "encoder.layer.1.attention.self.key.bias"}
    with pytest.raises(KeyError, match="missing.*encoder.layer.1.attention.self.key.bias"):
        load_hf_bert_state_dict(tower, missing)
    with pytest.raises(KeyError, match="unexpected.*encoder.layer.2.output.dense.weight"):
        load_hf_bert_state_dict(tower, dict(sd, **{"encoder.layer.2.output.dense.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match="embeddings.word_embeddings.weight"):
        load_hf_bert_state_dict(tower, dict(sd, **{"embeddings.word_embeddings.weight": torch.zeros(97, 128)}))


def test_lock_text_tower_groups():
    """Mirrors the BERT case of test_model_cpu.py for the new tower."""
    from mamba_clip_amd.model import ClipModel, HFBertTextEncoder, VisionTransformer

    def trainable(m):
        return {n for n, p in m.text.named_parameters() if p.requires_grad}

    def make():
        return ClipModel(VisionTransformer(img_size=32, patch=8, width=64, layers=1, heads=4, output_dim=16),
                         HFBertTextEncoder(vocab_size=100, context_length=8, max_positions=16, width=64, layers=2,
                                           heads=4, output_dim=16))
    bm = make()
    bm.lock_text_tower(unlocked_layers=1)
    t = trainable(bm)
    assert not {"tok.weight", "pos.weight", "tok_type.weight", "ln.weight"} & t
    assert not any(n.startswith("blocks.0.") for n in t)
    assert any(n.startswith("blocks.1.") for n in t) and any(n.startswith("proj.") for n in t)
    bm = make()
    bm.lock_text_tower()
    assert trainable(bm) == {"proj.0.weight", "proj.2.weight"}
    bm.lock_text_tower(freeze_layer_norm=False)
    t = trainable(bm)
    assert {"ln.weight", "ln.bias", "blocks.0.norm1.weight", "blocks.1.norm2.bias"} <= t
    assert not any(("attn" in n or "fc" in n) for n in t) and not {"tok.weight", "pos.weight", "tok_type.weight"} & t
    assert bm.side_priority == -1        # the text stream's priority beside a BERT tower


def test_config_key_builds():
    from mamba_clip_amd.cli import build_parser
    from mamba_clip_amd.model import MODEL_CONFIGS, BertTextEncoder, HFBertTextEncoder, build_clip
    assert "biomedclip-vit_b16-pubmedbert256-hf" in MODEL_CONFIGS
    with torch.device("meta"):
        m = build_clip("biomedclip-vit_b16-pubmedbert256-hf")
        old = build_clip("biomedclip-vit_b16-pubmedbert256")
    assert isinstance(m.text, HFBertTextEncoder) and isinstance(old.text, BertTextEncoder)
    t = m.text
    assert (t.tok.weight.shape, t.pos.weight.shape, t.tok_type.weight.shape) == ((30522, 768), (512, 768), (2, 768))
    assert len(t.blocks) == 12 and t.blocks[0].attn.heads == 12 and t.blocks[0].fc1.out_features == 3072
    assert t.ln.eps == t.blocks[0].norm1.eps == t.blocks[0].norm2.eps == 1e-12
    assert m.context_length == 256 and m.vocab_size == 30522
    # BERT-base without the pooler: 108.9 M parameters, plus the 768 -> 640 -> 512 projection
    n_bert = sum(p.numel() for n, p in t.named_parameters() if not n.startswith("proj."))
    assert n_bert == 108_891_648
    assert "biomedclip-vit_b16-pubmedbert256-hf" in build_parser().format_help().replace("\n", "").replace(" ", "")


@pytest.mark.parametrize("N", [7, 40, 256])
def test_pack_key_mask_against_loop(N):
    from mamba_clip_amd.ops import pack_key_mask
    g = torch.Generator().manual_seed(N)
    valid = torch.rand(6, N, generator=g) < 0.6
    valid[0] = True
    valid[1] = False
    valid[2, : N // 2] = True
    valid[2, N // 2:] = False
    words = pack_key_mask(valid)
    assert words.shape == (6, 8) and words.dtype == torch.int32
    for b in range(6):
        for t in range(8):
            want = 0
            for j in range(32):
                if 32 * t + j < N and bool(valid[b, 32 * t + j]):
                    want |= 1 << j
            assert int(words[b, t]) & 0xFFFFFFFF == want, (b, t)
    with pytest.raises(RuntimeError, match="at most 256"):
        pack_key_mask(torch.ones(1, 257, dtype=torch.bool))
