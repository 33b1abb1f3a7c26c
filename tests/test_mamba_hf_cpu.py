"""CPU checks of model.MambaTextEncoder against transformers.MambaModel (fixture
tests/golden/mamba_hf_tiny*.safetensors, written by tests/golden/make_golden_mamba.py from
`transformers` itself): the module wiring in fp32 through the CPU restatement ops, pooling at each
caption's last non-pad token, the strict weight loader, the config key and the padded synthetic
captions.  No HIP kernel runs: model.last_token_rmsnorm is replaced by the torch restatement below,
the way oracle_ops() replaces the other ops.

Tolerance: an fp32 forward + backward of a 2-layer tower differs from the fp64 one by ~1e-6
(normalised ||got - ref|| / ||ref||; the forward measured 5e-7); 1e-4 leaves two orders of margin
and admits no wrong formula (pooling row T - 1 instead of len - 1 alone moves a padded caption's row
by 1.2 - 1.4)."""
import pytest
import torch

from mamba_fixture import LENGTHS, build_tower, fixture, hidden_and_grads, nerr, pooled_ref

TOL = 1e-4


def last_token_rmsnorm_ref(tokens, pad_id, x, residual, weight, eps=1e-5):
    """ops.last_token_rmsnorm in torch: (y, pos)."""
    Bsz, T = tokens.shape
    pos = ((tokens != pad_id) * torch.arange(T, device=tokens.device)).amax(1)   # 0 when the row is all pad
    rows = torch.arange(Bsz, device=tokens.device)
    h = x[rows, pos].float()
    if residual is not None:
        h = h + residual[rows, pos].float()
    y = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps) * weight.float()
    return y.to(x.dtype), pos.int()


@pytest.fixture
def cpu_ops(monkeypatch):
    import mamba_clip_amd.model as M
    from oracle.cpu_model import oracle_ops
    monkeypatch.setattr(M, "last_token_rmsnorm", last_token_rmsnorm_ref, raising=False)
    with oracle_ops():
        yield


def test_tower_matches_transformers_fp32_cpu(cpu_ops):
    _, _, grads = fixture()
    tower = build_tower()
    hidden, got = hidden_and_grads(tower, "cpu")
    assert hidden.shape == (7, 128)
    e = nerr(hidden, pooled_ref())
    print(f"pooled rows {e:.3e}")
    assert e < TOL
    for b, n in enumerate(LENGTHS):
        assert nerr(hidden[b], pooled_ref()[b]) < TOL, n
    for name, ref in grads.items():
        e = nerr(got[name], ref)
        print(f"{name} {e:.3e}")
        assert e < TOL, name
    # pad positions receive no gradient in a causal tower pooled inside the caption
    assert not tower.embedding.weight.grad[0].any()


def test_pad_id_none_pools_the_last_position(cpu_ops):
    """Without pad_id the tower keeps pooling position T - 1: HF's row len - 1 only for the caption that
    fills the context."""
    _, extra, _ = fixture()
    tower = build_tower(pad_id=None)
    with torch.no_grad():
        hidden = tower.forward_hidden(extra["ids"])
    ref = pooled_ref()
    assert nerr(hidden[0], ref[0]) < TOL
    assert nerr(hidden[0], extra["last_hidden_state"][0, -1]) < TOL
    for b in range(1, len(LENGTHS)):
        e = nerr(hidden[b], ref[b])
        print(f"len {LENGTHS[b]}: row T-1 vs HF row len-1 {e:.3e}")
        assert e > 0.5, LENGTHS[b]


def test_forward_projects_the_pooled_row_and_pads_to_8(cpu_ops):
    _, extra, _ = fixture()
    tower = build_tower()
    ref = pooled_ref()
    with torch.no_grad():
        out = tower(extra["ids"])
        assert out.shape == (7, 32) and torch.equal(out, tower.proj(tower.forward_hidden(extra["ids"])))
        # 37 given tokens (the tower pads to 40 itself): the captions that fit are unchanged
        short = tower.forward_hidden(extra["ids"][:, :37])
        # an all-pad row pools position 0; a pad id inside a caption does not end it
        ids = extra["ids"].clone()
        ids[1] = 0
        ids[2, 5] = 0
        odd = tower.forward_hidden(ids)
        first = tower.forward_hidden(ids[1:2, :1])                        # that row's position 0 alone
        whole = build_tower(pad_id=None).forward_hidden(ids[2:3, :32])    # caption 2 to its end, row T - 1
    for b, n in enumerate(LENGTHS):
        if n <= 37:
            assert nerr(short[b], ref[b]) < TOL, n
    assert nerr(odd[1], first[0]) < TOL
    assert nerr(odd[2], whole[0]) < TOL and nerr(odd[0], ref[0]) < TOL


def test_restatement_positions():
    tokens = torch.tensor([[5, 0, 7, 0], [0, 0, 0, 0], [1, 2, 3, 4], [0, 9, 0, 0]])
    x = torch.randn(4, 8, 4)
    _, pos = last_token_rmsnorm_ref(tokens, 0, x, None, torch.ones(4))
    assert pos.tolist() == [2, 0, 3, 1]


def test_loader_is_strict():
    from mamba_clip_amd.model import load_hf_mamba_state_dict
    sd, _, _ = fixture()
    tower = build_tower()
    proj = tower.proj.weight.detach().clone()
    # a "backbone." prefix is stripped and MambaForCausalLM's lm_head is ignored
    ok = {"backbone." + k: v for k, v in sd.items()}
    ok["lm_head.weight"] = torch.zeros(96, 128)
    load_hf_mamba_state_dict(tower, ok)
    tower.load_hf_mamba_state_dict(sd)
    assert torch.equal(tower.proj.weight, proj)
    assert torch.equal(tower.embedding.weight, sd["embeddings.weight"])
    assert torch.equal(tower.norm_f, sd["norm_f.weight"])
    assert torch.equal(tower.layers[1].norm_weight, sd["layers.1.norm.weight"])
    for name in ("A_log", "D", "conv1d.weight", "conv1d.bias", "in_proj.weight", "x_proj.weight", "dt_proj.weight",
                 "dt_proj.bias", "out_proj.weight"):
        assert torch.equal(tower.layers[1].mixer.get_parameter(name), sd[f"layers.1.mixer.{name}"]), name
    missing = {k: v for k, v in sd.items() if k != "layers.1.mixer.dt_proj.bias"}
    with pytest.raises(KeyError, match="missing.*layers.1.mixer.dt_proj.bias"):
        load_hf_mamba_state_dict(tower, missing)
    with pytest.raises(KeyError, match="unexpected.*layers.2.norm.weight"):
        load_hf_mamba_state_dict(tower, dict(sd, **{"layers.2.norm.weight": torch.zeros(128)}))
    with pytest.raises(ValueError, match="embeddings.weight"):
        load_hf_mamba_state_dict(tower, dict(sd, **{"embeddings.weight": torch.zeros(97, 128)}))
    assert torch.equal(tower.embedding.weight, sd["embeddings.weight"])      # a rejected dict changes nothing


def test_config_key_builds():
    from mamba_clip_amd.cli import build_parser
    from mamba_clip_amd.model import MODEL_CONFIGS, MambaTextEncoder, build_clip
    hf, old = MODEL_CONFIGS["vit_b16-mamba130m-hf"], MODEL_CONFIGS["vit_b16-mamba130m"]
    assert hf["text"] == dict(old["text"], pad_id=0) and hf["vision"] == old["vision"]
    with torch.device("meta"):
        m = build_clip("vit_b16-mamba130m-hf")
        o = build_clip("vit_b16-mamba130m")
    assert isinstance(m.text, MambaTextEncoder) and m.text.pad_id == 0 and o.text.pad_id is None
    assert [tuple(p.shape) for p in m.text.parameters()] == [tuple(p.shape) for p in o.text.parameters()]
    # mamba-130m-hf's backbone: 129.1 M parameters (the tied lm_head is the embedding)
    assert sum(p.numel() for n, p in m.text.named_parameters() if not n.startswith("proj.")) == 129_135_360
    args = build_parser().parse_args(["--model", "vit_b16-mamba130m-hf", "--text-min-len", "8"])
    assert args.text_min_len == 8 and build_parser().parse_args([]).text_min_len is None


def _todays_synthetic_batch(batch, image_size, context_length, vocab_size, num_classes=2, seed=0):
    """data.synthetic_batch before text_min_len existed (float images), draw for draw."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    images = torch.randn(batch, 3, image_size, image_size, generator=g)
    texts = torch.randint(1, vocab_size - 1, (batch, context_length), generator=g)
    texts[:, -1] = vocab_size - 1
    targets = torch.randint(0, num_classes, (batch,), generator=g)
    return images, texts, targets


def _check_padded(texts, lo, ctx, eot):
    lengths = (texts != 0).sum(1)
    assert int(lengths.min()) >= lo and int(lengths.max()) <= ctx
    rows = torch.arange(texts.shape[0])
    assert (texts[rows, lengths - 1] == eot).all()
    assert ((torch.arange(ctx)[None] < lengths[:, None]) == (texts != 0)).all()     # right padding only
    return lengths


def test_text_min_len_default_is_unchanged_and_set_pads():
    from mamba_clip_amd.data import IsicShapedDataset, get_synthetic_data, synthetic_batch
    want = _todays_synthetic_batch(16, 8, 20, 50, seed=3)
    for kw in ({}, {"text_min_len": None}):
        got = synthetic_batch(16, 8, 20, 50, seed=3, **kw)
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    images, texts, targets = synthetic_batch(64, 8, 20, 50, seed=3, text_min_len=4)
    im0, tx0, tg0 = _todays_synthetic_batch(64, 8, 20, 50, seed=3)
    assert torch.equal(images, im0) and torch.equal(targets, tg0)        # the lengths are drawn last
    lengths = _check_padded(texts, 4, 20, 49)
    assert len(set(lengths.tolist())) > 4 and int(lengths.min()) < 20
    for b in range(64):       # in front of end-of-text the ids are the unpadded batch's
        assert torch.equal(texts[b, : lengths[b] - 1], tx0[b, : lengths[b] - 1])
    _check_padded(synthetic_batch(8, 8, 20, 50, seed=1, text_min_len=20)[1], 20, 20, 49)
    _check_padded(synthetic_batch(32, 8, 20, 50, seed=1, text_min_len=1)[1], 1, 20, 49)
    with pytest.raises(ValueError, match="text_min_len"):
        synthetic_batch(8, 8, 20, 50, text_min_len=21)

    a, b = IsicShapedDataset(32, 8, 20, 50, seed=5), IsicShapedDataset(32, 8, 20, 50, seed=5, text_min_len=None)
    g = torch.Generator().manual_seed(5)
    im = torch.randint(0, 256, (32, 8, 8, 3), dtype=torch.uint8, generator=g)
    tx = torch.randint(1, 49, (32, 20), generator=g)
    tx[:, -1] = 49
    tg = (torch.rand(32, generator=g) < 0.01).long()
    for ds in (a, b):
        assert torch.equal(ds.images, im) and torch.equal(ds.texts, tx) and torch.equal(ds.targets, tg)
    c = IsicShapedDataset(32, 8, 20, 50, seed=5, text_min_len=6)
    assert torch.equal(c.images, im) and torch.equal(c.targets, tg)
    _check_padded(c.texts, 6, 20, 49)

    data = get_synthetic_data(8, 2, 8, 20, 50, "cpu", seed=9, val_batches=1, text_min_len=5)
    for split in ("train", "val"):
        for _, t, _ in data[split].dataloader:
            _check_padded(t, 5, 20, 49)
