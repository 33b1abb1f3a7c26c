"""Patch dropout off the GPU: the selection (ops.patch_keep_indices), the tower's semantics on the CPU
restatement ops (open_clip PatchDropout with exclude_first_token=True) and the CLI flag.  No HIP kernel runs."""
import pytest
import torch
import torch.nn.functional as F

TINY = dict(img_size=32, patch=8, width=64, layers=2, heads=4, output_dim=32)


@pytest.mark.parametrize("n,p,want", [(196, 0.5, 98), (196, 0.75, 49), (16, 0.5, 8), (4, 0.99, 1)])
def test_n_keep(n, p, want):
    from mamba_clip_amd.model import VisionTransformer
    from oracle.cpu_model import oracle_ops
    side = int(n ** 0.5)
    vit = VisionTransformer(img_size=4 * side, patch=4, width=16, layers=1, heads=2, output_dim=8, patch_dropout=p)
    assert vit.pos_embed.shape[1] == n + 1
    with oracle_ops(), torch.no_grad():
        vit.train()
        vit(torch.randn(3, 3, 4 * side, 4 * side))
    assert vit.last_keep.shape == (3, want)


@pytest.mark.parametrize("batch,n,n_keep", [(5, 196, 98), (3, 16, 1), (4, 16, 16), (7, 6, 4)])
def test_keep_indices_sorted_distinct_and_inverse(batch, n, n_keep):
    from mamba_clip_amd.ops import patch_keep_indices
    torch.manual_seed(3)
    keep, slot = patch_keep_indices(batch, n, n_keep, "cpu")
    assert keep.dtype == torch.int32 and slot.dtype == torch.int32
    assert keep.shape == (batch, n_keep) and slot.shape == (batch, n)
    assert int(keep.min()) >= 0 and int(keep.max()) < n
    if n_keep > 1:
        assert bool((keep[:, 1:] > keep[:, :-1]).all())          # ascending, so no duplicates either
    for b in range(batch):
        kept = set(keep[b].tolist())
        for j in range(n):
            if j in kept:
                assert keep[b, slot[b, j]] == j
            else:
                assert slot[b, j] == -1
        assert sorted(slot[b][slot[b] >= 0].tolist()) == list(range(n_keep))


def test_keep_indices_follow_the_seed():
    from mamba_clip_amd.ops import patch_keep_indices
    torch.manual_seed(11)
    a = patch_keep_indices(8, 196, 98, "cpu")
    torch.manual_seed(11)
    b = patch_keep_indices(8, 196, 98, "cpu")
    torch.manual_seed(12)
    c = patch_keep_indices(8, 196, 98, "cpu")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0])
    g = torch.Generator().manual_seed(5)
    d = patch_keep_indices(8, 196, 98, "cpu", generator=g)
    e = patch_keep_indices(8, 196, 98, "cpu", generator=torch.Generator().manual_seed(5))
    assert torch.equal(d[0], e[0])
    rows = {tuple(r.tolist()) for r in a[0]}
    assert len(rows) > 1                                          # samples draw independently


def _two_vits(p):
    from mamba_clip_amd.model import VisionTransformer
    torch.manual_seed(0)
    base = VisionTransformer(**TINY)
    drop = VisionTransformer(**TINY, patch_dropout=p)
    drop.load_state_dict(base.state_dict())
    return base, drop


def test_eval_is_bitwise_the_tower_without_dropout():
    from oracle.cpu_model import oracle_ops
    base, drop = _two_vits(0.5)
    img = torch.randn(3, 3, 32, 32)
    with oracle_ops(), torch.no_grad():
        want = base.eval()(img)
        got = drop.eval()(img)
        assert drop.last_keep is None
        # an explicit keep is for training-mode tests only: eval ignores it
        ignored = drop(img, keep=torch.tensor([[0, 1]] * 3, dtype=torch.int32))
        assert drop.last_keep is None
        # p == 0 in training mode runs the full tower as well
        full_train = base.train()(img)
        assert base.last_keep is None
    assert torch.equal(got, want) and torch.equal(ignored, want) and torch.equal(full_train, want)


def _restated(vit, img, keep):
    """Full embed, cat the class token, add pos, gather the kept rows, the textbook pre-LN blocks."""
    B = img.shape[0]
    x = vit.patch_embed.proj(img).flatten(2).transpose(1, 2)
    x = torch.cat([vit.cls_token.expand(B, -1, -1), x], 1) + vit.pos_embed
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long), 1 + keep.long()], 1)
    x = x.gather(1, rows[:, :, None].expand(-1, -1, x.shape[-1]))
    for blk in vit.blocks:
        x = x + blk.attn(blk.norm1(x))
        x = x + blk.fc2(F.gelu(blk.fc1(blk.norm2(x))))
    return vit.head(vit.norm(x)[:, 0])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_train_with_explicit_keep_equals_plain_torch(dtype):
    from oracle.cpu_model import oracle_ops
    _, vit = _two_vits(0.5)
    vit = vit.to(dtype).train()
    img = torch.randn(4, 3, 32, 32, dtype=dtype)
    keep = torch.tensor([[0, 3, 5, 6, 9, 10, 12, 15], [1, 2, 3, 5, 6, 7, 8, 11], [0, 1, 2, 3, 12, 13, 14, 15],
                         [2, 3, 5, 7, 8, 11, 13, 14]], dtype=torch.int32)
    with oracle_ops():
        out = vit(img, keep=keep)
        assert torch.equal(vit.last_keep, keep)
        out.square().sum().backward()
        got_dpos = vit.pos_embed.grad.clone()
        vit.zero_grad()
        ref = _restated(vit, img, keep)
        ref.square().sum().backward()
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-5)
    want_dpos = vit.pos_embed.grad
    torch.testing.assert_close(got_dpos, want_dpos, rtol=1e-3, atol=1e-5 * float(want_dpos.abs().max()))
    nobody = [j for j in range(16) if not bool((keep == j).any())]     # patch 4: its position gets no gradient
    assert nobody and all(bool((got_dpos[0, 1 + j] == 0).all()) for j in nobody)


def test_random_draw_in_training_mode_follows_the_seed():
    from oracle.cpu_model import oracle_ops
    _, vit = _two_vits(0.5)
    vit.train()
    img = torch.randn(4, 3, 32, 32)
    with oracle_ops(), torch.no_grad():
        torch.manual_seed(7)
        a, ka = vit(img), vit.last_keep
        torch.manual_seed(7)
        b, kb = vit(img), vit.last_keep
        c, kc = vit(img), vit.last_keep
    assert ka.shape == (4, 8) and torch.equal(ka, kb) and torch.equal(a, b)
    assert not torch.equal(ka, kc)                                # the next forward draws again


def test_patch_dropout_range_is_checked():
    from mamba_clip_amd.model import VisionTransformer
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="patch_dropout"):
            VisionTransformer(**TINY, patch_dropout=bad)


def test_cli_flag_parses_and_rejects_out_of_range(capsys):
    from mamba_clip_amd.cli import build_parser
    p = build_parser()
    assert p.parse_args(["--synthetic"]).force_patch_dropout is None
    assert p.parse_args(["--synthetic", "--force-patch-dropout", "0.5"]).force_patch_dropout == 0.5
    assert p.parse_args(["--synthetic", "--force-patch-dropout", "0"]).force_patch_dropout == 0.0
    for bad in ("1.0", "-0.1"):
        with pytest.raises(SystemExit):
            p.parse_args(["--synthetic", f"--force-patch-dropout={bad}"])
        assert "--force-patch-dropout" in capsys.readouterr().err


def test_build_model_sets_the_tower_at_stage_1_only():
    from mamba_clip_amd.cli import build_parser
    from mamba_clip_amd.cli.main import build_model
    from mamba_clip_amd.model import build_clip, init_model
    base = ["--synthetic", "--model", "tiny-mamba-clip", "--force-patch-dropout", "0.75"]
    m1 = build_model(build_parser().parse_args(base), "cpu")
    assert m1.visual.patch_dropout == 0.75
    m2 = build_model(build_parser().parse_args(base + ["--stage", "2"]), "cpu")
    assert m2.clip_model.visual.patch_dropout == 0.0
    m0 = build_model(build_parser().parse_args(base[:3]), "cpu")
    assert m0.visual.patch_dropout == 0.0
    assert build_clip("tiny-mamba-clip", force_patch_dropout=0.25).visual.patch_dropout == 0.25
    assert init_model("tiny-mamba-clip", force_patch_dropout=0.5)[0].visual.patch_dropout == 0.5
    assert build_clip("tiny-mamba-clip").visual.patch_dropout == 0.0


def test_graphed_step_refuses_active_dropout_before_any_gpu_work():
    """The check sits in front of the warm-up and the capture: it raises with CPU tensors and no GPU."""
    from types import SimpleNamespace
    from mamba_clip_amd.model import build_clip
    from mamba_clip_amd.train import GraphedStep
    model = build_clip("tiny-mamba-clip", force_patch_dropout=0.5).train()
    args = SimpleNamespace(precision="fp32", balanced_mixup=None)
    with pytest.raises(ValueError, match="patch dropout"):
        GraphedStep(model, None, None, None, None, None, args)
