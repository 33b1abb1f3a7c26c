"""Patch dropout on the GPU (include/mc_ops.h: mc_patch_embed_input_gather, mc_token_embed_gather_fwd / _bwd;
ops.patch_im2col(keep=), ops.token_embed_gather; VisionTransformer(patch_dropout=); --force-patch-dropout).

The kernels move and add values without rounding of their own, so they are compared bit for bit: the
gather im2col with the rows of the full im2col, the token embedding with the torch expression it
replaces, the position-table gradient (integer-valued dm: every fp32 sum exact) with an fp64 index_add_.
The tower is compared with its unfused restatement -- full patch embed, token_embed, a row gather, the
same blocks -- at the fp32 tower tolerances of tests/test_model_gpu.py, and under bf16 autocast by the
error of both against the fp64 CPU module."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

MEAN, STD = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _random_keep(B, n, n_keep, g, exclude=None):
    """(B, n_keep) int32 sorted distinct indices in [0, n); no row holds `exclude`."""
    pool = torch.tensor([j for j in range(n) if j != exclude])
    rows = [pool[torch.randperm(len(pool), generator=g)[:n_keep]].sort().values for _ in range(B)]
    return torch.stack(rows).to(torch.int32)


# ---------------------------------------------------------------------------- 1. gather im2col
def _image(B, C, H, W, in_dt, seed):
    if in_dt == torch.uint8:
        return torch.randint(0, 256, (B, H, W, C), dtype=torch.uint8, generator=_gen(seed))
    return torch.randn(B, C, H, W, generator=_gen(seed)).to(in_dt)


def _check_gather(img, P, n, keep, out_dt, **norm):
    from mamba_clip_amd.ops import patch_im2col
    B = img.shape[0]
    img, keep = img.to(DEV), keep.to(DEV)
    full = patch_im2col(img, P, out_dt, **norm)
    got = patch_im2col(img, P, out_dt, keep=keep, **norm)
    rows = (torch.arange(B, device=DEV)[:, None] * n + keep.long()).reshape(-1)
    want = full.index_select(0, rows)
    assert got.dtype == out_dt and got.shape == want.shape
    torch.testing.assert_close(got, want, rtol=0, atol=0)
    return got, full


GATHER_SHAPES = [(3, 3, 32, 48, 16, 4), (2, 1, 8, 8, 4, 1), (2, 3, 24, 24, 8, 9)]
GATHER_DTYPES = [(torch.float32, torch.float32), (torch.float32, torch.bfloat16), (torch.bfloat16, torch.bfloat16),
                 (torch.float16, torch.float16), (torch.uint8, torch.bfloat16), (torch.uint8, torch.float32)]


@pytest.mark.parametrize("shape", GATHER_SHAPES)
@pytest.mark.parametrize("in_dt,out_dt", GATHER_DTYPES)
def test_gather_im2col_equals_rows_of_the_full_one(shape, in_dt, out_dt):
    B, C, H, W, P, n_keep = shape
    if in_dt == torch.uint8:
        C = 3 if out_dt == torch.bfloat16 else 1     # uint8 NHWC: C = 3 -> bf16 with mean / std, C = 1 -> f32
    n = (H // P) * (W // P)
    norm = dict(mean=MEAN, std=STD) if (in_dt == torch.uint8 and C == 3) else {}
    img = _image(B, C, H, W, in_dt, seed=H + P)
    keep = _random_keep(B, n, n_keep, _gen(n_keep))
    if n_keep == n:
        keep = torch.arange(n, dtype=torch.int32).expand(B, n).contiguous()
    got, full = _check_gather(img, P, n, keep, out_dt, **norm)
    if n_keep == n:
        torch.testing.assert_close(got, full, rtol=0, atol=0)      # keep = arange: the full output


def test_gather_im2col_unsorted_keep():
    B, C, H, W, P = 3, 3, 32, 48, 16
    img = _image(B, C, H, W, torch.float32, seed=1)
    keep = torch.tensor([[5, 0, 3, 1], [2, 4, 1, 0], [0, 5, 4, 2]], dtype=torch.int32)
    _check_gather(img, P, 6, keep, torch.bfloat16)


def test_gather_im2col_c2_shape_64_bit_offsets():
    """uint8, B = 256, 224 x 224 x 3 -> bf16, n_keep = 98: the rows of the 77 MB full output."""
    B, n = 256, 196
    img = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, generator=_gen(0))
    order = torch.rand(B, n, generator=_gen(1)).argsort(1)[:, :98].sort(1).values.to(torch.int32)
    _check_gather(img, 16, n, order, torch.bfloat16)


def test_gather_im2col_input_gradient_scatters_into_zeros():
    from mamba_clip_amd.ops import patch_im2col
    img = torch.randn(2, 3, 32, 32, device=DEV, requires_grad=True)
    keep = torch.tensor([[0, 5, 10], [3, 4, 15]], dtype=torch.int32, device=DEV)
    g = torch.randn(2 * 3, 3 * 64, device=DEV)
    patch_im2col(img, 8, torch.float32, keep=keep).backward(g)
    full = torch.zeros(2, 16, 192, device=DEV)
    full[torch.arange(2, device=DEV)[:, None], keep.long()] = g.view(2, 3, 192)
    ref = torch.nn.functional.fold(full.transpose(1, 2), (32, 32), 8, stride=8)
    assert torch.equal(img.grad, ref)


# ---------------------------------------------------------------------------- 2. / 3. token embedding
TOKEN_SHAPES = [(5, 6, 4, 64, torch.bfloat16), (3, 16, 1, 64, torch.float16), (4, 16, 16, 128, torch.float32),
                (64, 196, 49, 768, torch.bfloat16)]


def _token_inputs(B, n, n_keep, C, dt, seed=0):
    from mamba_clip_amd.ops import keep_slots
    g = _gen(seed + B + n)
    cls = torch.randn(1, 1, C, generator=g).to(DEV)
    pos = torch.randn(1, n + 1, C, generator=g).to(DEV)
    x = torch.randn(B, n_keep, C, generator=g).to(dt).to(DEV)
    # patch n - 1 is kept by no sample wherever a patch is dropped at all
    keep = _random_keep(B, n, n_keep, g, exclude=n - 1 if n_keep < n else None).to(DEV)
    return cls, pos, x, keep, keep_slots(keep, n)


def _token_embed_torch(cls, x, pos, keep):
    """cat([cls.to(dt), x], 1) + pos.to(dt), the table's rows taken per sample."""
    B = x.shape[0]
    pe = pos.to(x.dtype)
    prow = torch.cat([pe[:, :1].expand(B, -1, -1), pe[0][1 + keep.long()]], dim=1)
    return torch.cat([cls.to(x.dtype).expand(B, -1, -1), x], dim=1) + prow


@pytest.mark.parametrize("shape", TOKEN_SHAPES)
def test_token_embed_gather_fwd_bit_exact(shape):
    from mamba_clip_amd.ops import token_embed_gather
    B, n, n_keep, C, dt = shape
    cls, pos, x, keep, slot = _token_inputs(*shape)
    got = token_embed_gather(cls, x, pos, keep, slot)
    want = _token_embed_torch(cls, x, pos, keep)
    assert got.dtype == dt and got.shape == (B, n_keep + 1, C)
    torch.testing.assert_close(got, want, rtol=0, atol=0)


def test_token_embed_gather_odd_width_shape_error_and_torch_result():
    from mamba_clip_amd import _lib
    from mamba_clip_amd.ops import token_embed_gather
    B, n, n_keep, C, dt = 3, 6, 4, 12, torch.bfloat16
    cls, pos, x, keep, slot = _token_inputs(B, n, n_keep, C, dt)
    out = torch.full((B, n_keep + 1, C), 7.0, device=DEV, dtype=dt)
    p = _lib.TokenEmbedGatherParams()
    p.batch, p.n, p.n_keep, p.cols, p.dtype = B, n, n_keep, C, _lib.MC_DTYPE_BF16
    p.cls, p.pos, p.x, p.keep, p.out = cls.data_ptr(), pos.data_ptr(), x.data_ptr(), keep.data_ptr(), out.data_ptr()
    lib = _lib.load()
    assert lib.mc_token_embed_gather_fwd(ctypes.byref(p), _lib.stream_handle()) == -3          # MC_ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                            # nothing launched
    x.requires_grad_(True)
    cls.requires_grad_(True)
    pos.requires_grad_(True)
    got = token_embed_gather(cls, x, pos, keep, slot)
    torch.testing.assert_close(got, _token_embed_torch(cls, x, pos, keep), rtol=0, atol=0)
    got.float().sum().backward()                                                               # torch autograd
    assert pos.grad.shape == pos.shape and bool((pos.grad[0, n] == 0).all())


def _dpos_fp64(dm, slot, n_keep):
    B, _, C = dm.shape
    n = slot.shape[1]
    ref = torch.zeros(n + 1, C, dtype=torch.float64, device=dm.device)
    ref[0] = dm[:, 0].double().sum(0)
    b_idx, j_idx = ((slot >= 0) & (slot < n_keep)).nonzero(as_tuple=True)
    ref.index_add_(0, 1 + j_idx, dm[b_idx, 1 + slot[b_idx, j_idx].long()].double())
    return ref


def _dpos_kernel(dm, slot, n_keep, fill=float("nan")):
    from mamba_clip_amd import _lib
    B, _, C = dm.shape
    n = slot.shape[1]
    dpos = torch.full((n + 1, C), fill, device=DEV, dtype=torch.float32)
    p = _lib.TokenEmbedGatherParams()
    p.batch, p.n, p.n_keep, p.cols, p.dtype = B, n, n_keep, C, _lib.dtype_code(dm.dtype)
    p.dm, p.slot, p.dpos = dm.data_ptr(), slot.data_ptr(), dpos.data_ptr()
    _lib.check(_lib.load().mc_token_embed_gather_bwd(ctypes.byref(p), _lib.stream_handle()), "mc_token_embed_gather_bwd")
    return dpos


@pytest.mark.parametrize("shape", TOKEN_SHAPES)
def test_token_embed_gather_bwd_exact_and_writes_every_row(shape):
    B, n, n_keep, C, dt = shape
    _, _, _, keep, slot = _token_inputs(*shape)
    nobody = n - 1
    if n_keep == n:
        # every sample keeps every patch here: mark one position as not kept with values outside [0, n_keep)
        slot = slot.clone()
        slot[:, nobody] = torch.tensor([-1, n_keep, -7, n_keep + 5], dtype=torch.int32, device=DEV)[:B]
    assert not bool(((slot[:, nobody] >= 0) & (slot[:, nobody] < n_keep)).any())
    dm = torch.randint(-4, 5, (B, n_keep + 1, C), generator=_gen(B)).to(dt).to(DEV)
    dpos = _dpos_kernel(dm, slot, n_keep)                      # the table starts as NaN
    assert not bool(torch.isnan(dpos).any())
    assert bool((dpos[1 + nobody] == 0).all())
    torch.testing.assert_close(dpos.double(), _dpos_fp64(dm, slot, n_keep), rtol=0, atol=0)


@pytest.mark.parametrize("shape", TOKEN_SHAPES)
def test_token_embed_gather_autograd(shape):
    """d pos from the kernel, d cls = d pos[0], d x the view dm[:, 1:]."""
    from mamba_clip_amd.ops import token_embed_gather
    B, n, n_keep, C, dt = shape
    cls, pos, x, keep, slot = _token_inputs(*shape)
    for t in (cls, pos, x):
        t.requires_grad_(True)
    m = token_embed_gather(cls, x, pos, keep, slot)
    dm = torch.randint(-4, 5, (B, n_keep + 1, C), generator=_gen(n)).to(dt).to(DEV)
    dcls, dx, dpos = torch.autograd.grad(m, (cls, x, pos), dm)
    torch.testing.assert_close(dpos[0].double(), _dpos_fp64(dm, slot, n_keep), rtol=0, atol=0)
    assert torch.equal(dcls[0, 0], dpos[0, 0])
    assert dx.data_ptr() == dm[:, 1:].data_ptr() and dx.stride() == dm[:, 1:].stride() and dx.shape == x.shape
    if n_keep < n:
        assert bool((dpos[0, n] == 0).all())                   # patch n - 1: nobody kept it


@pytest.mark.parametrize("shape", TOKEN_SHAPES)
def test_token_embed_gather_bwd_deterministic_and_close_to_fp64(shape):
    B, n, n_keep, C, dt = shape
    _, _, _, keep, slot = _token_inputs(*shape)
    dm = torch.randn(B, n_keep + 1, C, generator=_gen(C)).to(dt).to(DEV)
    a = _dpos_kernel(dm, slot, n_keep)
    b = _dpos_kernel(dm, slot, n_keep, fill=3.0)
    assert torch.equal(a, b)
    torch.testing.assert_close(a.double(), _dpos_fp64(dm, slot, n_keep), rtol=1e-3, atol=1e-3 * B ** 0.5)


# ---------------------------------------------------------------------------- 4. / 5. the tower
KEEP_4x8 = [[0, 3, 5, 6, 9, 10, 12, 15], [1, 2, 3, 5, 6, 7, 8, 11], [0, 1, 2, 3, 12, 13, 14, 15],
            [2, 3, 5, 7, 8, 11, 13, 14]]      # 8 of 16 patches per image; nobody keeps patch 4


def _unfused_tower(vit, img, keep):
    """token_embed(cls, patch_embed(x), pos), a row gather, the same blocks and head."""
    from mamba_clip_amd.model import _run_blocks
    from mamba_clip_amd.ops import add_layernorm, token_embed
    B = img.shape[0]
    m = token_embed(vit.cls_token, vit.patch_embed(img), vit.pos_embed)
    rows = torch.cat([torch.zeros(B, 1, dtype=torch.long, device=img.device), 1 + keep.long()], 1)
    m = m.gather(1, rows[:, :, None].expand(-1, -1, m.shape[-1]))
    m, h = _run_blocks(vit.blocks, m, None, False)
    y, _ = add_layernorm(m[:, 0], h[:, 0], vit.norm.weight, vit.norm.bias, vit.norm.eps)
    return vit.head(y)


def _grads(vit, out, w):
    vit.zero_grad(set_to_none=True)
    (out.float() * w).sum().backward()
    return {k: p.grad.detach().clone() for k, p in vit.named_parameters()}


def test_tower_fp32_matches_unfused_restatement():
    from mamba_clip_amd.model import VisionTransformer
    torch.manual_seed(0)
    vit = VisionTransformer(img_size=32, patch=8, width=64, layers=2, heads=4, output_dim=32, patch_dropout=0.5)
    vit = vit.to(DEV).train()
    img = torch.randn(4, 3, 32, 32, device=DEV)
    keep = torch.tensor(KEEP_4x8, dtype=torch.int32, device=DEV)
    w = torch.randn(4, 32, device=DEV)
    out = vit(img, keep=keep)
    assert torch.equal(vit.last_keep, keep)
    got = _grads(vit, out, w)
    ref_out = _unfused_tower(vit, img, keep)
    ref = _grads(vit, ref_out, w)
    torch.testing.assert_close(out.detach(), ref_out.detach(), rtol=1e-4, atol=1e-5)
    assert set(got) == set(ref) and {"pos_embed", "cls_token", "patch_embed.proj.weight", "patch_embed.proj.bias"} <= set(got)
    for k in ref:
        torch.testing.assert_close(got[k], ref[k], rtol=1e-3, atol=1e-5 * float(ref[k].abs().max()), msg=k)
    assert bool((got["pos_embed"][0, 1 + 4] == 0).all())                  # patch 4: kept by nobody
    assert bool((got["pos_embed"][0, 1 + 3] != 0).any())


def test_tower_bf16_fused_attention_error_vs_fp64():
    """e_fused <= 2 * e_unfused against the fp64 CPU module, for the features and every parameter gradient.
    Both paths round at the same points; the factor 2 covers another GEMM tile order for the shorter M."""
    import copy
    from mamba_clip_amd.model import VisionTransformer
    from oracle.cpu_model import oracle_ops
    torch.manual_seed(0)
    cpu = VisionTransformer(img_size=32, patch=8, width=128, layers=2, heads=2, output_dim=32, patch_dropout=0.5)
    vit = copy.deepcopy(cpu).to(DEV).train()
    cpu = cpu.double().train()
    img = torch.randn(4, 3, 32, 32)
    keep = torch.tensor(KEEP_4x8, dtype=torch.int32)
    w = torch.randn(4, 32)
    with oracle_ops():
        ref_out = cpu(img.double(), keep=keep)
        (ref_out * w.double()).sum().backward()
    ref = {k: p.grad for k, p in cpu.named_parameters()}
    seen = []
    hook = vit.blocks[0].attn.register_forward_pre_hook(lambda mod, args: seen.append(args[0].shape[1]))
    img, keep, w = img.to(DEV), keep.to(DEV), w.to(DEV)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = vit(img, keep=keep)
    hook.remove()
    assert vit.blocks[0].attn.last_path == "fused" and seen == [9]        # class token + 8 patches
    fused = _grads(vit, out, w)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out_u = _unfused_tower(vit, img, keep)
    unfused = _grads(vit, out_u, w)
    err = lambda a, b: float((a.detach().double().cpu() - b).abs().max())  # noqa: E731
    rows = [("features", err(out, ref_out.detach()), err(out_u, ref_out.detach()))]
    rows += [(k, err(fused[k], ref[k]), err(unfused[k], ref[k])) for k in ref]
    for name, e_fused, e_unfused in rows:
        print(f"patch dropout bf16 tower: {name}: e_fused {e_fused:.3e} e_unfused {e_unfused:.3e}")
    for name, e_fused, e_unfused in rows:
        assert e_fused <= 2 * e_unfused, (name, e_fused, e_unfused)


# ---------------------------------------------------------------------------- 6. training
def test_cli_trains_with_patch_dropout(capsys, monkeypatch):
    import importlib
    import json
    from mamba_clip_amd.cli import main as cli_main_fn
    cli = importlib.import_module("mamba_clip_amd.cli.main")     # the package exports the function under this name
    built = []
    build = cli.build_model
    monkeypatch.setattr(cli, "build_model", lambda args, device: built.append(build(args, device)) or built[-1])
    rc = cli_main_fn(["--synthetic", "--model", "tiny-mamba-clip", "--force-patch-dropout", "0.5", "--epochs", "1",
                      "--benchmark"])
    assert rc == 0
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1]
    loss = json.loads(line)["final"]["loss"]
    assert loss is not None and loss == loss and abs(loss) != float("inf")
    visual = built[0].visual
    assert visual.patch_dropout == 0.5 and visual.last_keep.shape == (64, 8)      # default batch 64; 8 of 16 patches


def _train_args():
    return SimpleNamespace(precision="amp_bf16", lr=1e-3, wd=0.2, beta1=0.9, beta2=0.98, eps=1e-6,
                           grad_clip_norm=None, accum_freq=1)


def _three_steps(seed):
    from mamba_clip_amd.data import synthetic_batch
    from mamba_clip_amd.loss import ClipLoss
    from mamba_clip_amd.model import build_clip
    from mamba_clip_amd.train import create_optimizer, train_step
    torch.manual_seed(seed)
    model = build_clip("tiny-mamba-clip", force_patch_dropout=0.5).to(DEV).train()
    args = _train_args()
    opt = create_optimizer(model, args)
    img, txt, tgt = synthetic_batch(8, 32, model.text.context_length, model.text.vocab_size, device=DEV)
    losses, keeps = [], []
    for _ in range(3):
        losses.append(train_step(model, img, txt, tgt, ClipLoss(), opt, None, args)["loss"].detach().clone())
        keeps.append(model.visual.last_keep.clone())
    return model, torch.stack(losses), keeps, (img, txt)


def test_training_is_repeatable_from_the_seed_and_eval_is_full():
    m1, l1, k1, (img, txt) = _three_steps(5)
    m2, l2, k2, _ = _three_steps(5)
    assert bool(torch.isfinite(l1).all()) and torch.equal(l1, l2)
    assert all(torch.equal(a, b) for a, b in zip(k1, k2))
    assert k1[0].shape == (8, 8) and not torch.equal(k1[0], k1[1])               # a fresh mask every step
    for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n
    m1.eval()
    with torch.no_grad():
        a = m1(img, txt)["image_features"]
        assert m1.visual.last_keep is None
        b = m1(img, txt)["image_features"]
    assert torch.equal(a, b) and m1.visual.last_keep is None


def test_graphed_step_refuses_active_patch_dropout():
    from mamba_clip_amd.data import synthetic_batch
    from mamba_clip_amd.loss import ClipLoss
    from mamba_clip_amd.model import build_clip
    from mamba_clip_amd.train import GraphedStep, create_optimizer
    model = build_clip("tiny-mamba-clip", force_patch_dropout=0.5).to(DEV).train()
    args = _train_args()
    args.capturable = True
    opt = create_optimizer(model, args)
    img, txt, tgt = synthetic_batch(8, 32, model.text.context_length, model.text.vocab_size, device=DEV)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match="patch dropout"):
        GraphedStep(model, img, txt, tgt, ClipLoss(), opt, args)
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))    # no warm-up step ran
    assert model.visual.last_keep is None
