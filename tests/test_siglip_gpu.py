"""GPU checks of the pairwise sigmoid (SigLIP) loss: the fused kernels (mc_sigmoid_loss_fwd / _grad)
through ops.sigmoid_logits_loss against the fp64 reference of tests/siglip_ref.py, the blocked
backward, bitwise determinism, the no-N x N guarantee, SigLipLoss, a train step and the CLI.

Tolerances are the fused CE's (test_loss_gpu.py): loss within 1e-5 (fp32) / 1e-3 (bf16) relative
+ 1e-6; dX / dY max-abs error within 1e-5 / 1e-2 of max|want|.  dscale and dbias are sums that
cancel (dscale to ~1e-5 at large N on random features), so their error is measured against the sum
of the absolute contributions (siglip_ref: abs_dscale, abs_dbias) times the same 1e-5 / 1e-3,
+ 1e-6."""
import functools
import json
import math
from types import SimpleNamespace

import pytest
import torch

from siglip_ref import grad_block_ref, sigmoid_logits_loss_full_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [
    (5, 7, 8, 0),            # small rectangular
    (64, 64, 32, 0),         # one wave quadrant
    (130, 130, 40, 0),       # tile remainders both ways, K not a multiple of the slice; rows of 80 B (bf16) /
                             # 160 B (fp32) are 16-B multiples: the kAligned = true instances
    (130, 130, 38, 0),       # rows of 76 B / 152 B: the kAligned = false instances of kEpi 4 / 5, K % V != 0
    (257, 200, 64, 0),       # 3 x 2 tiles
    (384, 384, 64, 0),       # full tiles, vector path
    (100, 300, 32, 128),     # a rank's positives in a later tile column
    (64, 192, 32, -64),      # no row has a positive
    (128, 128, 32, 1 << 20),  # no row has a positive
]
NEGATIVE_ONLY = {(64, 192, 32, -64), (128, 128, 32, 1 << 20)}
SCALE_BIAS = [(10.0, -10.0), (3.0, 0.5)]


def _features(M, N, K, row_off, dtype, seed):
    """X = normalize(randn); Y_j = normalize(X_i + 0.7 randn) for the paired rows j = i + row_off (so
    positives differ from negatives), normalize(randn) for the rest; rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    X = torch.nn.functional.normalize(torch.randn(M, K, generator=g), dim=-1)
    Y = torch.randn(N, K, generator=g)
    noise = torch.randn(M, K, generator=g)
    i = torch.arange(M)
    j = i + row_off
    ok = (j >= 0) & (j < N)
    Y[j[ok]] = X[i[ok]] + 0.7 * noise[i[ok]]
    Y = torch.nn.functional.normalize(Y, dim=-1)
    return X.to(dtype), Y.to(dtype)


@functools.lru_cache(maxsize=None)
def _case(M, N, K, row_off, dtype, scale, bias):
    """(X, Y, fp64 reference on the same rounded inputs), computed once per case."""
    X, Y = _features(M, N, K, row_off, dtype, seed=M * 7 + N * 3 + K)
    return X, Y, sigmoid_logits_loss_full_ref(X, Y, scale, bias, row_off, 1.0 / M)


def _run(X, Y, scale, bias, row_off, coef):
    from mamba_clip_amd.ops import sigmoid_logits_loss
    xd, yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
    sd = torch.tensor(scale, device=DEV, requires_grad=True)
    bd = torch.tensor(bias, device=DEV, requires_grad=True)
    loss = sigmoid_logits_loss(xd, yd, sd, bd, row_off, coef)
    loss.backward()
    return loss.detach(), xd.grad, yd.grad, sd.grad, bd.grad


def _check(got, ref, dtype, tag):
    loss, dX, dY, ds, db = got
    tol = 1e-5 if dtype == torch.float32 else 1e-3
    gtol = 1e-5 if dtype == torch.float32 else 1e-2
    want = float(ref["loss"])
    errs = {"loss": (abs(float(loss) - want), tol * abs(want) + 1e-6)}
    for name, g in (("dX", dX), ("dY", dY)):
        errs[name] = (float((g.double().cpu() - ref[name]).abs().max()), gtol * float(ref[name].abs().max()))
    errs["dscale"] = (abs(float(ds) - float(ref["dscale"])), tol * float(ref["abs_dscale"]) + 1e-6)
    errs["dbias"] = (abs(float(db) - float(ref["dbias"])), tol * float(ref["abs_dbias"]) + 1e-6)
    print(tag, {k: f"{e:.3e} / {b:.3e}" for k, (e, b) in errs.items()}, f"loss {float(loss):.8g} ref {want:.8g}")
    for k, (e, b) in errs.items():
        assert e <= b, (tag, k, e, b)


@pytest.mark.parametrize("scale,bias", SCALE_BIAS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("M,N,K,row_off", SHAPES)
def test_sigmoid_logits_loss_matches_fp64(M, N, K, row_off, dtype, scale, bias):
    X, Y, ref = _case(M, N, K, row_off, dtype, scale, bias)
    if (M, N, K, row_off) in NEGATIVE_ONLY:
        # nothing but small-argument softplus terms at (10, -10): an inaccurate log(1 + e) shows here
        assert ref["positives"] == 0 and float(ref["loss"]) > 0
    else:
        assert ref["positives"] >= 1
    _check(_run(X, Y, scale, bias, row_off, 1.0 / M), ref, dtype, (M, N, K, row_off, dtype, scale, bias))


@pytest.mark.parametrize("M,N,K,aligned", [(130, 130, 38, False), (128, 128, 64, True)])
def test_sigmoid_loss_grad_every_dtype_pair_per_element(M, N, K, aligned):
    """mc_sigmoid_loss_grad called directly for one block: all four <TIn, TOut> pairs of the kEpi 5
    instances (the autograd op only ever asks for G in the operands' dtype), kAligned false (76-B /
    152-B rows, ragged tiles) and true (one full tile: vector stores), every element of G against fp64
    within siglip_ref.grad_block_ref's bound; G bitwise equal with and without the scale / bias sums."""
    from mamba_clip_amd import ops
    scale, bias, coef = 10.0, -10.0, 1.0 / M
    gout = torch.tensor(-0.37, device=DEV)
    gout64 = float(gout.cpu().double())
    sd, bd = torch.tensor(scale, device=DEV), torch.tensor(bias, device=DEV)
    for in_dt in (torch.bfloat16, torch.float32):
        X, Y = _features(M, N, K, 0, in_dt, seed=M * 7 + N * 3 + K)
        Xd, Yd = X.to(DEV), Y.to(DEV)
        assert (Xd.data_ptr() % 16 == 0 and (Xd.stride(0) * Xd.element_size()) % 16 == 0) == aligned
        for g_dt in (torch.bfloat16, torch.float32):
            ref, bound = grad_block_ref(X, Y, scale, bias, 0, coef, gout64, g_dt == torch.bfloat16)
            G0, _, _ = ops.sigmoid_loss_grad(Xd, Yd, sd, bd, 0, coef, gout, g_dt)
            G1, ds, db = ops.sigmoid_loss_grad(Xd, Yd, sd, bd, 0, coef, gout, g_dt, want_stats=True)
            assert G0.dtype == g_dt and torch.equal(G0, G1)
            assert bool(torch.isfinite(ds)) and bool(torch.isfinite(db))
            got = G0.double().cpu()
            assert bool(torch.isfinite(got).all())
            ratio = float(((got - ref).abs() / bound).max())
            print((M, N, K), in_dt, g_dt, f"G err / bound {ratio:.3f}")
            assert ratio <= 1.0, (in_dt, g_dt, ratio)


@pytest.mark.parametrize("M,N,K,row_off,dtype", [(300, 1100, 96, 400, torch.float32),
                                                 (640, 640, 128, 0, torch.bfloat16)])
def test_sigmoid_loss_blocked_backward(monkeypatch, M, N, K, row_off, dtype):
    """Several row blocks (dX, dscale, dbias) and several column blocks of the transposed problem (dY)."""
    from mamba_clip_amd import ops
    monkeypatch.setattr(ops, "CE_GRAD_BLOCK_ELEMS", 128 * 256)
    assert ops._block_rows(N) < M and ops._block_rows(M) < N
    X, Y, ref = _case(M, N, K, row_off, dtype, 10.0, -10.0)
    assert ref["positives"] >= 1
    _check(_run(X, Y, 10.0, -10.0, row_off, 1.0 / M), ref, dtype, ("blocked", M, N, K, row_off, dtype))


def test_sigmoid_loss_is_deterministic_and_float_scalars_match_device_scalars(monkeypatch):
    from mamba_clip_amd import ops
    monkeypatch.setattr(ops, "CE_GRAD_BLOCK_ELEMS", 128 * 256)       # several blocks: the stacked sums too
    M, N, K, row_off = 257, 200, 64, 0
    for dtype in (torch.float32, torch.bfloat16):
        X, Y = _features(M, N, K, row_off, dtype, seed=3)
        a = _run(X, Y, 10.0, -10.0, row_off, 1.0 / M)
        b = _run(X, Y, 10.0, -10.0, row_off, 1.0 / M)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        # python-float scale / bias: same bits for the loss and the feature gradients
        xd, yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
        loss = ops.sigmoid_logits_loss(xd, yd, 10.0, -10.0, row_off, 1.0 / M)
        loss.backward()
        assert torch.equal(loss.detach(), a[0]) and torch.equal(xd.grad, a[1]) and torch.equal(yd.grad, a[2])


def test_sigmoid_loss_does_not_synchronise(monkeypatch):
    """Forward and blocked backward with device-scalar scale / bias make no host synchronisation."""
    from mamba_clip_amd import ops
    monkeypatch.setattr(ops, "CE_GRAD_BLOCK_ELEMS", 128 * 256)
    X, Y = _features(257, 200, 64, 0, torch.bfloat16, seed=3)
    xd, yd = X.to(DEV).requires_grad_(True), Y.to(DEV).requires_grad_(True)
    sd = torch.tensor(10.0, device=DEV, requires_grad=True)
    bd = torch.tensor(-10.0, device=DEV, requires_grad=True)
    ops.sigmoid_logits_loss(xd, yd, sd, bd, 0, 1.0 / 257).backward()     # warm-up: library handles, code objects
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.sigmoid_logits_loss(xd, yd, sd, bd, 0, 1.0 / 257).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.isfinite(sd.grad) and torch.isfinite(bd.grad)


def test_sigmoid_loss_no_n_by_n_allocation_c5_size():
    """N = 8192, E = 512, bf16: forward + backward never allocate an N x N buffer, and the loss agrees
    with a row-blocked dense evaluation on the device (fp32 logits from gemm_nt, 1024 rows at a time)."""
    from mamba_clip_amd.ops import gemm_nt, sigmoid_logits_loss
    N, E = 8192, 512
    X, Y = _features(N, N, E, 0, torch.bfloat16, seed=5)
    img, txt = X.to(DEV), Y.to(DEV)
    s = torch.tensor(10.0, device=DEV, requires_grad=True)
    b = torch.tensor(-10.0, device=DEV, requires_grad=True)
    i_d, t_d = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = sigmoid_logits_loss(i_d, t_d, s, b, 0, 1.0 / N)
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < N * N * 2, f"peak {peak / 2**20:.1f} MiB >= one bf16 N x N"
    loss = loss.detach()
    dense = torch.zeros((), device=DEV, dtype=torch.float64)
    for r0 in range(0, N, 1024):
        z = gemm_nt(img[r0:r0 + 1024], txt, alpha=10.0) - 10.0
        rows = torch.arange(r0, r0 + 1024, device=DEV)
        z[rows - r0, rows] *= -1.0                                   # positives: softplus(-z)
        dense += torch.nn.functional.softplus(z.double()).sum()
    dense = float(dense) / N
    print("N=8192 loss", float(loss), "dense", dense, "peak MiB", peak / 2**20)
    assert abs(float(loss) - dense) <= 1e-3 * abs(dense)
    for t in (i_d.grad, t_d.grad, s.grad, b.grad):
        assert torch.isfinite(t).all()


def test_siglip_loss_module_equals_op():
    from mamba_clip_amd.loss import SigLipLoss
    from mamba_clip_amd.ops import sigmoid_logits_loss
    n, E = 96, 32
    X, Y = _features(n, n, E, 0, torch.float32, seed=9)
    img, txt = X.to(DEV), Y.to(DEV)
    s, b = torch.tensor(10.0, device=DEV), torch.tensor(-10.0, device=DEV)
    crit = SigLipLoss()
    out = crit(img, txt, s, b)
    assert set(out) == {"contrastive_loss"}
    want = sigmoid_logits_loss(img, txt, s, b, 0, 1.0 / n)
    assert torch.equal(out["contrastive_loss"], want)
    assert torch.equal(crit(img, txt, s, b, output_dict=False, target=torch.zeros(n, device=DEV)), want)
    # the inspection helpers restate the same loss densely
    z = crit.get_logits(img, txt, s, b)
    y = crit.get_ground_truth(img.device, z.dtype, n)
    dense = -torch.nn.functional.logsigmoid(y * z).sum() / n
    assert abs(float(dense) - float(want)) <= 1e-5 * float(want)


def test_siglip_loss_module_world_2_uses_rank_offset(monkeypatch):
    """rank 1 of 2: its b images against the gathered 2b texts, positives at column b + i, weight 1/b."""
    import torch.distributed.nn
    import mamba_clip_amd.loss as L
    b, E = 40, 32
    X_all, T_all = _features(2 * b, 2 * b, E, 0, torch.float32, seed=12)
    T_all, img = T_all.to(DEV), X_all[b:].to(DEV)
    monkeypatch.setattr(torch.distributed.nn, "all_gather", lambda t: (T_all[:b], T_all[b:]))
    calls = []
    real = L.sigmoid_logits_loss

    def spy(X, Y, scale, bias, row_off=0, coef=1.0):
        calls.append((tuple(X.shape), tuple(Y.shape), row_off, coef))
        return real(X, Y, scale, bias, row_off, coef)

    monkeypatch.setattr(L, "sigmoid_logits_loss", spy)
    s, bias = torch.tensor(10.0, device=DEV), torch.tensor(-10.0, device=DEV)
    loss = L.SigLipLoss(rank=1, world_size=2)(img, T_all[b:], s, bias)["contrastive_loss"]
    assert calls == [((b, E), (2 * b, E), b, 1.0 / b)]
    ref = sigmoid_logits_loss_full_ref(img.cpu(), T_all.cpu(), 10.0, -10.0, b, 1.0 / b)
    assert ref["positives"] == b
    assert abs(float(loss) - float(ref["loss"])) <= 1e-5 * float(ref["loss"]) + 1e-6


def test_siglip_train_step_tiny_model():
    from mamba_clip_amd.loss import ClipLoss, SigLipLoss
    from mamba_clip_amd.model import build_clip
    from mamba_clip_amd.ops import sigmoid_logits_loss
    from mamba_clip_amd.train import create_optimizer, train_step
    torch.manual_seed(0)
    model = build_clip("tiny-mamba-clip", init_logit_scale=math.log(10), init_logit_bias=-10).to(DEV)
    args = SimpleNamespace(precision="fp32", lr=1e-3, wd=0.1, beta1=0.9, beta2=0.98, eps=1e-8, grad_clip_norm=None)
    g = torch.Generator().manual_seed(2)
    images = torch.randn(8, 3, 32, 32, generator=g).to(DEV)
    texts = torch.randint(1, 999, (8, 16), generator=g).to(DEV)
    targets = torch.zeros(8, dtype=torch.long, device=DEV)
    opt = create_optimizer(model, args)
    with torch.no_grad():
        out = model(images, texts)
        assert "logit_bias" in out
        want = sigmoid_logits_loss(out["image_features"], out["text_features"], out["logit_scale"],
                                   out["logit_bias"], 0, 1.0 / 8)
    with pytest.raises(TypeError):                 # ClipLoss has no logit_bias argument: unchanged
        train_step(model, images, texts, targets, ClipLoss(), opt, None, args)
    bias_before = model.logit_bias.detach().clone()
    losses = train_step(model, images, texts, targets, SigLipLoss(), opt, None, args)
    loss = float(losses["contrastive_loss"].detach())
    assert math.isfinite(loss) and abs(loss - float(want)) <= 1e-5 * abs(float(want))
    assert model.logit_bias.grad is not None and model.logit_scale.grad is not None
    assert torch.isfinite(model.logit_bias.grad) and torch.isfinite(model.logit_scale.grad)
    assert float(model.logit_bias.grad) != 0.0
    assert not torch.equal(model.logit_bias.detach(), bias_before)


def test_cli_siglip_synthetic_tiny(capsys):
    from mamba_clip_amd.cli import main
    rc = main(["--synthetic", "--model", "tiny-mamba-clip", "--siglip", "--batch-size", "8",
               "--train-num-samples", "32", "--val-frequency", "1", "--benchmark"])
    assert rc == 0
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["final"]["loss"] is not None and math.isfinite(out["final"]["loss"])
    assert out["val"] and all(v is not None and math.isfinite(v) for v in out["val"].values())
    assert "val_loss" in out["val"]
