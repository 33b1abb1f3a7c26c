"""CPU checks of the SigLIP path around the kernels: the fp64 reference itself on a hand-computed
case, loss selection, the --siglip switch, the model factory's logit_scale / logit_bias init, and
the multi-process (gloo) host logic of SigLipLoss with the HIP op replaced by the reference (the op
itself is checked on the GPU in test_siglip_gpu.py)."""
import math
import os
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT
from siglip_ref import label_mask, sigmoid_logits_loss_full_ref, sigmoid_logits_loss_ref


def _sp(t):
    return math.log1p(math.exp(t))


def test_reference_on_hand_computed_3x4():
    """X = rows of 0/1, Y likewise, scale 2, bias -1, row_off 1: every z is -1, 1 or 3."""
    X = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    Y = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 0.0]])
    # dots = [[1 0 1 0], [0 1 1 0], [1 1 2 0]];  z = 2 dots - 1 = [[1 -1 1 -1], [-1 1 1 -1], [1 1 3 -1]]
    # positives at (0, 1), (1, 2), (2, 3): z = -1, 1, -1 -> softplus(-z) = sp(1), sp(-1), sp(1)
    # negatives: row 0: z = 1, 1, -1; row 1: -1, 1, -1; row 2: 1, 1, 3 -> softplus(z)
    want = (_sp(1) + _sp(-1) + _sp(1)) + (2 * _sp(1) + _sp(-1)) + (2 * _sp(-1) + _sp(1)) + (2 * _sp(1) + _sp(3))
    coef = 0.25
    got = sigmoid_logits_loss_ref(X, Y, 2.0, -1.0, row_off=1, coef=coef)
    assert got.dtype == torch.float64 and abs(float(got) - coef * want) < 1e-14
    full = sigmoid_logits_loss_full_ref(X, Y, 2.0, -1.0, row_off=1, coef=coef)
    assert abs(float(full["loss"]) - coef * want) < 1e-14 and full["positives"] == 3
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))  # noqa: E731
    z = [[1, -1, 1, -1], [-1, 1, 1, -1], [1, 1, 3, -1]]
    g = [[coef * (sig(z[i][j]) - (1.0 if j == i + 1 else 0.0)) for j in range(4)] for i in range(3)]
    dbias = sum(sum(r) for r in g)
    dots = [[1, 0, 1, 0], [0, 1, 1, 0], [1, 1, 2, 0]]
    dscale = sum(g[i][j] * dots[i][j] for i in range(3) for j in range(4))
    assert abs(float(full["dbias"]) - dbias) < 1e-14 and abs(float(full["dscale"]) - dscale) < 1e-14
    # dX[0] = scale * sum_j g[0][j] Y[j]
    dx0 = [2.0 * sum(g[0][j] * float(Y[j, k]) for j in range(4)) for k in range(2)]
    assert torch.allclose(full["dX"][0], torch.tensor(dx0, dtype=torch.float64), atol=1e-14)
    # the closed forms agree with autograd through the differentiable restatement
    Xr, Yr = X.double().requires_grad_(True), Y.double().requires_grad_(True)
    s, b = torch.tensor(2.0, dtype=torch.float64, requires_grad=True), torch.tensor(-1.0, dtype=torch.float64,
                                                                                    requires_grad=True)
    sigmoid_logits_loss_ref(Xr, Yr, s, b, row_off=1, coef=coef).backward()
    for got_t, name in ((Xr.grad, "dX"), (Yr.grad, "dY"), (s.grad, "dscale"), (b.grad, "dbias")):
        assert torch.allclose(got_t, full[name], rtol=1e-12, atol=1e-14), name


def test_reference_rows_without_a_positive():
    assert int(label_mask(64, 192, -64).sum()) == 0 and int(label_mask(128, 128, 1 << 20).sum()) == 0
    assert int(label_mask(100, 300, 128).sum()) == 100 and int(label_mask(5, 7, 0).sum()) == 5
    assert int(label_mask(4, 4, 2).sum()) == 2


def test_create_loss_selection():
    from mamba_clip_amd.loss import ClipLoss, SigLipLoss, create_loss
    base = dict(local_loss=True, gather_with_grad=True, rank=1, world_size=2)
    plain = create_loss(SimpleNamespace(**base))
    assert type(plain) is ClipLoss and plain.local_loss and plain.gather_with_grad and plain.cache_labels
    assert (plain.rank, plain.world_size) == (1, 2)
    assert type(create_loss(SimpleNamespace(siglip=False, **base))) is ClipLoss
    sig = create_loss(SimpleNamespace(siglip=True, **base))
    assert type(sig) is SigLipLoss and (sig.rank, sig.world_size) == (1, 2)


def test_siglip_flag_parses():
    from mamba_clip_amd.cli.main import build_parser
    p = build_parser()
    assert p.parse_args(["--synthetic"]).siglip is False
    a = p.parse_args(["--synthetic", "--model", "tiny-mamba-clip", "--siglip", "--local-loss"])
    assert a.siglip is True and a.local_loss is True
    assert "ignored" in p.format_help()


def test_build_clip_siglip_init():
    from mamba_clip_amd.model import build_clip, init_model
    m = build_clip("tiny-mamba-clip", init_logit_scale=math.log(10), init_logit_bias=-10)
    assert abs(float(m.logit_scale) - math.log(10)) < 1e-6 and float(m.logit_bias) == -10.0
    assert isinstance(m.logit_bias, torch.nn.Parameter) and m.logit_bias.requires_grad
    m2, _, _, _ = init_model("tiny-mamba-clip", init_logit_scale=math.log(10), init_logit_bias=-10)
    assert abs(float(m2.logit_scale) - math.log(10)) < 1e-6 and float(m2.logit_bias) == -10.0
    for d in (build_clip("tiny-mamba-clip"), init_model("tiny-mamba-clip")[0]):
        assert d.logit_bias is None and abs(float(d.logit_scale) - math.log(1 / 0.07)) < 1e-6


def test_siglip_loss_ground_truth_matrix():
    from mamba_clip_amd.loss import SigLipLoss
    y = SigLipLoss().get_ground_truth(torch.device("cpu"), torch.float32, 3)
    assert torch.equal(y, 2 * torch.eye(3) - 1)
    y = SigLipLoss(rank=1, world_size=2).get_ground_truth(torch.device("cpu"), torch.float64, 2, 4, row_off=2)
    assert torch.equal(y, torch.tensor([[-1, -1, 1, -1], [-1, -1, -1, 1]], dtype=torch.float64))


def test_evaluate_batch_loss_is_the_sigmoid_loss_for_a_biased_model():
    """eval._batch_clip_loss on host tensors: the sigmoid loss when the model emits a logit_bias,
    the CLIP cross-entropy (unchanged) when it does not."""
    from mamba_clip_amd.eval import _batch_clip_loss
    g = torch.Generator().manual_seed(4)
    img = torch.nn.functional.normalize(torch.randn(6, 16, generator=g), dim=-1)
    txt = torch.nn.functional.normalize(torch.randn(6, 16, generator=g), dim=-1)
    s, b = torch.tensor(10.0), torch.tensor(-10.0)
    want = sigmoid_logits_loss_ref(img, txt, 10.0, -10.0, 0, 1.0 / 6)
    assert abs(float(_batch_clip_loss(img, txt, s, b)) - float(want)) <= 1e-5 * float(want)
    logits = 10.0 * img @ txt.t()
    lab = torch.arange(6)
    ce = (torch.nn.functional.cross_entropy(logits, lab) + torch.nn.functional.cross_entropy(logits.t(), lab)) / 2
    assert abs(float(_batch_clip_loss(img, txt, s)) - float(ce)) <= 1e-6 * float(ce)


# ---------------------------------------------------------------- gloo: rank-local images x all texts
B_LOCAL, E = 3, 16
SCALE, BIAS = 4.0, -2.0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _features(world):
    g = torch.Generator().manual_seed(11 + world)
    n = B_LOCAL * world
    img = torch.nn.functional.normalize(torch.randn(n, E, generator=g, dtype=torch.float64), dim=-1)
    txt = torch.nn.functional.normalize(img + 0.7 * torch.randn(n, E, generator=g, dtype=torch.float64), dim=-1)
    return img, txt


def _worker(rank, world, port, q):
    try:
        import sys
        for p in (ROOT, os.path.join(ROOT, "mamba-clip_amd"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        import torch.distributed as dist
        import mamba_clip_amd.loss as L
        L.sigmoid_logits_loss = sigmoid_logits_loss_ref
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        img_all, txt_all = _features(world)
        sl = slice(rank * B_LOCAL, (rank + 1) * B_LOCAL)
        img, txt = img_all[sl].clone().requires_grad_(True), txt_all[sl].clone().requires_grad_(True)
        scale = torch.tensor(SCALE, dtype=torch.float64, requires_grad=True)
        bias = torch.tensor(BIAS, dtype=torch.float64, requires_grad=True)
        crit = L.SigLipLoss(rank=rank, world_size=world)
        loss = crit(img, txt, scale, bias)["contrastive_loss"]
        loss.backward()
        mean = loss.detach().clone()
        dist.all_reduce(mean)
        mean /= world
        ds, db = scale.grad.clone(), bias.grad.clone()
        dist.all_reduce(ds)
        dist.all_reduce(db)
        q.put((rank, {"mean_loss": float(mean), "img_grad": img.grad.numpy(), "txt_grad": txt.grad.numpy(),
                      "scale_grad_mean": float(ds / world), "bias_grad_mean": float(db / world)}))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, {"error": repr(e) + traceback.format_exc()}))


@pytest.mark.parametrize("world", [2, 4])
def test_siglip_loss_distributed_matches_whole_batch(world):
    """Each rank's (local images x all texts) term: the rank mean is the whole-batch loss, and after
    DDP's division by the world size every gradient is the whole-batch gradient."""
    import numpy as np
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    img, txt = _features(world)
    n = B_LOCAL * world
    want = sigmoid_logits_loss_full_ref(img, txt, SCALE, BIAS, 0, 1.0 / n)
    for r in range(world):
        assert "error" not in out[r], out[r].get("error")
        sl = slice(r * B_LOCAL, (r + 1) * B_LOCAL)
        np.testing.assert_allclose(out[r]["mean_loss"], float(want["loss"]), rtol=1e-9)
        np.testing.assert_allclose(out[r]["img_grad"] / world, want["dX"][sl].numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(out[r]["txt_grad"] / world, want["dY"][sl].numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(out[r]["scale_grad_mean"], float(want["dscale"]), rtol=1e-9)
        np.testing.assert_allclose(out[r]["bias_grad_mean"], float(want["dbias"]), rtol=1e-9)
