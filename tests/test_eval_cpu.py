"""Host-side checks of the evaluation layer (mamba_clip_amd/eval.py, ops.retrieval_ranks on host
tensors, the CLI flags).  No GPU."""
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def test_partial_auc_matches_reference_values():
    """tests/golden/eval_pauc.npz holds what the reference's partial_auc (eval.py:21-44, sklearn
    underneath) returned for each input (tests/golden/make_golden_eval.py): ties in the scores,
    an interpolation point between two ROC points, the whole curve, heavy imbalance."""
    from mamba_clip_amd.eval import partial_auc
    fx = np.load(os.path.join(GOLDEN, "eval_pauc.npz"))
    n = int(fx["n_cases"])
    assert n >= 8
    for k in range(n):
        got = partial_auc(fx[f"y_true_{k}"], fx[f"y_pred_{k}"], min_tpr=float(fx["min_tpr"][k]))
        assert abs(got - float(fx["expected"][k])) <= 1e-12, (k, got, float(fx["expected"][k]))
    with pytest.raises(ValueError):
        partial_auc([0, 1], [0.1, 0.9], min_tpr=1.0)


def test_partial_auc_interpolation_case_is_between_roc_points():
    """The fixture's few-positives case really interpolates: 1 - min_tpr is not an FPR of the curve."""
    from mamba_clip_amd.eval import _roc_curve
    fx = np.load(os.path.join(GOLDEN, "eval_pauc.npz"))
    y, p = fx["y_true_5"], fx["y_pred_5"]
    fpr, tpr = _roc_curve(np.abs(y - 1), -p)
    assert not np.any(np.isclose(fpr, 0.2))
    stop = np.searchsorted(fpr, 0.2, "right")
    assert tpr[stop] > tpr[stop - 1] and fpr[stop] > fpr[stop - 1]     # a diagonal (tied) segment


def test_retrieval_metrics_tie_rule_exclusion_and_one_based_ranks():
    from mamba_clip_amd.eval import retrieval_metrics
    gt_r = np.array([0, 0, 3, -1, 9, 20])
    eq_r = np.array([0, 2, 1, 0, 0, 0])
    # 0-based ranks 0, 2, 4, (excluded), 9, 20
    gt_c = np.array([0, 0, 0, 0])
    eq_c = np.array([0, 0, 0, 3])
    m = retrieval_metrics((gt_r, eq_r, gt_c, eq_c))
    assert m["image_to_text_mean_rank"] == pytest.approx((0 + 2 + 4 + 9 + 20) / 5 + 1)
    assert m["image_to_text_median_rank"] == 5.0
    assert m["image_to_text_R@1"] == pytest.approx(1 / 5)
    assert m["image_to_text_R@5"] == pytest.approx(3 / 5)
    assert m["image_to_text_R@10"] == pytest.approx(4 / 5)
    assert m["text_to_image_R@1"] == pytest.approx(3 / 4)       # the tied column is not a hit
    assert m["text_to_image_R@5"] == 1.0
    assert m["text_to_image_mean_rank"] == pytest.approx(3 / 4 + 1)
    assert m["text_to_image_median_rank"] == 1.0
    assert len(m) == 10
    # a collapsed model (every logit equal) must not look perfect
    n = 8
    z = np.zeros(n, dtype=np.int64)
    c = retrieval_metrics((z, z + n - 1, z, z + n - 1))
    assert c["image_to_text_R@1"] == 0.0 and c["text_to_image_R@5"] == 0.0
    assert c["image_to_text_mean_rank"] == n
    # torch tensors and the op's named tuple are accepted; nothing valid -> NaN
    e = retrieval_metrics((torch.tensor([-1]), torch.tensor([0]), torch.tensor([2]), torch.tensor([0])))
    assert np.isnan(e["image_to_text_R@1"]) and e["text_to_image_mean_rank"] == 3.0


def _brute(X, Y, scale, row_off, col_off):
    M, N = X.shape[0], Y.shape[0]
    S = [[scale * sum(float(X[i, k]) * float(Y[j, k]) for k in range(X.shape[1])) for j in range(N)]
         for i in range(M)]
    gt_r, eq_r, gt_c, eq_c = [], [], [], []
    for i in range(M):
        lab = i + row_off
        if not 0 <= lab < N:
            gt_r.append(-1), eq_r.append(0)
            continue
        gt_r.append(sum(1 for j in range(N) if j != lab and S[i][j] > S[i][lab]))
        eq_r.append(sum(1 for j in range(N) if j != lab and S[i][j] == S[i][lab]))
    for j in range(N):
        lab = j + col_off
        if not 0 <= lab < M:
            gt_c.append(-1), eq_c.append(0)
            continue
        gt_c.append(sum(1 for i in range(M) if i != lab and S[i][j] > S[lab][j]))
        eq_c.append(sum(1 for i in range(M) if i != lab and S[i][j] == S[lab][j]))
    return gt_r, eq_r, gt_c, eq_c, S


@pytest.mark.parametrize("row_off,col_off", [(0, 0), (2, -2), (-1, 1)])
def test_retrieval_ranks_host_path_matches_brute_force(row_off, col_off):
    from mamba_clip_amd.ops import retrieval_ranks
    g = torch.Generator().manual_seed(3)
    X = torch.randint(-3, 4, (5, 8), generator=g).float()
    Y = torch.randint(-3, 4, (7, 8), generator=g).float()
    Y[4] = Y[1]
    r = retrieval_ranks(X, Y, 0.5, row_off, col_off)
    gt_r, eq_r, gt_c, eq_c, S = _brute(X, Y, 0.5, row_off, col_off)
    assert r.gt_r.tolist() == gt_r and r.eq_r.tolist() == eq_r
    assert r.gt_c.tolist() == gt_c and r.eq_c.tolist() == eq_c
    assert r.gt_r.dtype == torch.int32
    assert sum(eq_r) + sum(eq_c) > 0
    St = torch.tensor(S, dtype=torch.float64)
    torch.testing.assert_close(r.lse_r.double(), torch.logsumexp(St, 1), rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(r.lse_c.double(), torch.logsumexp(St, 0), rtol=1e-6, atol=1e-5)
    if row_off == 0 and col_off == 0:
        Xs, Ys = X[:5], Y[:5]
        r2 = retrieval_ranks(Xs, Ys, torch.tensor(0.5))
        S2 = 0.5 * Xs.double() @ Ys.double().T
        lab = torch.arange(5)
        ref = (torch.nn.functional.cross_entropy(S2, lab) + torch.nn.functional.cross_entropy(S2.T, lab)) / 2
        assert abs(float(r2.loss) - float(ref)) < 1e-5


def test_retrieval_ranks_rejects_bad_arguments():
    from mamba_clip_amd.ops import retrieval_ranks
    X, Y = torch.zeros(4, 8), torch.zeros(4, 8)
    with pytest.raises(ValueError):
        retrieval_ranks(X, Y.bfloat16(), 1.0)
    with pytest.raises(ValueError):
        retrieval_ranks(X.half(), Y.half(), 1.0)
    with pytest.raises(ValueError):
        retrieval_ranks(X[0], Y, 1.0)
    with pytest.raises(ValueError):
        retrieval_ranks(X, torch.zeros(4, 9), 1.0)
    with pytest.raises(ValueError):
        retrieval_ranks(torch.zeros(8, 4).t(), Y, 1.0)          # K not contiguous
    with pytest.raises(ValueError):
        retrieval_ranks(X, Y, 1.0, row_off=1 << 31)


class _StubClassifier(torch.nn.Module):
    """Classifier-shaped model: (images, texts) -> (B, C) logits from the image mean."""

    def __init__(self, classes=2):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, classes))
        self.calls = 0

    def forward(self, images, texts=None):
        self.calls += 1
        return images.float().mean(dim=(1, 2, 3))[:, None] * self.w[None, :]


class _Loader:
    def __init__(self, batches):
        self.batches = batches
        self.num_samples = sum(b[0].shape[0] for b in batches)

    def __iter__(self):
        return iter(self.batches)


def _classifier_data(with_text=True, n_batches=3, b=8):
    g = torch.Generator().manual_seed(0)
    batches = []
    for _ in range(n_batches):
        t = torch.randint(0, 2, (b,), generator=g)
        img = torch.randn(b, 3, 4, 4, generator=g) + t[:, None, None, None].float()
        batches.append((img, torch.zeros(b, 5, dtype=torch.long), t) if with_text else (img, t))
    return {"val": types.SimpleNamespace(dataloader=_Loader(batches))}


def _args(**kw):
    base = dict(device="cpu", precision="fp32", rank=0, val_frequency=1, epochs=3)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_evaluate_gating():
    from mamba_clip_amd.eval import evaluate
    model, data = _StubClassifier(), _classifier_data()
    assert evaluate(model, data, 1, _args(val_frequency=0)) == {}
    assert evaluate(model, data, 1, _args(rank=1)) == {}
    assert evaluate(model, {}, 1, _args()) == {}
    assert evaluate(model, data, 1, _args(val_frequency=2)) == {}          # 1 % 2 != 0, not the last epoch
    assert model.calls == 0
    m = evaluate(model, data, 3, _args(val_frequency=2))                   # last epoch evaluates anyway
    assert m["epoch"] == 3 and m["num_samples"] == 24 and model.calls == 3
    assert evaluate(model, data, 2, _args(val_frequency=2))["epoch"] == 2


@pytest.mark.parametrize("with_text", [True, False])
def test_evaluate_classifier_reports_partial_auc_and_logs(tmp_path, with_text):
    from mamba_clip_amd.eval import evaluate, partial_auc
    model, data = _StubClassifier(), _classifier_data(with_text)
    model.train()
    m = evaluate(model, data, 1, _args(checkpoint_path=str(tmp_path)))
    assert model.training                                                  # mode restored
    assert not os.path.exists(tmp_path / "results.jsonl")                  # save_logs not set
    batches = data["val"].dataloader.batches
    logits = torch.cat([model(b[0]) for b in batches]).detach()
    tgts = torch.cat([b[-1] for b in batches])
    probs = torch.softmax(logits, dim=1)
    assert m["partial_auc"] == pytest.approx(partial_auc(tgts.numpy(), probs[:, 1].numpy()), abs=1e-12)
    assert m["val_loss"] == pytest.approx(float(torch.nn.functional.cross_entropy(logits, tgts)), rel=1e-5)
    assert "val_loss_full" not in m and m["num_samples"] == 24

    scalars = []
    tb = types.SimpleNamespace(add_scalar=lambda name, val, step: scalars.append((name, val, step)))
    model.eval()
    m2 = evaluate(model, data, 2, _args(checkpoint_path=str(tmp_path), save_logs=True), tb_writer=tb)
    assert not model.training
    lines = open(tmp_path / "results.jsonl").read().splitlines()
    assert len(lines) == 1 and json.loads(lines[0]) == m2
    assert ("val/partial_auc", m2["partial_auc"], 2) in scalars

    # one logit: softmax gives a single column of ones, duplicated to (0, 1) as in the reference
    # (whose cross-entropy only accepts class 0 there): constant scores, the chance-level area
    one = _StubClassifier(classes=1)
    zero = {"val": types.SimpleNamespace(dataloader=_Loader(
        [(b[0], torch.zeros_like(b[-1])) for b in data["val"].dataloader.batches]))}
    m3 = evaluate(one, zero, 1, _args())
    assert m3["val_loss"] == 0.0 and "partial_auc" in m3


def test_evaluate_clip_host_path_and_ddp_unwrap():
    """CLIP-shaped outputs on host tensors: per-batch loss weighted by samples, whole-set ranks;
    a wrapper exposing .module is bypassed (its own forward is never called)."""
    from mamba_clip_amd import eval as ev

    class Clip(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.p = torch.nn.Linear(48, 16, bias=False)

        def forward(self, images, texts):
            f = torch.nn.functional.normalize(self.p(images.flatten(1)), dim=-1)
            t = torch.nn.functional.normalize(f + 0.05 * texts.float()[:, :16], dim=-1)
            return {"image_features": f, "text_features": t, "logit_scale": torch.tensor(10.0)}

    class Wrapper(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.module = m

        def forward(self, *a):
            raise AssertionError("evaluate must run the unwrapped model")

    torch.manual_seed(0)
    data = _classifier_data(n_batches=3, b=8)
    data["val"].dataloader.batches = [(b[0], torch.randint(0, 5, (8, 16)), b[2])
                                      for b in data["val"].dataloader.batches]
    model = Wrapper(Clip())
    m = ev.evaluate(model, data, 1, _args(val_keep_features=True))
    assert model.training
    for d in ("image_to_text", "text_to_image"):
        for k in ("mean_rank", "median_rank", "R@1", "R@5", "R@10"):
            assert f"{d}_{k}" in m
        assert 0.0 <= m[f"{d}_R@1"] <= m[f"{d}_R@5"] <= m[f"{d}_R@10"] <= 1.0
    img, txt, scale = ev.last_features
    assert img.shape == (24, 16) and float(scale) == 10.0
    S = 10.0 * img.double() @ txt.double().T
    lab = torch.arange(24)
    full = (torch.nn.functional.cross_entropy(S, lab) + torch.nn.functional.cross_entropy(S.T, lab)) / 2
    assert m["val_loss_full"] == pytest.approx(float(full), rel=1e-5)
    per = []
    for k in range(3):
        Sb = S[8 * k:8 * k + 8, 8 * k:8 * k + 8]
        lb = torch.arange(8)
        per.append((torch.nn.functional.cross_entropy(Sb, lb) + torch.nn.functional.cross_entropy(Sb.T, lb)) / 2)
    assert m["val_loss"] == pytest.approx(float(sum(per) / 3), rel=1e-5)
    assert m["image_to_text_R@1"] == pytest.approx(float((S.argmax(1) == lab).double().mean()))
    ev.evaluate(model, data, 1, _args())
    assert ev.last_features is None


def test_parser_accepts_validation_flags():
    from mamba_clip_amd.cli.main import build_parser
    a = build_parser().parse_args(["--synthetic"])
    assert a.val_frequency == 0 and a.val_num_samples is None
    a = build_parser().parse_args(["--synthetic", "--val-frequency", "2", "--val-num-samples", "96"])
    assert a.val_frequency == 2 and a.val_num_samples == 96


def test_synthetic_val_loader_yields_distinct_batches():
    from mamba_clip_amd.data import get_synthetic_data
    d = get_synthetic_data(4, 2, 8, 6, 50, "cpu", seed=1)
    assert set(d) == {"train"}                                             # default: as before
    tr = list(d["train"].dataloader)
    assert torch.equal(tr[0][0], tr[1][0])                                 # the training loader repeats one batch
    d = get_synthetic_data(4, 2, 8, 6, 50, "cpu", seed=1, val_batches=3)
    val = list(d["val"].dataloader)
    assert len(val) == 3 and d["val"].dataloader.num_samples == 12
    assert not torch.equal(val[0][0], val[1][0]) and not torch.equal(val[1][1], val[2][1])
    again = list(d["val"].dataloader)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(val, again))        # stable across epochs
    assert torch.equal(list(d["train"].dataloader)[0][0], tr[0][0])
