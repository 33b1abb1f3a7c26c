"""Validation after each epoch (reference: src/mamba_clip/eval.py:21-178, called from pipeline.step).

  partial_auc(y_true, y_pred, min_tpr)   eval.py:21-44, in numpy alone (no sklearn in the product)
  retrieval_metrics(ranks)               mean / median rank and R@1/5/10, both directions
  evaluate(model, data, epoch, args, tb_writer=None, tokenizer=None)      eval.py:47-178

For CLIP outputs the reference reports the sample-weighted mean of the per-batch contrastive
losses, accumulates every feature on the host and stops: "all_image_features @
all_text_features will blow up memory and compute very quickly" (eval.py:65-66).  Here the
per-batch loss is the fused logits + CE kernel (no b x b logits), the features stay in one
preallocated device buffer, and one ``ops.retrieval_ranks`` call over the whole set gives the
retrieval metrics and the whole-set loss ``val_loss_full`` without an n x n matrix.

Ties count against the model: the 0-based rank of a label is gt + eq (the number of other
candidates scoring higher, plus those scoring exactly the same).  Identical captions are common
in report-style text, and a collapsed model whose logits are all equal must not score R@1 = 1.

For classifier outputs (stage 2): cross-entropy and the partial AUC above TPR 0.8.
wandb logging is not carried over.
"""
import json
import logging
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .utils import get_autocast, get_input_dtype, is_master

logger = logging.getLogger(__name__)

RETRIEVAL_KS = (1, 5, 10)

#: (image_features, text_features, logit_scale) of the latest CLIP evaluation, kept only when
#: ``args.val_keep_features`` is set (further whole-set metrics without a second pass).
last_features = None


def _roc_curve(y_true, y_score):
    """fpr, tpr at every distinct score, highest first, collinear points dropped (the curve
    sklearn.metrics.roc_curve returns with its defaults); positives are y_true == 1."""
    y_true = np.asarray(y_true).ravel() == 1
    y_score = np.asarray(y_score, dtype=np.float64).ravel()
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    idx = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true, dtype=np.float64)[idx]
    fps = 1.0 + idx - tps
    if tps.size > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps = fps[keep], tps[keep]
    tps, fps = np.r_[0.0, tps], np.r_[0.0, fps]
    with np.errstate(divide="ignore", invalid="ignore"):
        fpr = fps / fps[-1] if fps[-1] > 0 else np.full_like(fps, np.nan)
        tpr = tps / tps[-1] if tps[-1] > 0 else np.full_like(tps, np.nan)
    return fpr, tpr


def _trapezoid(x, y):
    return float(np.sum(np.diff(x) * (y[1:] + y[:-1]) / 2.0))


def partial_auc(y_true, y_pred, min_tpr=0.8):
    """Area of the ROC curve above TPR ``min_tpr`` (eval.py:21-44): the classes and scores are
    flipped, so it is the area under the flipped curve up to FPR 1 - min_tpr, with one point
    added at that FPR by linear interpolation.  Not normalised: the maximum is (1 - min_tpr)."""
    v_gt = np.abs(np.asarray(y_true) - 1)
    v_pred = -1.0 * np.asarray(y_pred, dtype=np.float64)
    max_fpr = abs(1 - min_tpr)
    fpr, tpr = _roc_curve(v_gt, v_pred)
    if max_fpr == 1:
        return _trapezoid(fpr, tpr)
    if max_fpr <= 0 or max_fpr > 1:
        raise ValueError("Expected min_tpr in range [0, 1), got: %r" % min_tpr)
    stop = np.searchsorted(fpr, max_fpr, "right")
    x_interp = [fpr[stop - 1], fpr[stop]]
    y_interp = [tpr[stop - 1], tpr[stop]]
    tpr = np.append(tpr[:stop], np.interp(max_fpr, x_interp, y_interp))
    fpr = np.append(fpr[:stop], max_fpr)
    return _trapezoid(fpr, tpr)


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def retrieval_metrics(ranks):
    """Metrics dict from the four count arrays (gt_r, eq_r, gt_c, eq_c) of ``ops.retrieval_ranks``
    (rows = images, columns = texts; longer tuples are accepted, the rest is ignored).

    For ``image_to_text`` (rows) and ``text_to_image`` (columns): ``_mean_rank``, ``_median_rank``
    (1-based) and ``_R@1``, ``_R@5``, ``_R@10``.  The 0-based rank is gt + eq: a tie counts against
    the model.  Entries with gt = -1 (label outside the matrix) are left out; a direction without
    any entry reports NaN."""
    gt_r, eq_r, gt_c, eq_c = (_np(a).astype(np.int64) for a in tuple(ranks)[:4])
    out = {}
    for name, gt, eq in (("image_to_text", gt_r, eq_r), ("text_to_image", gt_c, eq_c)):
        rank = (gt + eq)[gt >= 0]
        if rank.size == 0:
            vals = [float("nan")] * (2 + len(RETRIEVAL_KS))
        else:
            vals = [float(rank.mean()) + 1.0, float(np.median(rank)) + 1.0] + \
                   [float(np.mean(rank < k)) for k in RETRIEVAL_KS]
        out[f"{name}_mean_rank"], out[f"{name}_median_rank"] = vals[0], vals[1]
        for k, v in zip(RETRIEVAL_KS, vals[2:]):
            out[f"{name}_R@{k}"] = v
    return out


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


def _batch_clip_loss(image_features, text_features, logit_scale, logit_bias=None):
    """(CE(logits, arange) + CE(logits^T, arange)) / 2 of one batch; on the GPU through the fused
    logits + CE kernel (ClipLoss at world size 1), so no b x b logits are formed.  A model that
    carries a logit_bias trains on the pairwise sigmoid loss, and that is its validation loss
    (SigLipLoss at world size 1, fused as well)."""
    if logit_bias is not None:
        if image_features.is_cuda:
            from .loss import SigLipLoss
            return SigLipLoss()(image_features, text_features, logit_scale, logit_bias, output_dict=False)
        logits = logit_scale.float() * image_features.float() @ text_features.float().t() + logit_bias.float()
        signs = 2 * torch.eye(logits.shape[0]) - 1
        return -F.logsigmoid(signs * logits).sum() / logits.shape[0]
    if image_features.is_cuda:
        from .loss import ClipLoss
        return ClipLoss()(image_features, text_features, logit_scale, output_dict=False)
    logits = logit_scale.float() * image_features.float() @ text_features.float().t()
    labels = torch.arange(logits.shape[0])
    return (F.cross_entropy(logits, labels) + F.cross_entropy(logits.t(), labels)) / 2


class _FeatureBuffer:
    """Rows appended into one preallocated device tensor (grown by doubling if the loader yields
    more samples than it announced)."""

    def __init__(self, capacity):
        self.capacity, self.buf, self.n = max(int(capacity), 1), None, 0

    def append(self, feats):
        if feats.dtype not in (torch.bfloat16, torch.float32):
            feats = feats.float()
        b = feats.shape[0]
        if self.buf is None:
            self.buf = torch.empty(max(self.capacity, b), feats.shape[1], dtype=feats.dtype, device=feats.device)
        if self.n + b > self.buf.shape[0]:
            grown = torch.empty(max(2 * self.buf.shape[0], self.n + b), self.buf.shape[1], dtype=self.buf.dtype,
                                device=self.buf.device)
            grown[:self.n] = self.buf[:self.n]
            self.buf = grown
        self.buf[self.n:self.n + b] = feats
        self.n += b

    def rows(self):
        return self.buf[:self.n]


def evaluate(model, data, epoch, args, tb_writer=None, tokenizer=None):
    """Validation metrics of ``data["val"]`` on the master rank, or {} when evaluation is off, this
    is not an evaluation epoch (``epoch % val_frequency == 0`` or the last epoch) or the rank is
    not the master.  The model is run unwrapped (a DDP wrapper on one rank would wait for the
    others), in eval mode, and is left in the mode it came in."""
    global last_features
    metrics = {}
    if not is_master(args):
        return metrics
    val_frequency = getattr(args, "val_frequency", 0)
    if "val" not in data or not val_frequency:
        return metrics
    if not ((epoch % val_frequency) == 0 or epoch == getattr(args, "epochs", None)):
        return metrics

    device = torch.device(getattr(args, "device", "cuda"))
    precision = getattr(args, "precision", "fp32")
    autocast = get_autocast(precision) if device.type == "cuda" else get_autocast(None)
    input_dtype = get_input_dtype(precision)
    log_every = getattr(args, "log_every_n_steps", 10) or 1
    inner = _unwrap(model)
    was_training = model.training
    model.eval()
    try:
        dataloader = data["val"].dataloader
        samples_per_val = getattr(dataloader, "num_samples", 0)
        num_samples = 0
        cumulative_loss = torch.zeros((), device=device, dtype=torch.float32)
        img_buf, txt_buf = _FeatureBuffer(samples_per_val), _FeatureBuffer(samples_per_val)
        logit_scale = None
        all_probs, all_targets = [], []
        with torch.inference_mode():
            for i, batch in enumerate(dataloader):
                if len(batch) == 2:
                    images, targets = batch
                    texts = None
                else:
                    images, texts, targets = batch
                images = images.to(device=device, dtype=input_dtype, non_blocking=True)
                texts = texts.to(device=device, non_blocking=True) if texts is not None else None
                targets = targets.to(device=device, non_blocking=True)
                batch_size = images.shape[0]
                with autocast():
                    model_out = inner(images, texts) if texts is not None else inner(images)
                    if (isinstance(model_out, dict) and "image_features" in model_out
                            and "text_features" in model_out and "logit_scale" in model_out):
                        image_features = model_out["image_features"]
                        text_features = model_out["text_features"]
                        logit_scale = model_out["logit_scale"].mean()
                        img_buf.append(image_features)
                        txt_buf.append(text_features)
                        total_loss = _batch_clip_loss(image_features, text_features, logit_scale,
                                                      model_out.get("logit_bias"))
                    else:
                        logits = getattr(model_out, "logits", model_out)
                        total_loss = F.cross_entropy(logits.float(), targets)
                        probs = F.softmax(logits.float(), dim=1)
                        if probs.shape[1] == 1:
                            probs = torch.cat([1 - probs, probs], dim=1)
                        all_probs.append(probs)
                        all_targets.append(targets)
                cumulative_loss += total_loss.float() * batch_size
                num_samples += batch_size
                if (i % log_every) == 0:
                    logger.info(f"Eval Epoch: {epoch} [{num_samples} / {samples_per_val}]")

            if num_samples == 0:
                return metrics
            metrics["val_loss"] = (cumulative_loss / num_samples).item()
            if img_buf.n:
                ranks = ops.retrieval_ranks(img_buf.rows(), txt_buf.rows(), logit_scale)
                metrics["val_loss_full"] = float(ranks.loss.item())
                metrics.update(retrieval_metrics(ranks))
                last_features = ((img_buf.rows(), txt_buf.rows(), logit_scale)
                                 if getattr(args, "val_keep_features", False) else None)
            if all_probs:
                probs = torch.cat(all_probs, dim=0).cpu().numpy()
                tgts = torch.cat(all_targets, dim=0).cpu().numpy()
                metrics["partial_auc"] = partial_auc(tgts, probs[:, 1])
            metrics.update({"epoch": epoch, "num_samples": num_samples})
    finally:
        model.train(was_training)

    logger.info(f"Eval Epoch: {epoch} " + "\t".join(f"{k}: {v:.4f}" for k, v in metrics.items()))
    if tb_writer is not None:
        for name, val in metrics.items():
            tb_writer.add_scalar("val/" + name, val, epoch)
    if getattr(args, "save_logs", False):
        with open(os.path.join(args.checkpoint_path, "results.jsonl"), "a+") as f:
            f.write(json.dumps(metrics))
            f.write("\n")
    return metrics
