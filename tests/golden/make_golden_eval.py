"""Generate tests/golden/eval_pauc.npz from the REFERENCE's own partial_auc (eval.py:21-44).

Run in the build container only (needs /root/reference and scikit-learn, which the reference's
function calls; the tests read only the fixture):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval.py

The reference module is imported as-is, the way make_golden.py imports loss.py; nothing of its
text is stored here, only the inputs and the values it returned:
    n_cases, min_tpr[k], expected[k], y_true_<k>, y_pred_<k>
"""
import importlib
import os
import sys

import numpy as np

REF_SRC = "/root/reference/src"
HERE = os.path.dirname(os.path.abspath(__file__))


def cases():
    rng = np.random.default_rng(20240)
    out = []
    # continuous scores, informative, 30 % positives
    y = (rng.random(200) < 0.3).astype(np.int64)
    out.append((y, rng.normal(size=200) + 1.2 * y, 0.8))
    out.append((y, rng.normal(size=200) + 1.2 * y, 0.5))
    out.append((y, rng.normal(size=200) + 0.3 * y, 0.9))
    # the whole curve (max_fpr == 1)
    out.append((y, rng.normal(size=200) + 0.8 * y, 0.0))
    # heavy ties: scores on a grid of 11 values
    y = (rng.random(120) < 0.4).astype(np.int64)
    out.append((y, np.round(np.clip(0.5 + 0.25 * rng.normal(size=120) + 0.2 * y, 0, 1), 1), 0.8))
    # few positives with tied scores: the flipped curve's FPR moves in steps of 1/7 along
    # diagonal segments, so 1 - min_tpr = 0.2 falls strictly between two ROC points
    y = np.zeros(60, dtype=np.int64)
    y[rng.choice(60, 7, replace=False)] = 1
    out.append((y, np.round(0.4 * rng.random(60) + 0.35 * y, 1), 0.8))
    # ISIC-like imbalance, softmax-like probabilities
    y = (rng.random(1000) < 0.02).astype(np.int64)
    y[:3] = 1
    z = rng.normal(size=1000) + 2.0 * y
    out.append((y, 1.0 / (1.0 + np.exp(-z)), 0.8))
    # perfect separation, and a constant (collapsed) predictor
    y = np.r_[np.zeros(20, dtype=np.int64), np.ones(10, dtype=np.int64)]
    out.append((y, np.r_[rng.random(20) * 0.4, 0.6 + rng.random(10) * 0.4], 0.8))
    out.append((y, np.full(30, 0.5), 0.8))
    return out


def main():
    sys.path.insert(0, REF_SRC)
    ref = importlib.import_module("mamba_clip.eval")
    arrays = {}
    cs = cases()
    arrays["n_cases"] = np.array(len(cs))
    arrays["min_tpr"] = np.array([c[2] for c in cs], dtype=np.float64)
    arrays["expected"] = np.array([ref.partial_auc(c[0], c[1], min_tpr=c[2]) for c in cs], dtype=np.float64)
    for k, (y, p, _) in enumerate(cs):
        arrays[f"y_true_{k}"] = np.asarray(y, dtype=np.int64)
        arrays[f"y_pred_{k}"] = np.asarray(p, dtype=np.float64)
    np.savez(os.path.join(HERE, "eval_pauc.npz"), **arrays)
    print("wrote eval_pauc.npz:", arrays["expected"])


if __name__ == "__main__":
    main()
