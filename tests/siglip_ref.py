"""fp64 restatement of the pairwise sigmoid (SigLIP) loss with dense torch ops -- the reference
every SigLIP test compares against (include/mc_contrastive.h, mc_sigmoid_loss_*):

    z_ij = scale * sum_k X[i, k] Y[j, k] + bias
    y_ij = +1 if j == i + row_off else -1      (a row whose label column is outside [0, N): no positive)
    loss = coef * sum_ij softplus(-y_ij z_ij)
    dloss/dz_ij = coef * (sigmoid(z_ij) - [j == i + row_off])
"""
import torch
import torch.nn.functional as F


def label_mask(M, N, row_off=0, device=None):
    """Boolean (M, N): True where j == i + row_off."""
    rows = torch.arange(M, device=device)[:, None] + int(row_off)
    cols = torch.arange(N, device=device)[None, :]
    return rows == cols


def sigmoid_logits_loss_ref(X, Y, scale, bias, row_off=0, coef=1.0):
    """The loss as a differentiable fp64 scalar (X, Y, scale, bias: tensors or floats, any dtype)."""
    X, Y = X.double(), Y.double()
    scale = scale.double() if torch.is_tensor(scale) else float(scale)
    bias = bias.double() if torch.is_tensor(bias) else float(bias)
    z = scale * (X @ Y.t()) + bias
    y = torch.where(label_mask(X.shape[0], Y.shape[0], row_off, X.device), 1.0, -1.0).double()
    return coef * F.softplus(-y * z).sum()


def sigmoid_logits_loss_full_ref(X, Y, scale, bias, row_off=0, coef=1.0):
    """dict(loss, dX, dY, dscale, dbias, abs_dscale, abs_dbias, positives) from the closed forms, fp64.

    abs_dscale / abs_dbias are the sums of the absolute contributions
    coef * sum |sigmoid(z) - [label]| |z - bias| / scale   and   coef * sum |sigmoid(z) - [label]|:
    the scale gradient cancels to a small number, so errors are measured against these."""
    X, Y = X.detach().double(), Y.detach().double()
    scale, bias = float(scale), float(bias)
    dots = X @ Y.t()
    z = scale * dots + bias
    lab = label_mask(X.shape[0], Y.shape[0], row_off, X.device)
    y = torch.where(lab, 1.0, -1.0).double()
    g = coef * (torch.sigmoid(z) - lab.double())           # dloss/dz
    return {
        "loss": coef * F.softplus(-y * z).sum(),
        "dX": scale * (g @ Y),
        "dY": scale * (g.t() @ X),
        "dscale": (g * dots).sum(),
        "dbias": g.sum(),
        "abs_dscale": (g.abs() * dots.abs()).sum(),
        "abs_dbias": g.abs().sum(),
        "positives": int(lab.sum()),
    }


def grad_block_ref(X, Y, scale, bias, row_off, coef, gout, bf16_out):
    """(G, bound) of one mc_sigmoid_loss_grad block, G = gout * scale * coef * (sigmoid(z) - [label]), per
    element in fp64.  The kernel forms q = sigmoid(z) off the label and sigmoid(-z) on it without
    cancellation (e = exp(-|z|), 1 / (1 + e), e / (1 + e)), so its error is relative to q:
        |dG| <= |gout scale coef| q ((1 - q) dz + (8 + |z|) 2^-23) + half_ulp_bf16(G) [bf16 G] + 1e-30
    dz = eps_ij + 2^-23 (|z| + |bias|): the logit's accumulation bound (contrastive_ref.logits) and the
    roundings of scale * acc and + bias, through dq/dz = q (1 - q); (8 + |z|) 2^-23 is twice the fast
    exp ((2 + |z|) 2^-24), the reciprocal (1 ulp), 1 + e, e s, and the three products coef, gout, scale."""
    from contrastive_ref import TINY, half_ulp_bf16, logits
    S, eps = logits(X, Y, scale)
    z = S + bias
    lab = label_mask(X.shape[0], Y.shape[0], row_off)
    sig = torch.sigmoid(z)
    q = torch.where(lab, torch.sigmoid(-z), sig)
    G = gout * scale * coef * torch.where(lab, -q, q)
    dz = eps + 2.0 ** -23 * (z.abs() + abs(bias))
    bound = abs(gout * scale * coef) * q * ((1 - q) * dz + (8 + z.abs()) * 2.0 ** -23)
    return G, bound + (half_ulp_bf16(G) if bf16_out else 0.0) + TINY
