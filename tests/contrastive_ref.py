"""fp64 reference and per-element error bounds of the contrastive GEMM (csrc/contrastive.hip,
gemm_nt_kernel<TIn, TOut, kAligned, kEpi>).  Helper module of test_contrastive_ref_cpu.py and
test_contrastive_instances_gpu.py: no tests.

Everything is restated densely on the CPU in fp64 from the same rounded operands the kernel reads:
    S      = scale * X @ Y^T
    lse_r  = logsumexp over the columns of S, lse_c over its rows
    loss   = coef_r sum_i (lse_r[i] - S[i, i + row_off]) + coef_c sum_j (lse_c[j] - S[j + col_off, j])
             (a label outside S contributes its lse only, as ce_fused_reduce_kernel does)
    G      = gout * scale * (coef_r (softmax_row - onehot_r) + coef_c (softmax_col - onehot_c))
    dscale = sum(G_unscaled * S) / scale,  G_unscaled = G / scale

Bounds, per element and from reference quantities only (never from the kernel's output):
    eps_ij   = |scale| K 2^-23 sum_k |x_ik y_jk|     a K-term dot product summed in any order, the unit
               roundoff doubled because the MFMA's internal adds are not documented to round to nearest
               (test_retrieval_gpu._band uses and justifies the same bound)
    gemm     eps_ij + half_ulp_bf16(S_ij) [bf16 C] + 1e-30
    lse      1e-6 |lse| + 1e-5                        (the suite's fp32 lse tolerance, test_loss_gpu.py)
    loss     sum over its terms of |coef| (lse tolerance + eps of the label logit)
    G_ij     |gout scale| (|coef_r| p_r (eps_ij + tol_lse_r + C_EXP (2 + |S - lse_r|)) + the same with c)
             + half_ulp_bf16(G_ij) [bf16 G] + 1e-30
             p = exp(S - lse) is the fp64 softmax.  An error d in the exponent moves p by p d; __expf
             itself is one ulp of v_exp_f32 plus the rounding of x log2(e), relative (2 + |x|) 2^-24.
             The magnitude is p, not |p - onehot|: the label element cancels as p - 1, its error does not.
    dscale   1e-5 sum |G_unscaled S| / |scale| + sum (bound_ij / |gout scale|) |S_ij| / |scale| + 1e-6

half_ulp_bf16(x) = 2^(floor(log2 |x|) - 8) is half the spacing of the bf16 numbers at x: the error of
one correct rounding.  It lies in (|x| 2^-9, |x| 2^-8]; the flat |x| 2^-9 is half an ulp only at the
top of a binade, and below that no bf16 number at all lies within it of most x (the fp64 reference
itself, rounded to nearest, would fail: test_contrastive_ref_cpu.py), so the term is taken per binade.
"""
import types

import torch

LSE_RTOL = 1e-6
LSE_ATOL = 1e-5
# __expf relative error (2 + |x|) C_EXP.  2^-22 is derived from v_exp_f32's documented 1 ulp.  Measured on
# an MI355X: the largest fp32-G err / bound with this value is 0.058 over all cases, so
# it was not widened.
C_EXP = 2.0 ** -22
TINY = 1e-30
MIN_LABEL_GAP = 0.05


# (M, N, K, row_off, col_off, layout): the smallest shapes that reach each branch of the kernel.
# Layouts: "contig"; "base" X = buf[:, 1:K + 1] of a (K + 8)-column buffer (misaligned base, aligned
# stride); "stride" Y = buf[:, :K] of a (K + 1)-column buffer (row stride no multiple of 16 B).
CASES = [
    (5, 7, 4, 0, 0, "contig"),          # below one wave quadrant, K below one slice; bf16 rows of 8 B are
                                        # unaligned, fp32 rows of 16 B aligned
    (64, 64, 32, 0, 0, "contig"),       # exactly one live quadrant, the other three waves fully masked
    (128, 128, 64, 0, 0, "contig"),     # one full tile: vector stores, c_vec16 for 16-bit G
    (256, 128, 64, 0, 0, "contig"),     # two full tiles
    (128, 132, 64, 0, 0, "contig"),     # full tile with ldg % 8 == 4: c_vec && !c_vec16 on 16-bit G
    (128, 131, 32, 0, 0, "contig"),     # full tile with ldg % 4 != 0: c_vec == 0
    (130, 130, 38, 0, 0, "contig"),     # remainders both ways, K no multiple of the slice or of the vector;
                                        # rows of 76 B (bf16) / 152 B (fp32): unaligned in both dtypes
    (257, 200, 64, 0, 0, "contig"),     # 3 x 2 tiles, aligned, ragged
    (1030, 130, 38, 0, 0, "contig"),    # 9 tile rows: the second kGroupM group has gm = 1, 18 tiles are no
                                        # multiple of the 8 XCDs (xcd_remap remainder); unaligned
    (100, 300, 32, 128, -128, "contig"),     # labels in a later tile column
    (200, 200, 32, 70, -70, "contig"),       # the label diagonal leaves a tile mid-quadrant
    (300, 100, 32, -50, 0, "contig"),        # rows without a label; row and column labels differ
    (128, 128, 32, 1 << 20, 0, "contig"),    # no row label anywhere
    (130, 130, 40, 0, 0, "contig"),     # 80-B / 160-B rows: aligned (the tail slice runs the masked loads)
    (130, 130, 40, 0, 0, "base"),       # misaligned base, aligned stride
    (130, 130, 40, 0, 0, "stride"),     # row stride 82 B / 164 B
]
# kAligned each case must select, per input dtype (asserted from the operands with is_aligned)
CASE_ALIGNED = {
    (5, 7, 4, "contig"): {torch.bfloat16: False, torch.float32: True},
    (130, 130, 38, "contig"): {torch.bfloat16: False, torch.float32: False},
    (1030, 130, 38, "contig"): {torch.bfloat16: False, torch.float32: False},
    (130, 130, 40, "base"): {torch.bfloat16: False, torch.float32: False},
    (130, 130, 40, "stride"): {torch.bfloat16: False, torch.float32: False},
}
SCALE = 20.0
# one case at scale 100: exp(S - lse) spans its whole range
BIG_SCALE_CASE = (130, 130, 38, 0, 0, "contig")
BIG_SCALE = 100.0


def expect_aligned(case, dtype):
    M, N, K, _, _, layout = case
    return CASE_ALIGNED.get((M, N, K, layout), {}).get(dtype, True)


def case_seed(case):
    M, N, K, row_off = case[:4]
    return M * 7 + N * 3 + K + (row_off % 1000)


def is_aligned(t):
    """fill_operands' rule for the kAligned = true instance, from the operand itself: a 16-B aligned
    base pointer and a row stride that is a multiple of 16 B."""
    return t.data_ptr() % 16 == 0 and (t.stride(0) * t.element_size()) % 16 == 0


def features(M, N, K, row_off, col_off, dtype, seed):
    """X = normalize(randn).  Y_j = normalize(X_a + noise of norm ~0.5) with its label partner a = j - row_off
    (row a has its label in column j; at scale 20 the label's softmax is 0.9 .. 1, so p - 1 is no
    rounding artefact).  Where column j's own label row b = j + col_off is another row, Y_j =
    normalize(X_a + 0.9 X_b + noise of norm ~0.1), X_a and X_b made orthogonal first: both label logits
    stand out of the others (|cos| ~ K^-1/2) and differ from each other.  A column without a partner
    is normalize(randn).  Rounded to ``dtype``."""
    g = torch.Generator().manual_seed(seed)
    X = torch.nn.functional.normalize(torch.randn(M, K, generator=g), dim=-1)
    Y = torch.randn(N, K, generator=g)
    noise = torch.randn(N, K, generator=g) / K ** 0.5
    j = torch.arange(N)
    a, b = j - row_off, j + col_off
    ok_a, ok_b = (a >= 0) & (a < M), (b >= 0) & (b < M) & (b != a)
    pairs = sorted((max(int(a[k]), int(b[k])), min(int(a[k]), int(b[k]))) for k in j[ok_a & ok_b].tolist())
    for hi, lo in pairs:                                   # ascending: a row changes before it is a ``lo``
        X[hi] = torch.nn.functional.normalize(X[hi] - (X[hi] @ X[lo]) * X[lo], dim=-1)
    P = torch.zeros(N, K)
    P[ok_a] += X[a[ok_a]]
    P[ok_b] += 0.9 * X[b[ok_b]]
    any_p = ok_a | ok_b
    Y[any_p] = P[any_p] + torch.where(ok_a & ok_b, 0.1, 0.5)[any_p, None] * noise[any_p]
    Y = torch.nn.functional.normalize(Y, dim=-1)
    return X.to(dtype), Y.to(dtype)


def logits(X, Y, scale, drop_tail=0):
    """(S, eps) in fp64.  ``drop_tail`` leaves the last products out of the dot product (a wrong answer
    for the sharpness test); eps is always the bound of the full product."""
    Xd, Yd = X.double(), Y.double()
    K = Xd.shape[1]
    eps = abs(scale) * K * 2.0 ** -23 * (Xd.abs() @ Yd.abs().T)
    if drop_tail:
        Xd, Yd = Xd[:, :K - drop_tail], Yd[:, :K - drop_tail]
    return scale * (Xd @ Yd.T), eps


def label_masks(M, N, row_off, col_off):
    """Boolean (M, N) masks: [j == i + row_off] and [i == j + col_off]."""
    i = torch.arange(M)[:, None]
    j = torch.arange(N)[None, :]
    return j == i + row_off, i == j + col_off


def lse_tol(lse):
    return LSE_RTOL * lse.abs() + LSE_ATOL


def half_ulp_bf16(x):
    """Half the spacing of the bf16 numbers (8 significand bits) at |x|: 2^(floor(log2 |x|) - 8); 0 at 0."""
    _, e = torch.frexp(x.double().abs())                      # |x| = m 2^e, m in [0.5, 1)
    return torch.where(x == 0, torch.zeros_like(x, dtype=torch.float64), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 9))


def gemm_bound(S, eps, bf16_out):
    return eps + (half_ulp_bf16(S) if bf16_out else 0.0) + TINY


def forward_ref(S, eps, row_off, col_off, coef_r, coef_c):
    """lse_r, lse_c, the loss, its error budget and the label logits (tgt_*: value, has_*: in range)."""
    M, N = S.shape
    lab_r, lab_c = label_masks(M, N, row_off, col_off)
    lse_r, lse_c = torch.logsumexp(S, 1), torch.logsumexp(S, 0)
    has_r, has_c = lab_r.any(1), lab_c.any(0)
    tgt_r, tgt_c = (S * lab_r).sum(1), (S * lab_c).sum(0)
    loss = coef_r * (lse_r - tgt_r).sum()
    bound = abs(coef_r) * (lse_tol(lse_r) + (eps * lab_r).sum(1)).sum()
    if coef_c:
        loss = loss + coef_c * (lse_c - tgt_c).sum()
        bound = bound + abs(coef_c) * (lse_tol(lse_c) + (eps * lab_c).sum(0)).sum()
    return types.SimpleNamespace(lse_r=lse_r, lse_c=lse_c, loss=loss, loss_bound=bound, tgt_r=tgt_r, tgt_c=tgt_c,
                                 has_r=has_r, has_c=has_c, lab_r=lab_r, lab_c=lab_c)


def label_gap(S, fwd):
    """Smallest |label logit - any other logit of its row or column| over the in-range labels (inf
    without labels)."""
    gap = float("inf")
    idx = (fwd.lab_r | fwd.lab_c).nonzero()             # every label (i, j): its whole row i and column j
    if len(idx) == 0:
        return gap
    tv = S[idx[:, 0], idx[:, 1]][:, None]
    for lines, own in ((S[idx[:, 0], :], idx[:, 1]), (S[:, idx[:, 1]].T, idx[:, 0])):
        d = (lines - tv).abs()
        d[torch.arange(len(idx)), own] = float("inf")
        gap = min(gap, float(d.min()))
    return gap


def grad_ref(S, eps, lse_r, lse_c, row_off, col_off, coef_r, coef_c, gout, scale, bf16_out):
    """G, dscale and their bounds.  lse_r / lse_c None drops that term (as a NULL pointer does)."""
    M, N = S.shape
    lab_r, lab_c = label_masks(M, N, row_off, col_off)
    g = torch.zeros_like(S)
    e = torch.zeros_like(S)
    for lse, lab, coef in ((lse_r[:, None] if lse_r is not None else None, lab_r, coef_r),
                           (lse_c[None, :] if lse_c is not None else None, lab_c, coef_c)):
        if lse is None:
            continue
        t = S - lse
        p = torch.exp(t)
        g = g + coef * (p - lab.double())
        e = e + abs(coef) * p * (eps + lse_tol(lse) + C_EXP * (2.0 + t.abs()))
    G = gout * scale * g
    bound = abs(gout * scale) * e + (half_ulp_bf16(G) if bf16_out else 0.0) + TINY
    Gu = G / scale
    dscale = (Gu * S).sum() / scale
    dscale_bound = (1e-5 * (Gu * S).abs().sum() / abs(scale)
                    + ((bound / abs(gout * scale)) * S.abs()).sum() / abs(scale) + 1e-6)
    return types.SimpleNamespace(G=G, bound=bound, dscale=dscale, dscale_bound=dscale_bound)


def ratio(got, ref, bound):
    """max over all elements of |got - ref| / bound (a non-finite ``got`` gives inf)."""
    got = torch.as_tensor(got, dtype=torch.float64)
    r = (got - ref).abs() / bound
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())
