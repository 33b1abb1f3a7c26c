"""CPU checks of tests/contrastive_ref.py, the reference and bounds of test_contrastive_instances_gpu.py:
the case table's preconditions, that a correct fp32 evaluation (and one correct bf16 rounding of it)
stays inside the bounds, and that three wrong answers built into the reference are rejected by the
same bound functions the GPU tests use."""
import pytest
import torch

import contrastive_ref as R

DTYPES = [torch.bfloat16, torch.float32]
ALL = [(c, R.SCALE) for c in R.CASES] + [(R.BIG_SCALE_CASE, R.BIG_SCALE)]
SHARP = (130, 130, 38, 0, 0, "contig")     # ragged both ways, K % V = 6 (bf16) and 2 (fp32)


def _ref(case, scale, dtype):
    M, N, K, row_off, col_off, _ = case
    X, Y = R.features(M, N, K, row_off, col_off, dtype, R.case_seed(case))
    S, eps = R.logits(X, Y, scale)
    return X, Y, S, eps, R.forward_ref(S, eps, row_off, col_off, 1.0, 1.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_case_table_preconditions(dtype):
    """Label logits separated by >= 0.05, finite lse, loss budget below the separation, for every case;
    the table's kAligned column equals fill_operands' rule applied to operands laid out as the GPU test
    lays them out; kAligned = false is selected at least once (by the contiguous, the misaligned-base
    and the odd-stride route)."""
    routes = set()
    for case, scale in ALL:
        M, N, K, _, _, layout = case
        X, Y, S, _, fwd = _ref(case, scale, dtype)
        gap = R.label_gap(S, fwd)
        assert gap >= R.MIN_LABEL_GAP, (case, gap)
        assert bool(torch.isfinite(fwd.lse_r).all()) and bool(torch.isfinite(fwd.lse_c).all())
        assert float(fwd.loss_bound) < gap, (case, float(fwd.loss_bound), gap)
        if layout == "base":
            X = torch.zeros(M, K + 8, dtype=dtype)[:, 1:K + 1]
        elif layout == "stride":
            Y = torch.zeros(N, K + 1, dtype=dtype)[:, :K]
        assert X.data_ptr() % 16 == 0 or layout == "base"          # the allocator's alignment, as on the device
        aligned = R.is_aligned(X) and R.is_aligned(Y)
        assert aligned == R.expect_aligned(case, dtype), (case, dtype)
        if not aligned:
            routes.add(layout)
    assert routes == {"contig", "base", "stride"}


def test_half_ulp_bf16_is_the_rounding_error_bound():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(20000, generator=g).double() * torch.logspace(-6, 6, 20000, dtype=torch.float64)
    x = torch.cat([x, torch.tensor([0.0, 1.0, -2.0, 1.0 + 2.0 ** -8, 2.0 - 2.0 ** -9], dtype=torch.float64)])
    h = R.half_ulp_bf16(x)
    err = (x.float().bfloat16().double() - x).abs()
    assert bool((err <= h * (1 + 2.0 ** -20)).all())               # (the fp32 step in between is 2^-16 of h)
    assert float((err / h.clamp_min(1e-300)).max()) > 0.99         # and it is attained
    nz = x != 0
    assert bool((h[nz] > x[nz].abs() * 2.0 ** -9 * (1 - 1e-12)).all()) and bool((h[nz] <= x[nz].abs() * 2.0 ** -8).all())
    # the flat |x| 2^-9 is not a rounding bound: the correctly rounded value itself leaves it
    assert float((err[nz] / (x[nz].abs() * 2.0 ** -9)).max()) > 1.9


@pytest.mark.parametrize("case_scale", [ALL[0], ALL[6], ALL[11], ALL[12], ALL[-1]], ids=lambda v: str(v[0][:5]))
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_correct_fp32_evaluation_stays_inside_the_bounds(case_scale, dtype):
    """fp32 torch restatement of the three epilogues from the fp32-rounded fp64 logits: the bounds leave
    room for what a correct kernel does (fp32 exp, fp32 products, one rounding of the output)."""
    case, scale = case_scale
    row_off, col_off = case[3:5]
    _, _, S, eps, fwd = _ref(case, scale, dtype)
    S32 = S.float()
    for bf16_out in (False, True):
        C = S32.bfloat16() if bf16_out else S32
        assert R.ratio(C, S, R.gemm_bound(S, eps, bf16_out)) <= 1.0
    assert R.ratio(torch.logsumexp(S32, 1), fwd.lse_r, R.lse_tol(fwd.lse_r)) <= 1.0
    assert R.ratio(torch.logsumexp(S32, 0), fwd.lse_c, R.lse_tol(fwd.lse_c)) <= 1.0
    gout = float(torch.tensor(-0.37).double())
    for use_r, use_c in ((True, False), (False, True), (True, True)):
        g = torch.zeros_like(S32)
        if use_r:
            g = 1.0 * (torch.exp(S32 - fwd.lse_r.float()[:, None]) - fwd.lab_r.float())
        if use_c:
            g = g + 0.75 * (torch.exp(S32 - fwd.lse_c.float()[None, :]) - fwd.lab_c.float())
        G = g * (torch.tensor(-0.37) * torch.tensor(scale))
        ds = (g * torch.tensor(-0.37) * S32).sum() / scale
        for bf16_out in (False, True):
            ref = R.grad_ref(S, eps, fwd.lse_r if use_r else None, fwd.lse_c if use_c else None, row_off, col_off,
                             1.0, 0.75, gout, scale, bf16_out)
            assert R.ratio(G.bfloat16() if bf16_out else G, ref.G, ref.bound) <= 1.0
            assert R.ratio(ds, ref.dscale, ref.dscale_bound) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_three_wrong_answers_are_rejected(dtype):
    """(1) the label one-hot moved by one column, (2) any one element of row M - 1 or column N - 1 zeroed,
    (3) the last K % V products dropped from the dot product: each pushed through the bound functions of
    the GPU tests must exceed its bound."""
    case, scale = SHARP, R.SCALE
    M, N, K, row_off, col_off, _ = case
    X, Y, S, eps, fwd = _ref(case, scale, dtype)
    lse_r, lse_c = fwd.lse_r, fwd.lse_c

    def grad(S_=S, lr=lse_r, lc=lse_c, ro=row_off, co=col_off, bf16_out=False):
        return R.grad_ref(S_, eps, lr, lc, ro, co, 1.0, 0.75, 1.0, scale, bf16_out)

    # (1) one-hot moved by one column: the G block and the loss (a neighbour's logit as the target)
    for bf16_out in (False, True):
        ref = grad(bf16_out=bf16_out)
        assert R.ratio(grad(ro=row_off + 1).G, ref.G, ref.bound) > 1.0
        assert R.ratio(grad(co=col_off - 1).G, ref.G, ref.bound) > 1.0
    moved = R.forward_ref(S, eps, row_off + 1, col_off, 1.0, 1.0)
    assert R.ratio(moved.loss, fwd.loss, fwd.loss_bound) > 1.0
    one = fwd.loss + (fwd.tgt_r[M - 1] - S[M - 1, N - 2])          # a single row's target off by one column
    assert R.ratio(one, fwd.loss, fwd.loss_bound) > 1.0

    # (2) one zeroed element anywhere in the last row or column: |ref| > bound for each of them
    # (G's corner is the label of row M - 1 and column N - 1: there G = scale (p - 1) with p within 1e-4
    # of 1, less than the lse tolerance moves it, so its own value is inside its bound; a wrong label
    # position there is what (1) rejects.)
    for bf16_out in (False, True):
        g = grad(bf16_out=bf16_out)
        for ref_v, bound, skip_corner in ((S, R.gemm_bound(S, eps, bf16_out), False), (g.G, g.bound, True)):
            rel = ref_v.abs() / bound
            edge = torch.cat([rel[M - 1, :N - 1 if skip_corner else N], rel[:M - 1, N - 1]])
            assert float(edge.min()) > 1.0
    assert float((lse_r.abs() / R.lse_tol(lse_r))[M - 1]) > 1.0 and float((lse_c.abs() / R.lse_tol(lse_c))[N - 1]) > 1.0

    # (3) the K tail dropped (what a wrong nv = min(V, K - kk) or a vector-only loop would do)
    V = 16 // X.element_size()
    assert K % V != 0
    S3, _ = R.logits(X, Y, scale, drop_tail=K % V)
    for bf16_out in (False, True):
        assert R.ratio(S3, S, R.gemm_bound(S, eps, bf16_out)) > 1.0
        ref = grad(bf16_out=bf16_out)
        assert R.ratio(grad(S_=S3).G, ref.G, ref.bound) > 1.0
    f3 = R.forward_ref(S3, eps, row_off, col_off, 1.0, 1.0)
    assert R.ratio(f3.lse_r, lse_r, R.lse_tol(lse_r)) > 1.0
    assert R.ratio(f3.lse_c, lse_c, R.lse_tol(lse_c)) > 1.0
    assert R.ratio(f3.loss, fwd.loss, fwd.loss_bound) > 1.0
