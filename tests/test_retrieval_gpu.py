"""GPU checks of mc_retrieval_ranks (ops.retrieval_ranks) and of evaluate() on top of it.

The reference is a torch fp64 matmul of the same inputs followed by comparisons.  Integer-valued
features make every logit exactly representable in any summation order, so the counts must agree
exactly; random features are checked with a rounding sandwich (see _band)."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(X, Y, scale, row_off=0, col_off=0):
    """fp64 logits and, per direction, (gt, eq, valid, target, lse) by dense comparison."""
    S = scale * (X.double() @ Y.double().T)

    def side(S, off):
        n, other = S.shape
        lab = torch.arange(n) + off
        ok = (lab >= 0) & (lab < other)
        labc = lab.clamp(0, other - 1)
        t = S[torch.arange(n), labc]
        others = torch.ones_like(S, dtype=torch.bool)
        others[torch.arange(n), labc] = False
        gt = ((S > t[:, None]) & others).sum(1)
        eq = ((S == t[:, None]) & others).sum(1)
        gt = torch.where(ok, gt, torch.full_like(gt, -1))
        eq = torch.where(ok, eq, torch.zeros_like(eq))
        return gt, eq, ok, t, torch.logsumexp(S, 1)

    return S, side(S, row_off), side(S.T, col_off)


def _int_features(M, N, K, seed, dtype):
    """Integers in [-3, 3]; several rows of Y (and of X) are exact copies of others."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-3, 4, (M, K), generator=g).float()
    Y = torch.randint(-3, 4, (N, K), generator=g).float()
    for a, b in ((N - 1, 0), (N // 2, 1), (N // 3, N - 2), (2, N // 2)):
        Y[a] = Y[b]
    X[M - 1] = X[M // 2]
    return X.to(dtype), Y.to(dtype)


EXACT_CASES = [
    (5, 7, 8, 0, 0),
    (64, 64, 32, 0, 0),          # one wave quadrant live
    (130, 130, 40, 0, 0),        # tile remainders both ways, K no multiple of the slice; rows of 80 B (bf16) /
                                 # 160 B (fp32) are 16-B multiples: the kAligned = true instances
    (130, 130, 38, 0, 0),        # rows of 76 B / 152 B: the kAligned = false instances of kEpi 1 / 3, K % V != 0
    (257, 200, 64, 0, 0),        # 3 x 2 tiles
    (384, 384, 64, 0, 0),        # full tiles only, aligned path
    (100, 300, 32, 128, -128),   # labels in a later tile (local_loss); columns 0..127 have no label row
    (300, 100, 32, -50, 0),      # rows 0..49 have no label column
]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K,row_off,col_off", EXACT_CASES)
def test_retrieval_ranks_exact_on_integer_features(M, N, K, row_off, col_off, dtype):
    from mamba_clip_amd.ops import retrieval_ranks
    X, Y = _int_features(M, N, K, 100 + M + N, dtype)
    scale = 0.5
    S, (gt_r, eq_r, ok_r, t_r, lse_r), (gt_c, eq_c, ok_c, t_c, lse_c) = _ref(X, Y, scale, row_off, col_off)
    # the case must exercise both counters (checked from the reference alone)
    assert int((eq_r > 0).sum()) > 0 and int((gt_r > 0).sum()) > 0
    assert int((eq_c > 0).sum()) > 0 and int((gt_c > 0).sum()) > 0
    if row_off < 0:
        assert gt_r[:-row_off].eq(-1).all() and gt_r[-row_off:min(M, N - row_off)].ge(0).all()
    if col_off < 0:
        assert gt_c[:-col_off].eq(-1).all()

    Xd, Yd = X.to(DEV), Y.to(DEV)
    r = retrieval_ranks(Xd, Yd, scale, row_off, col_off)
    r2 = retrieval_ranks(Xd, Yd, scale, row_off, col_off)
    rs = retrieval_ranks(Xd, Yd, torch.tensor(scale, device=DEV), row_off, col_off)
    torch.cuda.synchronize()
    for name, want in (("gt_r", gt_r), ("eq_r", eq_r), ("gt_c", gt_c), ("eq_c", eq_c)):
        got = getattr(r, name)
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu().long(), want), name
        assert torch.equal(getattr(rs, name), got), f"{name} with a device scale"
    for a, b in zip(r, r2):
        assert torch.equal(a, b)                              # no atomics: repeated calls give the same bits
    if K == 38:
        # the same operands as views with a misaligned base and an aligned row stride (buf[:, 1:39] of 48
        # columns: 96-B / 192-B rows starting 2 B / 4 B in): kAligned = false by the base-pointer route,
        # NaN in the columns around the view
        assert Xd.data_ptr() % 16 == 0 and (Xd.stride(0) * Xd.element_size()) % 16 != 0
        views = []
        for t in (Xd, Yd):
            buf = torch.full((t.shape[0], 48), float("nan"), dtype=dtype, device=DEV)
            buf[:, 1:39] = t
            v = buf[:, 1:39]
            assert v.data_ptr() % 16 != 0 and (v.stride(0) * v.element_size()) % 16 == 0
            views.append(v)
        for a, b in zip(r, retrieval_ranks(views[0], views[1], scale, row_off, col_off)):
            assert torch.equal(a, b)
    torch.testing.assert_close(r.lse_r.cpu().double(), lse_r, rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(r.lse_c.cpu().double(), lse_c, rtol=1e-6, atol=1e-5)
    if bool(ok_r.all()) and bool(ok_c.all()):
        loss = 0.5 / M * (lse_r - t_r).sum() + 0.5 / N * (lse_c - t_c).sum()
        torch.testing.assert_close(r.loss.cpu().double(), loss, rtol=1e-6, atol=1e-5)


def _band(X, Y, scale, row_off=0, col_off=0):
    """Per direction (lo, hi, valid, inside): with S and the targets t in fp64 and
        delta_ij = scale * K * 2^-23 * (sum_k |x_ik y_jk| + sum_k |x_ik y_lk|)      (l the label)
    -- the bound for a K-term dot product summed in any order, the unit roundoff doubled because the
    MFMA's internal adds are not documented to round to nearest -- rounding can move a count only
    where |S - t| <= delta, so  lo = #{S > t + delta} <= gt  and  gt + eq <= hi = #{S >= t - delta}.
    ``inside`` counts the pairs within the band."""
    K = X.shape[1]
    S = scale * (X.double() @ Y.double().T)
    A = abs(scale) * K * 2.0 ** -23 * (X.double().abs() @ Y.double().abs().T)

    def side(S, A, off):
        n, other = S.shape
        lab = torch.arange(n) + off
        ok = (lab >= 0) & (lab < other)
        labc = lab.clamp(0, other - 1)
        t = S[torch.arange(n), labc][:, None]
        d = A + A[torch.arange(n), labc][:, None]
        others = torch.ones_like(S, dtype=torch.bool)
        others[torch.arange(n), labc] = False
        lo = ((S > t + d) & others).sum(1)
        hi = ((S >= t - d) & others).sum(1)
        inside = (((S - t).abs() <= d) & others)[ok].sum()
        return lo, hi, ok, int(inside)

    return side(S, A, row_off), side(S.T, A.T, col_off)


def _assert_sandwich(r, bands):
    for (gt, eq), (lo, hi, ok, _) in zip(((r.gt_r, r.eq_r), (r.gt_c, r.eq_c)), bands):
        gt, eq = gt.cpu().long(), eq.cpu().long()
        assert bool((gt[~ok] == -1).all()) and bool((eq[~ok] == 0).all())
        assert bool((lo[ok] <= gt[ok]).all())
        assert bool(((gt + eq)[ok] <= hi[ok]).all())


def test_retrieval_ranks_random_features_within_rounding_band():
    from mamba_clip_amd.ops import retrieval_ranks
    M, N, K, scale = 257, 200, 64, 10.0
    g = torch.Generator().manual_seed(11)
    X = torch.nn.functional.normalize(torch.randn(M, K, generator=g), dim=-1).bfloat16()
    Y = torch.nn.functional.normalize(torch.randn(N, K, generator=g), dim=-1).bfloat16()
    bands = _band(X, Y, scale)
    inside = bands[0][3] + bands[1][3]
    assert inside < 0.01 * 2 * M * N, f"{inside} pairs inside the rounding band: the check would be vacuous"
    r = retrieval_ranks(X.to(DEV), Y.to(DEV), scale)
    torch.cuda.synchronize()
    _assert_sandwich(r, bands)
    _, (_, _, _, _, lse_r), (_, _, _, _, lse_c) = _ref(X, Y, scale)
    torch.testing.assert_close(r.lse_r.cpu().double(), lse_r, rtol=1e-6, atol=1e-5)
    torch.testing.assert_close(r.lse_c.cpu().double(), lse_c, rtol=1e-6, atol=1e-5)


def test_retrieval_ranks_no_n_by_n_allocation_and_planted_ranks():
    """N = 8192, E = 512, bf16: peak memory during the call stays below N * N / 2 bytes, and a planted
    structure comes back exactly.  X[i] = e_(i mod E); Y[j] = w_j e_(j mod E) with
    w_j = 1 + sigma(j // E) / 4 for a permutation sigma of the 16 blocks.  Row i then sees w_j in the
    16 columns j = i (mod E) and 0 elsewhere: 15 - sigma(i // E) columns beat its label, none tie.
    Column j holds w_j in all 16 rows i = j (mod E): 15 ties, nothing greater."""
    from mamba_clip_amd.ops import retrieval_ranks
    N, E = 8192, 512
    g = torch.Generator().manual_seed(4)
    sigma = torch.randperm(N // E, generator=g)
    idx = torch.arange(N)
    X = torch.zeros(N, E)
    X[idx, idx % E] = 1.0
    Y = torch.zeros(N, E)
    Y[idx, idx % E] = 1.0 + sigma[idx // E].float() / 4
    Xd, Yd = X.bfloat16().to(DEV), Y.bfloat16().to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = retrieval_ranks(Xd, Yd, 2.0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert peak < N * N // 2, f"peak {peak / 2**20:.1f} MiB >= N * N / 2 bytes"
    assert torch.equal(r.gt_r.cpu().long(), 15 - sigma[idx // E])
    assert int(r.eq_r.abs().sum()) == 0
    assert int(r.gt_c.abs().sum()) == 0
    assert torch.equal(r.eq_c.cpu().long(), torch.full((N,), 15))
    w = 2.0 * (1.0 + sigma.double() / 4)
    lse_r = torch.log(torch.exp(w).sum() + (N - 16)).expand(N)
    torch.testing.assert_close(r.lse_r.cpu().double(), lse_r, rtol=1e-6, atol=1e-5)


def test_evaluate_tiny_clip_end_to_end():
    from mamba_clip_amd import eval as ev
    from mamba_clip_amd.data import get_synthetic_data
    from mamba_clip_amd.model import build_clip
    torch.manual_seed(0)
    model = build_clip("tiny-mamba-clip").to(DEV)
    model.train()
    text = model.text
    b = 8
    data = get_synthetic_data(b, 1, 32, text.context_length, text.vocab_size, DEV, seed=3, val_batches=3)
    args = types.SimpleNamespace(device=DEV, precision="amp_bf16", rank=0, val_frequency=1, epochs=1,
                                 val_keep_features=True)
    m = ev.evaluate(model, data, 1, args)
    assert model.training
    assert m["epoch"] == 1 and m["num_samples"] == 3 * b
    for k in ("val_loss", "val_loss_full"):
        assert m[k] == m[k] and abs(m[k]) < float("inf")
    names = [f"{d}_{k}" for d in ("image_to_text", "text_to_image")
             for k in ("mean_rank", "median_rank", "R@1", "R@5", "R@10")]
    assert all(n in m for n in names)
    for d in ("image_to_text", "text_to_image"):
        assert 0.0 <= m[f"{d}_R@1"] <= m[f"{d}_R@5"] <= m[f"{d}_R@10"] <= 1.0

    # dense fp64 recomputation from the features evaluate stored, within the rounding sandwich
    img, txt, scale = ev.last_features
    assert img.shape[0] == 3 * b and img.is_cuda
    img, txt, scale = img.cpu(), txt.cpu(), float(scale)
    (lo_r, hi_r, ok_r, _), (lo_c, hi_c, ok_c, _) = _band(img, txt, scale)
    zero_r, zero_c = torch.zeros_like(lo_r), torch.zeros_like(lo_c)
    best = ev.retrieval_metrics((lo_r, zero_r, lo_c, zero_c))      # every band pair resolved for the model
    worst = ev.retrieval_metrics((hi_r, zero_r, hi_c, zero_c))     # ... and against it
    for n in names:
        if "rank" in n:
            assert best[n] <= m[n] <= worst[n], n
        else:
            assert worst[n] <= m[n] <= best[n], n
    S = scale * img.double() @ txt.double().T
    lab = torch.arange(3 * b)
    full = (torch.nn.functional.cross_entropy(S, lab) + torch.nn.functional.cross_entropy(S.T, lab)) / 2
    assert abs(m["val_loss_full"] - float(full)) <= 1e-5 + 1e-5 * abs(float(full))
