"""Every reachable gemm_nt_kernel<TIn, TOut, kAligned, kEpi> instance of csrc/contrastive.hip with a
store, CE-statistics or CE-gradient epilogue (kEpi 0 / 1 / 2), per element against the fp64 reference
and bounds of tests/contrastive_ref.py.  (kEpi 3 / 4 / 5 run their unaligned instances in
test_retrieval_gpu.py / test_siglip_gpu.py; the fp8 panel and tile kernels in test_fp8_gpu.py.)

Each case asserts from its operands (contrastive_ref.is_aligned) which kAligned instance it selects,
and, on the reference alone and before any GPU call, that every in-range label logit differs from every
other logit of its row and column by >= 0.05 and that every lse is finite.  With coef = 1 the loss
budget of every case stays below that gap, so the loss check is a per-row target check.
No element is skipped; each test prints max(err / bound) per output (DESIGN.md 4.14 records them).
The fp8 instances of kEpi 1 / 2 run on quantised features and on integer operands (exact logits).
"""
import functools

import pytest
import torch

import contrastive_ref as R
from oracle.loss_ref import quant_rows_fp8_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
NAME = {torch.bfloat16: "bf16", torch.float32: "fp32", torch.float8_e4m3fn: "fp8"}
ALL = [(c, R.SCALE) for c in R.CASES] + [(R.BIG_SCALE_CASE, R.BIG_SCALE)]
COEF_R, COEF_C = 1.0, 0.75          # gradient tests: distinct, so swapped coefficients show
WORST = {}                          # (output, in dtype, out dtype) -> largest err / bound so far


def _id(v):
    case, scale = v
    return "x".join(str(d) for d in case[:3]) + f"_r{case[3]}_c{case[4]}_{case[5]}_s{scale:g}"


def _note(tag, key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{tag} {'/'.join(key)}: err/bound {ratio:.3f} (worst so far {WORST[key]:.3f})")


@functools.lru_cache(maxsize=None)
def _ref(case, scale, dtype):
    """(X, Y, S, eps, forward reference), once per case; the preconditions are asserted here, on the CPU."""
    M, N, K, row_off, col_off, _ = case
    X, Y = R.features(M, N, K, row_off, col_off, dtype, R.case_seed(case))
    S, eps = R.logits(X, Y, scale)
    fwd = R.forward_ref(S, eps, row_off, col_off, 1.0, 1.0)
    gap = R.label_gap(S, fwd)
    assert gap >= R.MIN_LABEL_GAP, (case, gap)
    assert bool(torch.isfinite(fwd.lse_r).all()) and bool(torch.isfinite(fwd.lse_c).all())
    assert float(fwd.loss_bound) < gap, (case, float(fwd.loss_bound), gap)   # one wrong target shows in the loss
    return X, Y, S, eps, fwd


def _operands(case, X, Y):
    """Device operands in the case's layout (pad columns hold NaN: an element read past K would show);
    asserts the alignment the case is in the table for."""
    M, N, K = case[:3]
    layout = case[5]
    Xd, Yd = X.to(DEV), Y.to(DEV)
    if layout == "base":
        buf = torch.full((M, K + 8), float("nan"), dtype=X.dtype, device=DEV)
        buf[:, 1:K + 1] = Xd
        Xd = buf[:, 1:K + 1]
        assert Xd.data_ptr() % 16 != 0 and (Xd.stride(0) * Xd.element_size()) % 16 == 0
    elif layout == "stride":
        buf = torch.full((N, K + 1), float("nan"), dtype=Y.dtype, device=DEV)
        buf[:, :K] = Yd
        Yd = buf[:, :K]
        assert Yd.data_ptr() % 16 == 0 and (Yd.stride(0) * Yd.element_size()) % 16 != 0
    else:
        assert Xd.is_contiguous() and Yd.is_contiguous()
    assert (R.is_aligned(Xd) and R.is_aligned(Yd)) == R.expect_aligned(case, X.dtype), (case, X.dtype)
    return Xd, Yd


SENTINEL = {torch.float32: (torch.int32, 0x7FC12345), torch.bfloat16: (torch.int16, 0x7FC5)}


def _out_view(M, N, dtype, kind):
    """A (M, N) view of a larger sentinel-filled buffer.  "odd": rows 2.., columns 3.. of (M + 3, N + 5)
    -- a misaligned C base, c_vec == 0 on full tiles; "vec": rows 2.., columns 8.. of (M + 3, W), W = N
    rounded up to 8, + 16 -- 16-B aligned with ldc > N, so full tiles keep their vector stores next to
    foreign columns."""
    it, pat = SENTINEL[dtype]
    r0, c0, W = (2, 3, N + 5) if kind == "odd" else (2, 8, (N + 7) // 8 * 8 + 16)
    buf = torch.full((M + 3, W), pat, dtype=it, device=DEV).view(dtype)
    view = buf[r0:r0 + M, c0:c0 + N]
    assert (view.data_ptr() % 16 == 0) == (kind == "vec")
    return buf, view, (r0, c0)


def _assert_outside_untouched(buf, M, N, origin, dtype):
    it, pat = SENTINEL[dtype]
    bits = buf.view(it).clone()
    r0, c0 = origin
    bits[r0:r0 + M, c0:c0 + N] = pat
    assert bool((bits == pat).all()), "bytes outside the out= view were written"


# ---------------------------------------------------------------- kEpi 0: ops.gemm_nt
@pytest.mark.parametrize("case_scale", ALL, ids=_id)
def test_gemm_nt_every_instance_per_element(case_scale):
    from mamba_clip_amd import _lib, ops
    case, scale = case_scale
    M, N, K = case[:3]
    alpha_dev = torch.tensor(scale, device=DEV)
    for in_dt in DTYPES:
        X, Y, S, eps, _ = _ref(case, scale, in_dt)
        Xd, Yd = _operands(case, X, Y)
        for out_dt in DTYPES:
            bound = R.gemm_bound(S, eps, out_dt == torch.bfloat16)
            worst = 0.0
            for dev_alpha in (False, True):
                kw = {"alpha_dev": alpha_dev} if dev_alpha else {"alpha": scale}
                for kind in (None, "odd", "vec"):
                    ops.GEMM_NT_RECORD = []
                    try:
                        if kind is None:
                            C = ops.gemm_nt(Xd, Yd, out_dtype=out_dt, **kw)
                        else:
                            buf, C, origin = _out_view(M, N, out_dt, kind)
                            assert ops.gemm_nt(Xd, Yd, out_dtype=out_dt, out=C, **kw) is C
                            _assert_outside_untouched(buf, M, N, origin, out_dt)
                        assert ops.GEMM_NT_RECORD == [_lib.MC_GEMM_KERNEL_TILE]
                    finally:
                        ops.GEMM_NT_RECORD = None
                    assert C.dtype == out_dt and C.shape == (M, N)
                    ratio = R.ratio(C.cpu(), S, bound)
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (case, NAME[in_dt], NAME[out_dt], dev_alpha, kind, ratio)
            _note(_id(case_scale), ("C", NAME[in_dt], NAME[out_dt]), worst)


# ---------------------------------------------------------------- kEpi 1: ops.ce_fused_fwd
def _fwd_ratios(tag, key_dt, got, S, eps, row_off, col_off, with_cols):
    """err / bound of lse_r, lse_c and the loss, printed; the caller asserts them."""
    loss, lse_r, lse_c = got
    fwd = R.forward_ref(S, eps, row_off, col_off, 1.0, 1.0 if with_cols else 0.0)
    r = {"lse_r": R.ratio(lse_r.cpu(), fwd.lse_r, R.lse_tol(fwd.lse_r))}
    if with_cols:
        r["lse_c"] = R.ratio(lse_c.cpu(), fwd.lse_c, R.lse_tol(fwd.lse_c))
    else:
        assert lse_c is None
    r["loss"] = R.ratio(loss.cpu(), fwd.loss, fwd.loss_bound)
    for name, v in r.items():
        _note(tag, (name, key_dt, "cols" if with_cols else "rows"), v)
    return {(name, with_cols): v for name, v in r.items()}


@pytest.mark.parametrize("case_scale", ALL, ids=_id)
def test_ce_fused_fwd_every_instance_per_row(case_scale):
    from mamba_clip_amd import ops
    case, scale = case_scale
    row_off, col_off = case[3:5]
    sc = torch.tensor(scale, device=DEV)
    for in_dt in DTYPES:
        X, Y, S, eps, _ = _ref(case, scale, in_dt)
        Xd, Yd = _operands(case, X, Y)
        for with_cols in (False, True):
            got = ops.ce_fused_fwd(Xd, Yd, sc, row_off, 1.0, col_off, 1.0 if with_cols else 0.0)
            for key, v in _fwd_ratios(_id(case_scale), NAME[in_dt], got, S, eps, row_off, col_off, with_cols).items():
                assert v <= 1.0, (case, NAME[in_dt], key, v)


@pytest.mark.parametrize("M,N,K", [(130, 130, 38), (257, 200, 64)])
def test_ce_fused_fwd_fp8_instance_per_row(M, N, K):
    """The <fp8, float, true, 1> instance on quant_rows_fp8 operands with their sx / sy factors, against
    the fp64 statistics of the dequantised values.  fp8 operands cannot be unaligned: the host rejects
    rows that are not 16-B aligned multiples of 16 B (fill_operands), so <fp8, *, false, *> never runs --
    asserted below with a 49-byte row stride.

    This test found the one kernel change of the suite: with v_mfma_f32_16x16x32_fp8_fp8 in the K loop the
    instance missed the lse tolerance by 13.7x (130 x 130) and 8.2x (257 x 200), |err| up to 3.9e-4 on
    lse ~ 17.7.  The instruction does not add real-valued fp8 products as an exact fp32 sum: |dS_ij| up to
    2.5e-5 scale sum_k |x_ik y_jk| = 4.5 eps_ij, two-sided, the same in every wave quadrant, edge tile and on
    the label diagonal, proportional to the scale, nothing on integers.  The fused-CE fp8 instances now
    convert the fragments to bf16 in registers (exact) and run the bf16 MFMA of the same shape."""
    from mamba_clip_amd import ops
    case = (M, N, K, 0, 0, "contig")
    X, Y = R.features(M, N, K, 0, 0, torch.float32, R.case_seed(case))
    (qx, ix), (qy, iy) = quant_rows_fp8_ref(X), quant_rows_fp8_ref(Y)
    Xq = qx.view(torch.float8_e4m3fn).double() * ix.double()[:, None]
    Yq = qy.view(torch.float8_e4m3fn).double() * iy.double()[:, None]
    S, eps = R.logits(Xq, Yq, R.SCALE)
    fwd = R.forward_ref(S, eps, 0, 0, 1.0, 1.0)
    gap = R.label_gap(S, fwd)
    assert gap >= R.MIN_LABEL_GAP and float(fwd.loss_bound) < gap
    assert bool(torch.isfinite(fwd.lse_r).all()) and bool(torch.isfinite(fwd.lse_c).all())

    Qx, sx = ops.quant_rows_fp8(X.to(DEV))
    Qy, sy = ops.quant_rows_fp8(Y.to(DEV))
    assert torch.equal(Qx.view(torch.uint8).cpu(), qx) and torch.equal(sx.cpu(), ix)    # the reference's operands
    assert torch.equal(Qy.view(torch.uint8).cpu(), qy) and torch.equal(sy.cpu(), iy)
    assert Qx.shape[1] % 16 == 0 and R.is_aligned(Qx) and R.is_aligned(Qy)
    sc = torch.tensor(R.SCALE, device=DEV)
    pad = torch.zeros(M, Qx.shape[1] + 1, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn)[:, :-1]
    assert not R.is_aligned(pad)
    with pytest.raises(RuntimeError, match="fp8 operands need"):
        ops.ce_fused_fwd(pad, Qy, sc, 0, 1.0, 0, 0.0, sx=sx, sy=sy)
    ratios = {}
    for with_cols in (False, True):
        got = ops.ce_fused_fwd(Qx, Qy, sc, 0, 1.0, 0, 1.0 if with_cols else 0.0, sx=sx, sy=sy)
        ratios.update(_fwd_ratios(f"fp8 {M}x{N}x{K}", "fp8", got, S, eps, 0, 0, with_cols))
    for key, v in ratios.items():
        assert v <= 1.0, (M, N, K, key, v)


def _int_fp8_features(M, N, K, seed):
    """Integers in [-3, 3] (exact in e4m3, every partial sum exact in fp32), Y_j = X_j for the paired rows."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-3, 4, (M, K), generator=g).float()
    Y = torch.randint(-3, 4, (N, K), generator=g).float()
    n = min(M, N)
    Y[:n] = X[:n]
    return X, Y


@pytest.mark.parametrize("M,N,K", [(130, 130, 48), (257, 200, 64)])
def test_fp8_instances_on_exact_integer_logits(M, N, K):
    """<fp8, float, true, 1> and <fp8, float | bf16, true, 2> with the MFMA's accumulation taken out:
    integer operands and scale 2^-3 make every logit, and every partial sum of it, exact in fp32, so the fp32 bounds apply to the fp8 instances' tile, edge and label arithmetic --
    independent of how the products are accumulated.
    No dequantisation factors: the operands are the integers themselves (sx = sy = NULL)."""
    from mamba_clip_amd import ops
    scale = 0.125
    X, Y = _int_fp8_features(M, N, K, M + N + K)
    S, eps = R.logits(X, Y, scale)
    fwd = R.forward_ref(S, eps, 0, 0, 1.0, 1.0)
    gap = R.label_gap(S, fwd)
    assert gap >= R.MIN_LABEL_GAP and float(fwd.loss_bound) < gap
    assert bool(torch.isfinite(fwd.lse_r).all()) and bool(torch.isfinite(fwd.lse_c).all())
    assert bool((S.float().double() == S).all())                       # exactly representable logits

    Qx, Qy = X.to(torch.float8_e4m3fn).to(DEV), Y.to(torch.float8_e4m3fn).to(DEV)
    assert torch.equal(Qx.float().cpu(), X) and R.is_aligned(Qx) and R.is_aligned(Qy)
    sc = torch.tensor(scale, device=DEV)
    tag = f"fp8 integers {M}x{N}x{K}"
    for with_cols in (False, True):
        got = ops.ce_fused_fwd(Qx, Qy, sc, 0, 1.0, 0, 1.0 if with_cols else 0.0)
        for key, v in _fwd_ratios(tag, "fp8int", got, S, eps, 0, 0, with_cols).items():
            assert v <= 1.0, (M, N, K, key, v)
    lr_d, lc_d = fwd.lse_r.float().to(DEV), fwd.lse_c.float().to(DEV)
    gout = torch.tensor(-0.37, device=DEV)
    gout64 = float(gout.cpu().double())
    for use_r, use_c in ((True, False), (False, True), (True, True)):
        for g_dt in DTYPES:
            ref = R.grad_ref(S, eps, fwd.lse_r if use_r else None, fwd.lse_c if use_c else None, 0, 0, COEF_R, COEF_C,
                             gout64, scale, g_dt == torch.bfloat16)
            G0, _ = ops.ce_fused_grad(Qx, Qy, sc, lr_d if use_r else None, lc_d if use_c else None, 0, COEF_R, 0, COEF_C,
                                      gout, g_dt, want_dscale=False)
            G1, ds = ops.ce_fused_grad(Qx, Qy, sc, lr_d if use_r else None, lc_d if use_c else None, 0, COEF_R, 0, COEF_C,
                                       gout, g_dt, want_dscale=True)
            assert G0.dtype == g_dt and torch.equal(G0, G1)
            rg, rd = R.ratio(G0.cpu(), ref.G, ref.bound), R.ratio(ds.cpu(), ref.dscale, ref.dscale_bound)
            _note(tag, ("G", "fp8int", NAME[g_dt]), rg)
            _note(tag, ("dscale", "fp8int", NAME[g_dt]), rd)
            assert rg <= 1.0 and rd <= 1.0, (M, N, K, use_r, use_c, NAME[g_dt], rg, rd)


# ---------------------------------------------------------------- kEpi 2: ops.ce_fused_grad, one block
@pytest.mark.parametrize("case_scale", ALL, ids=_id)
def test_ce_fused_grad_every_instance_per_element(case_scale):
    """All four <TIn, TOut> pairs; lse_r only, lse_c only (the transposed-problem call of
    ScaledLogitsCE.backward leaves the other NULL) and both; gout 1 and -0.37; with and without the
    logit_scale gradient (G bitwise equal).  The lse inputs are the fp64 reference's, rounded to fp32,
    not the forward kernel's: a forward error cannot cancel a backward one."""
    from mamba_clip_amd import ops
    case, scale = case_scale
    M, N, K, row_off, col_off, _ = case
    sc = torch.tensor(scale, device=DEV)
    for in_dt in DTYPES:
        X, Y, S, eps, fwd = _ref(case, scale, in_dt)
        Xd, Yd = _operands(case, X, Y)
        lr32, lc32 = fwd.lse_r.float(), fwd.lse_c.float()
        lr_d, lc_d = lr32.to(DEV), lc32.to(DEV)
        worst = {}
        for use_r, use_c in ((True, False), (False, True), (True, True)):
            for gout_v in (1.0, -0.37):
                gout = torch.tensor(gout_v, device=DEV)
                gout64 = float(gout.cpu().double())                      # the fp32 value the kernel reads
                for g_dt in DTYPES:
                    ref = R.grad_ref(S, eps, fwd.lse_r if use_r else None, fwd.lse_c if use_c else None, row_off,
                                     col_off, COEF_R, COEF_C, gout64, scale, g_dt == torch.bfloat16)
                    G0, none = ops.ce_fused_grad(Xd, Yd, sc, lr_d if use_r else None, lc_d if use_c else None, row_off,
                                                 COEF_R, col_off, COEF_C, gout, g_dt, want_dscale=False)
                    G1, ds = ops.ce_fused_grad(Xd, Yd, sc, lr_d if use_r else None, lc_d if use_c else None, row_off,
                                               COEF_R, col_off, COEF_C, gout, g_dt, want_dscale=True)
                    assert none is None and G0.dtype == g_dt and G0.shape == (M, N)
                    assert torch.equal(G0, G1), "G differs with the logit_scale gradient on"
                    rg = R.ratio(G0.cpu(), ref.G, ref.bound)
                    rd = R.ratio(ds.cpu(), ref.dscale, ref.dscale_bound)
                    kg, kd = ("G", NAME[in_dt], NAME[g_dt]), ("dscale", NAME[in_dt], NAME[g_dt])
                    worst[kg], worst[kd] = max(worst.get(kg, 0.0), rg), max(worst.get(kd, 0.0), rd)
                    assert rg <= 1.0, (case, NAME[in_dt], NAME[g_dt], use_r, use_c, gout_v, "G", rg)
                    assert rd <= 1.0, (case, NAME[in_dt], NAME[g_dt], use_r, use_c, gout_v, "dscale", rd,
                                       float(ds), float(ref.dscale), float(ref.dscale_bound))
        for key, v in worst.items():
            _note(_id(case_scale), key, v)


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_three_entry_points_bitwise_repeatable(dtype):
    """gemm_nt, ce_fused_fwd and ce_fused_grad twice on an unaligned, ragged case: the same bits."""
    from mamba_clip_amd import ops
    case, scale = (130, 130, 38, 0, 0, "contig"), R.SCALE
    X, Y, _, _, fwd = _ref(case, scale, dtype)
    Xd, Yd = _operands(case, X, Y)
    assert not R.is_aligned(Xd)
    sc = torch.tensor(scale, device=DEV)
    gout = torch.tensor(-0.37, device=DEV)
    lr, lc = fwd.lse_r.float().to(DEV), fwd.lse_c.float().to(DEV)

    def run():
        out = [ops.gemm_nt(Xd, Yd, alpha_dev=sc, out_dtype=dtype)]
        out += list(ops.ce_fused_fwd(Xd, Yd, sc, 0, 1.0, 0, 1.0))
        out += list(ops.ce_fused_grad(Xd, Yd, sc, lr, lc, 0, COEF_R, 0, COEF_C, gout, dtype, want_dscale=True))
        return out

    for a, b in zip(run(), run()):
        assert torch.equal(a, b)
