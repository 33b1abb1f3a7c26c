"""GPU parity of the glue kernels of ops.hip -- fused residual-add + RMSNorm, residual-add +
LayerNorm, causal depthwise conv1d -- against fp64 torch on the same rounded inputs, at every
template instance (NV 1 / 2 / 4 / 8), with the row loop and the software prefetch running
(more rows than waves), in fp32, bf16 and f16.  Run on an MI355X: pytest -m gpu.

Bounds (derived, not fitted to the kernels):
  element-wise outputs (y, dx, dres_in, conv y / dx), zero elements over
      |got - ref| <= A * max(1, max|ref|) + REL * |ref|
      16-bit outputs: A = 2e-5, REL = 2^-8 (bf16) / 2^-10 (f16): the half-ulp bound of the one output
                      rounding plus the fp32 slack
      fp32 outputs  : A = 2e-6, REL = 1e-5
  column reductions (dw, dbias, dx_colsum, conv dw / dbias), n = summed terms per output
      |got - ref| <= 1e-5 * max(1, sqrt(n)) + 1e-5 * |ref|
      (dx_colsum against the fp64 column sums of the kernel's own stored dx)
  saved statistics (mean, rstd): 1e-6 relative + 1e-6 absolute
  bit-exact: LayerNorm h = (x + res) rounded once to the dtype, RMSNorm res_out = x.float() + res,
      the want_colsum=False backward against the want_colsum=True one, a second backward run.

Worst measured err / bound on an MI355X, per kernel and output dtype (the bounds above unchanged):
                               fp32    bf16    f16
  add_layernorm_fwd  y         0.017   0.987   0.481
  add_layernorm_bwd  dx, dres  0.028   0.987   0.482
  add_rmsnorm_fwd    y         0.019   0.987   0.481
  add_rmsnorm_bwd    dx, dres_in 0.030 0.988   0.483   (dres_in is fp32 for every input dtype)
  causal_conv1d_fwd  y         0.018   0.982   0.471
  causal_conv1d_bwd  dx        0.064   0.980   0.475
  column sums (fp32, all input dtypes): LayerNorm dw / dbias / dx_colsum 0.050, RMSNorm dw 0.046,
      conv dw / dbias 0.026
  saved statistics (fp32, all input dtypes): LayerNorm mean 0.079, rstd 0.079; RMSNorm rstd 0.073
The 16-bit figures are the output rounding itself (an fp32 restatement on the CPU gives the same
0.99 / 0.48); A was not widened for any kernel.  The end-of-module report (pytest -s) prints this table.
"""
import math

import pytest
import torch

from oracle import models_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
A_ELEM = {F32: 2e-6, BF16: 2e-5, F16: 2e-5}
REL = {F32: 1e-5, BF16: 2.0 ** -8, F16: 2.0 ** -10}
EPS_RMS, EPS_LN = 1e-5, 1e-6

WORST = {}   # (kernel, output dtype) -> worst err / bound seen in this run


def _name(dt):
    return str(dt)[6:]


def _note(kernel, dt, ratio):
    key = (kernel, _name(dt))
    WORST[key] = max(WORST.get(key, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for (kernel, dt), r in sorted(WORST.items()):
        print(f"\nworst err/bound {kernel:24s} {dt:9s} {r:.3f}", end="")
    print()


def assert_elem(got, ref, kernel, what):
    """Element-wise output in got's dtype against the fp64 reference."""
    dt = got.dtype
    g, r = got.double(), ref.double().to(got.device)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    scale = max(1.0, float(r.abs().max())) if r.numel() else 1.0
    bound = A_ELEM[dt] * scale + REL[dt] * r.abs()
    err = (g - r).abs()
    ratio = float((err / bound).max()) if r.numel() else 0.0
    print(f"{kernel} {what} {_name(dt)}: err/bound {ratio:.3f}")
    bad = ~(err <= bound)   # NaN counts as bad
    assert not bad.any(), (f"{kernel} {what} ({_name(dt)}): {int(bad.sum())}/{bad.numel()} over the bound, "
                           f"worst err/bound {ratio:.3f}, max abs err {float(err.max()):.3e}")
    _note(kernel, dt, ratio)


def assert_colsum(got, ref, n, kernel, what):
    """fp32 column reduction over n terms per output against fp64."""
    assert got.dtype == F32
    g, r = got.double(), ref.double().to(got.device)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bound = 1e-5 * max(1.0, math.sqrt(n)) + 1e-5 * r.abs()
    err = (g - r).abs()
    ratio = float((err / bound).max())
    print(f"{kernel} {what} (n={n}): err/bound {ratio:.3f}")
    bad = ~(err <= bound)
    assert not bad.any(), (f"{kernel} {what}: {int(bad.sum())}/{bad.numel()} over the bound, "
                           f"worst err/bound {ratio:.3f}, max abs err {float(err.max()):.3e}")
    _note(kernel + " colsums", F32, ratio)


def assert_stat(got, ref, kernel, what):
    g, r = got.double(), ref.double().to(got.device)
    err = (g - r).abs()
    bound = 1e-6 * r.abs() + 1e-6
    bad = ~(err <= bound)
    ratio = float((err / bound).max())
    print(f"{kernel} {what}: err/bound {ratio:.3f}")
    assert not bad.any(), f"{kernel} {what}: {int(bad.sum())}/{bad.numel()} over 1e-6 rel + 1e-6 abs, worst err/bound {ratio:.3f}"
    _note(kernel + " " + what, F32, ratio)


class _RoundSTE(torch.autograd.Function):
    """fp64 -> dt -> fp64 rounding whose gradient passes unchanged (torch's own cast rounds the gradient too)."""

    @staticmethod
    def forward(ctx, h, dt):
        return h.to(dt).double()

    @staticmethod
    def backward(ctx, g):
        return g, None


# ---------------------------------------------------------------------------- norm shapes
# vectors per row 9, 64, 65, 128, 129, 257, 512 -> NV 1, 1, 2, 2, 4, 8, 8: a partial wave, exact fits, one
# vector more (only lane 0 holds a second / third / fifth vector) and the documented maximum
NVEC = [9, 64, 65, 128, 129, 257, 512]


def _cols(dt, nvec):
    return nvec * (4 if dt == F32 else 8)


# backward grid: 2048 waves.  3 rows: most waves idle; 4101 = 2 * 2048 + 5: five waves take three rows, the
# rest two (the prefetch carries and ends early on some waves, the accumulators add rows); 2049: exactly one
# wave loops -- at the two NV <= 2 boundary widths
FWD_BWD = [(rows, nvec) for nvec in NVEC for rows in (3, 4101)] + [(2049, 64), (2049, 65)]
# forward grid: at most 16384 waves; 32771 = 2 * 16384 + 3.  Two prefetching instances and one without.
FWD_LOOP = [(32771, 9), (32771, 65), (32771, 129)]
VARIANT_SHAPE = (4101, 65)


def _norm_inputs(kind, dt, rows, cols):
    """CPU inputs of one case (the seed depends on the case only): x, res, w, b, dy, dh."""
    g = torch.Generator().manual_seed(20000 + 131 * rows + cols + {F32: 0, BF16: 1, F16: 2}[dt])
    rdt = F32 if kind == "rms" else dt       # the RMSNorm residual stream is fp32
    x = (torch.randn(rows, cols, generator=g) + 0.25).to(dt)
    res = torch.randn(rows, cols, generator=g).to(rdt)
    w = 1 + 0.25 * torch.randn(cols, generator=g)
    b = 0.25 * torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g).to(dt)
    dh = torch.randn(rows, cols, generator=g).to(rdt)
    return x, res, w, b, dy, dh


def _ln_fwd_c(x, res, w, b, want_h=True):
    """mc_add_layernorm_fwd through the C ABI: y, h_out, mean, rstd."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    h = torch.empty_like(x) if want_h else None
    mean = torch.empty(rows, device=x.device, dtype=F32)
    rstd = torch.empty(rows, device=x.device, dtype=F32)
    _lib.check(lib.mc_add_layernorm_fwd(rows, cols, _lib.dtype_code(x.dtype), x.data_ptr(), _lib.ptr(res),
                                        w.data_ptr(), _lib.ptr(b), EPS_LN, y.data_ptr(), _lib.ptr(h),
                                        mean.data_ptr(), rstd.data_ptr(), _lib.stream_handle()),
               "mc_add_layernorm_fwd")
    return y, h, mean, rstd


def _rms_fwd_c(x, res, w):
    """mc_add_rmsnorm_fwd through the C ABI: y, res_out, rstd."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    rows, cols = x.shape
    y = torch.empty_like(x)
    h = torch.empty(rows, cols, device=x.device, dtype=F32)
    rstd = torch.empty(rows, device=x.device, dtype=F32)
    _lib.check(lib.mc_add_rmsnorm_fwd(rows, cols, _lib.dtype_code(x.dtype), x.data_ptr(), _lib.ptr(res),
                                      w.data_ptr(), EPS_RMS, y.data_ptr(), h.data_ptr(), rstd.data_ptr(),
                                      _lib.stream_handle()), "mc_add_rmsnorm_fwd")
    return y, h, rstd


def _rms_bwd_c(dy, dres, h, w, rstd, want_dres_in=True):
    """mc_add_rmsnorm_bwd through the C ABI (dres nullable): dx, dres_in, dw."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    rows, cols = dy.shape
    dx = torch.empty_like(dy)
    dres_in = torch.empty(rows, cols, device=dy.device, dtype=F32) if want_dres_in else None
    dw = torch.empty(cols, device=dy.device, dtype=F32)
    ws_b = lib.mc_add_rmsnorm_bwd_workspace_bytes(rows, cols)
    ws = torch.empty(ws_b, device=dy.device, dtype=torch.uint8)
    _lib.check(lib.mc_add_rmsnorm_bwd(rows, cols, _lib.dtype_code(dy.dtype), dy.data_ptr(), _lib.ptr(dres),
                                      h.data_ptr(), w.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                      _lib.ptr(dres_in), dw.data_ptr(), ws.data_ptr(), ws_b,
                                      _lib.stream_handle()), "mc_add_rmsnorm_bwd")
    return dx, dres_in, dw


# ---------------------------------------------------------------------------- LayerNorm
def _ln_case(dt, rows, nvec, with_res=True, with_bias=True, grad_h=True, backward=True):
    from mamba_clip_amd import ops
    cols = _cols(dt, nvec)
    x, res, w, b, dy, dh = (t.to(DEV) for t in _norm_inputs("ln", dt, rows, cols))
    if not with_res:
        res = None
    if not with_bias:
        b = None
    xd = x.clone().requires_grad_(True)
    rd = res.clone().requires_grad_(True) if with_res else None
    wd = w.clone().requires_grad_(True)
    bd = b.clone().requires_grad_(True) if with_bias else None
    y, h = ops.add_layernorm(xd, rd, wd, bd, EPS_LN)
    assert y.dtype == dt and y.shape == x.shape

    with torch.no_grad():
        yr, hr = R.add_layernorm_ref(x, res, w, b, EPS_LN, h_dtype=dt)
    assert_elem(y.detach(), yr, "add_layernorm_fwd", "y")
    if with_res:
        assert h.dtype == dt
        assert torch.equal(h.detach(), (x.double() + res.double()).to(dt)), "h != (x + res) rounded once"
    else:
        assert torch.equal(h.detach(), x)

    # saved statistics, straight from the C ABI (the same launch the autograd function makes)
    y2, h2, mean, rstd = _ln_fwd_c(x, res, w, b, want_h=with_res)
    assert torch.equal(y2, y.detach())
    if with_res:
        assert torch.equal(h2, h.detach())
    mu_r = hr.mean(-1)
    rs_r = torch.rsqrt((hr - mu_r[:, None]).pow(2).mean(-1) + EPS_LN)
    assert_stat(mean, mu_r, "add_layernorm_fwd", "mean")
    assert_stat(rstd, rs_r, "add_layernorm_fwd", "rstd")
    if not backward:
        return

    # fp64 gradients through the reference, h rounded straight-through
    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if with_res else None
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if with_bias else None
    hq = _RoundSTE.apply(xr + rr if with_res else xr, dt)
    yg, _ = R.add_layernorm_ref(hq, None, wr, br, EPS_LN)
    assert torch.equal(yg.detach(), yr)
    use_h = with_res and grad_h
    leaves_r = [t for t in (xr, rr, wr, br) if t is not None]
    outs_r, gouts_r = ([yg, hq], [dy.double(), dh.double()]) if use_h else ([yg], [dy.double()])
    gref = dict(zip([n for n, t in zip("xrwb", (xr, rr, wr, br)) if t is not None],
                    torch.autograd.grad(outs_r, leaves_r, gouts_r)))

    if with_res and not grad_h:
        # dh null: only the direct call reaches it (autograd hands the function a zero dh)
        dx, dw, db = ops._layernorm_bwd(h2, w, mean, rstd, dy, None, with_bias, want_colsum=True)
        got = {"x": dx, "r": dx, "w": dw, "b": db}
    else:
        leaves = [t for t in (xd, rd, wd, bd) if t is not None]
        outs, gouts = ([y, h], [dy, dh]) if use_h else ([y], [dy])
        g1 = torch.autograd.grad(outs, leaves, gouts, retain_graph=True)
        g2 = torch.autograd.grad(outs, leaves, gouts)
        for a, c in zip(g1, g2):
            assert torch.equal(a, c), "backward not bitwise repeatable"
        got = dict(zip([n for n, t in zip("xrwb", (xd, rd, wd, bd)) if t is not None], g1))
    assert got["x"].dtype == dt
    assert_elem(got["x"], gref["x"], "add_layernorm_bwd", "dx")
    if with_res:
        assert_elem(got["r"], gref["r"], "add_layernorm_bwd", "dres")
    assert_colsum(got["w"], gref["w"], rows, "add_layernorm_bwd", "dw")
    if with_bias:
        assert_colsum(got["b"], gref["b"], rows, "add_layernorm_bwd", "dbias")

    # the direct backward: dx_colsum, and the instance without it (kDxSum = false), bit for bit
    hk = h2 if with_res else x
    dhk = dh if use_h else None
    dx1, dw1, db1 = ops._layernorm_bwd(hk, w, mean, rstd, dy, dhk, with_bias, want_colsum=True)
    csum, _ = getattr(dx1, ops.COLSUM_ATTR)
    dx0, dw0, db0 = ops._layernorm_bwd(hk, w, mean, rstd, dy, dhk, with_bias, want_colsum=False)
    assert not hasattr(dx0, ops.COLSUM_ATTR)
    assert torch.equal(dx1, got["x"]) and torch.equal(dw1, got["w"])
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1), "want_colsum=False differs from want_colsum=True"
    if with_bias:
        assert torch.equal(db1, got["b"]) and torch.equal(db0, db1)
    else:
        assert db0 is None and db1 is None
    assert_colsum(csum, dx1.double().sum(0), rows, "add_layernorm_bwd", "dx_colsum")


@pytest.mark.parametrize("rows,nvec", FWD_BWD, ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_layernorm_fwd_bwd_instances(dt, rows, nvec):
    _ln_case(dt, rows, nvec)


@pytest.mark.parametrize("rows,nvec", FWD_LOOP, ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_layernorm_fwd_row_loop(dt, rows, nvec):
    _ln_case(dt, rows, nvec, backward=False)


@pytest.mark.parametrize("variant", ["no_res", "no_bias", "no_grad_h"])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_layernorm_variants(dt, variant):
    rows, nvec = VARIANT_SHAPE
    _ln_case(dt, rows, nvec, with_res=variant != "no_res", with_bias=variant != "no_bias",
             grad_h=variant != "no_grad_h")


# ---------------------------------------------------------------------------- RMSNorm
def _rms_case(dt, rows, nvec, with_res=True, grad_h=True, backward=True):
    from mamba_clip_amd import ops
    cols = _cols(dt, nvec)
    x, res, w, _, dy, dh = (t.to(DEV) for t in _norm_inputs("rms", dt, rows, cols))
    if not with_res:
        res = None
    xd = x.clone().requires_grad_(True)
    rd = res.clone().requires_grad_(True) if with_res else None
    wd = w.clone().requires_grad_(True)
    y, h = ops.add_rmsnorm(xd, rd, wd, EPS_RMS)
    assert y.dtype == dt and h.dtype == F32

    with torch.no_grad():
        yr, hr = R.rmsnorm_ref(x, res, w, EPS_RMS)
    assert_elem(y.detach(), yr, "add_rmsnorm_fwd", "y")
    assert torch.equal(h.detach(), x.float() + res if with_res else x.float()), "res_out != x.float() + res"

    y2, h2, rstd = _rms_fwd_c(x, res, w)
    assert torch.equal(y2, y.detach()) and torch.equal(h2, h.detach())
    assert_stat(rstd, torch.rsqrt(hr.pow(2).mean(-1) + EPS_RMS), "add_rmsnorm_fwd", "rstd")
    if not backward:
        return

    xr = x.double().requires_grad_(True)
    rr = res.double().requires_grad_(True) if with_res else None
    wr = w.double().requires_grad_(True)
    yg, hg = R.rmsnorm_ref(xr, rr, wr, EPS_RMS)
    leaves_r = [t for t in (xr, rr, wr) if t is not None]
    outs_r, gouts_r = ([yg, hg], [dy.double(), dh.double()]) if grad_h else ([yg], [dy.double()])
    gref = dict(zip([n for n, t in zip("xrw", (xr, rr, wr)) if t is not None],
                    torch.autograd.grad(outs_r, leaves_r, gouts_r)))

    if grad_h:
        leaves = [t for t in (xd, rd, wd) if t is not None]
        g1 = torch.autograd.grad([y, h], leaves, [dy, dh], retain_graph=True)
        g2 = torch.autograd.grad([y, h], leaves, [dy, dh])
        for a, c in zip(g1, g2):
            assert torch.equal(a, c), "backward not bitwise repeatable"
        got = dict(zip([n for n, t in zip("xrw", (xd, rd, wd)) if t is not None], g1))
    else:
        # dres null: only the C ABI reaches it (autograd hands the function a zero gradient for h)
        dx, dres_in, dw = _rms_bwd_c(dy, None, h2, w, rstd, want_dres_in=with_res)
        dxb, dres_inb, dwb = _rms_bwd_c(dy, None, h2, w, rstd, want_dres_in=with_res)
        assert torch.equal(dx, dxb) and torch.equal(dw, dwb), "backward not bitwise repeatable"
        if with_res:
            assert torch.equal(dres_in, dres_inb), "backward not bitwise repeatable"
        got = {"x": dx, "r": dres_in, "w": dw}
    assert got["x"].dtype == dt
    assert_elem(got["x"], gref["x"], "add_rmsnorm_bwd", "dx")
    if with_res:
        assert got["r"].dtype == F32
        assert_elem(got["r"], gref["r"], "add_rmsnorm_bwd", "dres_in")
    assert_colsum(got["w"], gref["w"], rows, "add_rmsnorm_bwd", "dw")


@pytest.mark.parametrize("rows,nvec", FWD_BWD, ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_rmsnorm_fwd_bwd_instances(dt, rows, nvec):
    _rms_case(dt, rows, nvec)


@pytest.mark.parametrize("rows,nvec", FWD_LOOP, ids=lambda v: str(v))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_rmsnorm_fwd_row_loop(dt, rows, nvec):
    _rms_case(dt, rows, nvec, backward=False)


@pytest.mark.parametrize("variant", ["no_res", "no_grad_h", "no_res_no_grad_h"])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_add_rmsnorm_variants(dt, variant):
    rows, nvec = VARIANT_SHAPE
    _rms_case(dt, rows, nvec, with_res=not variant.startswith("no_res"), grad_h=not variant.endswith("no_grad_h"))


# ---------------------------------------------------------------------------- rejected widths
SENTINEL = -7.0


@pytest.mark.parametrize("dt,cols", [(BF16, 100), (F16, 100), (BF16, 4104), (F16, 4104), (F32, 2052)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_norms_reject_unsupported_widths(dt, cols):
    """cols not a whole number of 16-B vectors, or one vector past the maximum: the error _lib.check
    raises, from every entry point, and no output byte written."""
    from mamba_clip_amd import _lib, ops
    lib = _lib.load()
    rows, code, st = 5, _lib.dtype_code(dt), _lib.stream_handle()
    x = torch.randn(rows, cols, device=DEV).to(dt)
    xf = x.float()
    w = torch.ones(cols, device=DEV)
    stat = torch.rand(rows, device=DEV) + 0.5
    outs = {n: torch.full((rows, cols), SENTINEL, device=DEV, dtype=d)
            for n, d in (("y", dt), ("h", dt), ("h32", F32), ("dx", dt), ("dres", F32))}
    outs.update({n: torch.full((cols,), SENTINEL, device=DEV) for n in ("dw", "db", "cs")})
    outs.update({n: torch.full((rows,), SENTINEL, device=DEV) for n in ("mean", "rstd")})
    ws = torch.empty(max(lib.mc_add_layernorm_bwd_workspace_bytes(rows, cols),
                         lib.mc_add_rmsnorm_bwd_workspace_bytes(rows, cols)), device=DEV, dtype=torch.uint8)
    p = {n: t.data_ptr() for n, t in outs.items()}
    calls = {
        "mc_add_layernorm_fwd": lambda: lib.mc_add_layernorm_fwd(
            rows, cols, code, x.data_ptr(), x.data_ptr(), w.data_ptr(), w.data_ptr(), EPS_LN, p["y"], p["h"],
            p["mean"], p["rstd"], st),
        "mc_add_layernorm_bwd": lambda: lib.mc_add_layernorm_bwd(
            rows, cols, code, x.data_ptr(), x.data_ptr(), x.data_ptr(), w.data_ptr(), stat.data_ptr(),
            stat.data_ptr(), p["dx"], p["dw"], p["db"], p["cs"], ws.data_ptr(), ws.numel(), st),
        "mc_add_rmsnorm_fwd": lambda: lib.mc_add_rmsnorm_fwd(
            rows, cols, code, x.data_ptr(), xf.data_ptr(), w.data_ptr(), EPS_RMS, p["y"], p["h32"], p["rstd"], st),
        "mc_add_rmsnorm_bwd": lambda: lib.mc_add_rmsnorm_bwd(
            rows, cols, code, x.data_ptr(), xf.data_ptr(), xf.data_ptr(), w.data_ptr(), stat.data_ptr(), p["dx"],
            p["dres"], p["dw"], ws.data_ptr(), ws.numel(), st),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match=rf"{name} failed \(code -3\)"):
            _lib.check(call(), name)
    xg = x.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match=r"mc_add_layernorm_fwd failed \(code -3\)"):
        ops.add_layernorm(xg, x, w, w)
    with pytest.raises(RuntimeError, match=r"mc_add_layernorm_fwd failed \(code -3\)"):
        ops.add_layernorm(xg, None, w, None)
    with pytest.raises(RuntimeError, match=r"mc_add_rmsnorm_fwd failed \(code -3\)"):
        ops.add_rmsnorm(xg, xf, w)
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert bool((t == SENTINEL).all()), f"{n} was written"


# ---------------------------------------------------------------------------- causal conv1d
# (B, D, L, K, silu): K = 1 and 2; the generic kernel at ragged L (K = 8 with the widest halo); the vector
# path with Mamba's K = 4 (the backward's halo kernel): several slices with 2-vector rows, and 33 vectors per
# row so that the 63-item wave steps and the slice boundaries fall inside rows; K = 2 on the vector path
CONV_CASES = [
    (3, 40, 17, 1, False),
    (3, 40, 17, 2, True),
    (2, 24, 13, 8, True),
    (2, 64, 80, 4, True),
    (130, 4, 16, 4, True),
    (37, 8, 264, 4, True),
    (2, 16, 24, 2, True),
]


def _conv_case(dt, layout, B, D, L, K, silu, with_bias=True):
    from mamba_clip_amd.ops import causal_conv1d
    g = torch.Generator().manual_seed(7000 + 17 * B + 5 * D + 3 * L + K)
    w = torch.randn(D, 1, K, generator=g)
    b = torch.randn(D, generator=g) if with_bias else None
    gy = torch.randn(B, D, L, generator=g).to(dt)
    if layout == "batch_major":       # rows [0, D) of a (B, 2 D, L) tensor, as the Mamba mixer's split
        big = torch.randn(B, 2 * D, L, generator=g).to(dt)
        x = big[:, :D]
        leaf = xd = big.to(DEV)[:, :D].detach().requires_grad_(True)
        assert xd.stride() == (2 * D * L, L, 1)
    else:                             # the channel-major (2 D, B L) GEMM output viewed (B, D, L)
        xz = torch.randn(2 * D, B * L, generator=g).to(dt)
        x = xz[:D].view(D, B, L).transpose(0, 1)
        leaf = xz.to(DEV).requires_grad_(True)
        xd = leaf[:D].view(D, B, L).transpose(0, 1)
    wd = w.to(DEV).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True) if with_bias else None
    y = causal_conv1d(xd, wd, bd, silu)
    assert y.dtype == dt and y.shape == (B, D, L)
    if layout == "channel_major":
        assert y.stride() == xd.stride()
    leaves = [leaf, wd] + ([bd] if with_bias else [])
    g1 = torch.autograd.grad(y, leaves, gy.to(DEV), retain_graph=True)
    g2 = torch.autograd.grad(y, leaves, gy.to(DEV))
    for a, c in zip(g1, g2):
        assert torch.equal(a, c), "backward not bitwise repeatable"

    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = b.double().requires_grad_(True) if with_bias else None
    yr = R.causal_conv1d_ref(xr, wr, br, silu)
    gr = torch.autograd.grad(yr, [xr, wr] + ([br] if with_bias else []), gy.double())

    assert_elem(y.detach().cpu(), yr.detach(), "causal_conv1d_fwd", "y")
    gx = g1[0]
    if layout == "channel_major":
        assert torch.count_nonzero(gx[D:]) == 0
        gx = gx[:D].view(D, B, L).transpose(0, 1)
    assert gx.dtype == dt
    assert_elem(gx.cpu(), gr[0], "causal_conv1d_bwd", "dx")
    assert_colsum(g1[1].cpu(), gr[1], B * L, "causal_conv1d_bwd", "dw")
    if with_bias:
        assert_colsum(g1[2].cpu(), gr[2], B * L, "causal_conv1d_bwd", "dbias")


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "b{}d{}L{}K{}{}".format(*c[:4], "silu" if c[4] else ""))
@pytest.mark.parametrize("layout", ["batch_major", "channel_major"])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_causal_conv1d_cases(dt, layout, case):
    _conv_case(dt, layout, *case)


@pytest.mark.parametrize("layout", ["batch_major", "channel_major"])
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_causal_conv1d_no_bias(dt, layout):
    _conv_case(dt, layout, 2, 64, 80, 4, True, with_bias=False)
