"""GPU parity of mc_last_token_rmsnorm_fwd / _bwd (ops.hip) -- the Mamba text tower's final norm on the
row of each caption's last non-pad token -- against fp64 torch on the same rounded inputs, through the
C ABI, in fp32, bf16 and f16.  Run on an MI355X: pytest -m gpu.

Bounds: those derived in test_norm_conv_gpu.py's header for mc_add_rmsnorm_*, restated, not widened:
  element-wise outputs (y, the pooled rows of dx / dres_in)
      |got - ref| <= A * max(1, max|ref|) + REL * |ref|
      16-bit outputs: A = 2e-5, REL = 2^-8 (bf16) / 2^-10 (f16); fp32 outputs (dres_in always): A = 2e-6, REL = 1e-5
  column sums (dw), n = batch terms per output:  |got - ref| <= 1e-5 * max(1, sqrt(n)) + 1e-5 * |ref|
  rstd: 1e-6 relative + 1e-6 absolute
  exact: pos; h_out = x.float() + res bit for bit; every row of dx / dres_in but pos[b] zero (the
      buffers hold NaN before the launch: the kernel writes all of them); a second backward bitwise equal.
The forward and backward launches run under torch.cuda.set_sync_debug_mode("error"): no host sync.

Shapes: one width per vector-count instance of the norm kernels (vectors per row 9, 65, 129, 257 -> NV 1, 2,
4, 8) plus the tower widths 768 and 1536; (T, Lp) = (1, 8), (37, 40), (77, 80), (300, 304) -- the last has
more tokens than the workgroup has threads, so the search loops; batch 7 holds a full caption, a
one-token caption, an all-pad row, pad ids inside captions and lengths around T / 2; batch 1 runs the
full, the one-token and the all-pad row alone.  pad_id 0, 1 and 2^40 + 3 with captions made of the id 3:
a compare of the low 32 bits would call every one of them pad.

Worst measured err / bound on an MI355X (the bounds above unchanged):
                     fp32    bf16    f16
  fwd y              0.016   0.983   0.479
  bwd dx             0.018   0.984   0.476
  bwd dres_in (fp32, all input dtypes) 0.022;  dw 0.030;  rstd 0.049
The 16-bit figures are the output rounding itself, as for mc_add_rmsnorm_* (test_norm_conv_gpu.py)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
A_ELEM = {F32: 2e-6, BF16: 2e-5, F16: 2e-5}
REL = {F32: 1e-5, BF16: 2.0 ** -8, F16: 2.0 ** -10}
EPS = 1e-5
NVEC = [9, 65, 129, 257]
TL = [(1, 8), (37, 40), (77, 80), (300, 304)]
BIG_PAD = 2 ** 40 + 3


def _name(dt):
    return str(dt)[6:]


def _widths(dt):
    return [n * (4 if dt == F32 else 8) for n in NVEC] + [768, 1536]


def assert_elem(got, ref, what):
    dt = got.dtype
    g, r = got.double(), ref.double().to(got.device)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bound = A_ELEM[dt] * max(1.0, float(r.abs().max())) + REL[dt] * r.abs()
    err = (g - r).abs()
    ratio = float((err / bound).max())
    print(f"{what} {_name(dt)}: err/bound {ratio:.3f}")
    bad = ~(err <= bound)   # NaN counts as bad
    assert not bad.any(), f"{what} ({_name(dt)}): {int(bad.sum())}/{bad.numel()} over the bound, worst {ratio:.3f}"


def assert_colsum(got, ref, n, what):
    assert got.dtype == F32
    g, r = got.double(), ref.double().to(got.device)
    bound = 1e-5 * max(1.0, math.sqrt(n)) + 1e-5 * r.abs()
    err = (g - r).abs()
    ratio = float((err / bound).max())
    print(f"{what} (n={n}): err/bound {ratio:.3f}")
    assert not (~(err <= bound)).any(), f"{what}: worst err/bound {ratio:.3f}"


def assert_stat(got, ref, what):
    g, r = got.double(), ref.double().to(got.device)
    err, bound = (g - r).abs(), 1e-6 * r.abs() + 1e-6
    ratio = float((err / bound).max())
    print(f"{what}: err/bound {ratio:.3f}")
    assert not (~(err <= bound)).any(), f"{what}: worst err/bound {ratio:.3f}"


def _tokens(kind, batch, T, pad_id, g):
    """(tokens (batch, T) int64 on the CPU, expected pos as a list, found by a plain loop)."""
    if pad_id == BIG_PAD:
        real = torch.full((batch, T), 3, dtype=torch.int64)     # the pad id's low 32 bits
        real[:, ::3] = 2 ** 41 + 3
    else:
        real = torch.randint(2, 90, (batch, T), generator=g)     # never 0 or 1
    if kind == "batch":
        lengths = [T, 1, 0, T, max(1, T // 2), min(T, T // 2 + 1), max(1, T - 1)][:batch]
    else:
        lengths = [{"full": T, "one": 1, "allpad": 0}[kind]] * batch
    tok = torch.full((batch, T), pad_id, dtype=torch.int64)
    for b, n in enumerate(lengths):
        tok[b, :n] = real[b, :n]
    if kind == "batch" and T >= 3:
        tok[3, T // 2] = pad_id          # pad ids inside a full caption ...
        tok[3, 0] = pad_id
        tok[4, 0] = pad_id               # ... and at the front of a short one (T // 2 >= 2 tokens for T >= 37)
    pos = []
    for b in range(batch):
        p = 0
        for t in range(T):
            if int(tok[b, t]) != pad_id:
                p = t
        pos.append(p)
    return tok, pos


def _fwd_c(tokens, pad_id, x, res, w):
    from mamba_clip_amd import _lib
    lib = _lib.load()
    batch, Lp, cols = x.shape
    y = torch.full((batch, cols), float("nan"), device=DEV, dtype=x.dtype)
    h = torch.full((batch, cols), float("nan"), device=DEV, dtype=F32)
    rstd = torch.full((batch,), float("nan"), device=DEV, dtype=F32)
    pos = torch.full((batch,), -7, device=DEV, dtype=torch.int32)
    torch.cuda.set_sync_debug_mode("error")
    try:
        rc = lib.mc_last_token_rmsnorm_fwd(batch, tokens.shape[1], Lp, cols, _lib.dtype_code(x.dtype), tokens.data_ptr(),
                                           pad_id, x.data_ptr(), _lib.ptr(res), w.data_ptr(), EPS, y.data_ptr(),
                                           h.data_ptr(), rstd.data_ptr(), pos.data_ptr(), _lib.stream_handle())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _lib.check(rc, "mc_last_token_rmsnorm_fwd")
    return y, h, rstd, pos


def _bwd_c(dy, h, w, rstd, pos, Lp, has_res):
    from mamba_clip_amd import _lib
    lib = _lib.load()
    batch, cols = h.shape
    dx = torch.full((batch, Lp, cols), float("nan"), device=DEV, dtype=dy.dtype)
    dres = torch.full((batch, Lp, cols), float("nan"), device=DEV, dtype=F32) if has_res else None
    dw = torch.full((cols,), float("nan"), device=DEV, dtype=F32)
    torch.cuda.set_sync_debug_mode("error")
    try:
        rc = lib.mc_last_token_rmsnorm_bwd(batch, Lp, cols, _lib.dtype_code(dy.dtype), dy.data_ptr(), h.data_ptr(),
                                           w.data_ptr(), rstd.data_ptr(), pos.data_ptr(), dx.data_ptr(), _lib.ptr(dres),
                                           dw.data_ptr(), _lib.stream_handle())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _lib.check(rc, "mc_last_token_rmsnorm_bwd")
    return dx, dres, dw


def _case(dt, cols, batch, T, Lp, pad_id=0, has_res=True, kind="batch"):
    g = torch.Generator().manual_seed(7000 + 131 * cols + 17 * T + batch + {F32: 0, BF16: 1, F16: 2}[dt])
    tok, want_pos = _tokens(kind, batch, T, pad_id, g)
    x = (torch.randn(batch, Lp, cols, generator=g) + 0.25).to(dt)
    res = torch.randn(batch, Lp, cols, generator=g) if has_res else None
    w = 1 + 0.25 * torch.randn(cols, generator=g)
    dy = torch.randn(batch, cols, generator=g).to(dt)
    xd, wd, dyd, tokd = x.to(DEV), w.to(DEV), dy.to(DEV), tok.to(DEV)
    resd = res.to(DEV) if has_res else None

    y, h, rstd, pos = _fwd_c(tokd, pad_id, xd, resd, wd)
    assert pos.tolist() == want_pos
    rows = torch.arange(batch)
    p = torch.tensor(want_pos)
    h32 = x[rows, p].float() + (res[rows, p] if has_res else 0)
    assert torch.equal(h.cpu(), h32), "h_out is not x.float() + res bit for bit"
    # fp64 on the same rounded inputs
    hr = (x[rows, p].double() + (res[rows, p].double() if has_res else 0)).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    rs = torch.rsqrt(hr.pow(2).mean(-1) + EPS)
    yr = hr * rs[:, None] * wr
    yr.backward(dy.double())
    assert_elem(y, yr.detach(), "fwd y")
    assert_stat(rstd, rs.detach(), "fwd rstd")

    dx, dres, dw = _bwd_c(dyd, h, wd, rstd, pos, Lp, has_res)
    dx2, dres2, dw2 = _bwd_c(dyd, h, wd, rstd, pos, Lp, has_res)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and (not has_res or torch.equal(dres, dres2))
    assert_colsum(dw, wr.grad, batch, "bwd dw")
    off = torch.ones(batch, Lp, dtype=torch.bool)
    off[rows, p] = False
    for name, got in (("dx", dx), ("dres_in", dres)):
        if got is None:
            continue
        got = got.cpu()
        assert_elem(got[rows, p], hr.grad, f"bwd {name}")
        rest = got[off]
        assert rest.numel() == batch * (Lp - 1) * cols and not rest.view(torch.uint8).any(), f"{name}: rows off pos not +0"


@pytest.mark.parametrize("TLp", TL, ids=lambda v: f"T{v[0]}")
@pytest.mark.parametrize("icol", range(6))
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_every_instance_batch7(dt, icol, TLp):
    _case(dt, _widths(dt)[icol], 7, *TLp)


@pytest.mark.parametrize("variant", ["full", "one", "allpad", "nores", "pad1", "padbig", "padbig_nores"])
@pytest.mark.parametrize("TLp", TL, ids=lambda v: f"T{v[0]}")
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_variants(dt, TLp, variant):
    cols = 768
    if variant in ("full", "one", "allpad"):
        _case(dt, cols, 1, *TLp, kind=variant)
        _case(dt, cols, 1, *TLp, kind=variant, has_res=False, pad_id=1)
    elif variant == "nores":
        _case(dt, cols, 7, *TLp, has_res=False)
    elif variant == "pad1":
        _case(dt, cols, 7, *TLp, pad_id=1)
    else:
        _case(dt, cols, 7, *TLp, pad_id=BIG_PAD, has_res=variant == "padbig")
        _case(dt, cols, 1, *TLp, pad_id=BIG_PAD, kind="full")


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_autograd_op_matches_add_rmsnorm_on_the_pooled_rows(dt):
    """ops.last_token_rmsnorm against ops.add_rmsnorm over all rows + a gather (the path of pad_id=None
    when every caption is full): same y bits, same dx / dres / dw within the kernels' bounds."""
    from mamba_clip_amd import ops
    g = torch.Generator().manual_seed(5)
    batch, T, Lp, cols = 7, 37, 40, 768
    tok, want_pos = _tokens("batch", batch, T, 0, g)
    x = torch.randn(batch, Lp, cols, generator=g).to(dt)
    res = torch.randn(batch, Lp, cols, generator=g)
    w = 1 + 0.25 * torch.randn(cols, generator=g)
    gy = torch.randn(batch, cols, generator=g).to(dt).to(DEV)
    rows, p = torch.arange(batch, device=DEV), torch.tensor(want_pos, device=DEV)
    leaves = [[t.to(DEV).requires_grad_(True) for t in (x, res, w)] for _ in range(2)]
    y, pos = ops.last_token_rmsnorm(tok.to(DEV), 0, *leaves[0], EPS)
    assert pos.dtype == torch.int32 and not pos.requires_grad and pos.tolist() == want_pos
    y.backward(gy)
    yr = ops.add_rmsnorm(*leaves[1], EPS)[0][rows, p]
    yr.backward(gy)
    assert torch.equal(y, yr)
    for name, a, b in zip(("dx", "dres"), leaves[0], leaves[1]):
        assert a.grad.shape == b.grad.shape and a.grad.dtype == b.grad.dtype
        assert_elem(a.grad, b.grad, name)
    assert_colsum(leaves[0][2].grad, leaves[1][2].grad, batch, "dw")


def test_rejects_what_add_rmsnorm_rejects():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    t = torch.zeros(2, 8, dtype=torch.int64, device=DEV)
    buf = torch.zeros(2 * 8 * 8192, device=DEV)
    p = buf.data_ptr()

    def fwd(cols, dtype, T=8, Lp=8):
        return lib.mc_last_token_rmsnorm_fwd(2, T, Lp, cols, dtype, t.data_ptr(), 0, p, None, p, EPS, p, p, p, p,
                                             _lib.stream_handle())

    def bwd(cols, dtype):
        return lib.mc_last_token_rmsnorm_bwd(2, 8, cols, dtype, p, p, p, p, p, p, None, p, _lib.stream_handle())

    def norm(cols, dtype):
        return lib.mc_add_rmsnorm_fwd(16, cols, dtype, p, None, p, EPS, p, p, p, _lib.stream_handle())
    for cols, dtype in ((12, _lib.MC_DTYPE_BF16), (6, _lib.MC_DTYPE_F32), (4104, _lib.MC_DTYPE_F16),
                        (2052, _lib.MC_DTYPE_F32), (0, _lib.MC_DTYPE_F32), (64, 7)):
        want = norm(cols, dtype)
        assert want != 0 and fwd(cols, dtype) == want and bwd(cols, dtype) == want, (cols, dtype)
    assert fwd(64, _lib.MC_DTYPE_F32, T=9, Lp=8) == -3 and b"T <= Lp" in lib.mc_last_error()
    assert fwd(64, _lib.MC_DTYPE_F32, T=0, Lp=8) == -3
    torch.cuda.synchronize()
