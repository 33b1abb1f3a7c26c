"""Pair scan backward with LDS-staged rows: every staging edge against the fp64 oracle.

The kernel copies each 32-position chunk of the u / delta / z / dout rows to LDS by DMA, which checks
no range, so the shapes reach a wave with fewer than 32 rows and waves with none (dim 32 / 96 / 160),
a one-sub-tile chunk, partial last chunks and more than two chunks (L), both saved-state layouts, both
dtypes, with and without z and softplus, and dense rows as well as the mixer's channel-major views.
Every run writes into NaN-prefilled buffers with guard bands, reads inputs whose row padding is NaN,
and is repeated for a bitwise comparison.  Tolerances are those of test_scan_gpu.py."""
import functools

import pytest
import torch

from oracle.scan_ref import selective_scan_ref_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
BATCH, N = 2, 16
PAD = 8          # row padding (elements) of the dense layout: rows stay 16-B aligned
GUARD = 64       # guard band (elements) on either side of an output
GRAD_REL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -9}   # test_scan_gpu.py
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
NAN32 = 0x7FC00001


def assert_grad_close(got, ref, dtype, what):
    got = got.float().cpu()
    ref = ref.float().cpu()
    scale = float(ref.abs().max().clamp_min(1e-6))
    tol = 2e-4 * scale + GRAD_REL[dtype] * ref.abs()
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (f"grad {what}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err "
                           f"{float(err.max()):.3e} (scale {scale:.3e})")


@functools.lru_cache(maxsize=None)
def _case(dim, L, dtype, z, sp):
    """CPU inputs and the oracle's gradients, computed once and shared by the layouts and intervals."""
    gen = torch.Generator().manual_seed(dim * 1000 + L)
    # the step dt = f(delta + bias) must be positive (the decay is exp(dt A), A < 0): with softplus any
    # delta will do; without it delta + bias is the step itself, so both are drawn positive
    raw = torch.randn(BATCH, dim, L, generator=gen)
    x = dict(
        u=torch.randn(BATCH, dim, L, generator=gen).to(dtype),
        delta=(0.5 * raw if sp else 0.02 + 0.25 * raw.abs()).to(dtype),
        A=-torch.exp(torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(dim, 1)
                     + 0.1 * torch.randn(dim, N, generator=gen)),
        B=torch.randn(BATCH, 1, N, L, generator=gen).to(dtype),
        C=torch.randn(BATCH, 1, N, L, generator=gen).to(dtype),
        D=torch.randn(dim, generator=gen),
        z=torch.randn(BATCH, dim, L, generator=gen).to(dtype) if z else None,
        delta_bias=torch.rand(dim, generator=gen) * 4 - 5 if sp else 0.1 * torch.rand(dim, generator=gen),
    )
    dout = torch.randn(BATCH, dim, L, generator=gen).to(dtype)
    ref = selective_scan_ref_grads(**x, delta_softplus=sp, dout=dout.double(), compute_dtype=torch.float64)
    return x, dout, ref


class Guarded:
    """A tensor view inside a flat buffer prefilled with a NaN bit pattern, guard bands included."""

    def __init__(self, shape, strides, dtype, extent):
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.pattern = NAN32 if dtype == torch.float32 else NAN16[dtype]
        self.flat = torch.full((extent + 2 * GUARD,), self.pattern, dtype=self.bits, device=DEV)
        self.view = self.flat.view(dtype).as_strided(shape, strides, GUARD)
        self.inside = torch.zeros(extent + 2 * GUARD, dtype=torch.bool, device=DEV)
        self.inside.as_strided(shape, strides, GUARD).fill_(True)

    def check(self, what):
        assert not torch.isnan(self.view).any(), f"{what}: NaN in the output"
        outside = self.flat[~self.inside]
        assert bool((outside == self.pattern).all()), f"{what}: {int((outside != self.pattern).sum())} elements outside the output changed"


def _rows(t, layout, fill_nan):
    """(B, D, L) CPU tensor -> device view in the layout; dense rows carry NaN padding past L."""
    Bsz, D, L = t.shape
    if layout == "cm":     # the mixer's views: batch stride L, channel stride B L
        v = t.transpose(0, 1).contiguous().to(DEV).transpose(0, 1)
        assert v.stride() == (L, Bsz * L, 1)
        return v
    big = torch.full((Bsz, D, L + PAD), float("nan") if fill_nan else 0.0, dtype=t.dtype)
    big[:, :, :L] = t
    return big.to(DEV)[:, :, :L]


def _rows_out(Bsz, D, L, dtype, layout):
    if layout == "cm":
        return Guarded((Bsz, D, L), (L, Bsz * L, 1), dtype, Bsz * D * L)
    return Guarded((Bsz, D, L), (D * (L + PAD), L + PAD, 1), dtype, Bsz * D * (L + PAD))


def _run_bwd(dx, dout, states, sp, layout):
    """mc_scan_bwd with every output in a guarded buffer (the interface's scan_bwd allocates its own)."""
    from mamba_clip_amd import _lib
    from mamba_clip_amd import selective_scan_interface as ssi
    lib = _lib.load()
    u, delta, z, Bm, Cm = dx["u"], dx["delta"], dx["z"], dx["B"], dx["C"]
    batch, dim, L = delta.shape
    dt = u.dtype
    out = dict(u=_rows_out(batch, dim, L, dt, layout), delta=_rows_out(batch, dim, L, dt, layout),
               B=Guarded((batch, 1, N, L), (N * L, N * L, L, 1), dt, batch * N * L),
               C=Guarded((batch, 1, N, L), (N * L, N * L, L, 1), dt, batch * N * L),
               A=Guarded((dim, N), (N, 1), torch.float32, dim * N),
               D=Guarded((dim,), (1,), torch.float32, dim),
               delta_bias=Guarded((dim,), (1,), torch.float32, dim))
    if z is not None:
        out["z"] = _rows_out(batch, dim, L, dt, layout)
    ws_bytes = lib.mc_scan_bwd_workspace_bytes(batch, dim, L, N, 1)
    ws = torch.empty(max(ws_bytes, 1), device=DEV, dtype=torch.uint8)
    p = _lib.ScanBwdParams()
    p.batch, p.dim, p.seqlen, p.dstate, p.n_groups = batch, dim, L, N, 1
    p.itype = p.wtype = _lib.dtype_code(dt)
    p.delta_softplus = int(sp)
    p.u_batch_stride, p.u_dim_stride = u.stride(0), u.stride(1)
    p.delta_batch_stride, p.delta_dim_stride = delta.stride(0), delta.stride(1)
    p.dout_batch_stride, p.dout_dim_stride = dout.stride(0), dout.stride(1)
    du, dd = out["u"].view, out["delta"].view
    p.du_batch_stride, p.du_dim_stride = du.stride(0), du.stride(1)
    p.ddelta_batch_stride, p.ddelta_dim_stride = dd.stride(0), dd.stride(1)
    if z is not None:
        dz = out["z"].view
        p.z_batch_stride, p.z_dim_stride = z.stride(0), z.stride(1)
        p.dz_batch_stride, p.dz_dim_stride = dz.stride(0), dz.stride(1)
        p.z, p.dz = z.data_ptr(), dz.data_ptr()
    dB, dC = out["B"].view, out["C"].view
    p.B_batch_stride, p.B_group_stride, p.B_dstate_stride = Bm.stride(0), Bm.stride(1), Bm.stride(2)
    p.C_batch_stride, p.C_group_stride, p.C_dstate_stride = Cm.stride(0), Cm.stride(1), Cm.stride(2)
    p.dB_batch_stride, p.dB_group_stride, p.dB_dstate_stride = dB.stride(0), dB.stride(1), dB.stride(2)
    p.dC_batch_stride, p.dC_group_stride, p.dC_dstate_stride = dC.stride(0), dC.stride(1), dC.stride(2)
    p.u, p.delta, p.A, p.B, p.C = u.data_ptr(), delta.data_ptr(), dx["A"].data_ptr(), Bm.data_ptr(), Cm.data_ptr()
    p.D, p.delta_bias = dx["D"].data_ptr(), dx["delta_bias"].data_ptr()
    p.dout, p.chunk_states = dout.data_ptr(), states.data_ptr()
    p.state_interval = ssi.states_interval(L, dim, states)
    p.du, p.ddelta, p.dB, p.dC = du.data_ptr(), dd.data_ptr(), dB.data_ptr(), dC.data_ptr()
    p.dA, p.dD, p.ddelta_bias = out["A"].view.data_ptr(), out["D"].view.data_ptr(), out["delta_bias"].view.data_ptr()
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws_bytes
    assert lib.mc_scan_bwd_kernel(p) == _lib.MC_SCAN_KERNEL_PAIR, "the case must run the pair kernel"
    _lib.check(lib.mc_scan_bwd(p, _lib.stream_handle(u.device)), "mc_scan_bwd")
    torch.cuda.synchronize()
    return out, p.state_interval


CASES = [(dim, L, dtype, z, sp)
         for dim in (32, 96, 160) for L in (8, 24, 32, 40, 72, 80, 136)
         for dtype in (torch.bfloat16, torch.float16) for z in (True, False) for sp in (True, False)]


@pytest.mark.parametrize("dim,L,dtype,z,sp", CASES,
                         ids=lambda v: str(v)[6:] if isinstance(v, torch.dtype) else str(v))
def test_scan_bwd_staged_rows(dim, L, dtype, z, sp, monkeypatch):
    from mamba_clip_amd import selective_scan_interface as ssi
    x, dout_cpu, ref = _case(dim, L, dtype, z, sp)
    for layout in ("dense", "cm"):
        dx = {k: (v.to(DEV) if v is not None else None) for k, v in x.items()}
        for k in ("u", "delta", "z"):
            if x[k] is not None:
                dx[k] = _rows(x[k], layout, True)
        for k in ("B", "C"):   # rows padded with NaN as well: a partial chunk reads past L
            big = torch.full((BATCH, 1, N, L + PAD), float("nan"), dtype=dtype)
            big[..., :L] = x[k]
            dx[k] = big.to(DEV)[..., :L]
        dout = _rows(dout_cpu, layout, True)
        for mb, interval in (("1024", 8), ("0", 0)):
            monkeypatch.setenv("MAMBA_CLIP_AMD_FINE_STATES_MB", mb)
            _, states, _ = ssi.scan_fwd(dx["u"], dx["delta"], dx["A"], dx["B"], dx["C"], dx["D"], dx["z"],
                                        dx["delta_bias"], sp, True, False)
            runs = [_run_bwd(dx, dout, states, sp, layout) for _ in range(2)]
            tag = f"{layout} interval {interval or 32}"
            if L > 8:   # at L = 8 the two state layouts coincide
                assert runs[0][1] == interval, tag
            got = runs[0][0]
            for k, g in got.items():
                g.check(f"{tag} d{k}")
                assert torch.equal(g.flat, runs[1][0][k].flat), f"{tag} d{k}: two runs differ"
                assert_grad_close(g.view, ref[k], g.view.dtype, f"{tag} d{k}")
