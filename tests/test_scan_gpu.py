"""GPU parity of the HIP selective scan against the oracle and the golden
vectors executed from the reference text.  Run on an MI355X: pytest -m gpu."""
import glob
import os

import pytest
import torch

from conftest import GOLDEN, golden_meta, load_golden
from oracle.scan_ref import selective_scan_ref, selective_scan_ref_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCAN_FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "scan_*.safetensors")))

# Tolerances (written here, per north_star: float within 1e-3 rel on bf16 logits/loss):
#   fp32 I/O : |gpu - ref| <= 2e-5 * max|ref| + 1e-4 * |ref|   (fp32 rounding, different op order, exp2 path)
#   16-bit out: one output-dtype ulp of rounding: 2^-8 relative (bf16) / 2^-11 (f16) + the fp32 term.
REL = {torch.float32: 1e-4, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -10}


def assert_scan_close(got, ref, dtype, what="out"):
    got = got.float().cpu()
    ref = ref.float().cpu()
    scale = float(ref.abs().max().clamp_min(1.0))
    tol = 2e-5 * scale + REL[dtype] * ref.abs()
    bad = (got - ref).abs() > tol
    assert not bad.any(), (f"{what}: {int(bad.sum())}/{bad.numel()} mismatches, "
                           f"max abs err {float((got - ref).abs().max()):.3e}")


def _lib_fn():
    from mamba_clip_amd.selective_scan_interface import selective_scan_fn
    return selective_scan_fn


@pytest.mark.parametrize("fname", SCAN_FILES)
def test_scan_fwd_matches_reference_golden(fname):
    selective_scan_fn = _lib_fn()
    g = load_golden(fname)
    meta = golden_meta(fname)
    sp, last = meta["softplus"] == "1", meta["last"] == "1"
    x = {k[3:]: v.to(DEV) for k, v in g.items() if k.startswith("in.")}
    res = selective_scan_fn(**x, delta_softplus=sp, return_last_state=last)
    out, ls = res if last else (res, None)
    assert out.dtype == g["out"].dtype and out.shape == g["out"].shape
    # vs the reference's fp32 pre-cast output
    assert_scan_close(out, g["out_f32"], out.dtype)
    if last:
        assert_scan_close(ls, g["last_state"], torch.float32, "last_state")


def _rand_case(batch, dim, L, N, G, itype, wtype, z=True, D=True, bias=True, seed=0, three_d=False):
    gen = torch.Generator().manual_seed(seed)
    u = torch.randn(batch, dim, L, generator=gen).to(itype)
    delta = (0.5 * torch.randn(batch, dim, L, generator=gen)).to(itype)
    A = -torch.exp(torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(dim, 1)
                   + 0.1 * torch.randn(dim, N, generator=gen))
    shp = (batch, N, L) if three_d else (batch, G, N, L)
    Bm = torch.randn(*shp, generator=gen).to(wtype)
    Cm = torch.randn(*shp, generator=gen).to(wtype)
    Dv = torch.randn(dim, generator=gen) if D else None
    zv = torch.randn(batch, dim, L, generator=gen).to(itype) if z else None
    bv = (torch.rand(dim, generator=gen) * 4 - 5) if bias else None
    return dict(u=u, delta=delta, A=A, B=Bm, C=Cm, D=Dv, z=zv, delta_bias=bv)


CASES = [
    # batch, dim, L, N, G, itype, wtype, z, three_d
    (2, 256, 64, 16, 1, torch.bfloat16, torch.bfloat16, True, False),      # aligned, full chunks
    (2, 512, 77, 16, 1, torch.bfloat16, torch.bfloat16, True, True),       # C2-like ragged L, 3-D B/C
    (1, 320, 100, 16, 2, torch.float32, torch.float32, False, False),      # ragged rows (H=160)
    (2, 128, 33, 8, 4, torch.float16, torch.float32, True, False),         # f16 / fp32 B,C, N=8
    (1, 64, 250, 32, 1, torch.float32, torch.bfloat16, True, False),       # N=32
    (3, 96, 5, 3, 3, torch.bfloat16, torch.float32, False, False),         # odd N, tiny L
    # 16-B aligned 16-bit rows take the backward's paired-tile path; odd tile counts
    # add one fully masked tile past L
    (2, 192, 40, 16, 1, torch.bfloat16, torch.bfloat16, True, False),      # 5 tiles (odd)
    (2, 128, 24, 16, 2, torch.float16, torch.bfloat16, False, False),      # 3 tiles, no z, G=2
    # long sequences take the state-split pair kernel (scan_fwd_pair.hip): ragged 32-channel blocks
    (2, 96, 1024, 16, 2, torch.bfloat16, torch.bfloat16, True, False),     # H=48: a full + a half block
    (1, 80, 544, 16, 1, torch.float16, torch.float32, False, False),       # 17 chunks, no z, H=80
    (2, 64, 1000, 16, 1, torch.bfloat16, torch.bfloat16, True, False),     # last chunk runs past L (masked)
    # L > 512 with fp32 B/C (the pair kernel declines): the LDS-staged one-channel kernel's other row modes
    # (L = 544 above is its whole-chunk mode)
    (1, 64, 520, 16, 1, torch.float16, torch.float32, True, False),        # aligned rows, ragged last chunk
    (1, 64, 515, 16, 1, torch.float16, torch.float32, True, False),        # element-wise rows
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"b{c[0]}d{c[1]}L{c[2]}N{c[3]}G{c[4]}{str(c[5])[6:]}")
def test_scan_fwd_random_vs_oracle(case):
    selective_scan_fn = _lib_fn()
    batch, dim, L, N, G, it, wt, z, three_d = case
    x = _rand_case(batch, dim, L, N, G, it, wt, z=z, three_d=three_d, seed=batch * 7 + dim)
    ref, ref_last = selective_scan_ref(**{k: v for k, v in x.items()}, delta_softplus=True,
                                       return_last_state=True, compute_dtype=torch.float64)
    # compare in fp64 with the pre-cast output: recompute without the cast
    ref32 = selective_scan_ref(**{k: (v.double() if v is not None and v.is_floating_point() else v)
                                  for k, v in x.items()}, delta_softplus=True, compute_dtype=torch.float64)
    out, last = selective_scan_fn(**{k: (v.to(DEV) if v is not None else None) for k, v in x.items()},
                                  delta_softplus=True, return_last_state=True)
    assert_scan_close(out, ref32, it)
    assert_scan_close(last, ref_last, torch.float32, "last_state")


def test_scan_fwd_strided_views_and_nosoftplus():
    """Non-contiguous batch/dim strides (L padded to 80) and softplus off."""
    selective_scan_fn = _lib_fn()
    x = _rand_case(2, 256, 77, 16, 1, torch.bfloat16, torch.bfloat16, seed=5)
    big = torch.zeros(2, 256, 80, dtype=torch.bfloat16)
    big[:, :, :77] = x["u"]
    u_view = big.to(DEV)[:, :, :77]
    assert u_view.stride(1) == 80
    out = selective_scan_fn(u_view, x["delta"].to(DEV), x["A"].to(DEV), x["B"].to(DEV), x["C"].to(DEV),
                            x["D"].to(DEV), x["z"].to(DEV), x["delta_bias"].to(DEV), delta_softplus=False)
    xx = dict(x)
    ref = selective_scan_ref(**{k: (v.double() if v is not None else None) for k, v in xx.items()},
                             delta_softplus=False, compute_dtype=torch.float64)
    assert_scan_close(out, ref, torch.bfloat16)


def test_scan_fwd_full_size_properties():
    """C4 shape (B=64, D=3072, L=4096, N=16, bf16, z): batch-slice determinism
    (bit-exact) and a sampled-channel check against the fp64 oracle."""
    selective_scan_fn = _lib_fn()
    torch.manual_seed(0)
    Bsz, D, L, N = 64, 3072, 4096, 16
    u = torch.randn(Bsz, D, L, device=DEV, dtype=torch.bfloat16)
    dt = (0.5 * torch.randn(Bsz, D, L, device=DEV)).to(torch.bfloat16)
    z = torch.randn(Bsz, D, L, device=DEV, dtype=torch.bfloat16)
    A = -torch.exp(torch.log(torch.arange(1, N + 1, dtype=torch.float32, device=DEV)).repeat(D, 1)
                   + 0.1 * torch.randn(D, N, device=DEV))
    Bm = torch.randn(Bsz, 1, N, L, device=DEV, dtype=torch.bfloat16)
    Cm = torch.randn(Bsz, 1, N, L, device=DEV, dtype=torch.bfloat16)
    Dv = torch.ones(D, device=DEV)
    bias = torch.rand(D, device=DEV) * 4 - 5
    out = selective_scan_fn(u, dt, A, Bm, Cm, Dv, z, bias, delta_softplus=True)
    # batch independence / determinism: re-run batch 5 alone, must be bit-identical
    b = 5
    out_b = selective_scan_fn(u[b:b + 1], dt[b:b + 1], A, Bm[b:b + 1], Cm[b:b + 1], Dv, z[b:b + 1], bias,
                              delta_softplus=True)
    assert torch.equal(out_b[0], out[b])
    # sampled channels vs fp64 oracle (channels 0..63 and 3008..3071 of batch 5)
    for d0 in (0, 3008):
        sl = slice(d0, d0 + 64)
        ref = selective_scan_ref(u[b:b + 1, sl].double().cpu(), dt[b:b + 1, sl].double().cpu(),
                                 A[sl].double().cpu(), Bm[b:b + 1].double().cpu(), Cm[b:b + 1].double().cpu(),
                                 Dv[sl].double().cpu(), z[b:b + 1, sl].double().cpu(), bias[sl].double().cpu(),
                                 delta_softplus=True, compute_dtype=torch.float64)
        assert_scan_close(out[b:b + 1, sl], ref, torch.bfloat16)


def test_scan_fwd_empty_and_errors():
    selective_scan_fn = _lib_fn()
    A = -torch.ones(64, 16, device=DEV)
    u = torch.randn(0, 64, 10, device=DEV)
    Bm = torch.randn(0, 1, 16, 10, device=DEV)
    assert selective_scan_fn(u, u, A, Bm, Bm).shape == (0, 64, 10)
    u = torch.randn(1, 64, 10, device=DEV)
    with pytest.raises(RuntimeError):
        selective_scan_fn(u, u, A, torch.randn(1, 3, 16, 10, device=DEV), torch.randn(1, 3, 16, 10, device=DEV))
    with pytest.raises(RuntimeError):
        B1 = torch.randn(1, 1, 16, 10, device=DEV)
        selective_scan_fn(u, u.half(), A, B1, B1)
    # dstate above MC_SCAN_MAX_DSTATE (32) is rejected, not run on a slow path
    with pytest.raises(RuntimeError):
        B64 = torch.randn(1, 1, 64, 10, device=DEV)
        selective_scan_fn(u, u, -torch.ones(64, 64, device=DEV), B64, B64)


# ----------------------------------------------------------------- backward
GRAD_REL = {torch.float32: 2e-4, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -9}


def assert_grad_close(got, ref, dtype, what):
    got = got.float().cpu()
    ref = ref.float().cpu()
    scale = float(ref.abs().max().clamp_min(1e-6))
    tol = 2e-4 * scale + GRAD_REL[dtype] * ref.abs()
    err = (got - ref).abs()
    bad = err > tol
    assert not bad.any(), (f"grad {what}: {int(bad.sum())}/{bad.numel()} mismatches, max abs err "
                           f"{float(err.max()):.3e} (scale {scale:.3e})")


def _check_backward(x, sp, dout, itype):
    selective_scan_fn = _lib_fn()
    leaves = {k: (v.to(DEV).detach().requires_grad_(True) if v is not None else None) for k, v in x.items()}
    out = selective_scan_fn(**leaves, delta_softplus=sp)
    out.backward(dout.to(DEV).to(out.dtype))
    ref = selective_scan_ref_grads(**{k: v for k, v in x.items()}, delta_softplus=sp,
                                   dout=dout.to(itype).double(), compute_dtype=torch.float64)
    for k, g in ref.items():
        got = leaves[k].grad
        assert got is not None, k
        # bf16 outputs of du / ddelta / dz / dB / dC are rounded once: compare at the output dtype's ulp
        dt = leaves[k].dtype
        assert_grad_close(got, g, dt if dt != torch.float32 else torch.float32, k)


@pytest.mark.parametrize("fname", SCAN_FILES)
def test_scan_bwd_matches_reference_golden(fname):
    g = load_golden(fname)
    sp = golden_meta(fname)["softplus"] == "1"
    x = {k[3:]: v for k, v in g.items() if k.startswith("in.")}
    _check_backward(x, sp, g["dout"], x["u"].dtype)
    # and against the reference text's own fp32 gradients (fp32-input cases)
    if x["u"].dtype == torch.float32:
        selective_scan_fn = _lib_fn()
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in x.items()}
        selective_scan_fn(**leaves, delta_softplus=sp).backward(g["dout"].to(DEV))
        for k, v in leaves.items():
            assert_grad_close(v.grad, g[f"grad.{k}"], v.grad.dtype, "golden " + k)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"b{c[0]}d{c[1]}L{c[2]}N{c[3]}G{c[4]}{str(c[5])[6:]}")
def test_scan_bwd_random_vs_oracle(case):
    batch, dim, L, N, G, it, wt, z, three_d = case
    x = _rand_case(batch, dim, L, N, G, it, wt, z=z, three_d=three_d, seed=batch * 11 + dim)
    dout = torch.randn(batch, dim, L, generator=torch.Generator().manual_seed(3))
    _check_backward(x, True, dout, it)


@pytest.mark.parametrize("L", [35, 41])
def test_scan_bwd_ragged_aligned_rows(L):
    """Inputs are views into rows padded to 48 (16-B aligned) with a ragged L
    (L=35: 5 tiles, L=41: 6 tiles).  The gradients are allocated dense, so
    their rows are not 16-B aligned and the backward takes its element-wise
    path.  Gradients reach the padded leaves through the views, and the
    padding stays untouched."""
    selective_scan_fn = _lib_fn()
    x = _rand_case(2, 192, L, 16, 1, torch.bfloat16, torch.bfloat16, seed=L)
    pads = {}
    for k in ("u", "delta", "z"):
        big = torch.zeros(2, 192, 48, dtype=torch.bfloat16)
        big[:, :, :L] = x[k]
        pads[k] = big.to(DEV).requires_grad_(True)
    leaves = {k: (v.to(DEV).detach().requires_grad_(True) if v is not None else None)
              for k, v in x.items() if k not in pads}
    views = {k: pads[k][:, :, :L] for k in pads}
    assert views["u"].stride(1) == 48
    dout = torch.randn(2, 192, L, generator=torch.Generator().manual_seed(4))
    out = selective_scan_fn(**views, **leaves, delta_softplus=True)
    out.backward(dout.to(DEV).to(out.dtype))
    ref = selective_scan_ref_grads(**x, delta_softplus=True, dout=dout.to(torch.bfloat16).double(),
                                   compute_dtype=torch.float64)
    for k, g in ref.items():
        got = pads[k].grad[:, :, :L] if k in pads else leaves[k].grad
        assert_grad_close(got, g, torch.bfloat16 if k in ("u", "delta", "z", "B", "C") else torch.float32, k)
    for k in pads:
        assert torch.count_nonzero(pads[k].grad[:, :, L:]) == 0, k


def test_scan_bwd_deterministic():
    """Slab reductions (no atomics): two backward passes are bit-identical."""
    selective_scan_fn = _lib_fn()
    x = _rand_case(4, 512, 200, 16, 1, torch.bfloat16, torch.bfloat16, seed=9)
    grads = []
    for _ in range(2):
        leaves = {k: v.to(DEV).requires_grad_(True) for k, v in x.items()}
        selective_scan_fn(**leaves, delta_softplus=True).backward(torch.ones(4, 512, 200, device=DEV, dtype=torch.bfloat16))
        grads.append({k: v.grad.clone() for k, v in leaves.items()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


# ----------------------------------------------------------------- grouped directions (SS2D cross-scan)
@pytest.mark.parametrize("Bsz,d,L,rev,ug,dt", [(2, 64, 35, 0b1100, 2, torch.float32),
                                               (1, 96, 256, 0b1100, 2, torch.float32),
                                               (2, 40, 36, 0b1010, 1, torch.bfloat16),
                                               (1, 128, 784, 0b0110, 4, torch.float32),
                                               (2, 64, 49, 0b1111, 2, torch.float16)])
def test_grouped_scan_matches_explicit_flips(Bsz, d, L, rev, ug, dt):
    """Mirrored addressing of reversed groups and shared u blocks inside the kernels vs the
    reference's explicit stack / flip / flip-back around a plain scan (oracle.cpu_model.grouped_scan_ref,
    fp64 autograd): outputs and every gradient.  L = 35 / 49 leave the mirrored 16-B blocks unaligned."""
    from mamba_clip_amd.selective_scan_interface import grouped_scan_fn
    from oracle.cpu_model import grouped_scan_ref
    N, G = 16, 4
    g = torch.Generator().manual_seed(L * 10 + d)
    u = torch.randn(Bsz, ug * d, L, generator=g).to(dt)
    delta = (0.5 * torch.randn(Bsz, G * d, L, generator=g)).to(dt)
    A = -torch.exp(torch.log(torch.arange(1, N + 1, dtype=torch.float32)).repeat(G * d, 1)
                   + 0.1 * torch.randn(G * d, N, generator=g))
    Bm = torch.randn(Bsz, G, N, L, generator=g)
    Cm = torch.randn(Bsz, G, N, L, generator=g)
    Dv = torch.randn(G * d, generator=g)
    bias = torch.rand(G * d, generator=g) * 4 - 5
    dout = torch.randn(Bsz, G * d, L, generator=g)
    ins = dict(u=u, delta=delta, A=A, B=Bm, C=Cm, D=Dv, delta_bias=bias)
    ref_in = {k: v.double().requires_grad_(True) for k, v in ins.items()}
    ref = grouped_scan_ref(**ref_in, delta_softplus=True, reverse_groups=rev, u_groups=ug)
    ref.backward(dout.to(dt).double())
    dev_in = {k: v.to(DEV).requires_grad_(True) for k, v in ins.items()}
    out = grouped_scan_fn(**dev_in, delta_softplus=True, reverse_groups=rev, u_groups=ug)
    assert out.shape == (Bsz, G * d, L) and out.dtype == dt
    assert_scan_close(out, ref.detach(), dt)
    out.backward(dout.to(DEV).to(dt))
    for k in ins:
        if k == "u" and dt != torch.float32 and ug < G:
            # du of a shared block = sum of G / ug groups' parts, each rounded once to the I/O dtype
            err = (dev_in[k].grad.float().cpu() - ref_in[k].grad.float()).abs()
            lim = (G // ug) * GRAD_REL[dt] * float(ref_in[k].grad.abs().max())
            assert float(err.max()) <= lim, (float(err.max()), lim)
            continue
        assert_grad_close(dev_in[k].grad, ref_in[k].grad, dev_in[k].dtype, k)


def test_grouped_scan_rejects_bad_configs():
    from mamba_clip_amd.selective_scan_interface import grouped_scan_fn
    A = -torch.ones(32, 16, device=DEV)
    Bm = torch.randn(1, 4, 16, 12, device=DEV)
    with pytest.raises(RuntimeError):   # u has the wrong number of shared blocks
        grouped_scan_fn(torch.randn(1, 24, 12, device=DEV), torch.randn(1, 32, 12, device=DEV), A, Bm, Bm,
                        reverse_groups=0b1100, u_groups=2)
    with pytest.raises(RuntimeError):   # mask beyond n_groups
        grouped_scan_fn(torch.randn(1, 16, 12, device=DEV), torch.randn(1, 32, 12, device=DEV), A, Bm, Bm,
                        reverse_groups=0b110000, u_groups=2)


def test_scan_fwd_pair_masked_chunk_ignores_nan_padding():
    """Pair kernel, L % 32 != 0: the last chunk reads u / delta past L (the row stride padding).
    Those positions are masked (dt = du = 0), so NaN / Inf in the padding cannot reach the state:
    out and last_state equal the result with zero padding (and the fp64 oracle)."""
    selective_scan_fn = _lib_fn()
    x = _rand_case(2, 64, 1000, 16, 1, torch.bfloat16, torch.bfloat16, seed=17)
    views = {}
    for k in ("u", "delta", "z"):
        big = torch.full((2, 64, 1024), float("nan"), dtype=torch.bfloat16)
        big[:, :, 1000:1008] = float("inf")
        big[:, :, :1000] = x[k]
        views[k] = big.to(DEV)[:, :, :1000]
        assert views[k].stride(1) == 1024
    rest = {k: v.to(DEV) for k, v in x.items() if k not in views}
    out, last = selective_scan_fn(**views, **rest, delta_softplus=True, return_last_state=True)
    dense = {k: v.to(DEV) for k, v in x.items()}
    out0, last0 = selective_scan_fn(**dense, delta_softplus=True, return_last_state=True)
    assert torch.isfinite(last).all() and torch.isfinite(out).all()
    assert torch.equal(out, out0) and torch.equal(last, last0)
    _, ref_last = selective_scan_ref(**x, delta_softplus=True, return_last_state=True, compute_dtype=torch.float64)
    assert_scan_close(last, ref_last, torch.float32, "last_state")


# ----------------------------------------------------------------- saved-state interval
@pytest.mark.parametrize("case", [(2, 256, 64, torch.bfloat16, True), (2, 96, 1000, torch.bfloat16, True),
                                  (1, 80, 544, torch.float16, False), (3, 128, 8, torch.bfloat16, True),
                                  (2, 192, 80, torch.bfloat16, True)])
def test_scan_bwd_fine_state_interval(case, monkeypatch):
    """The training forward saves the state every 8 positions where the pair kernel runs (the backward
    reads its sub-tiles' entry states instead of recomputing them, include/mc_scan.h state_interval):
    gradients vs the fp64 oracle at both intervals, and the two intervals within fp32 rounding of
    each other (the forward's and the backward's recurrences round the same terms)."""
    from mamba_clip_amd import selective_scan_interface as ssi
    batch, dim, L, it, z = case
    x = _rand_case(batch, dim, L, 16, 1, it, it, z=z, seed=L + dim)
    dout = torch.randn(batch, dim, L, generator=torch.Generator().manual_seed(8))
    grads = {}
    for mb in ("1024", "0"):
        monkeypatch.setenv("MAMBA_CLIP_AMD_FINE_STATES_MB", mb)
        dx = {k: (v.to(DEV) if v is not None else None) for k, v in x.items()}
        out, states, _ = ssi.scan_fwd(dx["u"], dx["delta"], dx["A"], dx["B"], dx["C"], dx["D"], dx["z"],
                                      dx["delta_bias"], True, True, False)
        fine = mb != "0"
        assert states.shape == ((batch, -(-L // 8), dim, 16) if fine else (batch, dim, -(-L // 32), 16))
        if fine and L > 8:
            assert ssi.states_interval(L, dim, states) == 8
        _check_backward(x, True, dout, it)
        g = ssi.scan_bwd(dx["u"], dx["delta"], dx["A"], dx["B"], dx["C"], dx["D"], dx["z"], dx["delta_bias"],
                         True, dout.to(DEV).to(it), states)
        grads[mb] = [t.float() if t is not None else None for t in g]
    for a, b in zip(grads["1024"], grads["0"]):
        if a is not None:
            assert float((a - b).abs().max()) <= 2e-2 * float(b.abs().max()) + 1e-6


def test_scan_bwd_generic_kernel_reads_fine_states():
    """Fine states from the pair forward, backward on the element-wise kernel (dout rows not 16-B
    aligned): it picks every fourth saved state.  Gradients vs the fp64 oracle."""
    from mamba_clip_amd import selective_scan_interface as ssi
    batch, dim, L = 2, 128, 96
    x = _rand_case(batch, dim, L, 16, 1, torch.bfloat16, torch.bfloat16, z=True, seed=21)
    dx = {k: (v.to(DEV) if v is not None else None) for k, v in x.items()}
    out, states, _ = ssi.scan_fwd(dx["u"], dx["delta"], dx["A"], dx["B"], dx["C"], dx["D"], dx["z"],
                                  dx["delta_bias"], True, True, False)
    assert states.shape == (batch, L // 8, dim, 16)
    dout = torch.randn(batch, dim, L, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    big = torch.zeros(batch, dim, L + 1, dtype=torch.bfloat16, device=DEV)
    big[:, :, 1:] = dout.to(DEV)
    dview = big[:, :, 1:]                      # rows start 2 B past a 16-B boundary
    du, ddelta, dA, dB, dC, dD, dz, dbias = ssi.scan_bwd(dx["u"], dx["delta"], dx["A"], dx["B"], dx["C"], dx["D"],
                                                         dx["z"], dx["delta_bias"], True, dview, states)
    ref = selective_scan_ref_grads(**x, delta_softplus=True, dout=dout.double(), compute_dtype=torch.float64)
    got = dict(u=du, delta=ddelta, A=dA, B=dB, C=dC, D=dD, z=dz, delta_bias=dbias)
    for k, g in ref.items():
        assert_grad_close(got[k], g, torch.bfloat16 if k in ("u", "delta", "z", "B", "C") else torch.float32, k)


# ----------------------------------------------------------------- the shipped pair kernels vs the reference text
PAIR_FILES = [f for f in SCAN_FILES if f.startswith("scan_pair_")]


@pytest.mark.parametrize("fine_mb", ["1024", "0"], ids=["fine_states", "chunk_states"])
@pytest.mark.parametrize("fname", PAIR_FILES)
def test_pair_kernels_match_reference_text_golden(fname, fine_mb, monkeypatch):
    """golden vectors executed from the reference's own text (model.py:83-169)
    at the lane-pair kernels' shapes (16-bit rows, N = 16, L % 8 == 0, incl. C2's padded L = 80).
    Asserts that the pair kernels are the ones dispatched (mc_scan_fwd_kernel / mc_scan_bwd_kernel),
    at both saved-state intervals, and compares output, last state and every gradient directly with
    the reference text's fp32 values (16-bit outputs within one ulp of their dtype + 2e-4 of max)."""
    from mamba_clip_amd import _lib
    from mamba_clip_amd import selective_scan_interface as ssi
    monkeypatch.setenv("MAMBA_CLIP_AMD_FINE_STATES_MB", fine_mb)
    monkeypatch.setattr(ssi, "RECORD_DISPATCH", True)
    monkeypatch.setattr(ssi, "DISPATCH", [])
    g = load_golden(fname)
    meta = golden_meta(fname)
    sp, last = meta["softplus"] == "1", meta["last"] == "1"
    leaves = {k[3:]: v.to(DEV).requires_grad_(True) for k, v in g.items() if k.startswith("in.")}
    res = ssi.selective_scan_fn(**leaves, delta_softplus=sp, return_last_state=last)
    out, ls = res if last else (res, None)
    assert_scan_close(out, g["out_f32"], out.dtype)
    if last:
        assert_scan_close(ls, g["last_state"], torch.float32, "last_state")
    out.backward(g["dout"].to(DEV).to(out.dtype))
    assert ssi.DISPATCH == [("fwd", _lib.MC_SCAN_KERNEL_PAIR), ("bwd", _lib.MC_SCAN_KERNEL_PAIR)], ssi.DISPATCH
    for k, v in leaves.items():
        ref = g[f"grad.{k}"]
        dt = v.grad.dtype
        assert v.grad.shape == ref.shape, k
        # the reference's gradient used dout in fp32, ours the 16-bit-rounded dout: that rounding
        # is inside the dtype's ulp term
        assert_grad_close(v.grad, ref, dt, "reference-text " + k)
