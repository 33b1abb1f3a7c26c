"""GPU parity of the fp8 similarity path (BASELINE config 5: stage-2 on frozen
features, fp8 MFMA similarity matmul).

The reference's similarity is ``logit_scale * I @ T^T`` in fp32/bf16
(model.py:1104-1112, loss.py:102-108); the fp8 route is build-defined, so it
is pinned in three layers against oracle/loss_ref.py:
  1. the quantiser is bit-exact with ``quant_rows_fp8_ref`` (torch's RNE
     float8_e4m3fn conversion of the same fp32 products);
  2. the fp8 MFMA GEMM matches the fp64 product of the dequantised operands
     within 2e-4 * max|ref|.  Integer data is reproduced exactly (test below),
     but v_mfma_f32_16x16x32_fp8_fp8 does not accumulate real-valued products
     as an exact fp32 sum: measured on MI355X, up to 1.6e-5 * max|ref| at
     K = 16 (bf16 / fp32 MFMA on the same data: ~1e-7) -- two orders below
     the e4m3 quantisation error of layer 3;
  3. against the reference's fp32 similarity the tolerance is the e4m3 bound
     written here: |logit err| <= 0.02 * logit_scale (cosine space 0.02; the
     3-bit mantissa gives <= 2^-4 relative error per operand); the
     contrastive loss within 2 * max|logit err| (CE is 1-Lipschitz in the
     sup-norm) and, for E >= 500, within 5e-3 relative.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle.loss_ref import clip_loss, quant_rows_fp8_ref, similarity_fp8_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("rows,cols,dtype", [(1, 16, torch.float32), (130, 512, torch.float32),
                                             (257, 40, torch.bfloat16), (64, 768, torch.float16),
                                             (8, 3, torch.float32)])
def test_quant_rows_fp8_bitexact(rows, cols, dtype):
    from mamba_clip_amd.ops import quant_rows_fp8
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    X = (torch.randn(rows, cols, generator=g) * torch.rand(rows, 1, generator=g) * 3).to(dtype)
    X[0, :] = 0                               # all-zero row: scale 1, zeros out
    q, inv = quant_rows_fp8(X.to(DEV))
    qr, invr = quant_rows_fp8_ref(X.float())
    assert q.shape == qr.shape and q.dtype == torch.float8_e4m3fn
    assert torch.equal(q.view(torch.uint8).cpu(), qr)
    assert torch.equal(inv.cpu(), invr)


def test_fp8_gemm_exact_integers_asymmetric():
    """Small integers are exact in e4m3: the product must be exact (catches a wrong lane map / transposed write)."""
    from mamba_clip_amd.ops import gemm_nt
    g = torch.Generator().manual_seed(1)
    for (M, N, K) in [(16, 16, 32), (128, 128, 64), (200, 130, 144), (64, 300, 512)]:
        A = torch.randint(-8, 9, (M, K), generator=g).float()
        B = torch.randint(-8, 9, (N, K), generator=g).float()
        B[:, 0] = torch.arange(N) % 9            # asymmetric
        ref = A.double() @ B.double().T
        C = gemm_nt(A.to(torch.float8_e4m3fn).to(DEV), B.to(torch.float8_e4m3fn).to(DEV)).cpu()
        assert torch.equal(C.double(), ref), (M, N, K)
    # identity against a non-symmetric B: C = B^T
    A = torch.eye(64)
    B = (torch.arange(64 * 64) % 17 - 8).float().reshape(64, 64)
    C = gemm_nt(A.to(torch.float8_e4m3fn).to(DEV), B.to(torch.float8_e4m3fn).to(DEV)).cpu()
    assert torch.equal(C, B.T.contiguous())


@pytest.mark.parametrize("M,N,K", [(256, 64, 64), (300, 200, 512), (1000, 520, 448), (64, 72, 128), (513, 1032, 320),
                                   (2048, 4096, 512), (130, 72, 192), (261, 136, 256), (70, 200, 384)])
def test_fp8_panel_kernel_exact_integers(M, N, K):
    """The register-panel fp8 kernel (K % 64, K <= 512, N % 8): exact on small integers in fp32 and bf16 output
    (|sums| <= 256 for bf16), ragged panels / n-ranges / K steps, row and column factors and a device alpha
    applied exactly (powers of two); the kernel asserted to be the panel kernel.  Every NKS = K / 64
    instance runs: 1, 2, 3 (130 x 72), 4 (261 x 136: a second, 5-row panel), 5, 6 (70 x 200), 7, 8."""
    from mamba_clip_amd import _lib, ops
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    B = torch.randint(-8, 9, (N, K), generator=g).float()
    B[:, 0] = torch.arange(N) % 9
    sa = 2.0 ** torch.randint(-3, 4, (M,), generator=g).float()
    sb = 2.0 ** torch.randint(-3, 4, (N,), generator=g).float()
    ref = 0.5 * sa[:, None].double() * sb[None, :].double() * (A.double() @ B.double().T)
    ops.GEMM_NT_RECORD = []
    try:
        C = ops.gemm_nt(A.to(torch.float8_e4m3fn).to(DEV), B.to(torch.float8_e4m3fn).to(DEV),
                        alpha_dev=torch.tensor(0.5, device=DEV), scale_a=sa.to(DEV), scale_b=sb.to(DEV)).cpu()
        assert ops.GEMM_NT_RECORD == [_lib.MC_GEMM_KERNEL_FP8_PANEL]
        assert torch.equal(C.double(), ref), (M, N, K)
        A3 = torch.randint(-1, 2, (M, K), generator=g).float()
        B3 = torch.randint(-1, 2, (N, K), generator=g).float()
        Kb = min(K, 256)
        A3[:, Kb:] = 0
        Cb = ops.gemm_nt(A3.to(torch.float8_e4m3fn).to(DEV), B3.to(torch.float8_e4m3fn).to(DEV),
                         out_dtype=torch.bfloat16).cpu()
        assert Cb.dtype == torch.bfloat16
        assert torch.equal(Cb.double(), A3.double() @ B3.double().T), (M, N, K)
    finally:
        ops.GEMM_NT_RECORD = None


@pytest.mark.parametrize("M,N,K", [(200, 130, 640), (64, 64, 640)])
def test_fp8_tile_kernel_exact_integers(M, N, K):
    """sim_fp8_kernel (K % 128 == 0, not panel-eligible: K > 512), fp32 and bf16 output: exact on small
    integers (|sums| <= 256 for bf16: products from {-1, 0, 1}, 256 columns of A live), ragged
    tiles, row and column factors and a device alpha applied exactly; the kernel asserted through
    GEMM_NT_RECORD.  N = 130 stores element-wise (ldc % 4 != 0), 64 x 64 is one live wave quadrant."""
    from mamba_clip_amd import _lib, ops
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randint(-8, 9, (M, K), generator=g).float()
    B = torch.randint(-8, 9, (N, K), generator=g).float()
    B[:, 0] = torch.arange(N) % 9            # asymmetric
    sa = 2.0 ** torch.randint(-3, 4, (M,), generator=g).float()
    sb = 2.0 ** torch.randint(-3, 4, (N,), generator=g).float()
    ref = 0.5 * sa[:, None].double() * sb[None, :].double() * (A.double() @ B.double().T)
    A3 = torch.randint(-1, 2, (M, K), generator=g).float()
    B3 = torch.randint(-1, 2, (N, K), generator=g).float()
    A3[:, torch.arange(K) % 5 >= 2] = 0       # 256 live products, spread over all five K steps
    ref3 = 2.0 * sa[:, None].double() * (A3.double() @ B3.double().T)
    assert int((A3 != 0).any(0).sum()) <= 256 and bool((A3[:, 512:] != 0).any())
    f8 = lambda t: t.to(torch.float8_e4m3fn).to(DEV)  # noqa: E731
    ops.GEMM_NT_RECORD = []
    try:
        C = ops.gemm_nt(f8(A), f8(B), alpha_dev=torch.tensor(0.5, device=DEV), scale_a=sa.to(DEV), scale_b=sb.to(DEV))
        Cb = ops.gemm_nt(f8(A3), f8(B3), alpha=2.0, out_dtype=torch.bfloat16, scale_a=sa.to(DEV))
        assert ops.GEMM_NT_RECORD == [_lib.MC_GEMM_KERNEL_FP8_TILE] * 2
    finally:
        ops.GEMM_NT_RECORD = None
    assert C.dtype == torch.float32 and torch.equal(C.cpu().double(), ref), (M, N, K)
    assert Cb.dtype == torch.bfloat16 and torch.equal(Cb.cpu().double(), ref3), (M, N, K)


def test_fp8_kernel_selection():
    """Shapes outside the panel kernel's range take the 16x16x128 tile kernel (K % 128) or the generic tiles."""
    from mamba_clip_amd import _lib, ops
    cases = [((64, 64, 64), _lib.MC_GEMM_KERNEL_FP8_PANEL), ((64, 60, 64), _lib.MC_GEMM_KERNEL_TILE),
             ((64, 64, 640), _lib.MC_GEMM_KERNEL_FP8_TILE), ((64, 64, 48), _lib.MC_GEMM_KERNEL_TILE),
             ((8192, 8192, 512), _lib.MC_GEMM_KERNEL_FP8_PANEL)]
    for (M, N, K), want in cases:
        A = torch.zeros(M, K, device=DEV).to(torch.float8_e4m3fn)
        B = torch.zeros(N, K, device=DEV).to(torch.float8_e4m3fn)
        ops.GEMM_NT_RECORD = []
        try:
            ops.gemm_nt(A, B)
            assert ops.GEMM_NT_RECORD == [want], ((M, N, K), ops.GEMM_NT_RECORD)
        finally:
            ops.GEMM_NT_RECORD = None


@pytest.mark.parametrize("n,E", [(8, 16), (256, 512), (1000, 512), (1024, 500)])
def test_similarity_fp8_matches_oracle_and_reference(n, E):
    from mamba_clip_amd.ops import similarity_fp8
    g = torch.Generator().manual_seed(n + E)
    I = F.normalize(torch.randn(n, E, generator=g), dim=-1)
    T = F.normalize(I + 0.5 * torch.randn(n, E, generator=g), dim=-1)
    scale = 100.0
    out = similarity_fp8(I.to(DEV), T.to(DEV), torch.tensor(scale, device=DEV)).cpu().double()
    exact = similarity_fp8_ref(I, T, scale)
    err = float((out - exact).abs().max() / exact.abs().max())
    print(f"fp8 GEMM vs fp64 dequantised product: max err / max|ref| = {err:.3e} (n={n}, E={E})")
    assert err <= 2e-4
    ref = scale * (I.double() @ T.double().T)
    assert (out - ref).abs().max() <= 0.02 * scale
    lab = torch.arange(n)
    l_ref = clip_loss(I.double(), T.double(), torch.tensor(scale, dtype=torch.float64))
    l_f8 = (F.cross_entropy(out, lab) + F.cross_entropy(out.T, lab)) / 2
    # CE is 1-Lipschitz in the sup-norm of its logits (both the lse and the target term)
    assert abs(float(l_f8) - float(l_ref)) <= 2 * float((out - ref).abs().max()) + 1e-9
    if E >= 500:                                              # CLIP-sized embeddings: loss within 5e-3 relative
        assert abs(float(l_f8) - float(l_ref)) <= 5e-3 * abs(float(l_ref))
    # bf16 output variant: same values within bf16 rounding
    outb = similarity_fp8(I.to(DEV), T.to(DEV), scale, out_dtype=torch.bfloat16).cpu().double()
    assert (outb - exact).abs().max() <= 2 ** -8 * exact.abs().max() + 1e-5


def test_similarity_fp8_c5_size_properties():
    """Config 5 size (gathered N = 1024 x 8 = 8192, E = 512): diagonal dominance and symmetry of a self-similarity."""
    from mamba_clip_amd.ops import similarity_fp8
    g = torch.Generator(device=DEV).manual_seed(5)
    I = F.normalize(torch.randn(8192, 512, device=DEV, generator=g), dim=-1)
    S = similarity_fp8(I, I, 100.0)
    assert S.shape == (8192, 8192) and torch.isfinite(S).all()
    # same operand, same quantisation: symmetric up to the MFMA's accumulation (A/B roles differ per element)
    assert (S - S.T).abs().max() <= 2e-4 * 100.0
    d = torch.diagonal(S)
    assert (d - 100.0).abs().max() <= 2.0                        # |q(x)|^2 ~ 1 within the fp8 bound
    assert torch.equal(S.argmax(dim=1).cpu(), torch.arange(8192))
    # bf16 logits (the same panel kernel, bf16 epilogue): the fp32 values rounded once
    Sb = similarity_fp8(I, I, torch.tensor(100.0, device=DEV), out_dtype=torch.bfloat16)
    assert Sb.dtype == torch.bfloat16 and Sb.shape == S.shape
    assert torch.equal(Sb, S.to(torch.bfloat16))


def test_clip_model_get_logits_fp8():
    from mamba_clip_amd.model import build_clip
    torch.manual_seed(0)
    m = build_clip("tiny-mamba-clip").to(DEV).eval()
    img = torch.randn(4, 3, 32, 32, device=DEV)
    txt = torch.randint(1, m.text.vocab_size, (4, m.text.context_length), device=DEV)
    with torch.no_grad():
        li, lt = m.get_logits(img, txt)
        fi, ft = m.get_logits(img, txt, precision="fp8")
    scale = float(m.logit_scale.exp())
    assert (fi - li).abs().max() <= 0.02 * scale
    torch.testing.assert_close(ft, fi.T)


@pytest.mark.parametrize("n,E", [(256, 512), (8192, 512)])
def test_clip_loss_fp8_fused_matches_oracle(n, E):
    """Fused fp8 logits + CE (no logits in memory) vs fp64 CE over the exact dequantised product
    (similarity_fp8_ref), and within the fp8 bound of the fp64 loss on the unquantised features."""
    from mamba_clip_amd.ops import clip_loss_fp8
    g = torch.Generator().manual_seed(n)
    I = F.normalize(torch.randn(n, E, generator=g), dim=-1)
    T = F.normalize(I + 0.5 * torch.randn(n, E, generator=g), dim=-1)
    scale = 50.0
    got = float(clip_loss_fp8(I.to(DEV), T.to(DEV), torch.tensor(scale, device=DEV)))
    S = similarity_fp8_ref(I, T, scale)
    lab = torch.arange(n)
    want = float((F.cross_entropy(S, lab) + F.cross_entropy(S.T, lab)) / 2)
    assert abs(got - want) <= 1e-5 * abs(want) + 1e-6, (got, want)
    l_ref = float(clip_loss(I.double(), T.double(), torch.tensor(scale, dtype=torch.float64)))
    assert abs(got - l_ref) <= 5e-3 * abs(l_ref)
