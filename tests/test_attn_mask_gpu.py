"""GPU checks of the key-masked fused attention (mc_attn_masked_fwd / _bwd, ops.PackedMaskedAttentionFn,
model.Attention with a padding mask) against an fp64 restatement of
softmax(q k^T / sqrt(D) + (valid ? 0 : -inf)) v on the same 16-bit inputs -- HF BertModel's
attention_mask[:, None, None, :]: one key mask per batch row, every query row computed.

Metric and limits are test_attn_gpu.py's: normalised error ||got - ref|| / ||ref|| <= 8e-3 for o,
<= 2e-2 for dq / dk / dv (the kernel rounds P and dS to the input dtype), lse to 1e-5.  On top: dk and
dv of masked keys are exact zeros, a full mask reproduces the unmasked kernels bit for bit, and two
runs agree bit for bit (no atomics)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64


def _ref(q, k, v, scale, valid):
    """fp64 masked attention + lse over the valid keys; q, k, v (B, N, H, D), valid (B, N) bool."""
    qd, kd, vd = (t.double() for t in (q, k, v))
    s = torch.einsum("bnhd,bmhd->bhnm", qd, kd) * scale
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.einsum("bhnm,bmhd->bnhd", torch.softmax(s, -1), vd)
    return o, lse


def _nerr(a, b, floor=1e-30):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(floor)).item()


def _packed(B, N, H, dt, g):
    return (torch.randn(B, N, 3 * H * D, generator=g) * 1.5).to(dt).to(DEV)


def _patterns(N, g):
    """Every mask pattern that exists at this length, as (name, (N,) bool); key 0 (CLS) is valid in
    all but the hole-over-tile-0 pattern of N <= 64."""
    def upto(n):
        m = torch.zeros(N, dtype=torch.bool)
        m[:n] = True
        return m
    pats = [("full", upto(N)), ("cut1", upto(1))]
    for edge in (32, 33, 64):                       # suffix cut at a tile edge
        if edge < N:
            pats.append((f"cut{edge}", upto(edge)))
    mid = {7: 3, 40: 20, 64: 50, 197: 100, 256: 150}.get(N, max(1, N // 2))
    pats.append((f"cut{mid}", upto(mid)))           # mid-tile; for N > 64 with wholly empty trailing tiles
    if N > 96:                                      # trailing tiles wholly empty behind a partial one
        pats.append(("cut70", upto(70)))
    hole = upto(N)                                  # a whole tile masked, valid keys after it
    if N > 64:
        hole[32:64] = False
    elif N > 32:
        hole[:32] = False
    else:
        hole[1:N - 1] = False
    pats.append(("hole", hole))
    sc = torch.rand(N, generator=g) < 0.5           # scattered bits
    sc[0] = True
    pats.append(("scattered", sc))
    return pats


def _mask_batches(N, B, g):
    """The patterns in batches of B rows (the last one filled up from the front)."""
    pats = _patterns(N, g)
    pats += pats[: -len(pats) % B]
    return [torch.stack([m for _, m in pats[i:i + B]]) for i in range(0, len(pats), B)]


def _run(qkv, H, valid, go):
    from mamba_clip_amd.ops import pack_key_mask, packed_attention
    x = qkv.detach().clone().requires_grad_(True)
    o = packed_attention(x, H, pack_key_mask(valid))
    o.backward(go)
    return o.detach(), x.grad


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N", [7, 40, 64, 197, 256])
def test_masked_attention_fwd_bwd_vs_fp64(N, dt):
    g = torch.Generator().manual_seed(100 + N)
    B, H = 4, 3
    C = H * D
    for valid_cpu in _mask_batches(N, B, g):
        valid = valid_cpu.to(DEV)
        qkv = _packed(B, N, H, dt, g)
        go = torch.randn(B, N, C, generator=g).to(dt).to(DEV)
        o, grad = _run(qkv, H, valid, go)
        ref_in = qkv.double().requires_grad_(True)
        q, k, v = ref_in.view(B, N, 3, H, D).unbind(2)
        ro, _ = _ref(q, k, v, D ** -0.5, valid)
        ro.reshape(B, N, C).backward(go.double())
        assert o.shape == (B, N, C) and o.dtype == dt
        e = _nerr(o, ro.reshape(B, N, C))
        print(f"N {N} {dt} o {e:.3e}")
        assert e < 8e-3
        dq, dk, dv = grad.view(B, N, 3, H, D).unbind(2)
        rq, rk, rv = ref_in.grad.view(B, N, 3, H, D).unbind(2)
        floor = 1e-3 * ref_in.grad.norm().item()
        for name, a, b in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
            e = _nerr(a, b, floor)
            print(f"N {N} {dt} {name} {e:.3e}")
            assert e < 2e-2, name
        # every row on its own as well (a wrong mask word of one batch row shows there)
        for b in range(B):
            assert _nerr(o[b], ro.reshape(B, N, C)[b]) < 8e-3, b
        # masked keys: dk, dv stored as exact zeros (the packed gradient is allocated uninitialised)
        dead = ~valid
        assert dk[dead].eq(0).all() and dv[dead].eq(0).all()
        assert torch.isfinite(grad).all()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("N", [7, 40, 64, 197, 256])
def test_full_mask_equals_unmasked_bitwise(N, dt):
    from mamba_clip_amd.ops import packed_attention
    g = torch.Generator().manual_seed(200 + N)
    B, H = 4, 3
    qkv = _packed(B, N, H, dt, g)
    go = torch.randn(B, N, H * D, generator=g).to(dt).to(DEV)
    o, grad = _run(qkv, H, torch.ones(B, N, dtype=torch.bool, device=DEV), go)
    x = qkv.detach().clone().requires_grad_(True)
    ou = packed_attention(x, H)
    ou.backward(go)
    assert torch.equal(o, ou.detach()) and torch.equal(grad, x.grad)


def test_masked_attention_lse_and_determinism():
    from mamba_clip_amd import _lib
    from mamba_clip_amd.ops import pack_key_mask
    g = torch.Generator().manual_seed(7)
    B, N, H = 6, 197, 12
    lengths = [197, 1, 32, 33, 100, 161]
    valid = (torch.arange(N)[None, :] < torch.tensor(lengths)[:, None])
    valid[4, 32:64] = False                                   # a hole over a whole tile
    valid = valid.to(DEV)
    qkv = _packed(B, N, H, torch.bfloat16, g)
    go = torch.randn(B, N, H * D, generator=g).to(torch.bfloat16).to(DEV)
    o1, g1 = _run(qkv, H, valid, go)
    o2, g2 = _run(qkv, H, valid, go)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)        # no atomics: bitwise reproducible
    # lse straight from the C ABI
    lib = _lib.load()
    words = pack_key_mask(valid)
    o = torch.empty(B, N, H * D, device=DEV, dtype=qkv.dtype)
    lse = torch.empty(B, H, N, device=DEV)
    p = _lib.AttnMaskedFwdParams()
    p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = B, H, N, D, _lib.MC_DTYPE_BF16, 0.125
    es = qkv.element_size()
    p.q, p.k, p.v = qkv.data_ptr(), qkv.data_ptr() + H * D * es, qkv.data_ptr() + 2 * H * D * es
    p.q_bs, p.q_ns, p.q_hs = qkv.stride(0), qkv.stride(1), D
    p.o, p.o_bs, p.o_ns, p.o_hs, p.lse = o.data_ptr(), o.stride(0), o.stride(1), D, lse.data_ptr()
    p.key_mask = words.data_ptr()
    _lib.check(lib.mc_attn_masked_fwd(p, _lib.stream_handle()), "mc_attn_masked_fwd")
    torch.cuda.synchronize()
    q, k, v = qkv.view(B, N, 3, H, D).unbind(2)
    _, rlse = _ref(q, k, v, 0.125, valid)
    assert (lse.double() - rlse).abs().max().item() < 1e-5 * max(1.0, rlse.abs().max().item())
    assert torch.equal(o, o1)


def test_persistent_backward_crosses_heads_with_different_masks():
    """288 (batch, head) pairs on 256 CUs at N = 64: the persistent backward moves to a head of another
    batch row and must re-read that row's mask words.  Every row has its own length, some with an
    empty trailing tile; a spread of heads is checked one by one."""
    g = torch.Generator().manual_seed(11)
    B, H, N = 24, 12, 64
    C = H * D
    lengths = torch.tensor([64, 1, 33, 32, 7, 50, 40, 17, 63, 2, 31, 48, 64, 12, 34, 29, 5, 57, 45, 20, 60, 3, 36, 25])
    valid = (torch.arange(N)[None, :] < lengths[:, None]).to(DEV)
    qkv = _packed(B, N, H, torch.bfloat16, g)
    go = torch.randn(B, N, C, generator=g).to(torch.bfloat16).to(DEV)
    o, grad = _run(qkv, H, valid, go)
    ref_in = qkv.double().requires_grad_(True)
    q, k, v = ref_in.view(B, N, 3, H, D).unbind(2)
    ro, _ = _ref(q, k, v, D ** -0.5, valid)
    ro.reshape(B, N, C).backward(go.double())
    assert _nerr(o, ro.reshape(B, N, C)) < 8e-3
    got = grad.view(B, N, 3, H, D).double()
    want = ref_in.grad.view(B, N, 3, H, D)
    for bh in list(range(0, B * H, 13)) + [255, 256, 257, B * H - 1]:   # incl. the first heads of the second sweep
        b, h = divmod(bh, H)
        # floor: 1e-3 of the head's whole gradient (a one-key row has dq = dk = 0 exactly)
        floor = 1e-3 * want[b, :, :, h].norm().item() + 1e-12
        for s in range(3):
            assert _nerr(got[b, :, s, h], want[b, :, s, h], floor) < 3e-2, (b, h, s)
    assert _nerr(got, want) < 2e-2
    dead = ~valid
    assert got[:, :, 1][dead].eq(0).all() and got[:, :, 2][dead].eq(0).all()


@pytest.mark.parametrize("N", [40, 256])
def test_tower_attention_masked_fused_matches_sdpa(N):
    """model.Attention with a padding mask under bf16 autocast: the fused masked path (qkv bias
    gradient from the kernel's dsum side channel) against the masked SDPA path, same weights."""
    from mamba_clip_amd.model import Attention
    from mamba_clip_amd.ops import pack_key_mask
    torch.manual_seed(N)
    m = Attention(768, 12).to(DEV)
    torch.nn.init.normal_(m.qkv.bias, std=0.5)
    B = 4
    x = torch.randn(B, N, 768, device=DEV)
    gy = torch.randn(B, N, 768, device=DEV)
    lengths = torch.tensor([N, 1, N // 2 + 1, 33], device=DEV)
    valid = torch.arange(N, device=DEV)[None, :] < lengths[:, None]
    runs = []
    for fused in (True, False):
        m.fused_attention = fused
        m.zero_grad()
        xx = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = m(xx, pack_key_mask(valid) if fused else None, valid)
        assert m.last_path == ("fused" if fused else "sdpa")
        (y.float() * gy).sum().backward()
        runs.append((y.detach().float(), xx.grad.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    (yf, gxf, gpf), (yu, gxu, gpu) = runs
    assert _nerr(yf, yu) < 1e-2
    assert _nerr(gxf, gxu) < 2e-2
    for n in gpu:
        e = _nerr(gpf[n], gpu[n])
        print(f"N {N} {n} {e:.3e}")
        assert e < 2e-2, n


def test_all_zero_mask_row_stays_finite():
    """Not a supported input (CLS is never padding); the kernels must still end and leave no NaN / inf."""
    g = torch.Generator().manual_seed(3)
    for N in (40, 256):
        B, H = 3, 2
        valid = torch.ones(B, N, dtype=torch.bool)
        valid[1] = False
        qkv = _packed(B, N, H, torch.bfloat16, g)
        go = torch.randn(B, N, H * D, generator=g).to(torch.bfloat16).to(DEV)
        o, grad = _run(qkv, H, valid.to(DEV), go)
        torch.cuda.synchronize()
        assert torch.isfinite(o).all() and torch.isfinite(grad).all()


def test_masked_attention_rejects_unsupported():
    from mamba_clip_amd import _lib
    from mamba_clip_amd.ops import pack_key_mask, packed_attention
    def words(n):
        return pack_key_mask(torch.ones(1, min(n, 256), dtype=torch.bool, device=DEV))
    with pytest.raises(RuntimeError, match="unsupported"):
        packed_attention(torch.zeros(1, 257, 3 * 64, device=DEV, dtype=torch.bfloat16), 1, words(257))
    with pytest.raises(RuntimeError, match="unsupported"):
        packed_attention(torch.zeros(1, 16, 3 * 128, device=DEV, dtype=torch.bfloat16), 1, words(16))
    with pytest.raises(RuntimeError, match="unsupported"):
        packed_attention(torch.zeros(1, 16, 3 * 64, device=DEV, dtype=torch.float32), 1, words(16))
    with pytest.raises(RuntimeError, match="key_mask"):      # the boolean mask instead of its packed words
        packed_attention(torch.zeros(1, 16, 3 * 64, device=DEV, dtype=torch.bfloat16), 1,
                         torch.ones(1, 16, dtype=torch.bool, device=DEV))
    # null mask at the C ABI
    lib = _lib.load()
    y = torch.zeros(1, 16, 3 * 64, device=DEV, dtype=torch.bfloat16)
    o = torch.empty(1, 16, 64, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(1, 1, 16, device=DEV)
    p = _lib.AttnMaskedFwdParams()
    p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = 1, 1, 16, 64, _lib.MC_DTYPE_BF16, 0.125
    p.q, p.k, p.v = y.data_ptr(), y.data_ptr() + 128, y.data_ptr() + 256
    p.q_bs, p.q_ns, p.q_hs = y.stride(0), y.stride(1), 64
    p.o, p.o_bs, p.o_ns, p.o_hs, p.lse = o.data_ptr(), o.stride(0), o.stride(1), 64, lse.data_ptr()
    with pytest.raises(RuntimeError, match="key_mask"):
        _lib.check(lib.mc_attn_masked_fwd(ctypes.byref(p), _lib.stream_handle()), "mc_attn_masked_fwd")
