"""fp64 reference of the causal fused attention (mc_attn_causal_fwd / _bwd) and a runner for the two
entry points.  Helper module of test_attn_causal_gpu.py: no tests.

reference() returns the namespace attn_ref.reference() returns, with P and dS zero above the diagonal
and valid = None, so attn_ref.bounds() / dsum_reference() apply unchanged: every term of those bounds
is a sum over P or dS, which are causal here; only the subnormal term sums |v| / |k| over all keys
instead of the keys j <= i, which makes the bound slightly loose, never wrong."""
import ctypes
import types

import torch

D = 64
INT = {2: torch.int16, 4: torch.int32}


def reference(q, k, v, dout, scale):
    """fp64 causal attention forward + backward; tensors (B, N, H, D), lse (B, H, N), P / dS (B, H, N, N)."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    N = q.shape[1]
    s = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = torch.einsum("bhnm,bmhd->bnhd", P, v)
    dP = torch.einsum("bnhd,bmhd->bhnm", dout, v)
    delta = (dout * o).sum(-1).permute(0, 2, 1)
    dS = P * (dP - delta[..., None])
    r = types.SimpleNamespace(q=q, k=k, v=v, dout=dout, scale=scale, valid=None, P=P, dS=dS, o=o, lse=lse)
    r.dq = scale * torch.einsum("bhnm,bmhd->bnhd", dS, k)
    r.dk = scale * torch.einsum("bhnm,bnhd->bmhd", dS, q)
    r.dv = torch.einsum("bhnm,bnhd->bmhd", P, dout)
    r.Dabs = (dout * o).abs().sum(-1).permute(0, 2, 1)
    return r


def bits(t):
    return t.contiguous().view(INT[t.element_size()])


def run(q, k, v, do, scale, layout="packed"):
    """mc_attn_causal_fwd then _bwd on q, k, v, do (B, N, H, D; 16-bit, on the device).
    layout "packed": q / k / v slices of a (B, N, 3, H, D) projection output, dense (B, N, H, D) o / dout,
    gradients into a packed (B, N, 3, H, D) buffer -- the towers' strides.
    layout "bhnd_rev": q, k, v, o, dout, dq, dk, dv each a tensor of its own, (B, H, N, D) with the batches
    stored in reverse order: base pointer at the last slab, NEGATIVE batch stride, head stride N D.
    Returns o, dq, dk, dv as (B, N, H, D), lse (B, H, N), dsum (B, 3, H, D)."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    B, N, H, _ = q.shape
    dt = q.dtype
    nan = float("nan")
    if layout == "packed":
        inb = torch.empty(B, N, 3, H, D, dtype=dt, device=q.device)
        qv, kv, vv = inb.unbind(2)
        o = torch.full((B, N, H, D), nan, dtype=dt, device=q.device)
        g = torch.empty(B, N, H, D, dtype=dt, device=q.device)
        dq, dk, dv = torch.full((B, N, 3, H, D), nan, dtype=dt, device=q.device).unbind(2)
        ptr = lambda t: t.data_ptr()  # noqa: E731
        strides = lambda t: (t.stride(0), t.stride(1), t.stride(2))  # noqa: E731
        view = lambda t: t  # noqa: E731
    elif layout == "bhnd_rev":
        mk = lambda fill: torch.full((B, H, N, D), fill, dtype=dt, device=q.device)  # noqa: E731
        qv, kv, vv, g = mk(0.0), mk(0.0), mk(0.0), mk(0.0)
        o, dq, dk, dv = mk(nan), mk(nan), mk(nan), mk(nan)
        ptr = lambda t: t[B - 1].data_ptr()  # noqa: E731
        strides = lambda t: (-t.stride(0), t.stride(2), t.stride(1))  # noqa: E731
        view = lambda t: t.flip(0).permute(0, 2, 1, 3)  # noqa: E731  (batch b lives in slab B - 1 - b)
    else:
        raise ValueError(layout)
    for dst, src in ((qv, q), (kv, k), (vv, v), (g, do)):
        if layout == "packed":
            dst.copy_(src)
        else:
            dst.copy_(src.permute(0, 2, 1, 3).flip(0))
    lse = torch.full((B, H, N), nan, dtype=torch.float32, device=q.device)
    dsum = torch.full((B, 3, H, D), nan, dtype=torch.float32, device=q.device)
    f, b = _lib.AttnFwdParams(), _lib.AttnBwdParams()
    for p in (f, b):
        p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = B, H, N, D, _lib.dtype_code(dt), scale
        p.q, p.k, p.v = ptr(qv), ptr(kv), ptr(vv)
        assert strides(qv) == strides(kv) == strides(vv)
        p.q_bs, p.q_ns, p.q_hs = strides(qv)
        p.o = ptr(o)
        assert strides(o) == strides(g)
        p.o_bs, p.o_ns, p.o_hs = strides(o)
        p.lse = lse.data_ptr()
    b.dout = ptr(g)
    b.dq, b.dk, b.dv = ptr(dq), ptr(dk), ptr(dv)
    assert strides(dq) == strides(dk) == strides(dv)
    b.dq_bs, b.dq_ns, b.dq_hs = strides(dq)
    b.dsum = dsum.data_ptr()
    stream = _lib.stream_handle()
    _lib.check(lib.mc_attn_causal_fwd(ctypes.byref(f), stream), "mc_attn_causal_fwd")
    _lib.check(lib.mc_attn_causal_bwd(ctypes.byref(b), stream), "mc_attn_causal_bwd")
    torch.cuda.synchronize()
    return types.SimpleNamespace(o=view(o), lse=lse, dq=view(dq), dk=view(dk), dv=view(dv), dsum=dsum)
