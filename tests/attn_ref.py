"""fp64 reference, per-element error bounds and a rounding emulation of the fused attention
(csrc/attention.hip).  Helper module of test_attn_bounds_cpu.py and test_attn_instances_gpu.py: no tests.

Tensors are (B, N, H, D) (any strides), lse is (B, H, N), P / dS are (B, H, N_query, N_key), valid is a
(B, N) bool key mask or None.  Everything runs on the device of its inputs.

Bounds.  u = unit roundoff of the I/O dtype (2^-8 bf16, 2^-11 f16), f = 2^-14 the fp32 term (exp2
argument and lse * log2e good to ~2^-17 at |logit| <= 64, fp32 accumulation over <= 256 terms below
that).  The kernel rounds P and dS to the I/O dtype before the second MFMA, reads the stored (rounded)
o for delta = rowsum(dO o) and rounds each output once.  With E_ij = 2u |dS_ij| + 2u P_ij Dabs_i,
Dabs_i = sum_d |dO_id o_id|:
    o_id   (2u + f) sum_j P_ij |v_jd|
    dv_jd  (2u + f) sum_i P_ij |dO_id|
    dq_id  scale sum_j (E_ij + f |dS_ij|) |k_jd| + u |dq_id|
    dk_jd  scale sum_i (E_ij + f |dS_ij|) |q_id| + u |dk_jd|
    lse    1e-5 max(1, |lse|)
All from reference quantities, never from the kernel's output.

Subnormal term.  The table's model fl(x) = x (1 + e), |e| <= u, fails below the smallest normal number
of the dtype: there the rounding error is absolute, up to s = half the smallest subnormal (2^-25 f16,
2^-134 bf16, i.e. nothing).  In the peaked regime most P and dS lie far below 2^-14 and the f16
emulation left the table's dk bound by a factor of 362 (test_attn_bounds_cpu.py), so every rounding
point carries its s as well (Higham's model fl(x) = x (1 + e) + eta): s per rounded P_ij or dS_ij (the
forward rounds p = P l with l >= 1, so at most s on P), summed against the other operand over the
valid keys / all queries, and s for the output's own rounding:
    o_id  += s sum_{valid j} |v_jd| + s          dv_jd += s sum_i |dO_id| + s
    dq_id += scale s sum_{valid j} |k_jd| + s    dk_jd += scale s sum_i |q_id| + s
(dk / dv of masked keys keep the bound 0: they are stored as exact zeros.)  For f16 at N = 256 and
|v| ~ 1 this is ~1e-5 absolute: far below one dropped or doubled key.
"""
import types

import torch

F32_TERM = 2.0 ** -14
LSE_TOL = 1e-5


def unit_roundoff(dtype):
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[dtype]


def half_subnormal(dtype):
    return {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}[dtype]


def _scores(q, k, scale, valid):
    s = torch.einsum("bnhd,bmhd->bhnm", q, k) * scale
    if valid is not None:
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    return s


def reference(q, k, v, dout, scale, valid=None):
    """fp64 attention forward + backward with the intermediates the bounds need."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    s = _scores(q, k, scale, valid)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    o = torch.einsum("bhnm,bmhd->bnhd", P, v)
    dP = torch.einsum("bnhd,bmhd->bhnm", dout, v)
    delta = (dout * o).sum(-1).permute(0, 2, 1)                    # (B, H, N)
    dS = P * (dP - delta[..., None])
    r = types.SimpleNamespace(q=q, k=k, v=v, dout=dout, scale=scale, valid=valid, P=P, dS=dS, o=o, lse=lse)
    r.dq = scale * torch.einsum("bhnm,bmhd->bnhd", dS, k)
    r.dk = scale * torch.einsum("bhnm,bnhd->bmhd", dS, q)
    r.dv = torch.einsum("bhnm,bnhd->bmhd", P, dout)
    r.Dabs = (dout * o).abs().sum(-1).permute(0, 2, 1)             # (B, H, N)
    return r


def bounds(r, dtype):
    """Per-element bounds of o, lse, dq, dk, dv (module docstring) from a reference()."""
    u, f, sc = unit_roundoff(dtype), F32_TERM, abs(r.scale)
    E = 2 * u * r.dS.abs() + 2 * u * r.P * r.Dabs[..., None]
    W = E + f * r.dS.abs()
    b = types.SimpleNamespace()
    b.o = (2 * u + f) * torch.einsum("bhnm,bmhd->bnhd", r.P, r.v.abs())
    b.dv = (2 * u + f) * torch.einsum("bhnm,bnhd->bmhd", r.P, r.dout.abs())
    b.dq = sc * torch.einsum("bhnm,bmhd->bnhd", W, r.k.abs()) + u * r.dq.abs()
    b.dk = sc * torch.einsum("bhnm,bnhd->bmhd", W, r.q.abs()) + u * r.dk.abs()
    b.lse = LSE_TOL * r.lse.abs().clamp_min(1.0)
    # subnormal term (module docstring)
    s = half_subnormal(dtype)
    B, N = r.q.shape[:2]
    live = (torch.ones(B, N, dtype=torch.bool, device=r.q.device) if r.valid is None else r.valid)[:, :, None, None].double()
    b.o = b.o + s * (r.v.abs() * live).sum(1, keepdim=True) + s
    b.dq = b.dq + sc * s * (r.k.abs() * live).sum(1, keepdim=True) + s
    b.dv = b.dv + live * (s * r.dout.abs().sum(1, keepdim=True) + s)
    b.dk = b.dk + live * (sc * s * r.q.abs().sum(1, keepdim=True) + s)
    return b


def dsum_reference(r, b):
    """(B, 3, H, D) sequence sums of dq | dk | dv and their bound, the sum over n of the per-element
    bounds (the kernel sums its unrounded fp32 tiles, so the per-element bounds, which include the
    output rounding, hold for every term)."""
    ref = torch.stack([r.dq.sum(1), r.dk.sum(1), r.dv.sum(1)], 1)
    bound = torch.stack([b.dq.sum(1), b.dk.sum(1), b.dv.sum(1)], 1)
    return ref, bound


def emulate(q, k, v, dout, scale, dtype, valid=None):
    """The kernel's algorithm in fp64 with its roundings to `dtype`: the forward rounds the
    unnormalised p = exp(s - max) before P V (the row sum uses the unrounded p) and the stored o; the
    backward recomputes P = exp(s - lse), rounds P (for dV) and dS = P (dP - delta) (for dQ / dK), takes
    delta from the stored o, and rounds dq, dk, dv once."""
    rd = lambda t: t.to(dtype).double()  # noqa: E731
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    s = _scores(q, k, scale, valid)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - m)
    l = p.sum(-1, keepdim=True)
    e = types.SimpleNamespace()
    e.lse = (m + torch.log(l)).squeeze(-1)
    e.o = rd(torch.einsum("bhnm,bmhd->bnhd", rd(p), v) / l.squeeze(-1).permute(0, 2, 1)[..., None])
    P = torch.exp(s - e.lse[..., None])
    dP = torch.einsum("bnhd,bmhd->bhnm", dout, v)
    delta = (dout * e.o).sum(-1).permute(0, 2, 1)
    dS = rd(P * (dP - delta[..., None]))
    e.dq = rd(scale * torch.einsum("bhnm,bmhd->bnhd", dS, k))
    e.dk = rd(scale * torch.einsum("bhnm,bnhd->bmhd", dS, q))
    e.dv = rd(torch.einsum("bhnm,bnhd->bmhd", rd(P), dout))
    return e


WORST = {}   # (what, tag) -> worst err / bound seen by assert_within, for the reports


def worst_ratio(got, ref, bound):
    """max over elements of |got - ref| / bound and its index.  bound == 0 demands err == 0; a NaN or
    inf in got counts as an infinite ratio."""
    got = got.double()
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.flatten()[flat]), idx, float(err.flatten()[flat]), float(bound.flatten()[flat])


def assert_within(got, ref, bound, what, tag=None):
    """Per element |got - ref| <= bound; fails with the worst err / bound and its index."""
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    ratio, idx, err, bnd = worst_ratio(got, ref, bound)
    if tag is not None:
        key = (what.split()[0], tag)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}: worst err/bound {ratio:.3f} at {idx}")
    assert ratio <= 1.0, f"{what}: err / bound = {ratio:.3f} at {idx} (err {err:.3e}, bound {bnd:.3e}, ref {float(ref[idx]):.6e}, got {float(got[idx]):.6e})"
    return ratio


def key_mask_patterns(N, g):
    """(4, N) bool, one pattern per batch row, NT = ceil(N / 32), r = keys in the last tile:
    (a) a prefix cut inside the last tile (ceil(r / 2) of its keys; the full row at r = 1);
    (b) a prefix cut that leaves at least one whole trailing tile empty (NT >= 2, else cut at 1);
    (c) a hole over a whole non-final tile with valid keys after it (NT >= 2; NT = 1: only the first and the last key);
    (d) random 50 % with key 0 valid."""
    NT = (N + 31) // 32
    r = N - 32 * (NT - 1)
    ar = torch.arange(N)
    a = ar < 32 * (NT - 1) + (r + 1) // 2
    b = ar < (max(1, 32 * (NT - 1) - 19) if NT >= 2 else 1)
    if NT >= 2:
        t = (NT - 1) // 2
        c = (ar < 32 * t) | (ar >= 32 * t + 32)
    else:
        c = (ar == 0) | (ar == N - 1)
    d = torch.rand(N, generator=g) < 0.5
    d[0] = True
    return torch.stack([a, b, c, d])


# ---- input regimes: (q, k, v, dout) fp32 on the CPU with values exact in bf16 and f16 where it matters,
# and valid (B, N) bool or None ----
def regime_plain(B, N, H, D, g):
    """The other attention tests' inputs: randn * 1.5 (logit std 2.25 at scale 1/8)."""
    mk = lambda: torch.randn(B, N, H, D, generator=g)  # noqa: E731
    return mk() * 1.5, mk() * 1.5, mk() * 1.5, mk(), None


def regime_peaked(B, N, H, D, scale, g, masked):
    """One key per query carries > 0.99 of the mass, logits reach about +-60 and none exceeds 64.
    Keys are random sign vectors (+-1, exact in 16 bits) and q_i = c k_{t(i)}: the target scores
    scale * c * D, every other key scale * c * (a sum of D random signs), 8 times smaller in std.
    For a third of the queries (i % 3 == 0) the target lies in the last, ragged key tile.
    Unmasked: c = 60 / (scale D) and every odd key is the negative of the even key before it, so a
    query whose target has such a partner also sees a logit of -60.
    Masked: the odd keys are masked and are 1.25 times the even key after them; targets are even
    keys >= 2 (so the single key of a one-key last tile can be one) and c = 48 / (scale D), so every query scores 48 on its (valid) target and 60 on the masked
    copy: the row maximum must come from the valid keys only."""
    last0 = 32 * ((N + 31) // 32 - 1)
    k = torch.randint(0, 2, (B, N, H, D), generator=g).float() * 2 - 1
    ar = torch.arange(N)
    tgt = torch.where(ar % 3 == 0, last0 + ar % (N - last0), (ar * 7 + 3) % N)
    npair = N // 2
    valid = None
    if masked:
        valid = torch.ones(B, N, dtype=torch.bool)
        valid[:, 1::2] = False
        tgt = (tgt - tgt % 2).clamp_min(2 if N >= 3 else 0)
        nxt = k[:, 2::2]
        k[:, 1:2 * nxt.shape[1]:2] = 1.25 * nxt
        c = 48.0 / (scale * D)
    else:
        k[:, 1::2] = -k[:, 0:2 * npair:2]
        c = 60.0 / (scale * D)
    c = float(torch.tensor(c).bfloat16())        # 8 significant bits: exact in both dtypes
    q = c * k[:, tgt]
    v = torch.randn(B, N, H, D, generator=g)
    dout = torch.randn(B, N, H, D, generator=g)
    return q, k, v, dout, valid


def regime_census(B, N, H, D, g, masked):
    """q = 0, so P = 1 / N_valid exactly; v[j, d] = j // D + 1 if d == j % D else 0, hence
    o[i, d] = sum over the valid j = d (mod D) of (j // D + 1) / N_valid: a dropped, duplicated or
    misplaced key changes an entry by at least 1 / N_valid while the bound is about u |o|.  dO is
    built the same way over the queries, so dv is the same census of the query rows.  k is random (dq
    sees it; dk = 0 exactly).  masked: pattern (d) of key_mask_patterns on every batch row."""
    q = torch.zeros(B, N, H, D)
    k = torch.randn(B, N, H, D, generator=g)
    ar = torch.arange(N)
    v = torch.zeros(B, N, H, D)
    v.permute(1, 3, 0, 2)[ar, ar % D] = (ar // D + 1).float()[:, None, None]
    valid = key_mask_patterns(N, g)[3][None].expand(B, N).clone() if masked else None
    return q, k, v, v.clone(), valid
