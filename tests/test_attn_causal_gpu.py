"""The causal fused attention (mc_attn_causal_fwd / _bwd, csrc/attention.hip with kCausal) through the C ABI,
element by element against the fp64 reference of tests/attn_causal_ref.py and the per-element bounds of
tests/attn_ref.py (bounds() with valid = None on causal P / dS: slightly loose in the subnormal term only).
No norms and no excluded element: one wrong row, key, lse lane or tile edge fails.

Lengths: every NT = ceil(N / 32) instance incl. the non-persistent backward (N > 224), a diagonal tile
that is the ragged last tile, one-key last tiles (33, 65, 97, 225), one token, one tile exactly.  Both
dtypes; the towers' packed strides and separate (B, H, N, D) tensors with a negative batch stride; plain
inputs and the census regime (q = 0: P_ij = 1 / (i + 1) exactly, so a dropped or extra key moves o by at
least 1 / (i + 1) against a bound of ~u |o|).  On top: one token gives o = v, dv = dout, dq = dk = 0 bit
for bit; rows < c of o, lse and dq do not depend on rows >= c of the inputs, bit for bit; a second run is
bit-identical; dsum within the sum of the per-element bounds; ops.packed_attention(causal=True) under
autograd gives the bits of the direct calls."""
import functools
import types

import pytest
import torch

import attn_causal_ref as cr
import attn_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64
B, H = 2, 3
SCALE = D ** -0.5
LENGTHS = [1, 2, 31, 32, 33, 64, 65, 77, 96, 97, 224, 225, 256]
DTYPES = [torch.bfloat16, torch.float16]
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst err / bound per output and dtype over this module's cases:")
    for name in ("o", "lse", "dq", "dk", "dv", "dsum"):
        print(f"  {name:5s}" + "".join(f"  {d} {ar.WORST.get((name, 'causal-' + d), float('nan')):.3f}" for d in ("bf16", "f16")))


@functools.lru_cache(maxsize=4)
def _case(N, dt, regime):
    """16-bit device inputs, their fp64 causal reference and bounds (computed once, shared, not modified)."""
    g = torch.Generator().manual_seed(1000 * N + (regime == "census"))
    inputs = ar.regime_plain(B, N, H, D, g) if regime == "plain" else ar.regime_census(B, N, H, D, g, masked=False)
    q, k, v, do = (t.to(dt).to(DEV) for t in inputs[:4])
    r = cr.reference(q, k, v, do, SCALE)
    return types.SimpleNamespace(q=q, k=k, v=v, do=do, dt=dt, r=r, b=ar.bounds(r, dt))


def _check(c, got, tag):
    for name in ("o", "lse", "dq", "dk", "dv"):
        ar.assert_within(getattr(got, name), getattr(c.r, name), getattr(c.b, name), f"{name} [{tag}]", "causal-" + NAME[c.dt])
    ref, bound = ar.dsum_reference(c.r, c.b)
    ar.assert_within(got.dsum, ref, bound, f"dsum [{tag}]", "causal-" + NAME[c.dt])


def _same_bits(a, b, what, names=("o", "lse", "dq", "dk", "dv", "dsum")):
    for name in names:
        x, y = cr.bits(getattr(a, name)), cr.bits(getattr(b, name))
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} elements"


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", LENGTHS)
def test_causal_attention_per_element_vs_fp64(N, dt):
    c = _case(N, dt, "plain")
    got = cr.run(c.q, c.k, c.v, c.do, SCALE, "packed")
    _check(c, got, f"plain packed N={N}")
    again = cr.run(c.q, c.k, c.v, c.do, SCALE, "packed")
    _same_bits(got, again, f"repeat N={N}")                       # no atomics: bitwise reproducible
    rev = cr.run(c.q, c.k, c.v, c.do, SCALE, "bhnd_rev")
    _check(c, rev, f"plain bhnd_rev N={N}")
    _same_bits(got, rev, f"layouts N={N}")                        # the strides change addresses only


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", LENGTHS)
def test_causal_attention_key_census(N, dt):
    c = _case(N, dt, "census")
    # P_ij = 1 / (i + 1) on and below the diagonal, exactly 0 above it
    i = torch.arange(N, device=DEV, dtype=torch.float64)
    want = (torch.ones(N, N, device=DEV, dtype=torch.float64).tril() / (i + 1)[:, None]).expand(B, H, N, N)
    assert (c.r.P - want).abs().max() < 1e-15
    for layout in ("packed", "bhnd_rev"):
        _check(c, cr.run(c.q, c.k, c.v, c.do, SCALE, layout), f"census {layout} N={N}")


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
def test_one_token_is_the_identity(dt):
    c = _case(1, dt, "plain")
    for layout in ("packed", "bhnd_rev"):
        got = cr.run(c.q, c.k, c.v, c.do, SCALE, layout)
        assert torch.equal(cr.bits(got.o), cr.bits(c.v)), layout
        assert torch.equal(cr.bits(got.dv), cr.bits(c.do)), layout
        zero = torch.zeros_like(cr.bits(got.dq))
        assert torch.equal(cr.bits(got.dq), zero) and torch.equal(cr.bits(got.dk), zero), layout
        assert torch.equal(got.dsum[:, :2], torch.zeros_like(got.dsum[:, :2]))


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", LENGTHS[1:])
def test_prefix_independence_bitwise(N, dt):
    """Rows < c of o, lse and dq are functions of rows < c of q, k, v, dout alone: other data in the rows
    >= c (other maxima, other sums, other tiles' contents) must not move one bit of them."""
    c = _case(N, dt, "plain")
    base = cr.run(c.q, c.k, c.v, c.do, SCALE, "packed")
    g = torch.Generator().manual_seed(N)
    for cut in sorted({1, 31, 32, 33, N - 1}):
        if not 1 <= cut < N:
            continue
        q, k, v, do = (t.clone() for t in (c.q, c.k, c.v, c.do))
        for t, s in ((q, 3.0), (k, 3.0), (v, 5.0), (do, 2.0)):
            t[:, cut:] = (torch.randn(B, N - cut, H, D, generator=g) * s).to(dt).to(DEV)
        got = cr.run(q, k, v, do, SCALE, "packed")
        for name, a, b in (("o", got.o[:, :cut], base.o[:, :cut]), ("lse", got.lse[..., :cut], base.lse[..., :cut]),
                           ("dq", got.dq[:, :cut], base.dq[:, :cut])):
            assert torch.equal(cr.bits(a), cr.bits(b)), f"N={N} cut={cut}: {name} rows < {cut} moved"
        assert not torch.equal(cr.bits(got.o[:, cut:]), cr.bits(base.o[:, cut:]))      # and the rest did change


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [77, 256])
def test_packed_attention_causal_autograd_matches_direct_calls(N, dt):
    from mamba_clip_amd.ops import COLSUM_ATTR, PackedCausalAttentionFn, packed_attention
    c = _case(N, dt, "plain")
    direct = cr.run(c.q, c.k, c.v, c.do, SCALE, "packed")
    qkv = torch.stack([c.q, c.k, c.v], 2).reshape(B, N, 3 * H * D).requires_grad_(True)
    o = packed_attention(qkv, H, causal=True)
    assert isinstance(o.grad_fn, PackedCausalAttentionFn._backward_cls)
    o.backward(c.do.reshape(B, N, H * D))
    assert torch.equal(cr.bits(o.detach().view(B, N, H, D)), cr.bits(direct.o))
    dq, dk, dv = qkv.grad.view(B, N, 3, H, D).unbind(2)
    for name, a in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(cr.bits(a), cr.bits(getattr(direct, name))), name
    # and it is not the unmasked function's result
    x = qkv.detach().clone().requires_grad_(True)
    assert not torch.equal(packed_attention(x, H).detach(), o.detach())
    with pytest.raises(ValueError, match="causal"):
        packed_attention(x, H, key_mask=torch.zeros(B, 8, dtype=torch.int32, device=DEV), causal=True)


def test_causal_rejects_unsupported():
    from mamba_clip_amd.ops import packed_attention
    with pytest.raises(RuntimeError, match="unsupported"):
        packed_attention(torch.zeros(1, 257, 3 * 64, device=DEV, dtype=torch.bfloat16), 1, causal=True)
    with pytest.raises(RuntimeError, match="unsupported"):
        packed_attention(torch.zeros(1, 16, 3 * 64, device=DEV, dtype=torch.float32), 1, causal=True)
