"""The per-element attention bounds of tests/attn_ref.py are not tighter than the algorithm: an fp64
emulation of the kernel with its roundings (P, dS, the stored o and every output rounded to the I/O
dtype) stays within them, for both dtypes, with every mask pattern, at N in {1, 33, 100, 256} and in
the input regimes of test_attn_instances_gpu.py (plain, peaked, peaked and masked, key census).
This is the evidence that a correct kernel can pass the GPU tests; the worst ratios are printed.
Also checks the helpers themselves against autograd.  No GPU."""
import pytest
import torch

import attn_ref as ar

B, H, D = 4, 2, 64
SCALE = 0.125
NS = [1, 33, 100, 256]
DTYPES = [torch.bfloat16, torch.float16]


def _inputs(regime, N, dt, g):
    if regime == "plain":
        q, k, v, do, valid = ar.regime_plain(B, N, H, D, g)
    elif regime == "plain-masked":
        q, k, v, do, _ = ar.regime_plain(B, N, H, D, g)
        valid = ar.key_mask_patterns(N, g)
    elif regime in ("peaked", "peaked-masked"):
        q, k, v, do, valid = ar.regime_peaked(B, N, H, D, SCALE, g, regime == "peaked-masked")
    else:
        q, k, v, do, valid = ar.regime_census(B, N, H, D, g, regime == "census-masked")
    return tuple(t.to(dt) for t in (q, k, v, do)) + (valid,)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("regime", ["plain", "plain-masked", "peaked", "peaked-masked", "census", "census-masked"])
def test_emulation_within_bounds(regime, N, dt):
    g = torch.Generator().manual_seed(1000 + N)
    q, k, v, do, valid = _inputs(regime, N, dt, g)
    r = ar.reference(q, k, v, do, SCALE, valid)
    assert r.P.sum(-1).sub(1).abs().max() < 1e-12
    assert (r.lse.abs().max() if N > 1 else 0) <= 64 and (torch.einsum("bnhd,bmhd->bhnm", r.q, r.k) * SCALE).abs().max() <= 64
    if regime.startswith("peaked") and N >= 33:
        assert r.P.amax(-1).min() > 0.99                       # one key per query carries the mass
        if valid is not None:                                  # ... and the largest logit is a masked key's
            s = torch.einsum("bnhd,bmhd->bhnm", r.q, r.k) * SCALE
            assert (~valid[:, None, None, :]).expand_as(s)[torch.arange(B)[:, None, None], torch.arange(H)[None, :, None],
                                                           torch.arange(N)[None, None, :], s.argmax(-1)].all()
    bnd = ar.bounds(r, dt)
    e = ar.emulate(q, k, v, do, SCALE, dt, valid)
    tag = f"{regime} N={N} {dt}"
    for name in ("o", "lse", "dq", "dk", "dv"):
        ar.assert_within(getattr(e, name), getattr(r, name), getattr(bnd, name), f"{name} [{tag}] emulation")


def test_reference_matches_autograd():
    """reference()'s dq / dk / dv are the gradients of its own forward."""
    g = torch.Generator().manual_seed(3)
    N = 45
    q, k, v, do, _ = ar.regime_plain(B, N, H, D, g)
    valid = ar.key_mask_patterns(N, g)
    for val in (None, valid):
        r = ar.reference(q, k, v, do, 0.3, val)
        qa, ka, va = (t.double().requires_grad_(True) for t in (q, k, v))
        s = torch.einsum("bnhd,bmhd->bhnm", qa, ka) * 0.3
        if val is not None:
            s = s.masked_fill(~val[:, None, None, :], float("-inf"))
        o = torch.einsum("bhnm,bmhd->bnhd", torch.softmax(s, -1), va)
        o.backward(do.double())
        for got, want in ((r.o, o.detach()), (r.dq, qa.grad), (r.dk, ka.grad), (r.dv, va.grad), (r.lse, torch.logsumexp(s, -1).detach())):
            assert (got - want).abs().max() <= 1e-12 * want.abs().max().clamp_min(1.0)
        if val is not None:
            assert r.dk[~val].eq(0).all() and r.dv[~val].eq(0).all()


def test_key_mask_patterns_have_the_stated_edges():
    g = torch.Generator().manual_seed(0)
    for NT in range(1, 9):
        for N in (32 * (NT - 1) + 1, 32 * NT - 13, 32 * NT):
            m = ar.key_mask_patterns(N, g)
            assert m.shape == (4, N) and m.any(1).all()
            words = [[int(m[p, 32 * t:32 * t + 32].sum()) for t in range(NT)] for p in range(4)]
            last = N - 32 * (NT - 1)
            assert 1 <= words[0][-1] <= last and all(w == 32 for w in words[0][:-1])       # (a) cut in the last tile
            if NT >= 2:
                assert words[1][-1] == 0 and m[1, 0]                                           # (b) empty trailing tile
                t = words[2].index(0)                                                          # (c) hole over a whole tile ...
                assert t < NT - 1 and sum(words[2][t + 1:]) > 0                                # ... valid keys after it
            assert m[3, 0]


def test_assert_within_reports_one_bad_element():
    ref = torch.ones(2, 5, 2, 4, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    got = ref.clone()
    got[1, 3, 0, 2] += 2e-3
    with pytest.raises(AssertionError, match=r"2\.000 at \(1, 3, 0, 2\)"):
        ar.assert_within(got, ref, bound, "x")
    got[1, 3, 0, 2] = float("nan")
    with pytest.raises(AssertionError, match="inf"):
        ar.assert_within(got, ref, bound, "x")
    assert ar.assert_within(ref + 5e-4, ref, bound, "x") == pytest.approx(0.5)
    with pytest.raises(AssertionError):                        # a zero bound demands an exact value
        ar.assert_within(ref + 1e-9, ref, torch.zeros_like(ref), "x")
