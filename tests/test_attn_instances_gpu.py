"""Every instance of the fused attention (csrc/attention.hip: forward / backward x bf16 / f16 x masked /
unmasked x NT = ceil(N / 32) = 1..8) through the C ABI, element by element against the fp64 reference
and the per-element bounds of tests/attn_ref.py (derived there; test_attn_bounds_cpu.py shows that the
algorithm itself stays within them).  No norms: one wrong row, key, lse lane or tile edge fails.

  1. every NT at three lengths (one key in the last tile, ragged, full), masks with a cut inside the
     last tile / an empty trailing tile / a hole over a whole tile / random bits; masked dk / dv exact
     zeros; a full mask bit-identical to the unmasked entry points
  2. scale 0.3 and 1.0 (the other tests only ever pass 1/8)
  3. q / k / v as separate (B, H, N, D) tensors and as slices of (B, N, H, 3, D); o / dout in a
     (B, N + 3, H, D + 8) buffer; dq / dk / dv in (3, B, H, N + 1, D + 8): within bounds, bit-identical
     to the packed layout, and no element outside the addressed set written (sentinel prefill, guard
     bands around every output buffer, lse and dsum included -- checked on every run of this file)
  4. peaked softmax with logits of +-60, the largest logit on a masked key, and an exact key census
  5. dsum against the fp64 sequence sums; dsum = NULL leaves dq / dk / dv bit-identical
  6. the persistent backward walking two heads per workgroup at NT 3..6

Worst err / bound measured on an MI355X over all 320 cases of this file (the module prints the table at
its end; no ratio above 1, so no kernel change; the fp64 emulation of test_attn_bounds_cpu.py, run in
place of the kernels, gives o 0.865 / 0.698, dq 0.323 / 0.316, dk 0.318 / 0.304, dv 0.824 / 0.762):
            o      lse    dq     dk     dv     dsum
    bf16    0.872  0.030  0.313  0.318  0.824  0.107
    f16     0.698  0.028  0.316  0.304  0.762  0.068
The largest: o 0.872 in the masked persistent sweep at N = 65 (59 x 5 heads), dv 0.824 in the peaked
regime at N = 129.
"""
import ctypes
import functools
import types

import pytest
import torch

import attn_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 64
GUARD = 64                      # sentinel elements in front of and behind every output buffer
SENT = {2: 0x7FC5, 4: 0x7FC54321}   # a NaN in bf16, f16 and fp32
INT = {2: torch.int16, 4: torch.int32}
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


class _Buf:
    """A sentinel-filled buffer with guard bands; views handed out are remembered, so that
    check_untouched() can tell addressed elements from the gaps between them."""

    def __init__(self, shape, dt):
        es = torch.empty((), dtype=dt).element_size()
        n = 1
        for s in shape:
            n *= s
        self.raw = torch.full((n + 2 * GUARD,), SENT[es], dtype=INT[es], device=DEV)
        self.sent = SENT[es]
        self.base = self.raw.view(dt)[GUARD:GUARD + n].view(shape)
        self.views = []

    def use(self, view):
        self.views.append(view)
        return view

    def check_untouched(self, what):
        mark = torch.zeros(self.raw.shape, dtype=torch.bool, device=DEV)
        for v in self.views:
            mark.as_strided(v.shape, v.stride(), v.storage_offset()).fill_(True)
        stray = (self.raw != self.sent) & ~mark
        assert not stray.any(), (f"{what}: {int(stray.sum())} elements outside the addressed set were written, "
                                 f"first at buffer element {int(stray.nonzero()[0]) - GUARD}")


def _strides(*views):
    s = views[0].stride()
    assert all(v.stride() == s for v in views) and s[3] == 1
    return s[0], s[1], s[2]


def run(q, k, v, do, scale, valid=None, layout="packed", dsum=True):
    """mc_attn[_masked]_fwd then _bwd on the values q, k, v, do (B, N, H, D; 16-bit, on the device),
    placed in `layout`.  Returns o, dq, dk, dv as (B, N, H, D) views of the buffers the kernels wrote,
    lse (B, H, N), dsum (B, 3, H, D) or None.  Every output buffer is checked for stray writes."""
    from mamba_clip_amd import _lib
    from mamba_clip_amd.ops import pack_key_mask
    lib = _lib.load()
    B, N, H, _ = q.shape
    dt = q.dtype
    if layout == "packed":          # the towers': q / k / v slices of (B, N, 3, H, D), dense o / dout, packed gradient
        inb = torch.empty(B, N, 3, H, D, dtype=dt, device=DEV)
        qv, kv, vv = inb.unbind(2)
        ob, gb, db = _Buf((B, N, H, D), dt), _Buf((B, N, H, D), dt), _Buf((B, N, 3, H, D), dt)
        o, g = ob.use(ob.base), gb.use(gb.base)
        dq, dk, dv = (db.use(t) for t in db.base.unbind(2))
    else:
        if layout == "bhnd":        # three separate (B, H, N, D) tensors: hs = N D, ns = D
            qv, kv, vv = (torch.empty(B, H, N, D, dtype=dt, device=DEV).permute(0, 2, 1, 3) for _ in range(3))
        elif layout == "bnh3d":     # slices of (B, N, H, 3, D): hs = 3 D, ns = 3 H D
            qv, kv, vv = torch.empty(B, N, H, 3, D, dtype=dt, device=DEV).unbind(3)
        else:
            raise ValueError(layout)
        ob, gb = _Buf((B, N + 3, H, D + 8), dt), _Buf((B, N + 3, H, D + 8), dt)   # gaps between rows and heads
        o, g = ob.use(ob.base[:, :N, :, :D]), gb.use(gb.base[:, :N, :, :D])
        db = _Buf((3, B, H, N + 1, D + 8), dt)                                       # strides unlike q's
        dq, dk, dv = (db.use(t.permute(0, 2, 1, 3)[:, :N, :, :D]) for t in db.base.unbind(0))
    for dst, src in ((qv, q), (kv, k), (vv, v), (g, do)):
        dst.copy_(src)
    lb = _Buf((B, H, N), torch.float32)
    lse = lb.use(lb.base)
    sb = _Buf((B, 3, H, D), torch.float32)
    ds = sb.use(sb.base) if dsum else None
    words = pack_key_mask(valid) if valid is not None else None
    code = _lib.MC_DTYPE_BF16 if dt == torch.bfloat16 else _lib.MC_DTYPE_F16

    f = (_lib.AttnMaskedFwdParams if words is not None else _lib.AttnFwdParams)()
    b = (_lib.AttnMaskedBwdParams if words is not None else _lib.AttnBwdParams)()
    for p in (f, b):
        p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = B, H, N, D, code, scale
        p.q, p.k, p.v = qv.data_ptr(), kv.data_ptr(), vv.data_ptr()
        p.q_bs, p.q_ns, p.q_hs = _strides(qv, kv, vv)
        p.o = o.data_ptr()
        p.o_bs, p.o_ns, p.o_hs = _strides(o, g)
        p.lse = lse.data_ptr()
        if words is not None:
            p.key_mask = words.data_ptr()
    b.dout = g.data_ptr()
    b.dq, b.dk, b.dv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    b.dq_bs, b.dq_ns, b.dq_hs = _strides(dq, dk, dv)
    b.dsum = ds.data_ptr() if dsum else None
    fwd, bwd = _entry_points(lib, words is not None)
    stream = _lib.stream_handle()
    _lib.check(fwd(ctypes.byref(f), stream), "attention forward")
    _lib.check(bwd(ctypes.byref(b), stream), "attention backward")
    torch.cuda.synchronize()
    for buf, what in ((ob, "o"), (gb, "dout (an input)"), (db, "dq / dk / dv"), (lb, "lse"), (sb, "dsum")):
        buf.check_untouched(f"{what} [{layout} N={N}]")
    return types.SimpleNamespace(o=o, lse=lse, dq=dq, dk=dk, dv=dv, dsum=ds)


def _entry_points(lib, masked):
    return (lib.mc_attn_masked_fwd, lib.mc_attn_masked_bwd) if masked else (lib.mc_attn_fwd, lib.mc_attn_bwd)


def _bits(t):
    return t.contiguous().view(INT[t.element_size()])


def assert_same_bits(a, b, what):
    for name in ("o", "lse", "dq", "dk", "dv", "dsum"):
        x, y = getattr(a, name), getattr(b, name)
        if x is None or y is None:
            continue
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs in {int((_bits(x) != _bits(y)).sum())} elements"


def _case(inputs, scale, dt, **kw):
    """Inputs (fp32, CPU) -> the 16-bit device tensors, their fp64 reference and bounds, the kernels' results."""
    q, k, v, do, valid = inputs
    q, k, v, do = (t.to(dt).to(DEV) for t in (q, k, v, do))
    valid = valid.to(DEV) if valid is not None else None
    r = ar.reference(q, k, v, do, scale, valid)
    assert (torch.einsum("bnhd,bmhd->bhnm", r.q, r.k) * scale).abs().max() <= 64   # the bounds' fp32 term assumes it
    return types.SimpleNamespace(q=q, k=k, v=v, do=do, valid=valid, scale=scale, dt=dt, r=r, b=ar.bounds(r, dt),
                                 got=run(q, k, v, do, scale, valid, **kw))


def check_fwd(c, tag):
    for name in ("o", "lse"):
        ar.assert_within(getattr(c.got, name), getattr(c.r, name), getattr(c.b, name), f"{name} [{tag}]", NAME[c.dt])


def check_bwd(c, tag):
    for name in ("dq", "dk", "dv"):
        ar.assert_within(getattr(c.got, name), getattr(c.r, name), getattr(c.b, name), f"{name} [{tag}]", NAME[c.dt])
    if c.valid is not None:     # masked keys: exact zeros (the buffers were prefilled with NaN)
        dead = ~c.valid
        assert c.got.dk[dead].eq(0).all() and c.got.dv[dead].eq(0).all(), f"{tag}: dk / dv of masked keys not zero"


def check_dsum(c, tag):
    """dsum is the sum over n of dq | dk | dv.  The kernel sums its unrounded fp32 tiles (before the 16-bit
    rounding of the stores), so every term is within its per-element bound and the sum within their sum."""
    ref, bound = ar.dsum_reference(c.r, c.b)
    ar.assert_within(c.got.dsum, ref, bound, f"dsum [{tag}]", NAME[c.dt])


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst err / bound per output and dtype over this module's cases:")
    for name in ("o", "lse", "dq", "dk", "dv", "dsum"):
        print(f"  {name:5s}" + "".join(f"  {d} {ar.WORST.get((name, d), float('nan')):.3f}" for d in ("bf16", "f16")))


# ------------------------------------------------------------------ 1. every instance, every edge
LENGTHS = [(NT, N) for NT in range(1, 9) for N in (32 * (NT - 1) + 1, 32 * NT - 13, 32 * NT)]
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=2)
def _instance_case(N, dt, masked):
    g = torch.Generator().manual_seed(7 * N + masked)
    B = 4 if masked else 2      # masked: one pattern per batch row
    q, k, v, do, _ = ar.regime_plain(B, N, 2, D, g)
    return _case((q, k, v, do, ar.key_mask_patterns(N, g) if masked else None), 0.125, dt)


@pytest.mark.parametrize("which,NT,N,dt,masked", [
    pytest.param(w, NT, N, dt, m, id=f"{w}-NT{NT}-N{N}-{NAME[dt]}-{'masked' if m else 'unmasked'}")
    for NT, N in LENGTHS for dt in DTYPES for m in (False, True) for w in ("fwd", "bwd")])
def test_every_instance(which, NT, N, dt, masked):
    assert (N + 31) // 32 == NT
    c = _instance_case(N, dt, masked)       # one forward + backward, shared by the fwd and the bwd case
    (check_fwd if which == "fwd" else check_bwd)(c, f"NT{NT} N={N} {NAME[dt]} {'masked' if masked else 'unmasked'}")


@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("NT,N", LENGTHS, ids=[f"NT{NT}-N{N}" for NT, N in LENGTHS])
def test_full_mask_equals_unmasked_bitwise(NT, N, dt):
    g = torch.Generator().manual_seed(300 + N)
    q, k, v, do = (t.to(dt).to(DEV) for t in ar.regime_plain(2, N, 2, D, g)[:4])
    plain = run(q, k, v, do, 0.125)
    full = run(q, k, v, do, 0.125, torch.ones(2, N, dtype=torch.bool, device=DEV))
    assert_same_bits(plain, full, f"full mask vs unmasked, N={N} {NAME[dt]}")


# ------------------------------------------------------------------ 2. scale
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [83, 243])
@pytest.mark.parametrize("scale", [0.3, 1.0])
def test_scale(scale, N, dt, masked):
    g = torch.Generator().manual_seed(N + int(10 * scale))
    B = 4 if masked else 2
    q, k, v, do, _ = ar.regime_plain(B, N, 2, D, g)
    if scale == 1.0:            # randn * 0.75: logit std 4.5, so |logit| stays far below 64 (asserted in _case)
        q, k = 0.5 * q, 0.5 * k
    c = _case((q, k, v, do, ar.key_mask_patterns(N, g) if masked else None), scale, dt)
    tag = f"scale {scale} N={N} {NAME[dt]}"
    check_fwd(c, tag)
    check_bwd(c, tag)
    check_dsum(c, tag)


# ------------------------------------------------------------------ 3. layouts and stray writes
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("layout", ["bhnd", "bnh3d"])
@pytest.mark.parametrize("N", [51, 243])
def test_layouts_and_stray_writes(N, layout, dt, masked):
    g = torch.Generator().manual_seed(N)
    B = 4 if masked else 2
    q, k, v, do, _ = ar.regime_plain(B, N, 2, D, g)
    inputs = (q, k, v, do, ar.key_mask_patterns(N, g) if masked else None)
    c = _case(inputs, 0.125, dt, layout=layout)      # run() checks that only addressed elements were written
    tag = f"{layout} N={N} {NAME[dt]}"
    check_fwd(c, tag)
    check_bwd(c, tag)
    check_dsum(c, tag)
    packed = run(c.q, c.k, c.v, c.do, 0.125, c.valid)
    assert_same_bits(c.got, packed, f"{tag} vs packed")


# ------------------------------------------------------------------ 4. input regimes
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [65, 129, 225])
@pytest.mark.parametrize("regime", ["peaked", "peaked-masked", "census", "census-masked"])
def test_input_regimes(regime, N, dt):
    g = torch.Generator().manual_seed(N)
    masked = regime.endswith("masked")
    if regime.startswith("peaked"):
        inputs = ar.regime_peaked(2, N, 2, D, 0.125, g, masked)
    else:
        inputs = ar.regime_census(2, N, 2, D, g, masked)
    c = _case(inputs, 0.125, dt)
    if regime.startswith("peaked"):     # the regime is what it claims (on the reference)
        assert c.r.P.amax(-1).min() > 0.99 and c.r.lse.abs().max() > 45
        top = c.r.P.argmax(-1)
        assert (top[..., 0::3] >= 32 * ((N + 31) // 32 - 1)).all()      # a third of the queries: the ragged last tile
    else:
        nv = N if c.valid is None else c.valid.sum(1)[:, None, None, None]
        live = torch.ones(2, N, dtype=torch.bool, device=DEV) if c.valid is None else c.valid
        want = (c.v.double() * live[:, :, None, None]).sum(1, keepdim=True) / nv
        assert (c.r.o - want).abs().max() < 1e-12 and c.r.dk.abs().max() == 0
    tag = f"{regime} N={N} {NAME[dt]}"
    check_fwd(c, tag)
    check_bwd(c, tag)


# ------------------------------------------------------------------ 5. dsum
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("dt", DTYPES, ids=NAME.get)
@pytest.mark.parametrize("N", [33, 100, 197, 256])
def test_dsum_and_null_dsum(N, dt, masked):
    g = torch.Generator().manual_seed(500 + N)
    B = 4 if masked else 2
    q, k, v, do, _ = ar.regime_plain(B, N, 2, D, g)
    c = _case((q, k, v, do, ar.key_mask_patterns(N, g) if masked else None), 0.125, dt)
    tag = f"N={N} {NAME[dt]} {'masked' if masked else 'unmasked'}"
    check_dsum(c, tag)
    check_bwd(c, tag)
    null = run(c.q, c.k, c.v, c.do, 0.125, c.valid, dsum=False)
    assert null.dsum is None
    assert_same_bits(c.got, null, f"dsum = NULL, {tag}")


# ------------------------------------------------------------------ 6. persistent sweep at NT 3..6
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("N", [65, 100, 129, 192])
def test_persistent_backward_two_heads_per_workgroup(N, masked):
    """H = 5 and B = ceil((CUs + 37) / 5): more (batch, head) pairs than CUs by 37..41, so that many
    workgroups of the persistent backward walk two heads (streaming the second one's q / dO / O during
    phase 2 of the first) and the rest walk one.  Masked: every batch row has its own length."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H = 5
    B = -(-(cus + 37) // H)
    g = torch.Generator().manual_seed(N)
    q, k, v, do, _ = ar.regime_plain(B, N, H, D, g)
    valid = None
    if masked:
        lengths = 1 + (37 * torch.arange(B)) % N
        lengths[0], lengths[1] = N, 1
        valid = torch.arange(N)[None, :] < lengths[:, None]
    c = _case((q, k, v, do, valid), 0.125, torch.bfloat16)
    tag = f"persistent N={N} B={B} H={H} {'masked' if masked else 'unmasked'}"
    check_fwd(c, tag)
    check_bwd(c, tag)          # per element over every head
    check_dsum(c, tag)
    again = run(c.q, c.k, c.v, c.do, 0.125, c.valid)
    assert_same_bits(c.got, again, f"{tag}: two runs")
