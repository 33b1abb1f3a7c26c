"""Host check of the attention kernels' 32-bit buffer offsets (include/mc_attn.h, "Token strides").
K / V in every kernel, and Q / dO / O in the N > 224 backward, are read at byte offset
n * ns * sizeof(T) under a range of ((N - 1) * ns + 64) * sizeof(T) bytes, with offset 2^31 as the
row that reads zero: a token stride that is negative, or whose range exceeds 2^31 bytes, must be
rejected with MC_ERR_SHAPE by all four entry points before anything is launched.  No GPU calls:
rejected calls return from validation, accepted ones have batch = 0."""
import ctypes

import pytest

MC_OK, MC_ERR_SHAPE = 0, -3
N, D, ES = 256, 64, 2
LIMIT = ((1 << 31) // ES - D) // (N - 1) // 8 * 8       # largest 16-B aligned ns with ((N - 1) ns + 64) * 2 <= 2^31


def _params(name, batch, q_ns=2304, o_ns=768):
    from mamba_clip_amd import _lib
    p = getattr(_lib, name)()
    p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = batch, 12, N, D, _lib.MC_DTYPE_BF16, 0.125
    p.q = p.k = p.v = p.o = p.lse = 4096
    p.q_bs, p.q_ns, p.q_hs = N * 2304, q_ns, 64
    p.o_bs, p.o_ns, p.o_hs = N * 768, o_ns, 64
    if "Bwd" in name:
        p.dout = p.dq = p.dk = p.dv = 4096
        p.dq_bs, p.dq_ns, p.dq_hs = N * 2304, 2304, 64
    if "Masked" in name:
        p.key_mask = 4096
    return p


ENTRY = [("mc_attn_fwd", "AttnFwdParams"), ("mc_attn_bwd", "AttnBwdParams"),
         ("mc_attn_masked_fwd", "AttnMaskedFwdParams"), ("mc_attn_masked_bwd", "AttnMaskedBwdParams")]


def test_limit_is_the_documented_one():
    assert LIMIT == 4210752 and ((N - 1) * LIMIT + D) * ES == 1 << 31
    assert ((N - 1) * (LIMIT + 8) + D) * ES > 1 << 31


@pytest.mark.parametrize("fn,cls", ENTRY)
def test_token_stride_out_of_range_is_rejected_before_launch(fn, cls):
    from mamba_clip_amd import _lib
    lib = _lib.load()
    call = getattr(lib, fn)
    # batch = 2 and bogus pointers: a launch would fault, so these must return from validation
    for bad in (LIMIT + 8, 1 << 24, 1 << 40, (1 << 62) + 8, -8, -2304):
        assert call(ctypes.byref(_params(cls, 2, q_ns=bad)), None) == MC_ERR_SHAPE, bad
        assert b"q_ns" in lib.mc_last_error(), lib.mc_last_error()
    if "bwd" in fn:                                      # o / dout of the backward go through o_ns
        for bad in (LIMIT + 8, -768):
            assert call(ctypes.byref(_params(cls, 2, o_ns=bad)), None) == MC_ERR_SHAPE, bad
            assert b"o_ns" in lib.mc_last_error(), lib.mc_last_error()
    # the limit scales with the sequence length: a stride that is fine at N = 256 ... and one that is
    # too large there but fine for a shorter sequence
    p = _params(cls, 0, q_ns=LIMIT + 8)
    p.seqlen = 255
    assert call(ctypes.byref(p), None) == MC_OK
    p.seqlen = 1                                         # one token: the stride is never multiplied
    p.q_ns = 1 << 40
    assert call(ctypes.byref(p), None) == MC_OK


@pytest.mark.parametrize("fn,cls", ENTRY)
def test_allowed_token_strides_pass_validation(fn, cls):
    """batch = 0: validation runs in full and nothing is launched."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    call = getattr(lib, fn)
    assert call(ctypes.byref(_params(cls, 0, q_ns=LIMIT)), None) == MC_OK, lib.mc_last_error()
    assert call(ctypes.byref(_params(cls, 0, o_ns=LIMIT)), None) == MC_OK, lib.mc_last_error()
    assert call(ctypes.byref(_params(cls, 0, q_ns=0, o_ns=0)), None) == MC_OK, lib.mc_last_error()
    # C2 / C3: packed (B, N, 3 * 768) qkv, (B, N, 768) o; image tower N = 197, text tower N = 77 / 256
    for n in (197, 77, 256):
        p = _params(cls, 0, q_ns=2304, o_ns=768)
        p.seqlen = n
        p.q_bs, p.o_bs = n * 2304, n * 768
        assert call(ctypes.byref(p), None) == MC_OK, (n, lib.mc_last_error())
