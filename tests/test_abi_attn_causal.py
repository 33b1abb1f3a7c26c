"""CPU-side checks of the causal attention ABI (mc_attn_causal_fwd / _bwd, include/mc_attn.h): the
symbols exist in the library, the binding table and the header, they take the unmasked parameter
structs, and bad arguments are rejected on the host with the codes of mc_attn_fwd / _bwd.  No GPU calls:
rejected calls return from validation (bogus pointers: a launch would fault), accepted ones have batch = 0,
as test_abi_attn_range.py does."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

MC_OK, MC_ERR_INVALID, MC_ERR_DTYPE, MC_ERR_SHAPE = 0, -1, -2, -3
N, D = 77, 64


def _params(name, batch=2):
    from mamba_clip_amd import _lib
    p = getattr(_lib, name)()
    p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = batch, 8, N, D, _lib.MC_DTYPE_BF16, 0.125
    p.q = p.k = p.v = p.o = p.lse = 4096
    p.q_bs, p.q_ns, p.q_hs = N * 1536, 1536, 64
    p.o_bs, p.o_ns, p.o_hs = N * 512, 512, 64
    if "Bwd" in name:
        p.dout = p.dq = p.dk = p.dv = 4096
        p.dq_bs, p.dq_ns, p.dq_hs = N * 1536, 1536, 64
    return p


ENTRY = [("mc_attn_causal_fwd", "AttnFwdParams"), ("mc_attn_causal_bwd", "AttnBwdParams")]


def test_symbols_in_library_binding_and_header():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mc_attn.h")).read()
    for fn, cls in ENTRY:
        call = getattr(lib, fn)
        assert call.restype is ctypes.c_int
        assert call.argtypes[0] is ctypes.POINTER(getattr(_lib, cls)) and call.argtypes[1] is ctypes.c_void_p
        struct = {"AttnFwdParams": "mc_attn_fwd_params", "AttnBwdParams": "mc_attn_bwd_params"}[cls]
        assert re.search(rf"int {fn}\(const {struct}\* p, void\* stream\);", header), fn


@pytest.mark.parametrize("fn,cls", ENTRY)
def test_causal_entry_checks_reject_before_launch(fn, cls):
    from mamba_clip_amd import _lib
    lib = _lib.load()
    call = getattr(lib, fn)
    assert call(None, None) == MC_ERR_INVALID
    p = _params(cls)
    p.head_dim = 32
    assert call(ctypes.byref(p), None) == MC_ERR_SHAPE and b"head_dim" in lib.mc_last_error()
    for n in (0, 257, -1):
        p = _params(cls)
        p.seqlen = n
        assert call(ctypes.byref(p), None) == MC_ERR_SHAPE and b"seqlen" in lib.mc_last_error(), n
    p = _params(cls)
    p.dtype = _lib.MC_DTYPE_F32                      # as mc_attn_fwd / _bwd: the dtype has its own code
    assert call(ctypes.byref(p), None) == MC_ERR_DTYPE
    p = _params(cls)
    p.k = 4096 + 8                                   # not 16-B aligned
    assert call(ctypes.byref(p), None) == MC_ERR_INVALID and b"aligned" in lib.mc_last_error()
    p = _params(cls)
    p.o_ns = 516                                     # rows not 16-B aligned
    assert call(ctypes.byref(p), None) == MC_ERR_INVALID and b"aligned" in lib.mc_last_error()
    p = _params(cls)
    p.lse = None
    assert call(ctypes.byref(p), None) == MC_ERR_INVALID
    if "bwd" in fn:
        p = _params(cls)
        p.dv = 4096 + 2
        assert call(ctypes.byref(p), None) == MC_ERR_INVALID
    # token strides: the limits of the unmasked entry points
    for bad in (-8, 1 << 40):
        p = _params(cls)
        p.q_ns = bad
        assert call(ctypes.byref(p), None) == MC_ERR_SHAPE and b"q_ns" in lib.mc_last_error(), bad
    assert fn.encode() in lib.mc_last_error()        # the message names the causal entry point


@pytest.mark.parametrize("fn,cls", ENTRY)
def test_causal_entry_accepts_the_tower_shapes(fn, cls):
    """batch = 0: validation runs in full and nothing is launched."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    call = getattr(lib, fn)
    for n in (1, 77, 256):
        p = _params(cls, 0)
        p.seqlen = n
        assert call(ctypes.byref(p), None) == MC_OK, (n, lib.mc_last_error())
