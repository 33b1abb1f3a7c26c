"""CPU-side checks of the masked attention ABI (mc_attn_masked_fwd / _bwd, include/mc_attn.h): the
ctypes mirrors match the C layout (offsets from compiling the header with gcc, as test_abi.py does
for the other structs), the unmasked fields sit where they sit in the unmasked structs, and bad
arguments are rejected on the host.  No GPU calls."""
import ctypes
import os
import subprocess
import tempfile

import pytest

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def _c_layout(cname, fields, extra=()):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mc_attn.h"', "int main(void){",
           f'printf("size %zu\\n", sizeof({cname}));']
    src += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src += list(extra) + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write("\n".join(src))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", INCLUDE, c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {k: int(v) for k, v in (line.split() for line in out if line)}


@pytest.mark.parametrize("cname,pyname,base", [("mc_attn_masked_fwd_params", "AttnMaskedFwdParams", "AttnFwdParams"),
                                               ("mc_attn_masked_bwd_params", "AttnMaskedBwdParams", "AttnBwdParams")])
def test_masked_struct_layout_matches_header(cname, pyname, base):
    from mamba_clip_amd import _lib
    cls, basecls = getattr(_lib, pyname), getattr(_lib, base)
    fields = [f for f, _ in cls._fields_]
    got = _c_layout(cname, fields, ['printf("words %d\\n", MC_ATTN_MASK_WORDS);'])
    assert got["size"] == ctypes.sizeof(cls)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f
    # the unmasked fields first, at the unmasked struct's offsets; key_mask last
    assert fields[:-1] == [f for f, _ in basecls._fields_] and fields[-1] == "key_mask"
    for f in fields[:-1]:
        assert getattr(cls, f).offset == getattr(basecls, f).offset, f
    assert got["words"] == _lib.MC_ATTN_MASK_WORDS == 8


def test_masked_attention_validation_without_launch():
    """Same rejections as mc_attn_fwd / _bwd (test_abi.py), plus the mask pointer."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    p = _lib.AttnMaskedFwdParams()
    p.batch, p.heads, p.seqlen, p.head_dim, p.dtype = 2, 12, 197, 128, _lib.MC_DTYPE_BF16
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -3 and b"head_dim" in lib.mc_last_error()
    p.head_dim, p.seqlen = 64, 257
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -3
    p.seqlen, p.dtype = 197, _lib.MC_DTYPE_F32
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -2
    p.dtype = _lib.MC_DTYPE_BF16
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -1          # null tensors
    p.q = p.k = p.v = p.o = p.lse = 4096
    p.q_bs, p.q_ns, p.q_hs, p.o_bs, p.o_ns, p.o_hs = 197 * 2304, 2304, 64, 197 * 768, 770, 64   # o_ns % 8 != 0
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -1 and b"aligned" in lib.mc_last_error()
    p.o_ns = 768
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -1 and b"key_mask" in lib.mc_last_error()   # null mask
    p.key_mask = 4098
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == -1 and b"key_mask" in lib.mc_last_error()   # 2-B aligned
    p.key_mask, p.batch = 4096, 0
    assert lib.mc_attn_masked_fwd(ctypes.byref(p), None) == 0           # empty batch: nothing launched
    assert lib.mc_attn_masked_fwd(None, None) == -1
    b = _lib.AttnMaskedBwdParams()
    b.batch, b.heads, b.seqlen, b.head_dim, b.dtype = 2, 12, 197, 64, _lib.MC_DTYPE_BF16
    assert lib.mc_attn_masked_bwd(ctypes.byref(b), None) == -1
    b.q = b.k = b.v = b.o = b.dout = b.lse = b.dq = b.dk = b.dv = 4096
    b.q_bs, b.q_ns, b.q_hs = 197 * 2304, 2304, 64
    b.o_bs, b.o_ns, b.o_hs = 197 * 768, 768, 64
    b.dq_bs, b.dq_ns, b.dq_hs = 197 * 2304, 2304, 64
    assert lib.mc_attn_masked_bwd(ctypes.byref(b), None) == -1 and b"key_mask" in lib.mc_last_error()
    b.seqlen = 257
    assert lib.mc_attn_masked_bwd(ctypes.byref(b), None) == -3
