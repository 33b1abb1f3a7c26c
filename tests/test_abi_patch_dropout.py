"""CPU-side checks of the patch-dropout C ABI (include/mc_ops.h: mc_patch_embed_input_gather,
mc_token_embed_gather_fwd / _bwd): struct layout against the header (offsets computed by compiling it
with gcc, as tests/test_abi.py does) and host validation without a launch.  No GPU calls."""
import ctypes
import os
import subprocess
import tempfile

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
FUNCS = ("mc_patch_embed_input_gather", "mc_token_embed_gather_fwd", "mc_token_embed_gather_bwd")


def _header_layout(struct, fields):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mc_ops.h"', "int main(void){",
           f'printf("size %zu\\n", sizeof({struct}));']
    src += [f'printf("{f} %zu\\n", offsetof({struct}, {f}));' for f in fields]
    src += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write("\n".join(src))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", INCLUDE, c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    return {k: int(v) for k, v in (line.split() for line in out if line)}


def test_token_embed_struct_layout_matches_header():
    from mamba_clip_amd import _lib
    cls = _lib.TokenEmbedGatherParams
    fields = [f for f, _ in cls._fields_]
    for f in ("batch", "n", "n_keep", "cols", "dtype", "cls", "pos", "x", "keep", "out", "dm", "slot", "dpos"):
        assert f in fields, f
    got = _header_layout("mc_token_embed_gather_params", fields)
    assert got["size"] == ctypes.sizeof(cls)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f


def test_patch_input_struct_did_not_grow():
    """The gather form takes keep / n_keep as arguments: mc_patch_input_params keeps its layout."""
    from mamba_clip_amd import _lib
    assert _header_layout("mc_patch_input_params", [])["size"] == ctypes.sizeof(_lib.PatchInputParams) == 64


def test_symbols_exported_and_bound():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    for name in FUNCS:
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_gather_im2col_validation_without_launch():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    fn = lib.mc_patch_embed_input_gather
    assert fn(None, None, 1, None) == -1
    p = _lib.PatchInputParams()
    p.batch, p.channels, p.height, p.width, p.patch = 2, 3, 32, 48, 16
    p.layout, p.in_dtype, p.out_dtype = _lib.MC_LAYOUT_NCHW, _lib.MC_DTYPE_F32, _lib.MC_DTYPE_BF16
    call = lambda k, nk: fn(ctypes.byref(p), k, nk, None)  # noqa: E731
    for bad in (0, -1, 7):                                     # 2 x 3 = 6 patches per image
        assert call(4096, bad) == -3 and b"n_keep" in lib.mc_last_error()
    assert call(4096, 6) == -1                                 # null img / out
    p.img = p.out = 4096
    assert call(None, 3) == -1 and b"keep" in lib.mc_last_error()
    assert call(4098, 3) == -1                                 # keep not 4-B aligned
    p.patch = 6
    assert call(4096, 3) == -3 and b"multiple of 4" in lib.mc_last_error()
    p.patch, p.in_dtype = 16, _lib.MC_DTYPE_U8
    assert call(4096, 3) == -2                                 # uint8 is NHWC
    p.in_dtype, p.batch, p.img, p.out = _lib.MC_DTYPE_F32, 0, None, None
    assert call(None, 3) == 0                                  # empty batch: no pointer is looked at


def test_token_embed_validation_without_launch():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    for name in FUNCS[1:]:
        fn = getattr(lib, name)
        bwd = name.endswith("bwd")
        assert fn(None, None) == -1
        p = _lib.TokenEmbedGatherParams()
        p.batch, p.n, p.n_keep, p.cols, p.dtype = 4, 16, 8, 64, _lib.MC_DTYPE_BF16
        call = lambda: fn(ctypes.byref(p), None)  # noqa: E731
        assert call() == -1 and b"null" in lib.mc_last_error()
        for f in ("cls", "pos", "x", "keep", "out", "dm", "slot", "dpos"):
            setattr(p, f, 4096)
        p.cols = 12                                            # no multiple of a 16-B vector: no launch
        assert call() == -3 and b"16-B vectors" in lib.mc_last_error()
        p.dtype = _lib.MC_DTYPE_F32
        p.cols = 6
        assert call() == -3
        p.cols = 64
        for field, bad in (("n_keep", 0), ("n_keep", 17), ("n", 0), ("batch", -1), ("cols", 0)):
            keep = getattr(p, field)
            setattr(p, field, bad)
            assert call() == -3, (name, field, bad)
            setattr(p, field, keep)
        p.dtype = _lib.MC_DTYPE_FP8_E4M3
        assert call() == -2
        p.dtype = _lib.MC_DTYPE_BF16
        for f in (("dm", "dpos") if bwd else ("cls", "pos", "x", "out")):
            setattr(p, f, 4100)                                # 4-B but not 16-B aligned
            assert call() == -1 and b"aligned" in lib.mc_last_error(), (name, f)
            setattr(p, f, 4096)
        setattr(p, "slot" if bwd else "keep", 4098)
        assert call() == -1
        q = _lib.TokenEmbedGatherParams()                      # empty batch: MC_OK with every pointer null
        q.batch, q.n, q.n_keep, q.cols, q.dtype = 0, 16, 8, 64, _lib.MC_DTYPE_F16
        assert fn(ctypes.byref(q), None) == 0
