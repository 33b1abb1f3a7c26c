"""CPU-side checks of the mc_retrieval_ranks C ABI (include/mc_contrastive.h): struct layout against
the header (offsets computed by compiling it with gcc, as tests/test_abi.py does), host validation
without a launch, workspace sizing.  No GPU calls."""
import ctypes
import os
import subprocess
import tempfile

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")


def test_retrieval_struct_layout_matches_header():
    from mamba_clip_amd import _lib
    cls = _lib.RetrievalParams
    fields = [f for f, _ in cls._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mc_contrastive.h"', "int main(void){",
           'printf("size %zu\\n", sizeof(mc_retrieval_params));']
    src += [f'printf("{f} %zu\\n", offsetof(mc_retrieval_params, {f}));' for f in fields]
    src += ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write("\n".join(src))
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", INCLUDE, c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = dict(line.split() for line in out if line)
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f in fields:
        assert int(got[f]) == getattr(cls, f).offset, f
    # the fused forward's struct is pinned elsewhere and must not have grown for this feature
    assert not hasattr(_lib.CEFusedParams, "gt_r")


def test_retrieval_symbols_exported_and_bound():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    for name in ("mc_retrieval_ranks", "mc_retrieval_ranks_workspace_bytes"):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_retrieval_validation_without_launch():
    """mc_retrieval_ranks rejects bad arguments on the host, before any launch."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    p = _lib.RetrievalParams()
    p.M, p.N, p.K, p.in_dtype = 4, 4, 8, _lib.MC_DTYPE_BF16
    assert lib.mc_retrieval_ranks(None, None) == -1
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -1 and b"null operand" in lib.mc_last_error()
    p.X = p.Y = 4096
    p.in_dtype = _lib.MC_DTYPE_FP8_E4M3
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -2 and b"bf16 or fp32" in lib.mc_last_error()
    p.in_dtype = 9
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -2
    p.in_dtype, p.row_off = _lib.MC_DTYPE_BF16, 1 << 31
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -3
    p.row_off, p.col_off = 0, -(1 << 31)
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -3
    p.col_off = 0
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -1 and b"null output" in lib.mc_last_error()
    p.gt_r = p.eq_r = p.gt_c = p.eq_c = p.lse_r = p.lse_c = p.loss_out = 4096
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -5          # no workspace
    need = lib.mc_retrieval_ranks_workspace_bytes(4, 4)
    p.workspace, p.workspace_bytes = 4096, need - 1
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -5          # short workspace
    p.workspace, p.workspace_bytes = 4100, need
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -5          # not 16-B aligned
    p.M = 0
    assert lib.mc_retrieval_ranks(ctypes.byref(p), None) == -3


def test_retrieval_workspace_is_not_n_by_n():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    n = 8192
    need = lib.mc_retrieval_ranks_workspace_bytes(n, n)
    assert need * 5 < n * n                   # 24 N^2 / 128 bytes: under a fifth of a byte per logit
    tiles = n // 128
    # (max, sumexp) float2 + one packed count word per row and tile column, both directions
    assert need >= 2 * n * tiles * (8 + 4)
    assert need > lib.mc_ce_fused_fwd_workspace_bytes(n, n, 1)
    assert lib.mc_retrieval_ranks_workspace_bytes(0, 5) == 0
    assert lib.mc_retrieval_ranks_workspace_bytes(5, 0) == 0
    assert lib.mc_retrieval_ranks_workspace_bytes(5, 7) % 16 == 0
