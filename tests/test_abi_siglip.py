"""CPU-side checks of the mc_sigmoid_loss_* C ABI (include/mc_contrastive.h): struct layout against
the header (offsets computed by compiling it with gcc, as tests/test_abi.py does), host validation
without a launch, workspace sizing.  No GPU calls."""
import ctypes
import os
import subprocess
import tempfile

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
FUNCS = ("mc_sigmoid_loss_fwd", "mc_sigmoid_loss_grad")


def _header_layout(struct, fields):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mc_contrastive.h"', "int main(void){",
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


def test_sigmoid_struct_layout_matches_header():
    from mamba_clip_amd import _lib
    cls = _lib.SigmoidLossParams
    fields = [f for f, _ in cls._fields_]
    for f in ("scale", "scale_dev", "bias", "bias_dev", "row_off", "coef", "loss_out", "gout_dev", "g_dtype",
              "g_times_scale", "G", "ldg", "dscale_out", "dbias_out", "workspace", "workspace_bytes"):
        assert f in fields, f
    got = _header_layout("mc_sigmoid_loss_params", fields)
    assert got["size"] == ctypes.sizeof(cls)
    for f in fields:
        assert got[f] == getattr(cls, f).offset, f


def test_neighbouring_structs_keep_their_sizes():
    """The sigmoid loss has a struct of its own: the fused CE's and the retrieval ranks' did not grow."""
    from mamba_clip_amd import _lib
    assert _header_layout("mc_ce_fused_params", [])["size"] == ctypes.sizeof(_lib.CEFusedParams) == 192
    assert _header_layout("mc_retrieval_params", [])["size"] == ctypes.sizeof(_lib.RetrievalParams) == 184
    assert not hasattr(_lib.CEFusedParams, "bias_dev") and not hasattr(_lib.RetrievalParams, "bias_dev")


def test_sigmoid_symbols_exported_and_bound():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    for name in FUNCS + tuple(f + "_workspace_bytes" for f in FUNCS):
        assert name in _lib.SYMBOLS and hasattr(lib, name)


def test_sigmoid_validation_without_launch():
    """Both entry points reject bad arguments on the host, before any launch."""
    from mamba_clip_amd import _lib
    lib = _lib.load()
    for name in FUNCS:
        fn = getattr(lib, name)
        grad = name.endswith("grad")
        p = _lib.SigmoidLossParams()
        p.M, p.N, p.K, p.in_dtype = 4, 4, 8, _lib.MC_DTYPE_BF16
        p.g_dtype, p.ldg = _lib.MC_DTYPE_F32, 4
        call = lambda: fn(ctypes.byref(p), None)  # noqa: E731
        assert fn(None, None) == -1
        assert call() == -1 and b"null operand" in lib.mc_last_error()
        p.X = 4096
        assert call() == -1                                    # Y still null
        p.Y = 4096
        p.in_dtype = _lib.MC_DTYPE_FP8_E4M3
        assert call() == -2 and b"bf16 or fp32" in lib.mc_last_error()
        p.in_dtype = 9
        assert call() == -2
        p.in_dtype = _lib.MC_DTYPE_F32
        for dim in ("M", "N", "K"):
            for bad in (0, -3):
                keep = getattr(p, dim)
                setattr(p, dim, bad)
                assert call() == -3, (name, dim, bad)
                setattr(p, dim, keep)
        for off in (1 << 30, -(1 << 30), 1 << 31, -(1 << 40)):
            p.row_off = off
            assert call() == -3, (name, off)
        p.row_off = (1 << 30) - 1                              # the largest offset is accepted ...
        assert call() == -1                                    # ... and the null output is what fails next
        p.row_off = 0
        assert call() == -1 and (b"null G" if grad else b"null loss_out") in lib.mc_last_error()
        need = getattr(lib, name + "_workspace_bytes")(4, 4)
        if grad:
            p.G = 4096
            p.g_dtype = _lib.MC_DTYPE_FP8_E4M3
            assert call() == -2
            p.g_dtype, p.ldg = _lib.MC_DTYPE_BF16, 3
            assert call() == -3                                # ldg < N
            p.ldg = 4
            p.dscale_out = 4096                                # the workspace is needed for the statistics only
            assert call() == -5
            p.dscale_out, p.dbias_out = None, 4096
            assert call() == -5
        else:
            p.loss_out = 4096
            assert call() == -5                                # no workspace
        p.workspace, p.workspace_bytes = 4096, need - 1
        assert call() == -5                                    # short workspace
        p.workspace, p.workspace_bytes = 4100, need
        assert call() == -5 and b"16-B aligned" in lib.mc_last_error()


def test_sigmoid_workspace_is_per_tile_not_n_by_n():
    from mamba_clip_amd import _lib
    lib = _lib.load()
    n = 8192
    tiles = (n // 128) ** 2
    fwd = lib.mc_sigmoid_loss_fwd_workspace_bytes(n, n)
    grad = lib.mc_sigmoid_loss_grad_workspace_bytes(n, n)
    assert fwd == 4 * tiles                                    # one float per 128 x 128 tile
    assert 2 * 4 * tiles <= grad <= 4 * 4 * tiles              # a few floats per tile
    assert grad * 1000 < n * n and fwd * 1000 < n * n          # far below one byte per logit
    for f in (lib.mc_sigmoid_loss_fwd_workspace_bytes, lib.mc_sigmoid_loss_grad_workspace_bytes):
        assert f(0, 5) == 0 and f(5, 0) == 0
        for m, k in ((5, 7), (129, 1), (300, 1100), (8192, 8192)):
            assert f(m, k) % 16 == 0 and f(m, k) >= 4 * (-(-m // 128)) * (-(-k // 128))
