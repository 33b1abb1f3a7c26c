"""Which scan kernel family a call selects, pinned at the boundaries of the choice.  Host queries only
(mc_scan_fwd_kernel, mc_scan_fwd_state_interval, mc_scan_bwd_kernel): params are built by hand around
made-up integer pointers, nothing is launched, no GPU is needed.

The rules (include/mc_scan.h, the pair eligibility in csrc/scan_common.h): the lane-pair kernels take
16-bit rows with wtype == itype, dstate 16, seqlen % 8 == 0 and no direction flags, when
  * every (batch, dim, seqlen) row tensor is 16-B aligned with batch / dim strides in whole 16-B vectors,
  * the rows of one workgroup (32 in the forward, 128 in the backward) fit 32-bit byte offsets:
    ((rows - 1) * |dim stride| + seqlen) * 2 < 2^31,
  * B / C are 16-B aligned with batch / group / dstate strides in whole vectors and dstate stride >= 0.
Anything else runs the general kernels; direction flags select the grouped-direction path; a call
without positions runs nothing.  A fine saved-state interval is honoured exactly where the forward
runs the pair kernel."""
import ctypes

import pytest

from mamba_clip_amd import _lib

NONE, PAIR, GENERIC, DIRS = (_lib.MC_SCAN_KERNEL_NONE, _lib.MC_SCAN_KERNEL_PAIR, _lib.MC_SCAN_KERNEL_GENERIC,
                             _lib.MC_SCAN_KERNEL_DIRS)
F32, BF16, F16 = _lib.MC_DTYPE_F32, _lib.MC_DTYPE_BF16, _lib.MC_DTYPE_F16
FINE, CHUNK = _lib.MC_SCAN_STATE_INTERVAL_FINE, _lib.MC_SCAN_CHUNK
BATCH, DIM, L, N, G = 2, 256, 80, 16, 1
FWD_ROWS, BWD_ROWS = 32, 128   # channels per workgroup of the two pair kernels

FWD_TENSORS = ("u", "delta", "z", "out")
BWD_TENSORS = ("u", "delta", "z", "dout", "du", "ddelta", "dz")


def _base(cls, tensors, dtype=BF16):
    """A pair-eligible call: dense (BATCH, DIM, L) rows, dense B / C, 256-B aligned made-up pointers."""
    p = cls()
    p.batch, p.dim, p.seqlen, p.dstate, p.n_groups = BATCH, DIM, L, N, G
    p.itype = p.wtype = dtype
    p.delta_softplus = 1
    addr = 1 << 20
    for t in tensors:
        setattr(p, t, addr)
        setattr(p, t + "_batch_stride", DIM * L)
        setattr(p, t + "_dim_stride", L)
        addr += 1 << 20
    for t in ("B", "C"):
        setattr(p, t, addr)
        setattr(p, t + "_batch_stride", G * N * L)
        setattr(p, t + "_group_stride", N * L)
        setattr(p, t + "_dstate_stride", L)
        addr += 1 << 20
    for t in ("A", "D", "delta_bias", "chunk_states", "workspace"):
        setattr(p, t, addr)
        addr += 1 << 20
    return p, addr


def fwd_params(dtype=BF16):
    p, _ = _base(_lib.ScanFwdParams, FWD_TENSORS, dtype)
    p.workspace_bytes = 1 << 20
    p.state_interval = FINE   # a request: mc_scan_fwd_state_interval resolves it
    return p


def bwd_params(dtype=BF16):
    p, addr = _base(_lib.ScanBwdParams, BWD_TENSORS, dtype)
    for t in ("dB", "dC", "dA", "dD", "ddelta_bias"):
        setattr(p, t, addr)
        addr += 1 << 20
    p.workspace_bytes = 1 << 24
    return p


def fwd_choice(p):
    lib = _lib.load()
    return lib.mc_scan_fwd_kernel(ctypes.byref(p)), lib.mc_scan_fwd_state_interval(ctypes.byref(p))


def bwd_choice(p):
    return _lib.load().mc_scan_bwd_kernel(ctypes.byref(p))


def last_inside(rows, seqlen=L, elem_bytes=2):
    """Largest dim stride (a whole number of 16-B vectors) whose rows still fit 32-bit byte offsets."""
    return ((1 << 31) // elem_bytes - seqlen - 1) // (rows - 1) // 8 * 8


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_pair_eligible(dtype):
    assert fwd_choice(fwd_params(dtype)) == (PAIR, FINE)
    assert bwd_choice(bwd_params(dtype)) == PAIR
    p = bwd_params(dtype)
    p.state_interval = FINE
    assert bwd_choice(p) == PAIR
    p = fwd_params(dtype)   # no gate: z and dz absent
    p.z = None
    assert fwd_choice(p) == (PAIR, FINE)
    q = bwd_params(dtype)
    q.z = q.dz = None
    assert bwd_choice(q) == PAIR


def _set_shape(p, **kw):
    for k, v in kw.items():
        setattr(p, k, v)


# one departure from the pair-eligible call each (fields common to both params structs)
DEPARTURES = {
    "L77": dict(seqlen=77),                      # rows stay 80 apart: only the length departs
    "N8": dict(dstate=8),
    "N17": dict(dstate=17),
    "fp32_rows": dict(itype=F32, wtype=F32),
    "wtype_ne_itype": dict(wtype=F16),
    "u_plus_2_bytes": dict(u=(1 << 20) + 2),
    "delta_plus_2_bytes": dict(delta=(2 << 20) + 2),
    "z_plus_2_bytes": dict(z=(3 << 20) + 2),
    "u_dim_stride_84": dict(u_dim_stride=84),
    "delta_batch_stride_plus_4": dict(delta_batch_stride=DIM * L + 4),
    "B_group_stride_plus_4": dict(B_group_stride=N * L + 4),
    "C_group_stride_plus_4": dict(C_group_stride=N * L + 4),
    "B_dstate_stride_negative": dict(B_dstate_stride=-L),
    "C_dstate_stride_negative": dict(C_dstate_stride=-L),
    "B_plus_2_bytes": dict(B=(8 << 20) + 2),
}


@pytest.mark.parametrize("name", sorted(DEPARTURES))
def test_single_departure_is_generic(name):
    p, q = fwd_params(), bwd_params()
    _set_shape(p, **DEPARTURES[name])
    _set_shape(q, **DEPARTURES[name])
    assert fwd_choice(p) == (GENERIC, CHUNK)
    assert bwd_choice(q) == GENERIC


def test_forward_only_rows():
    p = fwd_params()
    p.out = p.out + 2
    assert fwd_choice(p) == (GENERIC, CHUNK)
    p = fwd_params()
    p.out_dim_stride = 84
    assert fwd_choice(p) == (GENERIC, CHUNK)
    # out_y counts only with z (the pre-gate output exists only for a gated call)
    p = fwd_params()
    p.out_y, p.out_y_batch_stride, p.out_y_dim_stride = (1 << 28) + 2, DIM * L, L
    assert fwd_choice(p) == (GENERIC, CHUNK)
    p.z = None
    assert fwd_choice(p) == (PAIR, FINE)


@pytest.mark.parametrize("t", ["du", "ddelta", "dz", "dout"])
def test_backward_rows_misaligned(t):
    q = bwd_params()
    setattr(q, t, getattr(q, t) + 2)
    assert bwd_choice(q) == GENERIC
    q = bwd_params()
    setattr(q, t + "_dim_stride", 84)
    assert bwd_choice(q) == GENERIC


def test_span_bound_forward():
    """32 rows per workgroup: (31 * stride + L) * 2 < 2^31."""
    inside = last_inside(FWD_ROWS)
    assert ((FWD_ROWS - 1) * inside + L) * 2 < 1 << 31 <= ((FWD_ROWS - 1) * (inside + 8) + L) * 2
    for t in FWD_TENSORS:
        p = fwd_params()
        setattr(p, t + "_dim_stride", inside)
        assert fwd_choice(p) == (PAIR, FINE), t
        setattr(p, t + "_dim_stride", inside + 8)
        assert fwd_choice(p) == (GENERIC, CHUNK), t
        setattr(p, t + "_dim_stride", -inside)
        assert fwd_choice(p) == (PAIR, FINE), t
        setattr(p, t + "_dim_stride", -inside - 8)
        assert fwd_choice(p) == (GENERIC, CHUNK), t


def test_span_bound_backward():
    """128 rows per workgroup: (127 * stride + L) * 2 < 2^31; the forward's 32-row bound is far off."""
    inside = last_inside(BWD_ROWS)
    assert ((BWD_ROWS - 1) * inside + L) * 2 < 1 << 31 <= ((BWD_ROWS - 1) * (inside + 8) + L) * 2
    for t in BWD_TENSORS:
        q = bwd_params()
        setattr(q, t + "_dim_stride", inside)
        assert bwd_choice(q) == PAIR, t
        setattr(q, t + "_dim_stride", inside + 8)
        assert bwd_choice(q) == GENERIC, t
    p = fwd_params()
    p.u_dim_stride = inside + 8
    assert fwd_choice(p) == (PAIR, FINE)


def test_bc_span_bound():
    """B / C rows of one group: (15 * dstate stride + L) * 2 < 2^31."""
    inside = ((1 << 30) - L - 1) // 15 // 8 * 8
    for t in ("B", "C"):
        p, q = fwd_params(), bwd_params()
        setattr(p, t + "_dstate_stride", inside)
        setattr(q, t + "_dstate_stride", inside)
        assert fwd_choice(p) == (PAIR, FINE) and bwd_choice(q) == PAIR
        setattr(p, t + "_dstate_stride", inside + 8)
        setattr(q, t + "_dstate_stride", inside + 8)
        assert fwd_choice(p) == (GENERIC, CHUNK) and bwd_choice(q) == GENERIC


def test_direction_flags_and_empty_calls():
    for flags in (dict(reverse_groups=1), dict(u_groups=1), dict(reverse_groups=1, u_groups=1)):
        p, q = fwd_params(), bwd_params()
        p.z = q.z = q.dz = None   # the grouped path has no gate
        _set_shape(p, **flags)
        _set_shape(q, **flags)
        assert fwd_choice(p) == (DIRS, CHUNK)
        assert bwd_choice(q) == DIRS
    for empty in (dict(batch=0), dict(seqlen=0)):
        p, q = fwd_params(), bwd_params()
        _set_shape(p, **empty)
        _set_shape(q, **empty)
        assert fwd_choice(p) == (NONE, FINE)   # nothing runs; the interval still follows the pair rule
        assert bwd_choice(q) == NONE
        p.u_dim_stride = 84
        assert fwd_choice(p) == (NONE, CHUNK)
    lib = _lib.load()
    assert lib.mc_scan_fwd_kernel(None) == NONE and lib.mc_scan_bwd_kernel(None) == NONE
    assert lib.mc_scan_fwd_state_interval(None) == CHUNK


@pytest.mark.parametrize("request_", [0, CHUNK])
def test_default_interval_request_stays_default(request_):
    p = fwd_params()
    p.state_interval = request_
    assert fwd_choice(p) == (PAIR, CHUNK)
    p.seqlen = 77
    assert fwd_choice(p) == (GENERIC, CHUNK)


def test_zero_groups_is_answered_not_divided():
    """n_groups == 0 leaves the forward nothing to divide the channels into: its queries answer NONE /
    the default interval.  The backward's choice never divides: it answers as for any other group count."""
    p = fwd_params()
    p.n_groups = 0
    assert fwd_choice(p) == (NONE, CHUNK)


def test_backward_choice_ignores_group_count():
    q = bwd_params()
    q.n_groups = 0
    assert bwd_choice(q) == PAIR
    q.seqlen = 77
    assert bwd_choice(q) == GENERIC


# params the call rejects in its shape / dtype validation: the queries still answer from the choice
REJECTED = {
    "dim_not_divisible": dict(n_groups=3),
    "dim_negative": dict(dim=-256),
    "batch_negative": dict(batch=-1),
}


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_queries_answer_for_rejected_shapes(name):
    p, q = fwd_params(), bwd_params()
    _set_shape(p, **REJECTED[name])
    _set_shape(q, **REJECTED[name])
    assert fwd_choice(p) == (PAIR, FINE)
    assert bwd_choice(q) == PAIR
    p.dstate = q.dstate = 999
    assert fwd_choice(p) == (GENERIC, CHUNK)
    assert bwd_choice(q) == GENERIC
    p.dstate = q.dstate = N
    p.itype = q.itype = p.wtype = q.wtype = 7   # no such dtype: counted as 16-bit, as every code but F32
    assert fwd_choice(p) == (PAIR, FINE)
    assert bwd_choice(q) == PAIR


def test_backward_state_offsets_bound():
    """The pair backward addresses a workgroup's saved states with 32-bit byte offsets:
    128 * n_states * 16 * 4 < 2^31, i.e. fewer than 2^18 states per channel."""
    q = bwd_params()
    q.state_interval = FINE
    q.seqlen = 8 * ((1 << 18) - 1)
    assert bwd_choice(q) == PAIR
    q.seqlen = 8 * (1 << 18)
    assert bwd_choice(q) == GENERIC


def test_queries_leave_the_last_error_alone():
    lib = _lib.load()
    bad = fwd_params()
    bad.dstate = 999
    assert lib.mc_scan_fwd(ctypes.byref(bad), None) == -3
    msg = lib.mc_last_error()
    assert b"dstate" in msg
    p, q = fwd_params(), bwd_params()
    p.seqlen = q.seqlen = 77   # a fine request the forward cannot honour
    q.workspace = None
    assert fwd_choice(p) == (GENERIC, CHUNK) and bwd_choice(q) == GENERIC
    assert lib.mc_last_error() == msg
