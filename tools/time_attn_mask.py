"""Time the key-masked fused attention against the unmasked kernels at the C3 text-tower shape
(B 64, H 12, N 256, bf16): forward and backward, for a full mask and for caption-like lengths
(uniform in [16, 96]).  The unmasked kernels are the baseline.

    python tools/time_attn_mask.py [--out FILE.json] [--rounds 7] [--iters 200]

Method: device events around `iters` back-to-back launches of one kernel (C entry points through
ctypes, no autograd, buffers allocated once), after a warm-up of every variant; the variants are
run alternately, `rounds` times, and each figure is the median of its rounds with the min-max
spread beside it.  Needs the GPU; prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mamba-clip_amd"))

from mamba_clip_amd import _lib  # noqa: E402
from mamba_clip_amd.ops import pack_key_mask  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--seqlen", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_attn_mask: needs the GPU")
    dev = torch.device("cuda")
    lib = _lib.load()
    B, H, N, D = a.batch, a.heads, a.seqlen, 64
    C = H * D
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B, N, 3 * C, generator=g) * 1.5).bfloat16().to(dev)
    go = torch.randn(B, N, C, generator=g).bfloat16().to(dev)
    o = torch.empty(B, N, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=dev)
    dy = torch.empty_like(qkv)
    dsum = torch.empty(B, 3 * C, device=dev)
    lengths = torch.randint(16, 97, (B,), generator=g).clamp_max(N)
    masks = {"full": torch.ones(B, N, dtype=torch.bool),
             "captions": torch.arange(N)[None, :] < lengths[:, None]}
    words = {k: pack_key_mask(v.to(dev)) for k, v in masks.items()}
    st = _lib.stream_handle(dev)
    es = qkv.element_size()

    def fill(p):
        p.batch, p.heads, p.seqlen, p.head_dim, p.dtype, p.scale = B, H, N, D, _lib.MC_DTYPE_BF16, D ** -0.5
        p.q, p.k, p.v = qkv.data_ptr(), qkv.data_ptr() + C * es, qkv.data_ptr() + 2 * C * es
        p.q_bs, p.q_ns, p.q_hs = qkv.stride(0), qkv.stride(1), D
        p.o, p.o_bs, p.o_ns, p.o_hs, p.lse = o.data_ptr(), o.stride(0), o.stride(1), D, lse.data_ptr()
        return p

    def fill_bwd(p):
        fill(p)
        p.dout = go.data_ptr()
        p.dq, p.dk, p.dv = dy.data_ptr(), dy.data_ptr() + C * es, dy.data_ptr() + 2 * C * es
        p.dq_bs, p.dq_ns, p.dq_hs = dy.stride(0), dy.stride(1), D
        p.dsum = dsum.data_ptr()
        return p

    variants = {}
    fwd_u, bwd_u = fill(_lib.AttnFwdParams()), fill_bwd(_lib.AttnBwdParams())
    variants["unmasked"] = (lambda: lib.mc_attn_fwd(fwd_u, st), lambda: lib.mc_attn_bwd(bwd_u, st))
    for name, w in words.items():
        pf, pb = fill(_lib.AttnMaskedFwdParams()), fill_bwd(_lib.AttnMaskedBwdParams())
        pf.key_mask = pb.key_mask = w.data_ptr()
        variants[name] = (lambda pf=pf: lib.mc_attn_masked_fwd(pf, st), lambda pb=pb: lib.mc_attn_masked_bwd(pb, st))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            rc = fn()
        e1.record()
        e1.synchronize()
        _lib.check(rc, "time_attn_mask")
        return e0.elapsed_time(e1) * 1e3 / a.iters   # us per launch

    times = {f"{name}_{leg}": [] for name in variants for leg in ("fwd", "bwd")}
    for name, (fwd, bwd) in variants.items():   # warm-up; each backward reads the lse / o of its own forward
        for _ in range(20):
            _lib.check(fwd(), name)
            _lib.check(bwd(), name)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (fwd, bwd) in variants.items():
            times[f"{name}_fwd"].append(timed(fwd))
            times[f"{name}_bwd"].append(timed(bwd))
    res = {"shape": dict(batch=B, heads=H, seqlen=N, head_dim=D, dtype="bf16"), "iters": a.iters, "rounds": a.rounds,
           "caption_lengths": dict(min=int(lengths.min()), max=int(lengths.max()), mean=float(lengths.float().mean())),
           "us": {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
                  for k, v in times.items()}}
    for name in words:
        for leg in ("fwd", "bwd"):
            res["us"][f"{name}_{leg}"]["vs_unmasked"] = round(
                res["us"][f"{name}_{leg}"]["median"] / res["us"][f"unmasked_{leg}"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
