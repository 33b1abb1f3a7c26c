"""Time the causal fused attention (mc_attn_causal_fwd / _bwd) against the unmasked fused kernels at
the same shape and against torch's scaled_dot_product_attention(is_causal=True) under the towers'
backend priority (model._gpu_sdpa_backends), at the CLIP text shape (B 256, H 8, N 77) and at the
longest supported sequence (B 64, H 12, N 256), bf16: forward, and forward + backward.

    python tools/time_attn_causal.py [--out FILE.json] [--rounds 7] [--iters 500]

Method: device events around `iters` back-to-back repetitions of one leg, after a warm-up of every
variant (code objects loaded, SDPA's backend chosen, clocks up); the variants are run alternately in one
process, `rounds` times, and each figure is the median of its rounds with the min-max spread beside it.
The fused kernels are called through the C entry points on the towers' packed (B, N, 3 H D) layout,
buffers allocated once; SDPA runs through autograd on (B, H, N, D) tensors (its forward with gradients
required, as in training; forward + backward through torch.autograd.grad).  Needs the GPU; prints one
JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mamba-clip_amd"))

from mamba_clip_amd import _lib  # noqa: E402
from mamba_clip_amd.model import _gpu_sdpa_backends  # noqa: E402

SHAPES = ((256, 8, 77), (64, 12, 256))
D = 64


def legs(lib, dev, B, H, N):
    """{variant: (forward, forward + backward)} closures for one shape."""
    C = H * D
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B, N, 3 * C, generator=g) * 1.5).bfloat16().to(dev)
    go = torch.randn(B, N, C, generator=g).bfloat16().to(dev)
    o = torch.empty(B, N, C, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=dev)
    dy = torch.empty_like(qkv)
    dsum = torch.empty(B, 3 * C, device=dev)
    st = _lib.stream_handle(dev)
    es = qkv.element_size()
    keep = [qkv, go, o, lse, dy, dsum]

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

    out = {}
    for name, fwd, bwd in (("causal", lib.mc_attn_causal_fwd, lib.mc_attn_causal_bwd),
                           ("unmasked", lib.mc_attn_fwd, lib.mc_attn_bwd)):
        pf, pb = fill(_lib.AttnFwdParams()), fill_bwd(_lib.AttnBwdParams())

        def f(fwd=fwd, pf=pf):
            _lib.check(fwd(pf, st), "forward")

        def fb(fwd=fwd, bwd=bwd, pf=pf, pb=pb):
            _lib.check(fwd(pf, st), "forward")
            _lib.check(bwd(pb, st), "backward")
        out[name] = (f, fb)
        keep += [pf, pb]

    q, k, v = (t.permute(0, 2, 1, 3).contiguous().requires_grad_(True) for t in qkv.view(B, N, 3, H, D).unbind(2))
    gs = go.view(B, N, H, D).permute(0, 2, 1, 3).contiguous()

    def sf():
        with _gpu_sdpa_backends():
            return F.scaled_dot_product_attention(q, k, v, is_causal=True)

    def sfb():
        torch.autograd.grad(sf(), (q, k, v), gs)
    out["sdpa_causal"] = (sf, sfb)
    out["_keep"] = keep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_attn_causal: needs the GPU")
    dev = torch.device("cuda")
    lib = _lib.load()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters   # us per repetition

    results = []
    for B, H, N in SHAPES:
        variants = legs(lib, dev, B, H, N)
        buffers = variants.pop("_keep")      # the kernels' operands: alive until this shape is done
        for f, fb in variants.values():     # warm-up: every leg of every variant, long enough for the clocks
            for _ in range(50):
                f()
                fb()
        torch.cuda.synchronize()
        times = {f"{name}_{leg}": [] for name in variants for leg in ("fwd", "fwd_bwd")}
        for _ in range(a.rounds):
            for name, (f, fb) in variants.items():
                times[f"{name}_fwd"].append(timed(f))
                times[f"{name}_fwd_bwd"].append(timed(fb))
        us = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2))
              for k, v in times.items()}
        med = lambda k: us[k]["median"]  # noqa: E731
        res = {"shape": dict(batch=B, heads=H, seqlen=N, head_dim=D, dtype="bf16"), "iters": a.iters, "rounds": a.rounds,
               "us": us,
               "causal_vs_unmasked": {leg: round(med(f"causal_{leg}") / med(f"unmasked_{leg}"), 3) for leg in ("fwd", "fwd_bwd")},
               "causal_vs_sdpa": {leg: round(med(f"causal_{leg}") / med(f"sdpa_causal_{leg}"), 3) for leg in ("fwd", "fwd_bwd")}}
        res["default_rule"] = {"no_slower_than_sdpa": res["causal_vs_sdpa"]["fwd_bwd"] <= 1.0,
                               "within_1.05x_of_unmasked": res["causal_vs_unmasked"]["fwd_bwd"] <= 1.05}
        results.append(res)
        del variants, buffers
    line = json.dumps({"results": results})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
