"""Time the fused losses, forward and forward + backward, at a given N, E: the logits + CE
(mc_ce_fused_*) and, with --siglip, the pairwise sigmoid loss (mc_sigmoid_loss_*) on the same operands.

    python tools/time_ce.py --n 8192 --e 512 [--fp8] [--siglip]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mamba-clip_amd"))
from mamba_clip_amd.ops import clip_loss_fp8, scaled_logits_ce, sigmoid_logits_loss  # noqa: E402


def timed(fn, iters=20, warm=5):
    for _ in range(warm):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--siglip", action="store_true")
    a = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    X = torch.nn.functional.normalize(torch.randn(a.n, a.e, device="cuda", generator=g), dim=-1).bfloat16()
    Y = torch.nn.functional.normalize(torch.randn(a.n, a.e, device="cuda", generator=g), dim=-1).bfloat16()
    sc = torch.tensor(30.0, device="cuda")
    Xg, Yg, sg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True), sc.clone().requires_grad_(True)

    def fused():
        loss = scaled_logits_ce(Xg, Yg, sg, 0, 0.5 / a.n, 0, 0.5 / a.n)
        loss.backward()

    def fused_fwd():
        with torch.no_grad():
            scaled_logits_ce(X, Y, sc, 0, 0.5 / a.n, 0, 0.5 / a.n)

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    b0 = torch.cuda.memory_allocated()
    t_f = timed(fused)
    pk_f = torch.cuda.max_memory_allocated() - b0
    t_ff = timed(fused_fwd)
    flop = 2.0 * a.n * a.n * a.e
    print(f"N={a.n} E={a.e} bf16: fused fwd {t_ff:.3f} ms ({flop / t_ff / 1e9:.0f} TFLOP/s on the logits GEMM), "
          f"fused fwd+bwd {t_f:.3f} ms (peak +{pk_f / 2**20:.0f} MiB)")
    if a.fp8:
        t8 = timed(lambda: clip_loss_fp8(X, Y, sc))
        print(f"N={a.n} E={a.e} fp8 fused loss (incl. quantisation): {t8:.3f} ms")
    if a.siglip:
        # SigLIP's initial point (logit_scale = 10, logit_bias = -10), both learnable device scalars
        sl, bl = torch.tensor(10.0, device="cuda"), torch.tensor(-10.0, device="cuda")
        slg, blg = sl.clone().requires_grad_(True), bl.clone().requires_grad_(True)

        def siglip():
            sigmoid_logits_loss(Xg, Yg, slg, blg, 0, 1.0 / a.n).backward()

        def siglip_fwd():
            with torch.no_grad():
                sigmoid_logits_loss(X, Y, sl, bl, 0, 1.0 / a.n)

        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        b0 = torch.cuda.memory_allocated()
        t_s = timed(siglip)
        pk_s = torch.cuda.max_memory_allocated() - b0
        t_sf = timed(siglip_fwd)
        print(f"N={a.n} E={a.e} bf16 siglip: fused fwd {t_sf:.3f} ms ({flop / t_sf / 1e9:.0f} TFLOP/s on the logits "
              f"GEMM), fused fwd+bwd {t_s:.3f} ms (peak +{pk_s / 2**20:.0f} MiB)")


if __name__ == "__main__":
    main()
