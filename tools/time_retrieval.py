"""Time ops.retrieval_ranks (mc_retrieval_ranks: two sweeps of the similarity tiles, no N x N
matrix) at the evaluation shape N = 8192, E = 512, bf16, against what the same library offers
without it, measured in the same process:
  * ce_fused_fwd alone (one sweep: the statistics retrieval_ranks starts with), and
  * the dense way: gemm_nt to fp32 logits (268 MB), then torch comparisons and sums for the four
    count arrays.

    python tools/time_retrieval.py [--out profiles/retrieval/time_retrieval.json] [--rounds 7] [--iters 20]

Method: device events around `iters` back-to-back calls of one variant (torch-level ops, caching
allocator warm), after a warm-up of every variant; the variants run alternately, `rounds` times,
and each figure is the median of its rounds with the min-max spread beside it.  Peak memory of one
call is recorded per variant.  Needs the GPU; prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mamba-clip_amd"))

from mamba_clip_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "retrieval", "time_retrieval.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_retrieval: needs the GPU")
    dev = torch.device("cuda")
    N, E = a.n, a.e
    g = torch.Generator().manual_seed(0)
    X = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=-1).bfloat16().to(dev)
    Y = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=-1).bfloat16().to(dev)
    sc = torch.tensor(30.0, device=dev)

    def ranks():
        return ops.retrieval_ranks(X, Y, sc)

    def fused_fwd():
        return ops.ce_fused_fwd(X, Y, sc, 0, 0.5 / N, 0, 0.5 / N)

    def dense():
        S = ops.gemm_nt(X, Y, alpha_dev=sc)
        t = S.diagonal()
        gt_r, eq_r = (S > t[:, None]).sum(1), (S == t[:, None]).sum(1) - 1
        gt_c, eq_c = (S > t[None, :]).sum(0), (S == t[None, :]).sum(0) - 1
        return gt_r, eq_r, gt_c, eq_c

    variants = {"retrieval_ranks": ranks, "ce_fused_fwd": fused_fwd, "dense_gemm_nt_torch_counts": dense}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters   # us per call

    peak = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
        del out
    r, d = ranks(), dense()
    agree = all(bool(torch.equal(x.long(), y.long())) for x, y in zip(r[:4], d))
    times = {name: [] for name in variants}
    for _ in range(a.rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn))
    res = {"shape": dict(N=N, E=E, dtype="bf16", scale=30.0), "iters": a.iters, "rounds": a.rounds,
           "counts_equal_dense": agree,
           "peak_bytes": peak,
           "us": {k: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
                  for k, v in times.items()}}
    base = res["us"]["ce_fused_fwd"]["median"]
    res["retrieval_ranks_vs_ce_fused_fwd"] = round(res["us"]["retrieval_ranks"]["median"] / base, 3)
    res["dense_vs_retrieval_ranks"] = round(res["us"]["dense_gemm_nt_torch_counts"]["median"]
                                            / res["us"]["retrieval_ranks"]["median"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
