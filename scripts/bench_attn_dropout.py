"""The attention core with and without attention dropout at the c3 step's encoder shape (Lq = Lk =
300, N = 192 sequences, E = 512, bf16) for num_heads 8 and 4: forward + backward
(attn_forward + attn_backward on a packed qkv) of
  mh_p0     the fused multi-head kernels, p = 0          (the kernels of a step without dropout)
  mh_drop   the fused multi-head kernels, p = 0.1        (the mask regenerated in registers)
  gemm_p0   the GEMM + softmax path, p = 0
  gemm_drop the GEMM + softmax path, p = 0.1             (jmt_attn_dropout on P and on dP)
each captured once as a hipGraph (eager timing would measure the host's issue rate) and replayed
interleaved in one process, timed with events around `--inner` replays.
    python scripts/bench_attn_dropout.py [--rounds 30] [--inner 10] [--out file.jsonl]
Prints one JSON line per head count: the median, minimum and maximum us per forward + backward
of each variant and the drop / p0 ratios."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import functional as JF  # noqa: E402
from jmt import ops  # noqa: E402
from jmt.graph import GraphedStep  # noqa: E402

DEV = "cuda"
E = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=300)
    ap.add_argument("--N", type=int, default=192)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    cd, L, N = torch.bfloat16, args.L, args.N
    qkv = torch.randn(N, L, 3 * E, device=DEV).to(cd).permute(1, 0, 2)
    go = torch.randn(N, L, E, device=DEV).to(cd).permute(1, 0, 2)
    dqkv = torch.empty(N, L, 3 * E, device=DEV, dtype=cd).permute(1, 0, 2)
    lines = []
    for H in (8, 4):
        def variant(mh, p, H=H):
            want = "mh" if mh else "gemm"

            def fn():
                ops._attn_mh["on"] = mh
                try:
                    with JF.compute_mode(cd):
                        o, saved = JF.attn_forward(qkv, qkv, qkv, E, H, 0, E, 2 * E, drop_p=p)
                        assert saved[1].fwd == want, saved[1].fwd
                        JF.attn_backward(saved, go, dqkv, dqkv, dqkv)
                finally:
                    ops._attn_mh["on"] = True
            return fn

        variants = {"mh_p0": variant(True, 0.0), "mh_drop": variant(True, args.p),
                    "gemm_p0": variant(False, 0.0), "gemm_drop": variant(False, args.p)}
        graphs = {k: GraphedStep(fn).capture(warmup=3) for k, fn in variants.items()}
        times = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    g.replay()
                b.record()
                torch.cuda.synchronize()
                times[k].append(a.elapsed_time(b) * 1e3 / args.inner)
        med = {k: statistics.median(v) for k, v in times.items()}
        res = {"Lq": L, "Lk": L, "N": N, "H": H, "dtype": "bf16", "p": args.p,
               "p_eff": JF.attn_dropout_rate(args.p), "rounds": args.rounds, "inner": args.inner,
               "us": {k: round(v, 2) for k, v in med.items()},
               "us_min": {k: round(min(v), 2) for k, v in times.items()},
               "us_max": {k: round(max(v), 2) for k, v in times.items()},
               "mh_drop_over_p0": round(med["mh_drop"] / med["mh_p0"], 4),
               "gemm_drop_over_p0": round(med["gemm_drop"] / med["gemm_p0"], 4)}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
