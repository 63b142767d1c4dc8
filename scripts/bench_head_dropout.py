"""The V / A regressor pair with and without dropout at the c3 step's shape (rows = B*T = 19200,
E = 1024, k = 1, bf16): forward + backward of
  p0      MLPPairFn, p = (0, 0)                       (the default step's route)
  drop    MLPPairFn, p = (0.3, 0.5)                   (counter-based mask in the head kernels)
  torch   two MLPs as Linear -> ReLU -> torch dropout -> Linear, p = (0.3, 0.5)
          (the route dropout took before the HIP mask: no pair GEMM, no head kernels)
each captured once as a hipGraph (the step runs graphed; eager timing here would measure the
host's issue rate) and replayed interleaved in one process, timed with events around `--inner`
replays.
    python scripts/bench_head_dropout.py [--rounds 30] [--inner 20] [--out file.jsonl]
Prints one JSON line: the median us per forward + backward of each variant and the ratios."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import functional as JF  # noqa: E402
from jmt.graph import GraphedStep  # noqa: E402
from jmt.nn import MLP  # noqa: E402

DEV = "cuda"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=19200)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.manual_seed(0)
    E, cd, p = 1024, torch.bfloat16, (0.3, 0.5)
    va, aa = MLP(E, 128, 1, dropout=p[0]).to(DEV), MLP(E, 128, 1, dropout=p[1]).to(DEV)
    x = torch.randn(args.rows, E, device=DEV).to(cd).requires_grad_(True)
    gv = torch.randn(args.rows, 1, device=DEV)
    ga = torch.randn(args.rows, 1, device=DEV)

    def finish(v, a):
        x.grad = None
        torch.autograd.backward([v, a], [gv, ga])

    def pair(rates):
        def fn():
            with JF.compute_mode(cd):
                finish(*JF.mlp_pair(x, va, aa, out_dtype=torch.float32, p=rates))
        return fn

    def torch_route():
        with JF.compute_mode(cd):
            outs = []
            for m, rate in ((va, p[0]), (aa, p[1])):
                h = torch.nn.functional.dropout(m[0](x).relu(), rate, True)
                outs.append(m[len(m) - 1](h, out_dtype=torch.float32))
            finish(*outs)

    variants = {"p0": pair((0.0, 0.0)), "drop": pair(p), "torch": torch_route}
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
    res = {"rows": args.rows, "E": E, "k": 1, "dtype": "bf16", "p": list(p),
           "rounds": args.rounds, "inner": args.inner,
           "us": {k: round(v, 2) for k, v in med.items()},
           "us_min": {k: round(min(v), 2) for k, v in times.items()},
           "us_max": {k: round(max(v), 2) for k, v in times.items()},
           "drop_over_p0": round(med["drop"] / med["p0"], 4),
           "drop_over_torch": round(med["drop"] / med["torch"], 4)}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
