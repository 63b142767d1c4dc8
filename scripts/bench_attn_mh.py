"""The fused multi-head attention kernels (attn_mh.hip) against the GEMM + softmax path of the same
build, bf16, E = 512 with H = 8 (head dim 64) and H = 4 (head dim 128), at the benchmark's two
time-axis launches (N = 192 and N = 384 sequences of L = 300) and at N = 96, L = 1024.
Variants, same operands (q / k / v as column slices of one packed (L, N, 3E) buffer, gradients
into a packed buffer laid out like it):
  mh    functional.attn_forward / attn_backward as they dispatch (the "mh" plan);
  gemm  the same calls with ops._attn_mh off (batched GEMMs + softmax kernels, P kept).
Forward alone and forward + backward.  Each variant's `reps` calls are captured into one hipGraph;
the graphs are replayed interleaved, `rounds` rounds, and the median per call is reported (HIP
events around a replay).  Run it twice: the spread between the runs is the measurement's noise.
    python scripts/bench_attn_mh.py [N L H] [>> profiles/attn_mh.jsonl]"""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import functional as JF  # noqa: E402
from jmt import ops  # noqa: E402

E = 512


def graphed(fn, reps):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    torch.cuda.synchronize()
    return g


def replay_us(g, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def run(N, L, H, reps=4, rounds=9):
    cd = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(N, L, 3 * E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    go = torch.randn(N, L, E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    dqkv = torch.empty(N, L, 3 * E, device="cuda", dtype=cd).permute(1, 0, 2)

    def call(mh, backward):
        def fn():
            ops._attn_mh["on"] = mh
            try:
                with JF.compute_mode(cd):
                    o, saved = JF.attn_forward(qkv, qkv, qkv, E, H, 0, E, 2 * E)
                    assert saved[1].fwd == ("mh" if mh else "gemm")
                    if backward:
                        JF.attn_backward(saved, go, dqkv, dqkv, dqkv)
            finally:
                ops._attn_mh["on"] = True
        return fn

    graphs = {f"{kn}_{var}": graphed(call(var == "mh", kn == "fwdbwd"), reps)
              for kn in ("fwd", "fwdbwd") for var in ("mh", "gemm")}
    t = {n: [] for n in graphs}
    for _ in range(rounds):
        for n, gr in graphs.items():
            t[n].append(replay_us(gr, reps))
    med = {n: round(statistics.median(x), 2) for n, x in t.items()}
    spread = {n: [round(min(x), 2), round(max(x), 2)] for n, x in t.items()}
    rel = {f"{kn}_gemm/mh": round(med[f"{kn}_gemm"] / med[f"{kn}_mh"], 3)
           for kn in ("fwd", "fwdbwd")}
    print(json.dumps({"N": N, "L": L, "H": H, "dh": E // H, "reps": reps, "rounds": rounds,
                      "us_median": med, "us_min_max": spread, "ratio": rel}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 3:
        run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]))
    else:
        for H in (8, 4):
            for N, L in ((192, 300), (384, 300), (96, 1024)):
                run(N, L, H)
