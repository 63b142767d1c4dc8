"""Cost of key ranges in the whole-row attention forward and the P / dS backward kernel, at the c3
cross-attention launch (N = 6 x 64 = 384, L = 300, head_dim 512, bf16).  Variants, same operands:
  none  the entry points without ranges (the kernels every unmasked call launches);
  full  a table of [0, L) for every window (the range kernels with nothing masked);
  half  every window left-padded by L / 2 (valid keys [L / 2, L)).
Each variant's `reps` launches are captured into one hipGraph; the graphs are replayed
interleaved, `rounds` rounds, and the median per launch is reported (HIP events around a replay).
The range kernels mask and skip no tile, so `half` is expected to cost what `full` costs.
    python scripts/bench_attn_key_ranges.py [N L] [>> profiles/attn_key_ranges.jsonl]"""
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import ops  # noqa: E402


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


def run(N, L, B=64, reps=20, rounds=9):
    E = 512
    cd = torch.bfloat16
    dt = ops.dt(cd)
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(N, L, 3 * E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    st = (qkv.stride(0), qkv.stride(1))
    o = torch.empty(N, L, E, device="cuda", dtype=cd).permute(1, 0, 2)
    so = (o.stride(0), o.stride(1))
    lse = torch.empty(N * L, device="cuda")
    go = torch.randn(N, L, E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    ldp = ops.attn_dkdv_ldp(L)
    P = torch.zeros(N * L * ldp, device="cuda", dtype=cd)
    dS = torch.zeros_like(P)
    scale = 1.0 / math.sqrt(E)
    tab = lambda b, e: (torch.tensor([b, e] * B, dtype=torch.int32, device="cuda"), B)
    tables = {"none": None, "full": tab(0, L), "half": tab(L // 2, L)}

    def fwd(kr):
        kw = {} if kr is None else {"kr": kr}
        return lambda: ops.attn_fwd(dt, N, 1, L, L, E, q.data_ptr(), st, k.data_ptr(), st,
                                    v.data_ptr(), st, o.data_ptr(), so, scale, lse, **kw)

    def pds(kr):
        kw = {} if kr is None else {"kr": kr}
        return lambda: ops.attn_bwd(dt, N, 1, L, L, E, go.data_ptr(), so, o.data_ptr(), so,
                                    q.data_ptr(), st, k.data_ptr(), st, v.data_ptr(), st, lse, P,
                                    dS, ldp, None, (0, 0), scale, **kw)

    graphs = {}
    for name, kr in tables.items():
        graphs["fwd_" + name] = graphed(fwd(kr), reps)
    fwd(None)()                                     # o / lse of the unmasked forward for the backward
    for name, kr in tables.items():
        graphs["pds_" + name] = graphed(pds(kr), reps)
    t = {n: [] for n in graphs}
    for _ in range(rounds):
        for n, gr in graphs.items():
            t[n].append(replay_us(gr, reps))
    med = {n: round(statistics.median(x), 2) for n, x in t.items()}
    spread = {n: [round(min(x), 2), round(max(x), 2)] for n, x in t.items()}
    rel = {f"{kn}_{var}/none": round(med[f"{kn}_{var}"] / med[f"{kn}_none"], 4)
           for kn in ("fwd", "pds") for var in ("full", "half")}
    print(json.dumps({"N": N, "L": L, "table_entries": B, "reps": reps, "rounds": rounds,
                      "us_median": med, "us_min_max": spread, "ratio": rel}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2:
        run(int(sys.argv[1]), int(sys.argv[2]))
    else:
        run(384, 300)
