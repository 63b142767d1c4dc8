"""Attention-kernel micro-benchmark at the bench workload's cross-attention launch (N = 6 pairs x
64 windows = 384 sequences, L = 300, head_dim 512, bf16) and the c4 long window (N = 6 x 16,
L = 1024): jmt_attn_fwd and jmt_attn_bwd launched back to back, HIP events on the launch stream.
Algorithmic FLOP: fwd 4 N L^2 d; bwd (P recompute, dP, dQ) 6 N L^2 d.
    python scripts/bench_attn.py [N L reps]
    python scripts/bench_attn.py fwd-ab [rounds]   the forward alone at the c3 step's two
        launches (N = 384 cross-attention, N = 192 encoders, L = 300) and c4's (N = 96,
        L = 1024), the whole-row kernel (jmt_attn_set_fwd_rows 1) against the 64-row kernel (0),
        the two settings interleaved round by round; medians and ranges per setting"""
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import ops  # noqa: E402

PEAK = 2516.6


def timeit(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def run(N, L, reps, alias=False):
    E = 512
    cd = torch.bfloat16
    dt = ops.dt(cd)
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(N, L, 3 * E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    st = (qkv.stride(0), qkv.stride(1))
    skv = (qkv.stride(0), 0) if alias else st      # ablation: every sequence reads window 0's K/V
    o = torch.empty(N, L, E, device="cuda", dtype=cd).permute(1, 0, 2)
    so = (o.stride(0), o.stride(1))
    lse = torch.empty(N * L, device="cuda")
    go = torch.randn(N, L, E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
    ldp = -(-L // 8) * 8
    P = torch.empty(N * L * ldp, device="cuda", dtype=cd)
    dS = torch.empty_like(P)
    dq = torch.empty_like(o)
    scale = 1.0 / math.sqrt(E)
    fwd = lambda: ops.attn_fwd(dt, N, 1, L, L, E, q.data_ptr(), st, k.data_ptr(), skv,
                               v.data_ptr(), skv, o.data_ptr(), so, scale, lse)
    bwd = lambda: ops.attn_bwd(dt, N, 1, L, L, E, go.data_ptr(), so, o.data_ptr(), so,
                               q.data_ptr(), st, k.data_ptr(), skv, v.data_ptr(), skv, lse, P, dS,
                               ldp, dq.data_ptr(), so, scale)
    fwd()
    tf = timeit(fwd, reps)
    tb = timeit(bwd, reps)
    u = 2.0 * N * L * L * E
    r = {"N": N, "L": L, "alias_kv": alias, "fwd_us": round(tf, 1), "fwd_frac": round(2 * u / tf / 1e6 / PEAK, 4),
         "bwd_us": round(tb, 1), "bwd_frac_3products": round(3 * u / tb / 1e6 / PEAK, 4)}
    print(json.dumps(r), flush=True)


def fwd_ab(rounds=7, reps=20):
    """Forward A/B in one process: per shape, `rounds` rounds of (64-row, whole-row) timings."""
    import statistics
    from jmt import _lib
    lib = _lib.load()
    E = 512
    cd = torch.bfloat16
    dt = ops.dt(cd)
    scale = 1.0 / math.sqrt(E)
    for N, L in ((384, 300), (192, 300), (96, 1024)):
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(N, L, 3 * E, device="cuda", generator=g).to(cd).permute(1, 0, 2)
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        st = (qkv.stride(0), qkv.stride(1))
        o = torch.empty(N, L, E, device="cuda", dtype=cd).permute(1, 0, 2)
        so = (o.stride(0), o.stride(1))
        lse = torch.empty(N * L, device="cuda")
        fwd = lambda: ops.attn_fwd(dt, N, 1, L, L, E, q.data_ptr(), st, k.data_ptr(), st,
                                   v.data_ptr(), st, o.data_ptr(), so, scale, lse)
        t = {0: [], 1: []}
        try:
            for _ in range(rounds):
                for on in (0, 1):
                    lib.jmt_attn_set_fwd_rows(on)
                    t[on].append(timeit(fwd, reps))
        finally:
            lib.jmt_attn_set_fwd_rows(-1)
        u = 4.0 * N * L * L * E
        r = {"N": N, "L": L, "rounds": rounds}
        for on, name in ((0, "rows64"), (1, "rows128")):
            med = statistics.median(t[on])
            r[name + "_us"] = {"median": round(med, 1), "min": round(min(t[on]), 1),
                               "max": round(max(t[on]), 1)}
            r[name + "_frac"] = round(u / med / 1e6 / PEAK, 4)
        r["below_range"] = r["rows128_us"]["median"] < r["rows64_us"]["min"]
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "fwd-ab":
        fwd_ab(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    elif len(sys.argv) > 2:
        run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]) if len(sys.argv) > 3 else 20,
            len(sys.argv) > 4 and sys.argv[4] == "alias")
    else:
        run(384, 300, 20)
        run(96, 1024, 10)
