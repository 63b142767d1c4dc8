"""Optimizer-step bandwidth at the flagship model's flat-buffer size (c3: about 13.4 M fp32
elements): jmt_adam_step (no AMSGrad, bf16 shadow, zero_grad=1; csrc/adam.hip) against the
existing jmt_sgd_step_zero (nesterov, bf16 shadow; csrc/sgd.hip) as the yardstick, alternated in
one process, device events on the launching stream.
    python scripts/opt_step_bw.py [--n 13400064] [--sets 1] [--rounds 6] [--reps 50] [--out f.txt]
--sets K rotates the launches over K independent buffer sets: at K = 1 part of the working set
(Adam 456 MB, SGD 348 MB at the default n) survives in the 256 MB Infinity Cache from one launch
to the next, as it may between the steps of a small model; K = 4 puts every launch's data out of
the cache's reach, so the figure is what HBM delivers.
Bytes are algorithmic (what each kernel must move once per element):
    Adam 34 B = read p, g, m, v (16) + write p, g, m, v (16) + bf16 shadow (2)
    SGD  26 B = read p, g, buf (12) + write p, g, buf (12) + bf16 shadow (2)
Each round times `reps` launches of one kernel, then `reps` of the other; per kernel the median
round and the min..max spread over rounds are printed, and the Adam / SGD ratio per round (the
target is >= 0.9; a spread wider than that margin is said so rather than called a pass)."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import _lib, ops  # noqa: E402

DEV = "cuda"
HBM_ACHIEVABLE = 6.3e12     # B/s, the achievable HBM rate the shares are quoted against


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps          # seconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=13_400_064)
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    n = args.n
    g0 = torch.Generator(device=DEV).manual_seed(0)
    new = lambda: torch.randn(n, device=DEV, generator=g0)
    zeros = lambda: torch.zeros(n, device=DEV)
    shadow = lambda: torch.empty(n, dtype=torch.bfloat16, device=DEV)
    # separate buffers per kernel (and per set): neither finds the other's lines in a cache
    asets = [(new(), new(), zeros(), zeros(), shadow()) for _ in range(args.sets)]
    ssets = [(new(), new(), zeros(), shadow()) for _ in range(args.sets)]
    state = torch.tensor([1e-4, 0, 0, 0, 0, 0, 0, 0], dtype=torch.float32, device=DEV)
    s = ops.stream()
    _lib.call("jmt_opt_tick", state.data_ptr(), 0.9, 0.999, None, s)
    turn = [0, 0]

    def adam():
        p, g, m, v, sh = asets[turn[0] % args.sets]
        turn[0] += 1
        _lib.call("jmt_adam_step", n, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                  None, state.data_ptr(), 0.9, 0.999, 1e-8, 1e-4, 1.0, None, 1, sh.data_ptr(),
                  _lib.BF16, s)

    def sgd():
        p, g, b, sh = ssets[turn[1] % args.sets]
        turn[1] += 1
        _lib.call("jmt_sgd_step_zero", n, p.data_ptr(), g.data_ptr(), b.data_ptr(), 1e-4, 0.9,
                  0.0, 1e-4, 1, 0, 1.0, sh.data_ptr(), _lib.BF16, s)

    cases = {"adam": (adam, 34), "sgd_zero": (sgd, 26)}
    for fn, _ in cases.values():                    # warm-up
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    rates = {k: [] for k in cases}
    for r in range(args.rounds):
        order = list(cases) if r % 2 == 0 else list(cases)[::-1]
        for k in order:
            fn, bpe = cases[k]
            rates[k].append(bpe * n / timed(fn, args.reps))
    lines = [f"opt_step_bw: n = {n} elements, {args.sets} buffer set(s), {args.rounds} rounds x "
             f"{args.reps} launches per kernel, alternated; device "
             f"{torch.cuda.get_device_name(0)}"]
    for k, (_, bpe) in cases.items():
        v = rates[k]
        med = statistics.median(v)
        lines.append(f"{k:9s} {bpe} B/elem  median {med / 1e12:.3f} TB/s "
                     f"({1e6 * bpe * n / med:.1f} us/launch, {100 * med / HBM_ACHIEVABLE:.1f} % of "
                     f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s)  min {min(v) / 1e12:.3f}  max "
                     f"{max(v) / 1e12:.3f}  spread {100 * (max(v) - min(v)) / med:.1f} %")
    ratios = [a / b for a, b in zip(rates["adam"], rates["sgd_zero"])]
    spread = max((max(v) - min(v)) / statistics.median(v) for v in rates.values())
    lines.append("adam / sgd_zero bytes/s per round: " + " ".join(f"{x:.3f}" for x in ratios))
    rmed = statistics.median(ratios)
    if min(ratios) >= 0.9:
        verdict = "PASS (every round >= 0.9)"
    elif spread > 0.1:
        verdict = "UNDECIDED (run-to-run spread exceeds the 10 % margin)"
    else:
        verdict = "BELOW 0.9"
    lines.append(f"ratio median {rmed:.3f}  min {min(ratios):.3f}  max {max(ratios):.3f}  "
                 f"-> {verdict}")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
