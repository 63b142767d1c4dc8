"""What gradient-norm clipping costs (csrc/grad_norm.hip), two measurements in one process:

1. the norm pass (jmt_grad_norm: the read-only pass + the one-block fold, per-parameter segments
   as FusedSGD / FusedAdam pass them) against jmt_amp_check, the library's other read-only pass
   over the same flat gradient buffer, at the flagship model's parameter count, alternated;
   bytes are the buffer read once (4 B per element);
2. the graph-replayed c3-shaped training step (bf16, B = 64, T = 300, FusedSGD with the lr on the
   device and fuse_zero_grad) with max_grad_norm=None against max_grad_norm=1.0, alternated.

    python scripts/bench_grad_norm.py [--n 13400064] [--nseg 100] [--sets 1] [--rounds 7]
                                      [--reps 50] [--no-step] [--out profiles/grad_norm.txt]
--sets K rotates the launches over K buffers: at K = 1 the 54 MB buffer stays in the 256 MB
Infinity Cache from one launch to the next (as it does in the step, where the backward has just
written it); K = 8 puts it out of the cache's reach.  Warm-up launches first; each round times
`reps` launches between one event pair per kernel, order swapped every round; median and
min..max over the rounds are printed."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")]

import torch  # noqa: E402

from jmt import _lib, ops  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps          # seconds per call


def alternate(cases, rounds, reps, warm=10):
    for fn in cases.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in cases}
    for r in range(rounds):
        for k in (list(cases) if r % 2 == 0 else list(cases)[::-1]):
            t[k].append(timed(cases[k], reps))
    return t


def norm_vs_check(args, lines):
    n, K = args.n, args.sets
    gen = torch.Generator(device=DEV).manual_seed(0)
    bufs = [torch.randn(n, device=DEV, generator=gen) for _ in range(K)]
    # segments like a model's: a few large matrices and many small vectors, 64-element aligned
    nseg = args.nseg
    cuts = sorted({(i * (n // 64) // nseg) * 64 for i in range(nseg)} | {0})
    off = torch.tensor(cuts + [n], dtype=torch.int64, device=DEV)
    nseg = len(cuts)
    seg_norm = torch.zeros(nseg, device=DEV)
    nbytes = _lib.load().jmt_grad_norm_scratch(n, nseg)
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    state = torch.tensor([1e-4, 0, 0, 0, 0, 0, 1.0, 0], dtype=torch.float32, device=DEV)
    amp = torch.tensor([1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=DEV)
    s = ops.stream()
    turn = [0, 0, 0]

    def norm_seg():
        g = bufs[turn[0] % K]
        turn[0] += 1
        _lib.call("jmt_grad_norm", n, g.data_ptr(), state.data_ptr(), scratch.data_ptr(), nbytes,
                  off.data_ptr(), nseg, seg_norm.data_ptr(), 1.0, None, s)

    def norm_flat():
        g = bufs[turn[1] % K]
        turn[1] += 1
        _lib.call("jmt_grad_norm", n, g.data_ptr(), state.data_ptr(), scratch.data_ptr(), nbytes,
                  None, 0, None, 1.0, None, s)

    def check():
        g = bufs[turn[2] % K]
        turn[2] += 1
        _lib.call("jmt_amp_check", n, g.data_ptr(), amp.data_ptr(), s)

    t = alternate({"grad_norm": norm_seg, "grad_norm_noseg": norm_flat, "amp_check": check},
                  args.rounds, args.reps)
    lines.append(f"norm pass vs finiteness check: n = {n} fp32 ({4 * n / 1e6:.1f} MB), {nseg} "
                 f"segments, {K} buffer set(s), {args.rounds} rounds x {args.reps} launches, "
                 f"alternated; {torch.cuda.get_device_name(0)}")
    for k, v in t.items():
        med = statistics.median(v)
        lines.append(f"  {k:16s} median {med * 1e6:7.2f} us  ({4 * n / med / 1e12:.2f} TB/s)  min "
                     f"{min(v) * 1e6:.2f}  max {max(v) * 1e6:.2f} us")
    r = [a / b for a, b in zip(t["grad_norm"], t["amp_check"])]
    lines.append(f"  grad_norm / amp_check per round: " + " ".join(f"{x:.2f}" for x in r) +
                 f"  (median {statistics.median(r):.2f})")


def clipped_vs_unclipped_step(args, lines):
    from jmt import functional as JF
    from jmt.graph import GraphedStep
    from jmt.optim import FusedSGD, used_parameters
    from losses.loss import CCCLoss
    from models.fc_layer import FcLayer
    from models.two_transformers import Two_transformers
    B, T, cd = args.batch, args.seq, torch.bfloat16

    def build(max_grad_norm):
        torch.manual_seed(0)
        model = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", "FC", 2048).to(DEV)
        fc = FcLayer(1024, 512).to(DEV)
        gen = torch.Generator(device=DEV).manual_seed(1)
        audio = torch.randn(B, T, 1024, device=DEV, generator=gen)
        video = torch.randn(B, T, 2048, device=DEV, generator=gen)
        lv = (torch.rand(B, T, device=DEV, generator=gen) * 2 - 1).view(-1, B * T)
        la = (torch.rand(B, T, device=DEV, generator=gen) * 2 - 1).view(-1, B * T)
        crit = CCCLoss(1)
        one = torch.ones((), dtype=torch.float32, device=DEV)

        def fwd_bwd():
            with JF.compute_mode(cd):
                vo, ao = model(fc(audio), video)
                l1 = crit(vo.view(-1, B * T), lv)
                loss = crit.forward_add(ao.view(-1, B * T), la, l1)
                loss.backward(one)
            return loss

        params = used_parameters(fwd_bwd, list(model.parameters()) + list(fc.parameters()))
        opt = FusedSGD(params, lr=1e-4, momentum=0.9, dampening=0.0, weight_decay=1e-4,
                       nesterov=True, shadow_dtype=cd, fuse_zero_grad=True, device_lr=True,
                       max_grad_norm=max_grad_norm)

        def step():
            opt.zero_grad()
            loss = fwd_bwd()
            opt.step()
            return loss

        for _ in range(3):
            step()
        return GraphedStep(step).capture(warmup=1), opt

    ga, oa = build(None)
    gb, ob = build(1.0)
    t = alternate({"max_grad_norm=None": ga.replay, "max_grad_norm=1.0": gb.replay},
                  args.rounds, args.step_reps, warm=5)
    lines.append(f"graph-replayed step, bf16, B = {B}, T = {T}, FusedSGD(device_lr, "
                 f"fuse_zero_grad), {oa.numel} parameters in {len(oa.params)} tensors: "
                 f"{args.rounds} rounds x {args.step_reps} replays, alternated")
    for k, v in t.items():
        med = statistics.median(v)
        lines.append(f"  {k:20s} median {med * 1e3:.4f} ms/step  min {min(v) * 1e3:.4f}  max "
                     f"{max(v) * 1e3:.4f}")
    d = [b - a for a, b in zip(t["max_grad_norm=None"], t["max_grad_norm=1.0"])]
    lines.append(f"  clipped - unclipped per round (us): " + " ".join(f"{x * 1e6:.1f}" for x in d) +
                 f"  (median {statistics.median(d) * 1e6:.1f}; last norm "
                 f"{float(ob.grad_norm()):.4g}, coefficient {float(ob.clip_coef()):.4g})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=13_400_064)
    ap.add_argument("--nseg", type=int, default=100)
    ap.add_argument("--sets", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=300)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.load()
    lines = []
    norm_vs_check(args, lines)
    if not args.no_step:
        clipped_vs_unclipped_step(args, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
