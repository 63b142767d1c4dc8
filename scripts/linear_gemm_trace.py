#!/usr/bin/env python
"""Which GEMM / column-sum / copy launches one training step asks of jmt.ops, and what it
computes — to compare two commits that must launch the same and give the same bits (the
linear-layer GEMM helpers of jmt/linear_gemm.py against the hand-written ones before them).

    python scripts/linear_gemm_trace.py --out RESULT.json [--full DIR]
    python scripts/linear_gemm_trace.py --compare PARENT.json BRANCH.json

Every arm (a model, a compute dtype, a set of environment switches — they are read at import)
is one fresh child process, one after the other, each under its own time limit; the run stops
at the first child that fails.  A child wraps ops.gemm, ops.colsum, ops.colsum_grouped and
ops.copy2d by module attribute and runs one forward + backward of a tests.parity.build_tt model
at (B, T) = (4, 64) — B T a multiple of 64: the K-segment weight gradients apply — and (3, 20).

Per call the trace holds every integer, float and flag argument as it is (defaults filled in),
every pointer / tensor argument as (rank of the address's first appearance in the trace, dtype,
shape), whether `done` was given, `defer`, and the set of address ranks in `keep`.  `ldcin` is
recorded as 0 where no `c_in` is given (ops.gemm reads it with c_in only).  The result file is
one line per arm: a short hash per call (without `keep`), the `keep` sets, the SHA-256 of the
loss and of both predictions, and one SHA-256 over the digests of all parameter gradients (and
which parameters have none); --full DIR also writes the readable traces and every digest.

--compare: the call hashes and the digests must be equal, and every `keep` of the second file a
superset of the first's.  One line per arm; it says so where the calls agree in everything but
the addresses their buffers landed at (a second hash per call masks the ranks), and where the
first file kept a tensor that is no operand (a, b, c, dbias) of its launch.
"""
import argparse
import hashlib
import inspect
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "joint-multimodal-transformer-6th-abaw_amd")
SHAPES = ((4, 64), (3, 20))
FROZEN = ("mm_transformer.physiological_encoder.layers.0.feed_forward.0.bias",
          "mm_transformer.cross_attention_p.in_proj_weight",
          "mm_transformer.out_layer1.bias", "vregressor.3.weight")
SWITCHES = ("JMT_WGRAD_DEFER", "JMT_WGRAD_MERGE", "JMT_FUSED_BGRAD", "JMT_WGRAD_GROUP",
            "JMT_GROUPED", "JMT_FUSED_HEAD")


def arms():
    tf = ("TRANSFORMER", "FC", "bf16")
    out = [("default", *tf, {}, False)]
    out += [(f"{k}={v}", *tf, {k: v}, False) for k, v in (
        ("JMT_WGRAD_DEFER", "0"), ("JMT_WGRAD_DEFER", "single"), ("JMT_WGRAD_MERGE", "0"),
        ("JMT_FUSED_BGRAD", "0"), ("JMT_WGRAD_GROUP", "0"), ("JMT_GROUPED", "0"),
        ("JMT_FUSED_HEAD", "0"))]
    out += [("fp32", "TRANSFORMER", "FC", "fp32", {}, False),
            ("self_atten", "TRANSFORMER", "SELF_ATTEN", "bf16", {}, False),
            ("none_fc", "NONE", "FC", "bf16", {}, False),
            ("fc_fc", "FC", "FC", "bf16", {}, False),
            ("frozen", *tf, {}, True)]
    return out


# ------------------------------------------------------------------------------ child
def child(spec_json: str, out: str) -> None:
    sys.path[:0] = [REPO, PKG]
    import torch
    from jmt import functional as JF, ops
    from tests.parity import build_tt
    from losses.loss import CCCLoss
    name, jm, fmt, cdn, _, frozen = json.loads(spec_json)
    cd = {"bf16": torch.bfloat16, "fp32": torch.float32}[cdn]
    ranks, trace = {}, []

    def rank(addr):
        return None if addr is None else ranks.setdefault(int(addr), len(ranks))

    def norm(k, v):
        if isinstance(v, torch.Tensor):
            return [rank(v.data_ptr()), str(v.dtype), list(v.shape)]
        if isinstance(v, (list, tuple)):
            if k in ("a", "b", "c", "c_in"):
                return [rank(p) for p in v]
            return [norm(k, t) for t in v]
        if k.endswith("_ptr"):
            return rank(v)
        return v

    def wrap(fname):
        orig = getattr(ops, fname)
        sig = inspect.signature(orig)

        def f(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            args = dict(ba.arguments)
            args.pop("device", None)
            done, keep = args.pop("done", None), args.pop("keep", ())
            if "ldcin" in args and args["c_in"] is None:
                args["ldcin"] = 0
            rec = {"fn": fname, "args": {k: norm(k, v) for k, v in args.items()}}
            if fname == "gemm":
                rec["done"] = done is not None
                rec["keep"] = sorted({rank(t.data_ptr()) for t in keep
                                      if isinstance(t, torch.Tensor)})
            trace.append(rec)
            return orig(*a, **kw)

        setattr(ops, fname, f)

    for fname in ("gemm", "colsum", "colsum_grouped", "copy2d"):
        wrap(fname)

    def digest(t):
        t = t.detach().contiguous().cpu()
        if t.dtype == torch.bfloat16:
            t = t.view(torch.int16)
        return hashlib.sha256(t.numpy().tobytes()).hexdigest()

    res = {}
    for B, T in SHAPES:
        m, fc = build_tt({"H": 1, "L": 1, "jm": jm, "fmt": fmt, "vin": 2048})
        named = list(m.named_parameters()) + [("fc." + k, p) for k, p in fc.named_parameters()]
        if frozen:
            left = set(FROZEN)
            for k, p in named:
                if k in left:
                    p.requires_grad_(False)
                    left.discard(k)
            assert not left, left
        g = torch.Generator().manual_seed(3)
        a = torch.randn(B, T, 1024, generator=g).cuda()
        v = torch.randn(B, T, 2048, generator=g).cuda()
        yv = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
        ya = (torch.rand(1, B * T, generator=g) * 2 - 1).cuda()
        crit = CCCLoss(1)
        ranks.clear()
        del trace[:]
        with JF.compute_mode(cd):
            vo, ao = m(fc(a), v)
            loss = crit(vo.reshape(1, -1), yv) + crit(ao.reshape(1, -1), ya)
            loss.backward()
        torch.cuda.synchronize()
        dig = {"loss": digest(loss), "vo": digest(vo), "ao": digest(ao)}
        dig.update({"grad." + k: digest(p.grad) if p.grad is not None else None
                    for k, p in named})
        res[f"{B}x{T}"] = {"trace": list(trace), "digest": dig}
    with open(out, "w") as f:
        json.dump(res, f)


# ------------------------------------------------------------------------------ parent
def _mask(k, v):
    """An argument without its address ranks."""
    if k in ("a", "b", "c", "c_in") and isinstance(v, list):
        return len(v)
    if k.endswith("_ptr"):
        return None
    if isinstance(v, list) and len(v) == 3 and isinstance(v[1], str):       # one tensor
        return v[1:]
    if isinstance(v, list) and k in ("bias_tab", "dbias_tab", "dbs"):
        return [t and t[1:] for t in v]
    return v


def _call_hash(rec, addresses=True) -> str:
    r = {k: v for k, v in rec.items() if k != "keep"}
    if not addresses:       # what is launched, not where its buffers landed
        r["args"] = {k: _mask(k, v) for k, v in r["args"].items()}
    return hashlib.sha256(json.dumps(r, sort_keys=True).encode()).hexdigest()[:8]


def _operand_ranks(rec) -> list:
    flat = lambda v: [r for t in v for r in flat(t)] if isinstance(v, list) else \
        [v] if isinstance(v, int) else []
    return sorted({r for k in ("a", "b", "c", "dbias_tab")
                   for t in rec["args"].get(k) or () for r in flat(t if k != "dbias_tab" else
                                                                    (t or [None])[:1])})


def run(out: str, full: str) -> int:
    results, rc = {}, 0
    tmp = out + ".child"
    for spec in arms():
        name, env_add = spec[0], spec[4]
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(env_add)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child",
                                json.dumps(spec), tmp], env=env, capture_output=True, text=True,
                               timeout=300)
            err = None if r.returncode == 0 else \
                f"exit {r.returncode}: " + (r.stderr.strip().splitlines() or ["?"])[-1]
        except subprocess.TimeoutExpired:
            err = "time limit"
        if err is not None:
            results[name] = {"error": err}
            print(f"{name}: FAILED {err}", flush=True)
            rc = 1
            break
        with open(tmp) as f:
            res = json.load(f)
        os.remove(tmp)
        for shape, d in res.items():
            arm = f"{name} {shape}"
            if full:
                os.makedirs(full, exist_ok=True)
                with open(os.path.join(full, arm.replace(" ", "_") + ".jsonl"), "w") as f:
                    for rec in d["trace"]:
                        f.write(json.dumps(rec, sort_keys=True) + "\n")
                    f.write(json.dumps({"digest": d["digest"]}, sort_keys=True) + "\n")
            queued = [rec for rec in d["trace"] if rec.get("done")]
            dig = d["digest"]
            grads = sorted((k, v) for k, v in dig.items() if k.startswith("grad."))
            results[arm] = {"calls": " ".join(_call_hash(rec) for rec in d["trace"]),
                            "shapes": " ".join(_call_hash(rec, False) for rec in d["trace"]),
                            "keep": [rec["keep"] for rec in queued],
                            "operands": [_operand_ranks(rec) for rec in queued],
                            "digest": {"loss": dig["loss"], "vo": dig["vo"], "ao": dig["ao"],
                                       "grads": hashlib.sha256(json.dumps(grads).encode())
                                       .hexdigest(),
                                       "no_grad": [k[5:] for k, v in grads if v is None]}}
            print(f"{arm}: {len(d['trace'])} calls", flush=True)
    with open(out, "w") as f:       # one line per arm
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: " + json.dumps(v, separators=(",", ":"))
                                  for k, v in sorted(results.items())) + "\n}\n")
    return rc


def compare(pa: str, pb: str) -> int:
    with open(pa) as f:
        A = json.load(f)
    with open(pb) as f:
        Bq = json.load(f)
    bad = 0
    for arm in sorted(set(A) | set(Bq)):
        a, b = A.get(arm), Bq.get(arm)
        if a is None or b is None or "error" in a or "error" in b:
            why = "missing" if a is None or b is None else \
                f"first: {a.get('error', 'ran')}; second: {b.get('error', 'ran')}"
            print(f"{arm}: NOT COMPARED ({why})")
            bad += 1
            continue
        notes, extra = [], []
        for r in (a, b):
            r["calls"], r["shapes"] = r["calls"].split(), r["shapes"].split()
        if a["shapes"] != b["shapes"]:
            i = next((i for i, (x, y) in enumerate(zip(a["shapes"], b["shapes"])) if x != y),
                     min(len(a["shapes"]), len(b["shapes"])))
            notes.append(f"calls differ from #{i} ({len(a['calls'])} vs {len(b['calls'])})")
        elif a["calls"] != b["calls"]:
            i = next(i for i, (x, y) in enumerate(zip(a["calls"], b["calls"])) if x != y)
            extra.append(f"same arguments, but buffers land at other addresses from call #{i}")
        else:
            lost = [set(x) - set(y) for x, y in zip(a["keep"], b["keep"])]
            n = sum(bool(l & set(o)) for l, o in zip(lost, a["operands"]))
            if n:
                notes.append(f"keep lacks operands of {n} of {len(lost)} queued launches")
            elif any(lost):
                extra.append(f"the first also kept {sum(map(len, lost))} tensor(s) that are no "
                             "operand of their launch")
        dd = [k for k in a["digest"] if a["digest"][k] != b["digest"].get(k)]
        if dd:
            notes.append(f"digests differ: {dd}")
        more = sum(len(y) - len(x) for x, y in zip(a["keep"], b["keep"]))
        print(f"{arm}: " + ("; ".join(notes + extra) if notes else "; ".join(
            [f"same {len(a['calls'])} calls, same bits, keep +{max(more, 0)} tensors"] + extra)))
        bad += bool(notes)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--full", default="")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--child", nargs=2)
    ns = ap.parse_args()
    if ns.child:
        child(*ns.child)
    elif ns.compare:
        sys.exit(compare(*ns.compare))
    else:
        sys.exit(run(ns.out, ns.full))
