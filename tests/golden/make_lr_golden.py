"""Generate tests/golden/lr_sched.json by running the REFERENCE's own lr schedulers on CPU.

Run in the build container (where /root/reference exists):
    python tests/golden/make_lr_golden.py

The reference's my_lr_scheduler (MyStepLR, MyCosineLR) is imported with bytecode writing disabled
and stepped on a torch.optim.SGD dummy; for each case the lr right after construction and after
each of N scheduler.step() calls is recorded (repr-exact floats).  The reference's sources never
leave this script: the fixture is data (the recorded learning rates and the arguments that
produced them)."""
from __future__ import annotations

import json
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

CASES = [
    # the shipped configuration: the clamp engages at epoch 160
    dict(name="mystep_shipped", cls="MyStepLR", base_lr=1e-4, epochs=200,
         kwargs=dict(step_size=40, gamma=0.1, min_lr=1e-7)),
    dict(name="mystep_3", cls="MyStepLR", base_lr=1e-4, epochs=20,
         kwargs=dict(step_size=3, gamma=0.1, min_lr=1e-7)),
    # the clamp engages at epoch 21
    dict(name="mycosine", cls="MyCosineLR", base_lr=1e-4, epochs=25,
         kwargs=dict(coef=0.5, max_epochs=20, min_lr=1e-7)),
]


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    import my_lr_scheduler as ref
    out = []
    for case in CASES:
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=case["base_lr"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")        # scheduler.step() before optimizer.step()
            sched = getattr(ref, case["cls"])(opt, **case["kwargs"])
            lrs = [opt.param_groups[0]["lr"]]
            for _ in range(case["epochs"]):
                opt.step()
                sched.step()
                lrs.append(opt.param_groups[0]["lr"])
        out.append(dict(case, lrs=lrs))
    path = os.path.join(HERE, "lr_sched.json")
    with open(path, "w") as f:
        json.dump({"torch": torch.__version__, "cases": out}, f, indent=1)
        f.write("\n")
    print(f"wrote {path}: " + ", ".join(f"{c['name']} ({len(c['lrs'])} values)" for c in out))


if __name__ == "__main__":
    main()
