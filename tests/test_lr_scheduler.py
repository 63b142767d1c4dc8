"""jmt.lr_scheduler (host only) against the reference's recorded schedules
(tests/golden/lr_sched.json, written by tests/golden/make_lr_golden.py from the reference's
MyStepLR / MyCosineLR) and against torch's own schedulers stepped live, plus the optimizer /
scheduler factory of jmt.config.  No GPU and no library: the schedulers drive a stub with
set_lr / get_lr."""
import copy
import json
import os
import warnings

import pytest
import torch

from jmt import config
from jmt import lr_scheduler as S

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lr_sched.json")
CFG = os.path.join(HERE, "golden", "config_file.json")


class StubOpt:
    def __init__(self, lr):
        self.lr = lr
        self.calls = 0

    def set_lr(self, lr):
        self.lr = lr
        self.calls += 1

    def get_lr(self):
        return self.lr


def _run(sched, opt, epochs):
    lrs = [opt.get_lr()]
    for _ in range(epochs):
        sched.step()
        lrs.append(opt.get_lr())
    return lrs


def _cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_reference_schedules_reproduced(case):
    opt = StubOpt(case["base_lr"])
    sched = getattr(S, case["cls"])(opt, **case["kwargs"])
    got = _run(sched, opt, case["epochs"])
    want = case["lrs"]
    assert len(got) == len(want) == case["epochs"] + 1
    for e, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-12 * abs(b), (case["name"], e, a, b)
    assert sched.get_last_lr() == [got[-1]] and sched.last_epoch == case["epochs"]


def test_recorded_landmarks():
    """The fixture holds what the issue quotes: the shipped mystep clamps at epoch 160 and sits
    one ulp above the clamp at 120; mycosine moves at construction and clamps at epoch 21."""
    by = {c["name"]: c["lrs"] for c in _cases()}
    ms = by["mystep_shipped"]
    assert ms[0] == 1e-4 and ms[120] == 1.0000000000000002e-07 and ms[159] > 1e-7
    assert ms[160] == 1e-7 and ms[200] == 1e-7
    mc = by["mycosine"]
    assert mc[0] != 1e-4 and mc[20] > 1e-7 and mc[21] == 1e-7


def _torch_run(make, epochs, base=1e-2):
    p = torch.nn.Parameter(torch.zeros(1))
    topt = torch.optim.SGD([p], lr=base)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ts = make(topt)
        lrs = [topt.param_groups[0]["lr"]]
        for _ in range(epochs):
            topt.step()
            ts.step()
            lrs.append(topt.param_groups[0]["lr"])
    return lrs


TL = torch.optim.lr_scheduler


@pytest.mark.parametrize("name,mine,theirs,rel,absol", [
    ("step", lambda o: S.StepLR(o, step_size=7, gamma=0.3),
     lambda o: TL.StepLR(o, step_size=7, gamma=0.3), 1e-9, 0.0),
    ("multistep", lambda o: S.MultiStepLR(o, milestones=[4, 9, 9, 21], gamma=0.5),
     lambda o: TL.MultiStepLR(o, milestones=[4, 9, 9, 21], gamma=0.5), 1e-9, 0.0),
    # torch's cosine is recursive: it differs from the closed form in the last bits, and past
    # T_max (12 < 30 epochs) it comes back up, as the closed form does
    ("cosine", lambda o: S.CosineAnnealingLR(o, T_max=12, eta_min=1e-5),
     lambda o: TL.CosineAnnealingLR(o, T_max=12, eta_min=1e-5), 1e-6, 1e-12),
    ("cosine_long", lambda o: S.CosineAnnealingLR(o, T_max=100, eta_min=1e-7),
     lambda o: TL.CosineAnnealingLR(o, T_max=100, eta_min=1e-7), 1e-6, 1e-12),
], ids=lambda v: v if isinstance(v, str) else None)
def test_matches_torch_schedulers(name, mine, theirs, rel, absol):
    opt = StubOpt(1e-2)
    got = _run(mine(opt), opt, 30)
    want = _torch_run(theirs, 30)
    for e, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= max(rel * abs(b), absol), (name, e, a, b)


@pytest.mark.parametrize("make", [
    lambda o: S.MyStepLR(o, step_size=3, gamma=0.1, min_lr=1e-7),
    lambda o: S.MyCosineLR(o, coef=0.5, max_epochs=20, min_lr=1e-7),
    lambda o: S.MultiStepLR(o, milestones=[2, 11], gamma=0.2),
], ids=["mystep", "mycosine", "multistep"])
def test_state_dict_round_trip_resumes(make):
    a = StubOpt(1e-4)
    sa = make(a)
    _run(sa, a, 9)
    sd = copy.deepcopy(sa.state_dict())
    assert "opt" not in sd
    rest = _run(sa, a, 12)[1:]
    b = StubOpt(1e-4)                      # a fresh optimizer and scheduler, then resume
    sb = make(b)
    sb.load_state_dict(sd)
    assert b.get_lr() == sd["_last_lr"] and sb.last_epoch == 9
    assert _run(sb, b, 12)[1:] == rest


def test_construction_performs_the_initial_step():
    o = StubOpt(1e-4)
    s = S.MyStepLR(o, step_size=40, gamma=0.1, min_lr=1e-7)
    assert o.calls == 1 and s.last_epoch == 0 and o.get_lr() == 1e-4 and s.base_lr == 1e-4


# ------------------------------------------------------------------ the config factory

def _cfg(**mp):
    cfg = config.load(CFG)
    cfg["model_params"].update(mp)
    return cfg


def test_shipped_config_yields_mystep():
    o = StubOpt(1e-4)
    s = config.scheduler(config.load(CFG), o)
    assert type(s) is S.MyStepLR
    assert (s.step_size, s.gamma, s.min_lr) == (40, 0.1, 1e-7)
    assert s.base_lr == 1e-4 and s.last_epoch == 0


def test_optimizer_factory_pairs_optimizer_and_scheduler(monkeypatch):
    from jmt import optim
    made = []

    class Fake(StubOpt):
        def __init__(self, params, lr, **kw):
            super().__init__(lr)
            made.append((type(self).__name__, params, kw))

    class FakeSGD(Fake):
        pass

    class FakeAdam(Fake):
        pass

    monkeypatch.setattr(optim, "FusedSGD", FakeSGD)
    monkeypatch.setattr(optim, "FusedAdam", FakeAdam)
    opt, sched = config.optimizer(config.load(CFG), ["p"], fuse_zero_grad=True)
    assert isinstance(opt, FakeSGD) and type(sched) is S.MyStepLR and sched.opt is opt
    name, params, kw = made[-1]
    assert params == ["p"] and kw == dict(device_lr=True, momentum=0.9, dampening=0.0,
                                          weight_decay=1e-4, nesterov=True, fuse_zero_grad=True)
    opt, sched = config.optimizer(_cfg(opt__name_optimizer="adam", opt__lr_scheduler="False"),
                                  ["p"])
    assert isinstance(opt, FakeAdam) and sched is None
    assert made[-1][2] == dict(betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, amsgrad=False)
    with pytest.raises(ValueError, match="rmsprop"):
        config.optimizer(_cfg(opt__name_optimizer="rmsprop"), ["p"])


def test_adam_kwargs_parses_the_shipped_keys():
    kw = config.adam_kwargs(config.load(CFG))
    assert kw == dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, amsgrad=False)
    assert config.adam_kwargs(_cfg(opt__amsgrad="yes", opt__beta2=0.98))["amsgrad"] is True


def test_every_scheduler_name():
    o = StubOpt(1e-4)
    assert type(config.scheduler(_cfg(opt__name_lr_scheduler="step"), o)) is S.StepLR
    s = config.scheduler(_cfg(opt__name_lr_scheduler="cosine"), StubOpt(1e-4))
    assert type(s) is S.CosineAnnealingLR and (s.T_max, s.eta_min) == (100, 1e-7)
    s = config.scheduler(_cfg(opt__name_lr_scheduler="mycosine", opt__coef=0.5), StubOpt(1e-4))
    assert type(s) is S.MyCosineLR and (s.coef, s.max_epochs, s.min_lr) == (0.5, 20.0, 1e-7)
    s = config.scheduler(_cfg(opt__name_lr_scheduler="multistep", opt__milestones=[30, 10]),
                         StubOpt(1e-4))
    assert type(s) is S.MultiStepLR and s.milestones == [10, 30]
    assert config.scheduler(_cfg(opt__lr_scheduler="False"), o) is None


def test_unknown_and_unsupported_names_raise():
    with pytest.raises(ValueError, match="warmup"):
        config.scheduler(_cfg(opt__name_lr_scheduler="warmup"), StubOpt(1e-4))
    with pytest.raises(NotImplementedError, match="reduce_on_plateau"):
        config.scheduler(_cfg(opt__name_lr_scheduler="reduce_on_plateau"), StubOpt(1e-4))


def test_mycosine_without_coef_raises_keyerror():
    with pytest.raises(KeyError, match="opt__coef"):
        config.scheduler(_cfg(opt__name_lr_scheduler="mycosine"), StubOpt(1e-4))
    with pytest.raises(KeyError, match="opt__milestones"):
        config.scheduler(_cfg(opt__name_lr_scheduler="multistep"), StubOpt(1e-4))
