"""The reference's run configuration (config_file.json schema + parseit.py's command-line override
convention) read into the fusion model, optimizer and window shape this framework trains.

* load(path): the JSON file as the reference reads it (parseit.py:561-575);
* override(cfg, argv): parseit.py:293-345's rules — `--<top-level key>`, `--<model_params key>`
  (including every `opt__*` optimizer key), `--{train,val,test}_params__<key>` (the params dict
  or its loader_params); an unknown key raises as the reference does (ValueError /
  NotImplementedError); values are converted to the type the file holds (bools accept the
  reference's str2bool spellings);
* fusion_model(cfg): Two_transformers built as main.py:473-481 (vision_in_ft = 512: the R2D1 /
  ResNet18 features, main.py:469);
* sgd_kwargs(cfg): the `opt__*` SGD hyper-parameters (instantiator.py:30-36, the reference's
  optimizer for name_optimizer == "sgd"); adam_kwargs(cfg): the Adam ones (instantiator.py:40-46);
* optimizer(cfg, params): (FusedSGD with a device lr | FusedAdam, lr scheduler or None) as
  instantiator.get_optimizer_for_params pairs them; scheduler(cfg, opt) is its second half;
* window(cfg): (batch_size, T) of a training batch: T = seq_length // subseq_length clips.
"""
from __future__ import annotations

import copy
import json
from typing import Dict, List, Sequence, Tuple

_PARAM_SETS = ("train_params", "val_params", "test_params")


def str2bool(v) -> bool:
    """parseit.py:53-63."""
    if isinstance(v, bool):
        return v
    s = str(v).lower()
    if s in ("yes", "true", "t", "y", "1"):
        return True
    if s in ("no", "false", "f", "n", "0"):
        return False
    raise ValueError(f"boolean value expected, got {v!r}")


def load(path: str) -> dict:
    with open(path, "r") as f:
        return json.load(f)


def _convert(old, val: str):
    if isinstance(old, bool):
        return str2bool(val)
    if isinstance(old, int):
        return int(val)
    if isinstance(old, float):
        return float(val)
    return val


def _pairs(argv: Sequence[str]) -> List[Tuple[str, str]]:
    out = []
    i = 0
    while i < len(argv):
        a = argv[i]
        if not a.startswith("--"):
            raise ValueError(f"expected --key, got {a!r}")
        if "=" in a:
            k, v = a[2:].split("=", 1)
            i += 1
        else:
            if i + 1 >= len(argv):
                raise ValueError(f"missing value for {a}")
            k, v = a[2:], argv[i + 1]
            i += 2
        out.append((k, v))
    return out


def override(cfg: dict, argv: Sequence[str]) -> dict:
    """A copy of cfg with parseit.py's `--key value` overrides applied."""
    cfg = copy.deepcopy(cfg)
    for k, v in _pairs(argv):
        if k in cfg and not isinstance(cfg[k], dict):
            cfg[k] = _convert(cfg[k], v)
        elif k in cfg.get("model_params", {}):
            cfg["model_params"][k] = _convert(cfg["model_params"][k], v)
        elif any(k.startswith(s + "__") for s in _PARAM_SETS):
            s, sub = k.split("__", 1)
            params = cfg[s]
            if sub in params and not isinstance(params[sub], dict):
                params[sub] = _convert(params[sub], v)
            elif sub in params.get("loader_params", {}):
                params["loader_params"][sub] = _convert(params["loader_params"][sub], v)
            else:
                raise NotImplementedError(f"Unknown key {k}")
        else:
            raise ValueError(f"Key {k} was not found in args. ... [NOT OK]")
    return cfg


def fusion_model(cfg: dict, vision_in_ft: int = 512, **kw):
    """main.py:473-481.  An optional `attn_dropout` (not in the reference's file) sets dropout
    on the attention probabilities of every attention module (jmt.nn.set_attention_dropout);
    absent means 0."""
    from models.two_transformers import Two_transformers
    from .nn import set_attention_dropout
    mp = cfg["model_params"]
    model = Two_transformers(v_dropout=float(mp["v_dropout"]), a_dropout=float(mp["a_dropout"]),
                             num_heads=int(mp["num_heads"]), num_layers=int(mp["num_layers"]),
                             joint_modalities=mp["joint_modalities"],
                             output_format=mp["output_format"], vision_in_ft=vision_in_ft, **kw)
    p = float(mp.get("attn_dropout") or 0.0)
    if p != 0.0:
        set_attention_dropout(model, p)
    return model


def sgd_kwargs(cfg: dict) -> Dict[str, float]:
    mp = cfg["model_params"]
    name = str(mp.get("opt__name_optimizer", "sgd")).lower()
    if name != "sgd":
        raise NotImplementedError(f"opt__name_optimizer {name!r}: the fused optimizer is SGD")
    return dict(lr=float(mp["opt__lr"]), momentum=float(mp["opt__momentum"]),
                dampening=float(mp["opt__dampening"]),
                weight_decay=float(mp["opt__weight_decay"]),
                nesterov=str2bool(mp["opt__nesterov"]))


def adam_kwargs(cfg: dict) -> dict:
    """The `opt__*` Adam hyper-parameters (instantiator.py:40-46)."""
    mp = cfg["model_params"]
    return dict(lr=float(mp["opt__lr"]), betas=(float(mp["opt__beta1"]), float(mp["opt__beta2"])),
                eps=float(mp["opt__eps_adam"]), weight_decay=float(mp["opt__weight_decay"]),
                amsgrad=str2bool(mp["opt__amsgrad"]))


def _need(mp: dict, key: str, what: str):
    if key not in mp:
        raise KeyError(f"{key} (model_params) is required by {what}")
    return mp[key]


def scheduler(cfg: dict, opt):
    """The lr scheduler of instantiator.py:52-107 on `opt` (anything with get_lr / set_lr), or
    None when `opt__lr_scheduler` is off.  `mycosine` needs `opt__coef` (not in the shipped
    file) and `max_epochs`, `multistep` needs `opt__milestones`: KeyError naming the key."""
    from . import lr_scheduler as S
    mp = cfg["model_params"]
    if not str2bool(mp.get("opt__lr_scheduler", False)):
        return None
    name = str(mp["opt__name_lr_scheduler"]).lower()
    last = int(mp.get("opt__last_epoch", -1))
    what = f"opt__name_lr_scheduler {name!r}"
    if name == "step":
        return S.StepLR(opt, step_size=int(_need(mp, "opt__step_size", what)),
                        gamma=float(_need(mp, "opt__gamma", what)), last_epoch=last)
    if name == "cosine":
        return S.CosineAnnealingLR(opt, T_max=int(_need(mp, "opt__t_max", what)),
                                   eta_min=float(_need(mp, "opt__min_lr", what)), last_epoch=last)
    if name == "mystep":
        return S.MyStepLR(opt, step_size=int(_need(mp, "opt__step_size", what)),
                          gamma=float(_need(mp, "opt__gamma", what)), last_epoch=last,
                          min_lr=float(_need(mp, "opt__min_lr", what)))
    if name == "mycosine":
        return S.MyCosineLR(opt, coef=float(_need(mp, "opt__coef", what)),
                            max_epochs=int(_need(mp, "max_epochs", what)),
                            min_lr=float(_need(mp, "opt__min_lr", what)), last_epoch=last)
    if name == "multistep":
        return S.MultiStepLR(opt, milestones=_need(mp, "opt__milestones", what),
                             gamma=float(_need(mp, "opt__gamma", what)), last_epoch=last)
    if name == "reduce_on_plateau":
        raise NotImplementedError("opt__name_lr_scheduler 'reduce_on_plateau': a schedule driven "
                                  "by the validation metric is not implemented")
    raise ValueError(f"opt__name_lr_scheduler {name!r} is not one of step, cosine, mystep, "
                     "mycosine, multistep")


def optimizer(cfg: dict, params, **kw):
    """(optimizer, scheduler or None) as instantiator.get_optimizer_for_params builds them:
    FusedSGD with the lr on the device (so the schedule reaches a captured step) or FusedAdam by
    `opt__name_optimizer`, the scheduler by `opt__lr_scheduler` / `opt__name_lr_scheduler`.  kw
    goes to the optimizer (shadow_dtype, fuse_zero_grad, max_grad_norm).  An optional
    `opt__clip_grad_norm` (not in the reference's file) turns gradient-norm clipping on at that
    threshold; absent or <= 0 is off, and an explicit max_grad_norm keyword wins."""
    from . import optim
    if "max_grad_norm" not in kw:
        clip = cfg["model_params"].get("opt__clip_grad_norm")
        if clip is not None and float(clip) > 0:
            kw["max_grad_norm"] = float(clip)
    name = str(cfg["model_params"].get("opt__name_optimizer", "sgd")).lower()
    if name == "sgd":
        opt = optim.FusedSGD(params, device_lr=True, **sgd_kwargs(cfg), **kw)
    elif name == "adam":
        opt = optim.FusedAdam(params, **adam_kwargs(cfg), **kw)
    else:
        raise ValueError(f"opt__name_optimizer {name!r} is neither 'sgd' nor 'adam'")
    return opt, scheduler(cfg, opt)


def window(cfg: dict, split: str = "train_params") -> Tuple[int, int]:
    p = cfg[split]
    return int(p["loader_params"]["batch_size"]), int(p["seq_length"]) // int(p["subseq_length"])
