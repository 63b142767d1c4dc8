"""jmt.nn.MultiheadAttention(key_padding_mask=...) against torch.nn.MultiheadAttention on the CPU
in fp32: same weights, a left-padded bool mask (the reference's collate pads short clips on the
left), output and every parameter and input gradient under the objective mean(w * out).

fp32 compute runs the GEMM + range-softmax path at the project's fp32 tolerances (DESIGN.md §2:
rel 1e-4 outputs, 1e-3 gradients); bf16 runs the whole-row kernels at L = 70 and the short ones at
L = 16 under the kernel tolerances of tests/test_gpu_attn_key_ranges.py (outputs 1e-2 max(|ref|,
1); gradients 16 u of the largest reference entry, u = 2^-8).  Without key ranges the module
raised NotImplementedError for any mask."""
import pytest
import torch

from jmt import functional as JF
from jmt import nn as jnn

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H = 512, 1

CASES = [(70, 3, (0, 23, 41)), (16, 4, (0, 5, 15, 9))]      # L, N, left padding per sequence


def _modules(seed):
    g = torch.Generator().manual_seed(seed)
    ref = torch.nn.MultiheadAttention(E, H)
    with torch.no_grad():
        ref.in_proj_weight.copy_(torch.randn(3 * E, E, generator=g) * E ** -0.5)
        ref.in_proj_bias.copy_(torch.randn(3 * E, generator=g) * 0.1)
        ref.out_proj.weight.copy_(torch.randn(E, E, generator=g) * E ** -0.5)
        ref.out_proj.bias.copy_(torch.randn(E, generator=g) * 0.1)
    m = jnn.MultiheadAttention(E, H)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV), g


def _reference(ref, x, w, mask):
    xr = x.clone().requires_grad_(True)
    out, _ = ref(xr, xr, xr, key_padding_mask=mask, need_weights=False)
    (w * out).mean().backward()
    grads = {k: p.grad for k, p in ref.named_parameters()}
    grads["input"] = xr.grad
    return out.detach(), grads


@pytest.mark.parametrize("cd", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("L,N,pads", CASES, ids=["L70", "L16"])
@pytest.mark.parametrize("as_ranges", [False, True], ids=["mask", "ranges"])
def test_mha_key_padding_mask_matches_torch(cd, L, N, pads, as_ranges):
    ref, m, g = _modules(11 + L)
    x = torch.randn(L, N, E, generator=g)
    w = torch.randn(L, N, E, generator=g)
    mask = torch.zeros(N, L, dtype=torch.bool)
    for n, p in enumerate(pads):
        mask[n, :p] = True
    out_r, grads_r = _reference(ref, x, w, mask)

    xd = x.to(DEV).requires_grad_(True)
    with JF.compute_mode(cd):
        kpm = JF.key_ranges(mask.to(DEV)) if as_ranges else mask.to(DEV)
        out, none = m(xd, xd, xd, key_padding_mask=kpm)
        (w.to(DEV) * out.float()).mean().backward()
    torch.cuda.synchronize()
    assert none is None
    grads = {k: p.grad for k, p in m.named_parameters()}
    grads["input"] = xd.grad

    if cd == torch.float32:
        otol = 1e-4 * out_r.abs().max().item()
        grel = 1e-3
    else:
        otol = 1e-2 * max(out_r.abs().max().item(), 1.0)
        grel = 16 * 2.0 ** -8
    oerr = (out.float().cpu() - out_r).abs().max().item()
    print(f"out err {oerr:.3e} tol {otol:.3e}")
    assert oerr <= otol
    for k, gr in grads_r.items():
        err = (grads[k].float().cpu() - gr).abs().max().item()
        tol = grel * gr.abs().max().item()
        print(f"{k} err {err:.3e} tol {tol:.3e}")
        assert err <= tol, k


def test_other_masks_still_raise():
    _, m, g = _modules(3)
    x = torch.randn(16, 2, E, generator=g).to(DEV)
    with pytest.raises(NotImplementedError):
        m(x, x, x, attn_mask=torch.zeros(16, 16, device=DEV))
    with pytest.raises(NotImplementedError):
        m(x, x, x, is_causal=True)
    with pytest.raises(NotImplementedError):       # float key padding masks
        m(x, x, x, key_padding_mask=torch.zeros(2, 16, device=DEV))
    with pytest.raises(ValueError):                # every key of a sequence masked
        m(x, x, x, key_padding_mask=torch.ones(2, 16, dtype=torch.bool, device=DEV))
    JF.check_key_ranges()
