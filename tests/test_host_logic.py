"""Host-side logic of the drop-in modules that needs no GPU: module/class identity, constructor
signatures, state_dict keys and shapes identical to the reference, layout bookkeeping."""
import inspect
import os

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import pytest
import torch

from jmt import functional as F
from jmt import dist as jdist
from oracle import jmt_ref as R


def _keys_shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("jm,fmt,vin,L", [("TRANSFORMER", "FC", 2048, 1),
                                          ("TRANSFORMER", "SELF_ATTEN", 2048, 2),
                                          ("NONE", "FC", 2048, 1), ("FC", "FC", 512, 1)])
def test_two_transformers_state_dict_matches_reference(jm, fmt, vin, L):
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, 1, L, jm, fmt, vin)
    assert _keys_shapes(m) == R.two_transformers_shapes(L, jm, fmt, vin)


def test_golden_key_sets_cover_our_params(golden):
    from models.two_transformers import Two_transformers
    m = Two_transformers(0.0, 0.0, 8, 2, "TRANSFORMER", "FC", 2048)
    gkeys = {k.split("/", 1)[1].rsplit(":", 1)[0] for k in golden
             if k.startswith("tr_fc_h8l2/") and k.endswith(":norm")}
    ours = set(m.state_dict())
    assert ours <= gkeys


def test_intra_modal_state_dict():
    from models.intra_modal_transformer_fusion import Intra_modal_transformer_fusion
    m = Intra_modal_transformer_fusion(512, 1, 512, 1)
    assert _keys_shapes(m) == R.intra_modal_shapes(512, 1)


def test_constructor_signatures_match_reference():
    from models.two_transformers import Two_transformers
    from models.mm_multi_transformers import MultimodalTransformer_w_JR, FeatureConcatFC
    from models.mm_transformers import MultimodalTransformer_wo_JR
    from models.intra_modal_transformer_fusion import Intra_modal_transformer_fusion
    from models.fc_layer import FcLayer
    from losses.loss import CCCLoss, CELoss, CCC_CE_Loss
    from losses.CCCLoss import CCCLoss as CCCLossIgnore
    sig = lambda c: list(inspect.signature(c.__init__).parameters)[1:]
    # the reference's positional parameters in order; the one extra (digitize_num: configs[4]'s
    # expression-style head) comes after them with a default that keeps the reference behaviour
    assert sig(Two_transformers) == ["v_dropout", "a_dropout", "num_heads", "num_layers",
                                     "joint_modalities", "output_format", "vision_in_ft",
                                     "digitize_num"]
    assert inspect.signature(Two_transformers.__init__).parameters["digitize_num"].default == 1
    assert sig(MultimodalTransformer_w_JR) == ["visual_dim", "audio_dim", "num_heads",
                                               "hidden_dim", "num_layers", "output_format"]
    assert sig(MultimodalTransformer_wo_JR) == sig(MultimodalTransformer_w_JR)
    assert sig(FeatureConcatFC) == ["visual_dim", "audio_dim"]
    assert sig(Intra_modal_transformer_fusion) == ["feat_dim", "num_heads", "hidden_dim",
                                                   "num_layers", "reduce_dim_for_audio"]
    assert sig(FcLayer) == ["input_dim", "output_dim"]
    assert sig(CCCLoss) == ["digitize_num", "range", "eps"]
    assert sig(CELoss) == ["digitize_num", "range", "weights"]
    assert sig(CCC_CE_Loss) == ["digitize_num", "range", "alpha", "beta"]
    assert sig(CCCLossIgnore) == ["ignore"]


def test_constructor_asserts_like_reference():
    from models.two_transformers import Two_transformers
    with pytest.raises(AssertionError):
        Two_transformers(0, 0.0, 1, 1, "TRANSFORMER")        # v_dropout must be a float
    with pytest.raises(AssertionError):
        Two_transformers(0.0, 0.0, 1, 1, "BOGUS")
    with pytest.raises(AssertionError):
        Two_transformers(0.0, 0.0, 1, 1, "NONE", "SELF_ATTEN")


def test_hash_init_applies_to_our_modules():
    from models.two_transformers import Two_transformers
    from oracle.hashinit import init_module_, param_value
    m = Two_transformers(0.0, 0.0, 1, 1, "TRANSFORMER", "FC", 2048)
    init_module_(m, "")
    w = m.mm_transformer.out_layer1.weight.detach().numpy()
    assert (w == param_value("mm_transformer.out_layer1.weight", w.shape)).all()


def test_rows_layout_of_permuted_views():
    x = torch.zeros(4, 7, 16)          # (B, T, E) memory
    v = x.permute(1, 0, 2)             # (T, B, E) seq-first view
    L = F.Rows(v)
    assert L.rows == 28 and L.ld == 16 and L.perm == [1, 0] and L.t.data_ptr() == x.data_ptr()
    y = L.like(8, torch.float32)
    assert y.shape == (7, 4, 8) and y.permute(1, 0, 2).is_contiguous()
    # (S, B*T, E) view of a (B*T, S, E) buffer (the SELF_ATTEN stack) and its last-token slice
    buf = torch.zeros(6, 3, 16)
    s = buf.permute(1, 0, 2)
    last = s[-1:]
    Ll = F.Rows(last)
    assert Ll.rows == 6 and Ll.ld == 48
    # a non-collapsible view falls back to a copy
    assert F.Rows(torch.zeros(4, 6, 16)[:, ::2]).ld == 32   # uniform row stride: no copy
    nc = torch.zeros(4, 6, 16)[:, :3]
    Ln = F.Rows(nc)
    assert Ln.ld == 16 and Ln.t.is_contiguous()


def test_shard_range_matches_dataparallel_scatter():
    # torch.nn.DataParallel scatters dim 0 in chunks of ceil(B / g)
    for B, g in [(64, 8), (64, 3), (10, 4)]:
        chunks = torch.arange(B).chunk(g)
        for r in range(g):
            lo, hi = jdist.shard_range(B, r, g)
            ref = chunks[r] if r < len(chunks) else torch.arange(0)
            assert list(range(lo, hi)) == ref.tolist()


def test_compute_dtype_policy():
    assert F.compute_dtype() == torch.float32
    with F.compute_mode(torch.bfloat16):
        assert F.compute_dtype() == torch.bfloat16
    assert F.compute_dtype() == torch.float32


def test_bench_synthetic_batches_identical_across_world_sizes():
    """bench.py's per-global-window generators: 2 ranks x 3 windows == 1 rank x 6 windows."""
    import importlib
    import sys
    sys.path.insert(0, REPO_ROOT)
    bench = importlib.import_module("bench")
    one = bench.synthetic_batch(6, 5, 8, 16, 0, "cpu")
    two = [bench.synthetic_batch(3, 5, 8, 16, r, "cpu") for r in range(2)]
    for k in range(2):                                    # audio, video
        assert torch.equal(one[k], torch.cat([two[0][k], two[1][k]], 0))
    for k in range(2, 4):                                 # labels (1, B*T)
        assert torch.equal(one[k].view(6, 5), torch.cat([t[k].view(3, 5) for t in two], 0))


def test_attn_plan_table():
    """functional.attn_plan (no GPU, no tensors): one row per forward path, per backward path,
    per reason to leave the default backward and per switch; the shared-query answer for the
    CrossAttention6 layout.  Operands as (aligned, row stride): q / dq in a packed (L, N, 3E)
    buffer, k / v / dk / dv in a packed (L, N, 2E) one, o / dO (L, N, E)."""
    from jmt import _lib, ops
    from jmt.functional import AttnOperand as Op, AttnPlan, attn_plan
    bf, f32, E = torch.bfloat16, torch.float32, 512
    lib = _lib.load()

    def plan(cd, Lq, Lk, N, fwd=None, grads=True, **kw):
        d = dict(q=Op(True, 3 * E), k=Op(True, 2 * E), v=Op(True, 2 * E), o=Op(True, E))
        if grads:
            d.update(go=Op(True, E), dq=Op(True, 3 * E), dk=Op(True, 2 * E), dv=Op(True, 2 * E))
        d.update(kw)
        return attn_plan(cd, N, 1, Lq, Lk, E, fwd=fwd, **d)

    sl = (1 << 23) + 1024                      # 128 rows x sl x 2 B > 2 GiB
    assert plan(bf, 6, 6, 3) == AttnPlan("small", False, "small", False)
    assert plan(bf, 20, 32, 2) == AttnPlan("short", False, "short", False)
    assert plan(bf, 64, 64, 1) == AttnPlan("fused", False, "pds_dkdv", False)
    assert plan(bf, 65, 33, 2) == AttnPlan("fused", True, "pds_dkdv", True)
    assert plan(bf, 65, 33, 2, grads=False) == AttnPlan("fused", True, None, False)
    assert plan(f32, 6, 6, 3) == AttnPlan("small", False, "small", False)
    # reasons to leave the default backward
    assert plan(bf, 65, 33, 2, dq=Op(False, 3 * E)) == AttnPlan("fused", True, "bwd64_dkdv", False)
    assert plan(bf, 65, 33, 2, k=Op(False, 2 * E)) == AttnPlan("fused", True, "bwd64_dkdv", False)
    assert plan(bf, 65, 33, 2, dk=Op(False, 2 * E)) == AttnPlan("fused", True, "bwd64_gemm", False)
    assert plan(bf, 70, 129, 1, dk=Op(True, sl), dv=Op(True, sl)) == \
        AttnPlan("fused", True, "bwd64_gemm", False)
    # (Lq + 128) x ldp 16-bit values reach 1 GiB: no P / dS kernel; at Lq = 32768 the Lq rows
    # of P reach 2 GiB as well: no attn_dkdv either
    assert plan(bf, 16384, 32768, 1) == AttnPlan("fused", True, "bwd64_dkdv", False)
    assert plan(bf, 32768, 32768, 1) == AttnPlan("fused", True, "bwd64_gemm", False)
    assert plan(f32, 65, 33, 2) == AttnPlan("gemm", False, "gemm", False)
    # a misaligned source leaves the small / short kernels
    assert plan(bf, 6, 6, 3, q=Op(False, 3 * E)).fwd == "fused"
    assert plan(bf, 20, 32, 2, v=Op(False, 2 * E)).fwd == "fused"
    # the switches, read at every call
    for sw, args, want in (
            (ops._attn_fused, (bf, 65, 33, 2), AttnPlan("gemm", False, "gemm", False)),
            (ops._attn_fused, (bf, 6, 6, 3), AttnPlan("gemm", False, "gemm", False)),
            (ops._attn_short, (bf, 20, 32, 2), AttnPlan("fused", False, "pds_dkdv", False)),
            (ops._attn_dkdv, (bf, 65, 33, 2), AttnPlan("fused", True, "bwd64_gemm", False)),
            (ops._attn_pds, (bf, 65, 33, 2), AttnPlan("fused", True, "bwd64_dkdv", False))):
        sw["on"] = False
        try:
            assert plan(*args) == want, (args, plan(*args))
            # the backward of a forward that ran fused stays on the fused kernels' state
            if sw is ops._attn_fused:
                assert plan(*args, fwd="fused").bwd == "pds_dkdv"
        finally:
            sw["on"] = True
    lib.jmt_attn_set_fwd_rows(0)
    try:
        assert plan(bf, 65, 33, 2) == AttnPlan("fused", False, "pds_dkdv", False)
    finally:
        lib.jmt_attn_set_fwd_rows(-1)
    assert plan(bf, 65, 33, 2) == AttnPlan("fused", True, "pds_dkdv", True)
    # CrossAttention6 (B = 1): six sequences of T rows in one packed (6, T, 3E) buffer, dQKV laid
    # out like it, dO batch-major with row stride E
    for T, want in ((65, True), (64, False)):
        q, k, v = (Op(True, 3 * E),) * 3
        od = Op(True, E)
        p = attn_plan(bf, 6, 1, T, T, E, q, k, v, od, od, q, k, v)
        assert (p.fwd, p.bwd, p.shared_q) == ("fused", "pds_dkdv", want)


def test_set_side_enabled_off_is_the_only_mode():
    """The weight-gradient side stream is gone; bench.py still calls its switch around the probe
    steps: False is accepted and does nothing, True is an error."""
    from jmt import streams
    assert streams.set_side_enabled(False) is None
    with pytest.raises(ValueError, match="side stream .* was removed"):
        streams.set_side_enabled(True)


def test_side_stream_in_the_environment_fails_the_import():
    """JMT_SIDE_STREAM=1 is refused when jmt.streams is imported (a fresh process: the switch is
    read once), so a benchmark run that asks for the removed mode ends before it measures."""
    import subprocess
    import sys
    pkg = os.path.join(REPO_ROOT, "joint-multimodal-transformer-6th-abaw_amd")
    env = dict(os.environ, JMT_SIDE_STREAM="1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, sys.argv[1]); "
                        "import jmt.streams", pkg], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "ValueError" in r.stderr and "side stream" in r.stderr and "was removed" in r.stderr, \
        r.stderr[-2000:]
