"""Host tests of training through the global context: the fp64 yardsticks of the GPU tests
(tests/golden/gen_attn_grad_goldens.py: attn_grad_f64, pool_grad_f64, module_grad_f64) against the
reference's fp64 autograd gradients in tests/golden/attn_grad.npz, the new C entry points'
declarations and argument checks, and the train-mode dropout refusal.  No GPU is needed.

The three helpers are pinned per gradient tensor to 1e-10 of the tensor's largest entry (gmax), the
bound of test_tree_grad_host.py.  One tensor has no scale of its own: the gradient of the attention's
k_proj.bias is sum_{b,k} dK[b,k,:], analytically 0 (softmax is shift invariant), so its fp64 value is
rounding noise of a sum whose terms have size S = max_c sum_{b,k} |dK[b,k,c]| (stored by the
generator): it is pinned to 1e-10 S."""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, golden

sys.path.insert(0, GOLDEN)
import gen_attn_grad_goldens as AG  # noqa: E402

from velocity_asr import attention  # noqa: E402

REL = 1e-10


@pytest.fixture(scope="module")
def gold():
    return golden("attn_grad.npz")


@functools.lru_cache(maxsize=None)
def _module(name):
    return AG.module_grad_f64(name)


def test_fixture_lists_every_case(gold):
    assert list(gold["attn"]) == sorted(AG.ATTN)
    assert list(gold["pool"]) == sorted(AG.POOL)
    assert list(gold["modules"]) == sorted(AG.MODULES)


@pytest.mark.parametrize("name", sorted(AG.ATTN))
def test_attention_inputs_and_fp64_gradients_match_the_fixture(name, gold):
    inp, own = AG.attn_case_f64(name)
    assert np.array_equal(AG.sha_of([inp[k] for k in "qkvg"]), gold[f"{name}/sha"])
    for k in ("dq", "dK", "dV"):
        assert AG.stored_error(gold, f"{name}/{k}", own[k]) <= REL * float(gold[f"{name}/gmax/{k}"]), (name, k)


def test_one_key_has_no_query_or_key_gradient(gold):
    """Kp = 1 (or kps[b] = 1): p = 1 whatever q and k, so dq = dK = 0 exactly and dV = sum_t dout_t."""
    inp, own = AG.attn_case_f64("kp1")
    for k in ("dq", "dK"):
        assert not own[k].any() and float(gold[f"kp1/gmax/{k}"]) == 0.0 and float(gold[f"kp1/e_ref/{k}"]) == 0.0
    assert np.allclose(own["dV"][:, 0], inp["g"].astype(np.float64).sum(axis=1), rtol=1e-13, atol=0)
    for name in ("ragged20", "ragged64"):
        _, own = AG.attn_case_f64(name)
        kps = AG.ATTN[name]["kps"]
        assert kps[1] == 1 and not own["dq"][1].any() and not own["dK"][1].any()
        for b, n in enumerate(kps):
            assert not own["dK"][b, n:].any() and not own["dV"][b, n:].any() and own["dV"][b, :n].all()


@pytest.mark.parametrize("name", sorted(AG.POOL))
def test_pooling_inputs_and_fp64_gradient_match_the_fixture(name, gold):
    c = AG.POOL[name]
    inp = AG.pool_inputs(c)
    assert np.array_equal(AG.sha_of([inp["x"], inp["g"]]), gold[f"{name}/sha"])
    own = AG.pool_grad_f64(inp["g"], c["L"], c.get("lens"), c.get("ks"))
    assert AG.stored_error(gold, f"{name}/dx", own) <= REL * float(gold[f"{name}/gmax/dx"])
    for b, n in enumerate(c.get("lens", [])):
        assert not own[b, n:].any()
    # the gradient of a mean: every bin's weights sum to 1
    assert np.allclose(own.sum(axis=1)[0], inp["g"].astype(np.float64)[0, :c.get("ks", [c["K"]])[0]].sum(axis=0), atol=1e-12)


@pytest.mark.parametrize("L,K", [(8, 8), (9, 4), (64, 16), (501, 64), (37, 1), (600, 75), (75, 18)])
def test_a_row_lies_in_at_most_two_bins(L, K):
    P = AG.pool_matrix(L, K)
    assert np.allclose(P.sum(axis=1), 1.0) and ((P > 0).sum(axis=0) >= 1).all() and ((P > 0).sum(axis=0) <= 2).all()


@pytest.mark.parametrize("name", sorted(AG.MODULES))
def test_module_grad_f64_matches_the_reference(name, gold):
    own, extra = _module(name)
    assert sorted(own) == AG.module_grad_names(name)
    assert AG.sha_of(AG.module_state(name)[1:]).tolist() == gold[f"{name}/sha"].tolist()
    kb = AG.KBIAS if AG.MODULES[name]["kind"] == "ctx" else "k_proj.bias"
    S = float(gold[f"{name}/S/{kb}"])
    assert abs(float(extra["S"].max()) - S) <= REL * S
    for k in own:
        scale = S if k == kb else float(gold[f"{name}/gmax/{k}"])
        assert AG.stored_error(gold, f"{name}/{k}", own[k]) <= REL * scale, (name, k)
    # the cancelling sum: its fp64 value is noise far below its terms
    assert float(gold[f"{name}/gmax/{kb}"]) <= 1e-12 * S


def test_pool_sizes_follow_the_modules_rule():
    for L, want in ((137, (64, 16)), (600, (75, 18)), (40, (40, 16)), (2100, (262, 64))):
        assert AG.pool_sizes(L) == want
        p1, p2 = attention.AdaptivePool(level=1, d_model=4), attention.AdaptivePool(level=2, d_model=4)
        k1 = min(p1._compute_pool_size(L), L)
        assert (k1, min(p2._compute_pool_size(k1, k1), k1)) == want
    m = AG.MODULES["ctx_ragged"]
    assert [AG.pool_sizes(n) for n in m["lengths"]] == [(75, 18), (64, 16)]


def test_abi_declares_and_exports_the_global_context_backward():
    from velocity_asr import _lib
    names = _lib.header_functions()
    L = _lib.load()
    header = open(f"{REPO}/include/vasr.h").read()
    for n in ("vasr_pooled_attention_bwd_f32", "vasr_pooled_attention_bwd_workspace_floats",
              "vasr_adaptive_pool_bwd_f32"):
        assert n in names and n in _lib._SIGNATURES and hasattr(L, n) and f" {n}(" in header, n
    assert L.vasr_version() == _lib.ABI_VERSION == 21 and "#define VASR_ABI_VERSION 21\n" in header


def test_workspace_is_one_partial_per_64_token_tile():
    from velocity_asr import _lib, ops
    L = _lib.load()
    ws = L.vasr_pooled_attention_bwd_workspace_floats
    assert ops.ATTN_BWD_TILE == AG.TILE == 64
    assert ws(32, 501, 16, 4, 12) == 32 * 8 * 16 * 96
    assert ws(3, 65, 64, 4, 12) == 3 * 2 * 64 * 96 and ws(3, 128, 2, 2, 32) == 3 * 2 * 2 * 128
    assert ws(3, 64, 16, 4, 12) == 0 and ws(3, 1, 16, 4, 12) == 0  # one tile writes dkv itself
    assert ws(0, 501, 16, 4, 12) == 0 and ws(3, 0, 16, 4, 12) == 0


def test_abi_refuses_bad_attention_backward_arguments():
    from velocity_asr import _lib
    L = _lib.load()
    fake = 256  # aligned non-null pointer values: the checks return before any dereference or launch

    def bwd(q=fake, ld_q=48, kv=fake, dout=fake, dq=fake, dkv=fake, ws=fake, nws=1 << 30, B=1, Lq=100, Kp=16, heads=4,
            hd=12, kps=None):
        return L.vasr_pooled_attention_bwd_f32(q, ld_q, kv, dout, dq, dkv, ws, nws, B, Lq, Kp, heads, hd, kps, None)

    for null in ("q", "kv", "dout", "dq", "dkv"):
        assert bwd(**{null: None}) == -1 and b"null pointer" in L.vasr_last_error(), null
    for bad in (dict(Kp=0), dict(Kp=65), dict(hd=0), dict(hd=33), dict(heads=0), dict(heads=9, hd=32), dict(Lq=-1),
                dict(B=-1)):
        assert bwd(**bad) == -1 and b"unsupported shape" in L.vasr_last_error(), bad
    assert bwd(ld_q=47) == -1 and b"ld_q" in L.vasr_last_error()
    assert bwd(Kp=64, heads=8, hd=32, ld_q=256) == -1 and b"64 KiB" in L.vasr_last_error()
    assert bwd(heads=3, hd=5, ld_q=15) == -1 and b"multiple of 4" in L.vasr_last_error()
    assert bwd(kv=264) == -1 and b"16-byte aligned" in L.vasr_last_error()
    need = 2 * 16 * 96
    assert bwd(nws=need - 1) == -1 and f"workspace of {need - 1} floats, {need} needed".encode() in L.vasr_last_error()
    assert bwd(ws=None) == -1 and b"workspace" in L.vasr_last_error()
    assert bwd(B=70000) == -1 and b"too large" in L.vasr_last_error()
    assert bwd(B=0) == 0 and bwd(B=0, ws=None, nws=0) == 0  # nothing to do: no launch


def test_abi_refuses_bad_pooling_backward_arguments():
    from velocity_asr import _lib
    L = _lib.load()
    fake = 256

    def bwd(g=fake, dx=fake, B=1, Lq=9, C=5, K=4, lens=None, ks=None):
        return L.vasr_adaptive_pool_bwd_f32(g, dx, B, Lq, C, K, lens, ks, None)

    assert bwd(g=None) == -1 and b"null pointer" in L.vasr_last_error()
    assert bwd(dx=None) == -1 and b"null pointer" in L.vasr_last_error()
    for bad in (dict(K=0), dict(K=10), dict(Lq=0, K=0), dict(C=0), dict(B=-1)):
        assert bwd(**bad) == -1 and b"1 <= K <= L" in L.vasr_last_error(), bad
    assert bwd(lens=fake) == -1 and b"go together" in L.vasr_last_error()
    assert bwd(ks=fake) == -1 and b"go together" in L.vasr_last_error()
    assert bwd(B=0) == 0 and bwd(B=0, lens=fake, ks=fake) == 0


def test_attention_refuses_train_mode_dropout():
    m = attention.MultiHeadAttention(d_model=24, num_heads=4, attention_dim=48, dropout=0.1)
    x, mem = torch.zeros(1, 5, 24), torch.zeros(1, 3, 24)
    assert m.training
    with pytest.raises(NotImplementedError, match="dropout on the attention probabilities"):
        m.forward_differentiable(x, mem, mem)
    ctx = attention.HierarchicalGlobalContext(d_model=16, num_heads=4, attention_dim=48, global_ssm_layers=1)
    assert ctx.cross_attention.training and ctx.cross_attention.dropout.p == 0.1
    with pytest.raises(NotImplementedError, match="mask"):
        m.eval().forward_differentiable(x, mem, mem, mask=torch.ones(1))
    if not torch.cuda.is_available():  # eval, or dropout 0 in train mode: past the refusal, on to the device check
        with pytest.raises(RuntimeError, match="HIP device"):
            m.eval().forward_differentiable(x, mem, mem)
        m0 = attention.MultiHeadAttention(d_model=24, num_heads=4, attention_dim=48, dropout=0.0)
        with pytest.raises(RuntimeError, match="HIP device"):
            m0.forward_differentiable(x, mem, mem)


def test_modules_and_operators_have_the_differentiable_path():
    for cls in (attention.AdaptivePool, attention.MultiHeadAttention, attention.GatedFusion,
                attention.HierarchicalGlobalContext):
        assert callable(getattr(cls, "forward_differentiable"))
    with pytest.raises(ValueError, match="pooled_attention"):
        attention.pooled_attention(torch.zeros(1, 5, 48), torch.zeros(1, 3, 48), 4)
    with pytest.raises(ValueError, match="go together"):
        attention.adaptive_avg_pool(torch.zeros(1, 5, 4), 2, lengths=[5])
    # GatedFusion's differentiable forward is torch ops alone: the reference's function, on any device
    f = attention.GatedFusion(d_model=32)
    a, b = torch.randn(2, 3, 32), torch.randn(2, 3, 32)
    gate = torch.sigmoid(f.gate_proj[0](torch.cat([a, b], -1)))
    want = f.out_proj(gate * f.local_proj(a) + (1 - gate) * f.global_proj(b))
    assert torch.allclose(f.forward_differentiable(a, b), want, atol=1e-6)
