"""GPU tests of training through the global context: the differentiable operators
velocity_asr.attention.pooled_attention and adaptive_avg_pool (the inference kernels forwards,
vasr_pooled_attention_bwd_f32 / vasr_adaptive_pool_bwd_f32 backwards) and forward_differentiable of
MultiHeadAttention and HierarchicalGlobalContext, against the fp64 gradients of
tests/golden/gen_attn_grad_goldens.py (attn_grad_f64 / pool_grad_f64 / module_grad_f64, pinned to the
reference's fp64 autograd by test_attn_grad_host.py).

Token-tile edges.  The attention's backward gives a workgroup 64 tokens (ops.ATTN_BWD_TILE), so its
edges are the multiples of 64 and nothing else: L = 63 / 64 (one tile, which writes dkv itself) against
65 (two tiles: the workspace and the tile-sum launch), and 127 / 128 (two tiles) against 129 (three).
The pooling's backward has no tile: one lane per element.

Tolerance, per case and per gradient tensor, absolute: e_hip = max |HIP - fp64| <=
max(4 e_ref, 8 * 2^-23 * gmax), with e_ref = max |reference fp32 - reference fp64| and gmax = max |fp64|
of that tensor from tests/golden/attn_grad.npz (the project's bound: test_tree_grad_gpu.py).  Two
places where that bound degenerates, both derived and not measured:
  * k_proj.bias of the attention: its gradient is sum_{b,k} dK[b,k,:], analytically 0 (softmax is
    shift invariant).  gmax is rounding noise there; the scale is S = max_c sum_{b,k} |dK_fp64[b,k,c]|
    (in the npz): max(4 e_ref, 8 * 2^-23 * S).
  * Kp = 1 or kps[b] = 1: dq and dK are exactly 0 in the reference, the difference of two equal terms
    of size u = max_{t,h} sum_j |dout_j v_j| * max|k| / sqrt(hd) for dq (max|q| for dK): 8 * 2^-23 * u.
Every test prints e_ref, e_hip, the bound and their ratio per tensor; DESIGN.md has the table measured
on an MI355X.
"""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, record_metric

sys.path.insert(0, GOLDEN)
import gen_attn_grad_goldens as AG  # noqa: E402

from velocity_asr import attention, ops  # noqa: E402

pytestmark = pytest.mark.gpu

ULP8 = 8.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def gold():
    return golden("attn_grad.npz")


@functools.lru_cache(maxsize=None)
def _attn(name):
    """(case, device tensors q, kv, g, kps, fp64 gradients) computed once and left unchanged."""
    c = AG.ATTN[name]
    inp, want = AG.attn_case_f64(name)
    for v in want.values():
        v.setflags(write=False)
    t = {k: torch.from_numpy(v).cuda() for k, v in inp.items()}
    kps = torch.tensor(c["kps"], dtype=torch.int32).cuda() if "kps" in c else None
    return c, t["q"], torch.cat([t["k"], t["v"]], -1).contiguous(), t["g"], kps, want


def _run_attn(q, kv, g, heads, kps, needs=("q", "kv")):
    qt, kvt = q.clone().requires_grad_("q" in needs), kv.clone().requires_grad_("kv" in needs)
    out = attention.pooled_attention(qt, kvt, heads, key_lengths=kps)
    out.backward(g)
    return out.detach(), qt.grad, kvt.grad


def _report(case, k, e_ref, e_hip, tol, worst, metric):
    ratio = e_hip / tol if tol > 0 else (0.0 if e_hip == 0 else float("inf"))
    worst[(case, k)] = ratio
    print(f"{case} {k}: e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  bound {tol:.3e}  ratio {ratio:.3f}  "
          f"(worst so far {max(worst.values()):.3f})")
    record_metric(metric, case=case, tensor=k, e_ref=e_ref, e_hip=e_hip, bound=tol, ratio=ratio)
    return [(k, e_hip, tol)] if e_hip > tol else []


def _check(gold, case, k, got, want, worst, metric, scale=None):
    """One tensor against max(4 e_ref, 8 ulp scale), scale = gmax unless given; returns the misses."""
    e_ref = float(gold[f"{case}/e_ref/{k}"])
    tol = max(4.0 * e_ref, ULP8 * (float(gold[f"{case}/gmax/{k}"]) if scale is None else scale))
    e_hip = float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())
    return _report(case, k, e_ref, e_hip, tol, worst, metric)


def _one_key_scale(q, kv, g, heads, b):
    """u of utterance b for (dq, dK) when it has one key (the module docstring)."""
    A = q.shape[-1]
    hd = A // heads
    k0, v0 = kv[b, 0, :A].double(), kv[b, 0, A:].double()
    t = (g[b].double().abs() * v0.abs()).view(-1, heads, hd).sum(-1).max().item() / np.sqrt(hd)
    return t * k0.abs().max().item(), t * q[b].double().abs().max().item()


_worst = {}


@pytest.mark.parametrize("name", list(AG.ATTN))
def test_attention_gradients_match_fp64(name, gold):
    c, q, kv, g, kps, want = _attn(name)
    A = q.shape[-1]
    out, dq, dkv = _run_attn(q, kv, g, c["heads"], kps)
    B, L, Kp = c["B"], c["L"], c["Kp"]
    plain = ops.pooled_attention(q.reshape(B * L, A), kv.reshape(B * Kp, 2 * A), B, L, Kp, c["heads"], kps=kps)
    assert torch.equal(out, plain.view(B, L, A))  # the forward is the inference kernel, bitwise
    assert dq.shape == q.shape and dkv.shape == kv.shape and dq.dtype == dkv.dtype == torch.float32
    assert torch.isfinite(dq).all() and torch.isfinite(dkv).all()
    got = dict(dq=dq, dK=dkv[..., :A], dV=dkv[..., A:])
    ones = [b for b in range(B) if (c["kps"][b] if "kps" in c else Kp) == 1]
    fails = []
    for k in ("dq", "dK", "dV"):
        if Kp == 1 and k != "dV":  # the whole tensor is exactly 0 in the reference: the bound is u
            assert float(gold[f"{name}/gmax/{k}"]) == 0.0 and not want[k].any()
            u = max(_one_key_scale(q, kv, g, c["heads"], b)[k == "dK"] for b in range(B))
            fails += _report(name, k, 0.0, float(got[k].abs().max()), ULP8 * u, _worst, "attn_grad_abs_err")
            continue
        fails += _check(gold, name, k, got[k], want[k], _worst, "attn_grad_abs_err")
        if k != "dV":
            for b in ones:  # an utterance with one key inside a ragged batch: its rows against its own u
                u = _one_key_scale(q, kv, g, c["heads"], b)[k == "dK"]
                fails += _report(name, f"{k}[{b}]", 0.0, float(got[k][b].abs().max()), ULP8 * u, _worst,
                                 "attn_grad_abs_err")
    if "kps" in c:
        for b, n in enumerate(c["kps"]):
            assert not dkv[b, n:].any(), (name, b)  # rows past kps[b] are written, as exact zeros
    record_metric("attn_grad_worst_ratio", case=name, ratio=max(v for (n, _), v in _worst.items() if n == name))
    assert not fails, (name, fails)


@pytest.mark.parametrize("name", ["h4x12", "h4x5", "l129", "ragged64"])
def test_strided_query_rows(name):
    """q as a column slice of a wider buffer (ld_q > A): bitwise the contiguous result."""
    c, q, kv, g, kps, _ = _attn(name)
    B, L, Kp, A = c["B"], c["L"], c["Kp"], q.shape[-1]
    wide = torch.full((B * L, A + 8), float("nan"), device="cuda")
    wide[:, 4:4 + A] = q.reshape(B * L, A)
    qs = wide[:, 4:4 + A]
    assert qs.stride(0) == A + 8
    args = (kv.reshape(B * Kp, 2 * A), g.reshape(B * L, A), B, L, Kp, c["heads"])
    want = ops.pooled_attention_bwd(q.reshape(B * L, A), *args, kps=kps)
    got = ops.pooled_attention_bwd(qs, *args, kps=kps)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.isfinite(got[0]).all()


@pytest.mark.parametrize("name", ["h4x12", "h2x32", "l65", "workload", "ragged64", "lds_kp64_a128"])
def test_backward_is_deterministic_and_batch_invariant(name):
    """Two backward runs are bitwise equal (no atomics), and each utterance alone at B = 1 gives
    bitwise its rows of the batched dq and dkv."""
    c, q, kv, g, kps, _ = _attn(name)
    a, b = _run_attn(q, kv, g, c["heads"], kps), _run_attn(q, kv, g, c["heads"], kps)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    for i in range(c["B"]):
        alone = _run_attn(q[i:i + 1], kv[i:i + 1], g[i:i + 1], c["heads"], None if kps is None else kps[i:i + 1])
        assert all(torch.equal(x, y[i:i + 1]) for x, y in zip(alone, a)), (name, i)


def test_only_the_inputs_that_need_it_get_a_gradient():
    c, q, kv, g, kps, _ = _attn("h4x12")
    _, dq, dkv = _run_attn(q, kv, g, c["heads"], kps)
    _, dq1, none = _run_attn(q, kv, g, c["heads"], kps, needs=("q",))
    assert none is None and torch.equal(dq1, dq)
    _, none, dkv1 = _run_attn(q, kv, g, c["heads"], kps, needs=("kv",))
    assert none is None and torch.equal(dkv1, dkv)
    plain = attention.pooled_attention(q, kv, c["heads"])  # nothing requires grad: the inference kernel alone
    assert not plain.requires_grad and plain.grad_fn is None
    with torch.no_grad():
        assert torch.equal(attention.pooled_attention(q.clone().requires_grad_(), kv, c["heads"]), plain)
    x = torch.randn(2, 9, 5, device="cuda")
    assert attention.adaptive_avg_pool(x, 4).grad_fn is None
    assert attention.adaptive_avg_pool(x.clone().requires_grad_(), 4).grad_fn is not None


@pytest.mark.parametrize("name", ["l65", "l129", "workload", "ragged64"])
def test_no_stale_reads_of_the_workspace(name):
    """The tile partials pre-filled with NaN change nothing: every element is written before it is read."""
    c, q, kv, g, kps, _ = _attn(name)
    B, L, Kp, A = c["B"], c["L"], c["Kp"], q.shape[-1]
    args = (q.reshape(B * L, A), kv.reshape(B * Kp, 2 * A), g.reshape(B * L, A), B, L, Kp, c["heads"])
    n = ops.L.lib().vasr_pooled_attention_bwd_workspace_floats(B, L, Kp, c["heads"], c["hd"])
    assert n == B * -(-L // ops.ATTN_BWD_TILE) * Kp * 2 * A
    clean = ops.pooled_attention_bwd(*args, kps=kps)
    dirty = ops.pooled_attention_bwd(*args, kps=kps, workspace=torch.full((n,), float("nan"), device="cuda"))
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1]) and torch.isfinite(dirty[1]).all()


def test_no_tokens_gives_a_zero_key_gradient():
    B, Kp, heads, A = 3, 16, 4, 48
    kv = torch.randn(B * Kp, 2 * A, device="cuda")
    e = torch.empty(0, A, device="cuda")
    dq, dkv = ops.pooled_attention_bwd(e, kv, e, B, 0, Kp, heads)
    assert dq.shape == (0, A) and dkv.shape == kv.shape and not dkv.any()


# ------------------------------------------------------------------ pooling
@functools.lru_cache(maxsize=None)
def _pool(name):
    c = AG.POOL[name]
    inp = AG.pool_inputs(c)
    want = AG.pool_grad_f64(inp["g"], c["L"], c.get("lens"), c.get("ks"))
    want.setflags(write=False)
    return c, torch.from_numpy(inp["x"]).cuda(), torch.from_numpy(inp["g"]).cuda(), want


_worst_pool = {}


@pytest.mark.parametrize("name", list(AG.POOL))
def test_pooling_gradient_matches_fp64(name, gold):
    c, x, g, want = _pool(name)
    lens, ks = c.get("lens"), c.get("ks")
    xt = x.clone().requires_grad_()
    out = attention.adaptive_avg_pool(xt, c["K"], lengths=lens, sizes=ks)
    dl = None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()
    dk = None if ks is None else torch.tensor(ks, dtype=torch.int32).cuda()
    assert torch.equal(out.detach(), ops.adaptive_pool(x, c["K"], lens=dl, ks=dk))  # bitwise the inference kernel
    gg = g.clone()
    for b, n in enumerate(ks or []):
        gg[b, n:] = float("nan")  # bins past ks[b] of g are never read
    out.backward(gg)
    dx = xt.grad
    assert dx.shape == x.shape and torch.isfinite(dx).all()
    for b, n in enumerate(lens or []):
        assert not dx[b, n:].any(), (name, b)  # rows past lens[b] are written, as exact zeros
    fails = _check(gold, name, "dx", dx, want, _worst_pool, "pool_grad_abs_err")
    xt.grad = None
    attention.adaptive_avg_pool(xt, c["K"], lengths=lens, sizes=ks).backward(gg)
    assert torch.equal(xt.grad, dx)  # run to run bitwise
    for b in range(c["B"]):  # an utterance alone: bitwise its rows of the batch
        one = x[b:b + 1].clone().requires_grad_()
        attention.adaptive_avg_pool(one, c["K"], lengths=lens and lens[b:b + 1], sizes=ks and ks[b:b + 1]).backward(
            gg[b:b + 1])
        assert torch.equal(one.grad, dx[b:b + 1]), (name, b)
    assert not fails, (name, fails)


# ------------------------------------------------------------------ modules
def _module(name):
    mc = AG.MODULES[name]
    if mc["kind"] == "mha":
        m = attention.MultiHeadAttention(d_model=mc["d_model"], num_heads=mc["heads"], attention_dim=mc["attention_dim"])
    else:
        m = attention.HierarchicalGlobalContext(d_model=mc["d_model"], num_heads=mc["heads"],
                                                attention_dim=mc["attention_dim"], global_ssm_layers=mc["layers"],
                                                global_ssm_state_dim=mc["state_dim"])
    sd, *tensors = AG.module_state(name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval(), [torch.from_numpy(v).cuda() for v in tensors]


_worst_module = {}


@pytest.mark.parametrize("name", list(AG.MODULES))
def test_forward_differentiable_reaches_every_parameter(name, gold):
    mc = AG.MODULES[name]
    m, tensors = _module(name)
    want, extra = AG.module_grad_f64(name)
    if mc["kind"] == "mha":
        query, memory, g = tensors
        query, memory = query.requires_grad_(), memory.requires_grad_()
        out = m.forward_differentiable(query, memory, memory)
        inputs = {"input": query, "memory": memory}
        kb = "k_proj.bias"
    else:
        x, g = tensors
        x = x.requires_grad_()
        out = m.forward_differentiable(x, lengths=mc.get("lengths"))
        inputs = {"input": x}
        kb = AG.KBIAS
    valid = torch.from_numpy(np.abs(extra["out"]).sum(-1) > 0).cuda()  # (a ragged batch: its frames alone)
    fwd = (out.detach().double().cpu().numpy() - extra["out"])[valid.cpu().numpy()]
    assert np.abs(fwd).max() <= 1e-4 * np.abs(extra["out"]).max()  # the same function (a sanity check, not the bound)
    (out * g).sum().backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    got.update({k: v.grad for k, v in inputs.items()})
    assert sorted(got) == AG.module_grad_names(name)
    fails = []
    for k in AG.module_grad_names(name):
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        scale = float(gold[f"{name}/S/{kb}"]) if k == kb else None
        fails += _check(gold, name, k, got[k], want[k], _worst_module, "attn_grad_module_abs_err", scale=scale)
    for b, n in enumerate(mc.get("lengths", [])):
        assert not inputs["input"].grad[b, n:].any()  # zero upstream gradient on the padded frames
    assert not fails, (name, fails)
