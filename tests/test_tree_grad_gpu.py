"""GPU tests of the differentiable tree scan (velocity_asr.ssm.selective_scan(scan_mode="parallel"):
the inference kernels forwards, vasr_ssm_tree_bwd_f32 backwards; forward_differentiable of
SelectiveSSM, SSMBlock and GlobalSSM) against the fp64 gradients of
tests/golden/gen_tree_grad_goldens.py (tree_grad_f64 / module_grad_f64, pinned to the reference's fp64
autograd by test_tree_grad_host.py).

Tolerance, per case and per gradient tensor, absolute: e_hip = max |HIP - fp64| <=
max(4 e_ref, 8 * 2^-23 * gmax), with e_ref = max |reference fp32 - reference fp64| and gmax = max |fp64|
of that tensor (tests/golden/tree_grad.npz): the project's bound for the same fp32 algorithm in
another operation order (test_scan_grad_gpu.py, test_ctc_grad_gpu.py).  Both tree modes
(VASR_SCAN_FMA=1 and =0) run.  test_gradients_match_fp64 prints e_ref, e_hip, the bound and their ratio
for every tensor; DESIGN.md has the table measured on an MI355X.
"""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, record_metric

sys.path.insert(0, GOLDEN)
import gen_tree_grad_goldens as TG  # noqa: E402

from velocity_asr import ops, ssm  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_NAMES = [n for n in TG.CASES if n != "x_only"]
KEYS = ("x", "dt", "A", "B", "C", "D", "z")
ULP8 = 8.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def gold():
    return golden("tree_grad.npz")


@pytest.fixture(params=["1", "0"], ids=["fma", "nofma"])
def fma(request, monkeypatch):
    monkeypatch.setenv("VASR_SCAN_FMA", request.param)
    assert ssm._tree_mode() == (2 if request.param == "1" else 0)
    return request.param


@functools.lru_cache(maxsize=None)
def _want(name):
    """(inputs, fp64 gradients) of a case on the host, computed once and left unchanged."""
    inp, gr = TG.case_grad_f64(name)
    for v in list(inp.values()) + list(gr.values()):
        if v is not None:
            v.setflags(write=False)
    return inp, gr


@functools.lru_cache(maxsize=None)
def _dev(name):
    inp, _ = _want(name)
    return {k: None if v is None else torch.from_numpy(np.array(v)).cuda() for k, v in inp.items()}


def _run(d, needs=KEYS):
    """(out, {key: grad}) of the tree's selective_scan with the inputs in `needs` requiring grad."""
    t = {k: None if d[k] is None else d[k].clone().requires_grad_(k in needs) for k in KEYS}
    out = ssm.selective_scan(t["x"], t["dt"], t["A"], t["B"], t["C"], t["D"], t["z"], scan_mode="parallel")
    out.backward(d["g"])
    return out.detach(), {k: None if t[k] is None else t[k].grad for k in KEYS}


def _bound(gold, name, k):
    return max(4.0 * float(gold[f"{name}/e_ref/{k}"]), ULP8 * float(gold[f"{name}/gmax/{k}"]))


def _check(gold, name, k, got, want, worst, metric):
    """Print and record one tensor's figures; returns (k, e_hip, bound) where the bound is missed."""
    e_ref, tol = float(gold[f"{name}/e_ref/{k}"]), _bound(gold, name, k)
    e_hip = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    # (a bound of 0: the gradient is exactly 0 -- l1's dA, dB, dC, ddt -- and so must the device's be)
    ratio = e_hip / tol if tol > 0 else (0.0 if e_hip == 0 else float("inf"))
    worst[(name, k)] = ratio
    print(f"{name} {k}: e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  bound {tol:.3e}  ratio {ratio:.3f}  "
          f"(worst so far {max(worst.values()):.3f})")
    record_metric(metric, case=name, tensor=k, e_ref=e_ref, e_hip=e_hip, bound=tol, ratio=ratio)
    return [(k, e_hip, tol)] if e_hip > tol else []


_worst = {}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_match_fp64(name, fma, gold):
    d = _dev(name)
    _, want = _want(name)
    out, got = _run(d)
    assert out.dtype == torch.float32 and out.shape == d["x"].shape
    fails = []
    for k in KEYS:
        if d[k] is None:
            assert got[k] is None
            continue
        g = got[k]
        assert g is not None and g.is_cuda and g.dtype == torch.float32 and g.shape == d[k].shape, k
        assert torch.isfinite(g).all(), (name, k)
        fails += _check(gold, name, "d" + k, g, want["d" + k], _worst, f"tree_grad_abs_err_fma{fma}")
    record_metric("tree_grad_worst_ratio", case=name, fma=fma,
                  ratio=max(v for (n, _), v in _worst.items() if n == name))
    assert not fails, (name, fails)


def _packed(d):
    """ops-level operands of a case: (x, z or None, dt, bc (M, 2N') padded, A', A2', D)."""
    B, L, Di = d["x"].shape
    N = d["A"].numel()
    bc, Ap = ssm._pad_states(d["B"], d["C"], d["A"], N, ops.scan_state_dim(N))
    A2 = Ap * torch.tensor(ops.LOG2E, dtype=torch.float32)
    dt = d["dt"].reshape(B * L, Di).contiguous()
    if d["z"] is None:
        return d["x"].reshape(B * L, Di).contiguous(), None, dt, bc, Ap, A2, d["D"]
    xz = torch.cat([d["x"].reshape(B * L, Di), d["z"].reshape(B * L, Di)], 1)
    return xz[:, :Di], xz[:, Di:], dt, bc, Ap, A2, d["D"]


@pytest.mark.parametrize("name", ["l1", "l17", "l501", "n16", "n32", "n128", "n48", "di48_b2_l37", "big_dt", "ungated"])
def test_training_forward_is_bitwise_the_inference_kernel(name, fma):
    d = _dev(name)
    B, L, Di = d["x"].shape
    x, z, dt, bc, Ap, A2, D = _packed(d)
    mode = ssm._tree_mode()
    if z is not None:
        want = ops.ssm_scan(torch.cat([x, z], 1), dt, bc, A2, D, B, L, mode).view(B, L, Di)
    else:
        want = ops.ssm_scan_ungated(x, dt, bc, A2, D, B, L, mode).view(B, L, Di)
    out, _ = _run(d)
    assert torch.equal(out, want)
    with torch.no_grad():  # nothing requires grad: the inference kernel and nothing else
        got = ssm.selective_scan(d["x"], d["dt"], d["A"], d["B"], d["C"], d["D"], d["z"], scan_mode="parallel")
    assert torch.equal(got, want) and not got.requires_grad
    if z is not None:  # the same inputs without the gate: the ungated kernel
        t = {k: d[k].clone().requires_grad_() for k in ("x", "dt", "A", "B", "C", "D")}
        y = ops.ssm_scan_ungated(x.contiguous(), dt, bc, A2, D, B, L, mode).view(B, L, Di)
        assert torch.equal(ssm.selective_scan(**t, scan_mode="parallel").detach(), y)


@pytest.mark.parametrize("name", ["di48_b2_l37", "n16", "ungated"])
def test_backward_is_deterministic_and_batch_invariant(name):
    """Two backward runs are bitwise equal (no atomics), and each utterance alone at B = 1 gives
    bitwise its rows of the batched dx, ddt, dz, dB and dC (dA and dD sum over the batch)."""
    d = _dev(name)
    _, a = _run(d)
    _, b = _run(d)
    for k in KEYS:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k], b[k]), k
    for i in range(d["x"].shape[0]):
        one = {k: v[i:i + 1] if v is not None and v.dim() == 3 else v for k, v in d.items()}
        _, alone = _run(one)
        for k in ("x", "dt", "z", "B", "C"):
            if d[k] is not None:
                assert torch.equal(alone[k], a[k][i:i + 1]), (name, i, k)


def test_only_the_inputs_that_need_it_get_a_gradient(gold):
    d = _dev("x_only")
    _, want = _want("x_only")
    _, got = _run(d, needs=("x",))
    assert all(got[k] is None for k in KEYS if k != "x")
    e = float(np.abs(got["x"].cpu().numpy().astype(np.float64) - want["dx"]).max())
    assert e <= _bound(gold, "x_only", "dx")
    assert torch.equal(got["x"], _run(d)[1]["x"])


@pytest.mark.parametrize("name", ["l17", "l257", "l513", "n48", "ungated"])
def test_no_stale_reads_of_workspace_or_outputs(name):
    """Everything the backward is handed to write -- outputs and workspace -- pre-filled with NaN
    changes nothing: every element is written before it is read."""
    d = _dev(name)
    B, L, Di = d["x"].shape
    M = B * L
    x, z, dt, bc, Ap, A2, D = _packed(d)
    N = A2.numel()
    g = d["g"].reshape(M, Di).contiguous()
    clean = ops.ssm_tree_bwd(x, z, dt, bc, Ap, A2, D, g, B, L)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    dirty = dict(dx=nan(M, Di), ddt=nan(M, Di), dz=nan(M, Di) if z is not None else None, dB=nan(M, N), dC=nan(M, N),
                 dA_part=nan(B, Di, N), dD_part=nan(B, Di))
    ws = nan(ops.L.lib().vasr_ssm_tree_bwd_workspace_floats(B, L, Di, N))
    got = ops.ssm_tree_bwd(x, z, dt, bc, Ap, A2, D, g, B, L, out=dirty, workspace=ws)
    assert got is dirty
    for k, v in clean.items():
        assert (v is None and got[k] is None) or (torch.isfinite(got[k]).all() and torch.equal(got[k], v)), k


def _module(name):
    mc = TG.MODULES[name]
    if mc["kind"] == "ssm":
        m = ssm.SelectiveSSM(d_model=mc["d_model"], state_dim=mc["state_dim"], expand_ratio=TG.EXPAND,
                             scan_mode="parallel")
    elif mc["kind"] == "block":
        m = ssm.SSMBlock(d_model=mc["d_model"], state_dim=mc["state_dim"], expand_ratio=TG.EXPAND,
                         kernel_size=TG.KERNEL_SIZE, scan_mode="parallel")
    else:
        m = ssm.GlobalSSM(d_model=mc["d_model"], num_layers=mc["layers"], state_dim=mc["state_dim"])
    sd, x, g = TG.module_state(name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.cuda().eval(), x, g


_worst_module = {}


@pytest.mark.parametrize("name", list(TG.MODULES))
def test_forward_differentiable_reaches_every_parameter(name, gold):
    m, x, g = _module(name)
    kw = {} if name == "global" else dict(tree_scan=True)  # GlobalSSM's scan is always the tree
    xt = torch.from_numpy(x).cuda().requires_grad_()
    out = m.forward_differentiable(xt, **kw)
    with torch.no_grad():  # the module's own inference forward (its own kernels): close, not bitwise
        assert torch.allclose(out, m(xt), atol=1e-4, rtol=1e-4)
    (out * torch.from_numpy(g).cuda()).sum().backward()
    want = TG.module_grad_f64(name)
    got = {k: p.grad for k, p in m.named_parameters()}
    got["input"] = xt.grad
    assert sorted(got) == TG.module_grad_names(name)
    fails = []
    for k in TG.module_grad_names(name):
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        fails += _check(gold, name, k, got[k], want[k], _worst_module, "tree_grad_module_abs_err")
    assert not fails, (name, fails)


@pytest.mark.parametrize("name", list(TG.MODULES)[:2])
def test_tree_scan_keyword_leaves_a_sequential_module_alone(name):
    """For a "sequential" module tree_scan=True differentiates the module's own scan, the
    recurrence: bitwise forward_differentiable(x)."""
    mc = TG.MODULES[name]
    cls = ssm.SelectiveSSM if mc["kind"] == "ssm" else ssm.SSMBlock
    m = cls(d_model=mc["d_model"], state_dim=mc["state_dim"], scan_mode="sequential")
    sd, x, _ = TG.module_state(name)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda().eval()
    xt = torch.from_numpy(x).cuda().requires_grad_()
    a, b = m.forward_differentiable(xt), m.forward_differentiable(xt, tree_scan=True)
    assert a.requires_grad and torch.equal(a.detach(), b.detach())
    par, _, _ = _module(name)
    assert not torch.equal(par.forward_differentiable(xt, tree_scan=True).detach(), a.detach())  # another function
