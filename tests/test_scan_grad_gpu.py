"""GPU tests of the differentiable selective scan (velocity_asr.ssm.selective_scan: vasr_ssm_scan_save_f32
forward, vasr_ssm_scan_bwd_f32 backward; SelectiveSSM.forward_differentiable) against the fp64
gradients of tests/golden/gen_scan_grad_goldens.py (scan_grad_f64 / module_grad_f64, pinned to the
reference's fp64 autograd by test_scan_grad_host.py).

Tolerance, per case and per gradient tensor, absolute: e_hip = max |HIP - fp64| <=
max(4 e_ref, 8 * 2^-23 * gmax), with e_ref = max |reference fp32 - reference fp64| and gmax = max |fp64|
of that tensor (tests/golden/scan_grad.npz).  The factor 4 is the project's convention for the same
fp32 algorithm with another exp and summation order (test_ctc_grad_gpu.py); the floor is 8 ulp at the
tensor's largest entry.  test_gradients_match_fp64 prints e_ref, e_hip and the bound of every tensor;
DESIGN.md section 4 has the table measured on an MI355X.

The forward value is compared bitwise with the inference kernel (ops.ssm_scan, mode 1).  The ungated
form has no inference entry point of its own at mode 1, so it is compared with the gated launch at
z = 128: silu(128) = 128 / (1 + exp(-128)) is exactly 128 in float32 (exp(-128) rounds to 0), the
gated output is then y * 128 exactly, and dividing by 128 gives y back, bitwise.
"""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, record_metric

sys.path.insert(0, GOLDEN)
import gen_scan_grad_goldens as SG  # noqa: E402

from velocity_asr import ops, ssm  # noqa: E402

pytestmark = pytest.mark.gpu

CASE_NAMES = [n for n in SG.CASES if n != "x_only"]
KEYS = ("x", "dt", "A", "B", "C", "D", "z")
ULP8 = 8.0 * 2.0 ** -23


@pytest.fixture(scope="module")
def gold():
    return golden("scan_grad.npz")


@functools.lru_cache(maxsize=None)
def _want(name):
    """(inputs, fp64 gradients) of a case on the host, computed once and left unchanged."""
    inp, gr = SG.case_grad_f64(name)
    for v in list(inp.values()) + list(gr.values()):
        if v is not None:
            v.setflags(write=False)
    return inp, gr


@functools.lru_cache(maxsize=None)
def _dev(name):
    inp, _ = _want(name)
    return {k: None if v is None else torch.from_numpy(np.array(v)).cuda() for k, v in inp.items()}


def _run(d, needs=KEYS):
    """(out, {key: grad}) of selective_scan with the inputs in `needs` requiring grad."""
    t = {k: None if d[k] is None else d[k].clone().requires_grad_(k in needs) for k in KEYS}
    out = ssm.selective_scan(t["x"], t["dt"], t["A"], t["B"], t["C"], t["D"], t["z"])
    out.backward(d["g"])
    return out.detach(), {k: None if t[k] is None else t[k].grad for k in KEYS}


def _bound(gold, name, k):
    return max(4.0 * float(gold[f"{name}/e_ref/{k}"]), ULP8 * float(gold[f"{name}/gmax/{k}"]))


_worst = {}


@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_match_fp64(name, gold):
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
        e_ref, tol = float(gold[f"{name}/e_ref/d{k}"]), _bound(gold, name, "d" + k)
        e_hip = float(np.abs(g.cpu().numpy().astype(np.float64) - want["d" + k]).max())
        # (l1's dA is exactly 0, h_{-1} = 0: bound 0, and the device gives exact zeros)
        ratio = e_hip / tol if tol > 0 else (0.0 if e_hip == 0 else float("inf"))
        _worst[(name, k)] = ratio
        print(f"{name} d{k}: e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  bound {tol:.3e}  ratio {ratio:.3f}  "
              f"(worst so far {max(_worst.values()):.3f})")
        record_metric("scan_grad_abs_err", case=name, tensor="d" + k, e_ref=e_ref, e_hip=e_hip, bound=tol)
        if e_hip > tol:
            fails.append((k, e_hip, tol))
    record_metric("scan_grad_worst_ratio", case=name, ratio=max(v for (n, _), v in _worst.items() if n == name))
    assert not fails, (name, fails)


def _packed(d, z):
    """ops-level operands of a case: (xz (M, 2Di), dt, bc (M, 2N') padded, A', A2', D, N')."""
    B, L, Di = d["x"].shape
    N = d["A"].numel()
    bc, Ap = ssm._pad_states(d["B"], d["C"], d["A"], N, ops.scan_state_dim(N))
    A2 = Ap * torch.tensor(ops.LOG2E, dtype=torch.float32)
    xz = torch.cat([d["x"].reshape(B * L, Di), z.reshape(B * L, Di)], 1)
    return xz, d["dt"].reshape(B * L, Di).contiguous(), bc, Ap, A2, d["D"]


@pytest.mark.parametrize("name", ["l1", "l17", "l501", "n16", "n32", "n128", "n48", "di48_b2_l37", "big_dt"])
def test_training_forward_is_bitwise_the_inference_kernel(name):
    d = _dev(name)
    B, L, Di = d["x"].shape
    xz, dt, bc, Ap, A2, D = _packed(d, d["z"])
    want = ops.ssm_scan(xz, dt, bc, A2, D, B, L, 1).view(B, L, Di)
    out, _ = _run(d)
    assert torch.equal(out, want)
    with torch.no_grad():  # nothing requires grad: the inference kernel itself
        assert torch.equal(ssm.selective_scan(d["x"], d["dt"], d["A"], d["B"], d["C"], d["D"], d["z"]), want)
    # ungated: the gated launch at z = 128, whose gate is exactly 128, divided out (module docstring)
    unit = torch.full_like(d["x"], 128.0)
    assert torch.equal(unit * torch.sigmoid(unit), unit)
    y = ops.ssm_scan(_packed(d, unit)[0], dt, bc, A2, D, B, L, 1).view(B, L, Di) / 128.0
    t = {k: d[k].clone().requires_grad_() for k in ("x", "dt", "A", "B", "C", "D")}
    assert torch.equal(ssm.selective_scan(**t).detach(), y)
    assert torch.equal(ssm.selective_scan(d["x"], d["dt"], d["A"], d["B"], d["C"], d["D"]), y)


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


@pytest.mark.parametrize("name", ["l17", "n48", "ungated"])
def test_no_stale_reads_of_workspace_or_outputs(name):
    """Checkpoints aside, everything the backward is handed to write -- outputs and the partial-sum
    workspace -- pre-filled with NaN changes nothing: every element is written before it is read."""
    d = _dev(name)
    B, L, Di = d["x"].shape
    M = B * L
    xz, dt, bc, Ap, A2, D = _packed(d, d["z"] if d["z"] is not None else d["x"])
    x, z = xz[:, :Di], (xz[:, Di:] if d["z"] is not None else None)
    N = A2.numel()
    g = d["g"].reshape(M, Di).contiguous()
    out, ckpt = ops.ssm_scan_save(x if z is not None else x.contiguous(), z, dt, bc, A2, D, B, L)
    x = x if z is not None else x.contiguous()
    clean = ops.ssm_scan_bwd(x, z, dt, bc, Ap, A2, D, g, ckpt, B, L)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")  # noqa: E731
    dirty = dict(dx=nan(M, Di), ddt=nan(M, Di), dz=nan(M, Di) if z is not None else None, dB=nan(M, N), dC=nan(M, N),
                 dA_part=nan(B, Di, N), dD_part=nan(B, Di))
    ws = nan(ops.L.lib().vasr_ssm_scan_bwd_workspace_floats(B, L, Di, N))
    got = ops.ssm_scan_bwd(x, z, dt, bc, Ap, A2, D, g, ckpt, B, L, out=dirty, workspace=ws)
    for k, v in clean.items():
        assert (v is None and got[k] is None) or (torch.isfinite(got[k]).all() and torch.equal(got[k], v)), k


def test_forward_differentiable_reaches_every_parameter(gold):
    sd, x, g = SG.module_state()
    m = ssm.SelectiveSSM(d_model=SG.MODULE["d_model"], state_dim=SG.MODULE["state_dim"],
                         expand_ratio=SG.MODULE["expand_ratio"], scan_mode="sequential")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m = m.cuda()
    xt = torch.from_numpy(x).cuda().requires_grad_()
    out = m.forward_differentiable(xt)
    with torch.no_grad():  # the inference forward of the same module (its own GEMMs): close, not bitwise
        assert torch.allclose(out, m.eval()(xt), atol=1e-4, rtol=1e-4)
    (out * torch.from_numpy(g).cuda()).sum().backward()
    want = SG.module_grad_f64(sd, x, g)
    got = {k: p.grad for k, p in m.named_parameters()}
    got["input"] = xt.grad
    assert set(got) == set(SG.MODULE_GRADS)
    fails = []
    for k in SG.MODULE_GRADS:
        assert got[k] is not None and torch.isfinite(got[k]).all(), k
        e_ref = float(gold[f"module/e_ref/{k}"])
        tol = max(4.0 * e_ref, ULP8 * float(gold[f"module/gmax/{k}"]))
        e_hip = float(np.abs(got[k].cpu().numpy().astype(np.float64) - want[k]).max())
        print(f"module {k}: e_ref {e_ref:.3e}  e_hip {e_hip:.3e}  bound {tol:.3e}  ratio {e_hip / tol:.3f}")
        record_metric("scan_grad_abs_err", case="module", tensor=k, e_ref=e_ref, e_hip=e_hip, bound=tol)
        if e_hip > tol:
            fails.append((k, e_hip, tol))
    assert not fails, fails
    mamba = ssm.SelectiveSSM(d_model=8, state_dim=64, scan_mode="mamba").cuda()
    mamba.load_state_dict(m.state_dict())
    assert torch.equal(mamba.forward_differentiable(xt).detach(), out.detach())
