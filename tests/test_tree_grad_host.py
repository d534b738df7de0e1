"""Host tests of the differentiable tree scan (scan_mode="parallel"): the fp64 yardsticks of the GPU
tests (tests/golden/gen_tree_grad_goldens.py: tree_grad_f64, module_grad_f64) against the reference's
fp64 autograd gradients in tests/golden/tree_grad.npz, the closed form of the tree's state against
the oracle's tree, the new C entry points' declarations and argument checks, and the workspace
condition.  No GPU is needed.

tree_grad_f64 and module_grad_f64 are pinned per gradient tensor to 1e-10 of the tensor's largest
entry (gmax); measured when the fixture was written: 2.8e-15 (l501) and 4.2e-15 (global) at worst."""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, golden

sys.path.insert(0, GOLDEN)
import gen_tree_grad_goldens as TG  # noqa: E402

from oracle import velocity_ref as R  # noqa: E402
from velocity_asr import ssm  # noqa: E402

CASE_NAMES = sorted(TG.CASES)


@pytest.fixture(scope="module")
def gold():
    return golden("tree_grad.npz")


@functools.lru_cache(maxsize=None)
def _case(name):
    return TG.case_grad_f64(name)


def test_fixture_lists_every_case(gold):
    assert list(gold["names"]) == CASE_NAMES
    assert list(gold["modules"]) == sorted(TG.MODULES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_inputs_match_the_stored_checksum(name, gold):
    inp, _ = _case(name)
    assert np.array_equal(TG.inputs_sha(inp), gold[f"{name}/sha"])
    assert (inp["z"] is None) == (not TG.CASES[name].get("gated", True))
    if TG.CASES[name].get("big_dt"):
        assert 3.5 < float(inp["dt"].max()) <= 4.0
        # a = exp(dt A) underflows to 0 in float32 for the larger n at the larger dt
        assert (np.exp(inp["dt"].astype(np.float64).max() * inp["A"]) < 1e-45).mean() > 0.4


@pytest.mark.parametrize("name", CASE_NAMES)
def test_tree_grad_f64_matches_the_reference(name, gold):
    c = TG.CASES[name]
    _, own = _case(name)
    full = TG.is_full(c)
    for k in TG.GRADS:
        if own[k] is None:
            assert k == "dz" and f"{name}/gmax/{k}" not in gold.files
            continue
        tol = 1e-10 * float(gold[f"{name}/gmax/{k}"])
        if k not in TG.PER_FRAME or full:
            assert np.abs(own[k] - gold[f"{name}/{k}"]).max() <= tol, (name, k)
            continue
        frames = gold[f"{name}/frames"]
        assert np.array_equal(frames, TG.sample_frames(c))
        at = np.stack([own[k][b][frames[b]] for b in range(c["B"])])
        assert np.abs(at - gold[f"{name}/{k}_at"]).max() <= tol, (name, k)
        # a frame's sum has up to Di (or N) terms of size <= gmax
        assert np.abs(own[k].sum(axis=2) - gold[f"{name}/{k}_rowsum"]).max() <= tol * own[k].shape[2], (name, k)


def test_one_step_has_no_state(gold):
    """L = 1: h_0 = 0 whatever the inputs, so dA = dB = dC = ddt = 0 exactly and dx = gy D."""
    inp, own = _case("l1")
    for k in ("dA", "dB", "dC", "ddt"):
        assert not own[k].any() and float(gold[f"l1/gmax/{k}"]) == 0.0, k
    z = inp["z"].astype(np.float64)
    assert np.allclose(own["dx"], inp["g"] * z / (1.0 + np.exp(-z)) * inp["D"].astype(np.float64), rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", sorted(TG.MODULES))
def test_module_grad_f64_matches_the_reference(name, gold):
    own = TG.module_grad_f64(name)
    assert sorted(own) == TG.module_grad_names(name)
    for k in own:
        assert own[k].shape == gold[f"{name}/{k}"].shape, k
        assert np.abs(own[k] - gold[f"{name}/{k}"]).max() <= 1e-10 * float(gold[f"{name}/gmax/{k}"]), k


@pytest.mark.parametrize("L", [1, 2, 3, 5, 16, 17, 37, 64, 100])
def test_closed_form_state_is_the_oracles_tree(L):
    """tree_state_f64 (h_t = sum over the set bits of t of P_e R_S) against the oracle's tree scan:
    oracle.parallel_scan's own scan (associative_scan_stream, which takes the arrays' dtype) in
    float64, and parallel_scan itself, which rounds to float32, to float32 accuracy."""
    r = np.random.RandomState(L)
    Bsz, Di, N = 2, 3, 4
    x, Bm, Cm = (r.standard_normal(s) for s in ((Bsz, L, Di), (Bsz, L, N), (Bsz, L, N)))
    dt = np.log1p(np.exp(r.standard_normal((Bsz, L, Di)) - 1.0))
    A, D = -np.arange(1.0, N + 1), r.standard_normal(Di)
    a = np.exp(dt[..., None] * A)
    b = (x * dt)[..., None] * Bm[:, :, None, :]
    h = TG.tree_state_f64(a, b)
    want = R.associative_scan_stream(a, b)
    assert want.dtype == np.float64
    assert np.abs(h - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert not h[:, 0].any()
    y = np.einsum("bldn,bln->bld", h, Cm) + x * D
    f = lambda v: v.astype(np.float32)  # noqa: E731
    y32 = R.parallel_scan(f(x), f(dt), f(A), f(Bm), f(Cm), f(D))
    assert np.abs(y - y32).max() <= 2e-5 * max(np.abs(y).max(), 1.0)
    out, _ = TG.tree_grad_f64(x, dt, A, Bm, Cm, D, None, np.zeros_like(x))
    assert np.array_equal(out, y)


def _args(B=1, L=5, Di=16, N=64):
    t = lambda *s: torch.zeros(*s)  # noqa: E731
    return dict(x=t(B, L, Di), dt=t(B, L, Di), A=t(N), B=t(B, L, N), C=t(B, L, N), D=t(Di), z=t(B, L, Di))


def test_selective_scan_refuses_an_unknown_scan_mode():
    with pytest.raises(ValueError, match="scan_mode"):
        ssm.selective_scan(**_args(), scan_mode="bogus")
    a = _args()
    a["B"] = torch.zeros(1, 5, 32)  # the same validation for the tree
    with pytest.raises(ValueError, match="selective_scan"):
        ssm.selective_scan(**a, scan_mode="parallel")


def test_modules_have_the_differentiable_forward():
    m = ssm.SelectiveSSM(d_model=8, state_dim=64, expand_ratio=2, scan_mode="parallel")
    with pytest.raises(NotImplementedError, match="tree scan"):  # the default keeps refusing the tree
        m.forward_differentiable(torch.zeros(1, 4, 8))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):  # tree_scan=True passes on to the device check
            m.forward_differentiable(torch.zeros(1, 4, 8), tree_scan=True)
    for cls in (ssm.SSMBlock, ssm.LocalSSMProcessor, ssm.GlobalSSM):
        assert callable(getattr(cls, "forward_differentiable"))


def test_abi_declares_and_exports_the_tree_backward():
    from velocity_asr import _lib
    names = _lib.header_functions()
    L = _lib.load()
    header = open(f"{REPO}/include/vasr.h").read()
    for n in ("vasr_ssm_tree_bwd_f32", "vasr_ssm_tree_bwd_workspace_floats"):
        assert n in names and n in _lib._SIGNATURES and hasattr(L, n) and f" {n}(" in header, n
    assert L.vasr_version() == _lib.ABI_VERSION


def test_workspace_is_below_half_a_state_array():
    """A per-step state array is B L Di N floats; the backward keeps 7 floats per 16-step chunk,
    channel and state, and one dD partial per chunk and channel."""
    from velocity_asr import _lib
    L = _lib.load()
    B, Lq, Di, N = 32, 501, 384, 64
    got = L.vasr_ssm_tree_bwd_workspace_floats(B, Lq, Di, N)
    assert got == B * 32 * Di * (7 * N + 1)
    assert 0 < got < B * Lq * Di * N // 2
    assert L.vasr_ssm_tree_bwd_workspace_floats(32, 64, 384, 32) == 32 * 4 * 384 * (7 * 32 + 1)
    assert L.vasr_ssm_tree_bwd_workspace_floats(1, 1, 16, 48) == 0  # no kernel instance: pad to 64


def test_abi_refuses_bad_tree_backward_arguments():
    from velocity_asr import _lib
    L = _lib.load()
    fake = 256  # aligned non-null pointer values: the checks return before any dereference or launch
    bwd = lambda z, dz, Di, ws, N=64, Lq=20, wsp=fake: L.vasr_ssm_tree_bwd_f32(  # noqa: E731
        fake, Di, z, Di, fake, Di, fake, 2 * N, fake, fake, fake, fake, Di, fake, fake, dz, fake, fake, fake, fake, wsp,
        ws, 1, Lq, Di, N, None)
    rc = L.vasr_ssm_tree_bwd_f32(None, 0, None, 0, None, 0, None, 0, None, None, None, None, 0, None, None, None, None,
                                 None, None, None, None, 0, 1, 1, 16, 64, None)
    assert rc == -1 and b"null" in L.vasr_last_error()
    assert bwd(fake, None, 16, 1 << 20) == -1 and b"go together" in L.vasr_last_error()
    assert bwd(fake, fake, 16, 1 << 20, Lq=8193) == -1 and b"bad shape" in L.vasr_last_error()
    assert bwd(fake, fake, 16, 1 << 20, N=48) == -2 and b"state dim" in L.vasr_last_error()
    assert bwd(fake, fake, 24, 1 << 20) == -2 and b"multiple of 16" in L.vasr_last_error()
    need = 2 * 16 * (7 * 64 + 1)
    assert bwd(fake, fake, 16, need - 1) == -1 and f"workspace of {need - 1} floats, {need} needed".encode() in L.vasr_last_error()
    assert bwd(fake, fake, 16, need, wsp=260) == -1 and b"16-byte aligned" in L.vasr_last_error()
    assert bwd(fake, fake, 16, 0, Lq=0) == 0  # nothing to do: no launch
