"""Host tests of the differentiable selective scan: the fp64 yardstick of the GPU tests
(tests/golden/gen_scan_grad_goldens.py: scan_grad_f64, module_grad_f64) against the reference's fp64
autograd gradients in tests/golden/scan_grad.npz, the fixture's input checksums, and the argument
checks of velocity_asr.ssm.selective_scan / SelectiveSSM.forward_differentiable that run before any
kernel.  No GPU is needed.

scan_grad_f64 is pinned per gradient tensor to 1e-10 of the tensor's largest entry (gmax); measured
when the fixture was written: 1.1e-15 at worst (n128)."""

import functools
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import gen_scan_grad_goldens as SG  # noqa: E402

from velocity_asr import ssm  # noqa: E402

CASE_NAMES = sorted(SG.CASES)


@pytest.fixture(scope="module")
def gold():
    return golden("scan_grad.npz")


@functools.lru_cache(maxsize=None)
def _case(name):
    return SG.case_grad_f64(name)


def test_fixture_lists_every_case(gold):
    assert list(gold["names"]) == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_inputs_match_the_stored_checksum(name, gold):
    inp, _ = _case(name)
    assert np.array_equal(SG.inputs_sha(inp), gold[f"{name}/sha"])
    assert (inp["z"] is None) == (not SG.CASES[name].get("gated", True))
    if SG.CASES[name].get("big_dt"):
        assert 5.0 < float(inp["dt"].max()) <= 6.0
        # a = exp(dt A) underflows to 0 in float32 for most n at the larger dt
        assert (np.exp(inp["dt"].astype(np.float64).max() * inp["A"]) < 1e-45).mean() > 0.5


@pytest.mark.parametrize("name", CASE_NAMES)
def test_scan_grad_f64_matches_the_reference(name, gold):
    c = SG.CASES[name]
    _, own = _case(name)
    full = SG.is_full(c)
    for k in SG.GRADS:
        if own[k] is None:
            assert k == "dz" and f"{name}/gmax/{k}" not in gold.files
            continue
        tol = 1e-10 * float(gold[f"{name}/gmax/{k}"])
        if k not in SG.PER_FRAME or full:
            assert np.abs(own[k] - gold[f"{name}/{k}"]).max() <= tol, (name, k)
            continue
        frames = gold[f"{name}/frames"]
        assert np.array_equal(frames, SG.sample_frames(c))
        at = np.stack([own[k][b][frames[b]] for b in range(c["B"])])
        assert np.abs(at - gold[f"{name}/{k}_at"]).max() <= tol, (name, k)
        # a frame's sum has up to Di (or N) terms of size <= gmax
        assert np.abs(own[k].sum(axis=2) - gold[f"{name}/{k}_rowsum"]).max() <= tol * own[k].shape[2], (name, k)


def test_module_grad_f64_matches_the_reference(gold):
    sd, x, g = SG.module_state()
    own = SG.module_grad_f64(sd, x, g)
    for k in SG.MODULE_GRADS:
        assert np.abs(own[k] - gold[f"module/{k}"]).max() <= 1e-10 * float(gold[f"module/gmax/{k}"]), k


def _args(B=1, L=5, Di=16, N=64, dtype=torch.float32):
    t = lambda *s: torch.zeros(*s, dtype=dtype)  # noqa: E731
    return dict(x=t(B, L, Di), dt=t(B, L, Di), A=t(N), B=t(B, L, N), C=t(B, L, N), D=t(Di), z=t(B, L, Di))


@pytest.mark.parametrize("bad", [
    dict(x=torch.zeros(5, 16)),                      # rank
    dict(A=torch.zeros(1, 64)),
    dict(D=torch.zeros(1, 16)),
    dict(z=torch.zeros(5, 16)),
    dict(dt=torch.zeros(1, 5, 8)),                   # shape
    dict(B=torch.zeros(1, 5, 32)),
    dict(C=torch.zeros(1, 4, 64)),
    dict(D=torch.zeros(8)),
    dict(z=torch.zeros(2, 5, 16)),
    dict(x=torch.zeros(1, 5, 16, dtype=torch.float64)),   # dtype
    dict(dt=torch.zeros(1, 5, 16, dtype=torch.bfloat16)),
    dict(A=torch.zeros(64, dtype=torch.float16)),
    dict(B=torch.zeros(1, 5, 64, dtype=torch.int32)),
])
def test_selective_scan_refuses_bad_arguments(bad):
    a = _args()
    a.update(bad)
    with pytest.raises(ValueError, match="selective_scan"):
        ssm.selective_scan(**a)


def test_selective_scan_refuses_a_channel_count_the_kernel_cannot_split():
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):  # shapes are fine: the device check is next
            ssm.selective_scan(**_args())
        return
    a = {k: v.cuda() for k, v in _args(Di=24).items()}
    with pytest.raises(ValueError, match="multiple of 16"):
        ssm.selective_scan(**a)


def test_forward_differentiable_is_for_the_recurrence_only():
    m = ssm.SelectiveSSM(d_model=8, state_dim=64, expand_ratio=2, scan_mode="parallel")
    with pytest.raises(NotImplementedError, match="tree scan"):
        m.forward_differentiable(torch.zeros(1, 4, 8))
    for mode in ("sequential", "mamba"):
        assert hasattr(ssm.SelectiveSSM(d_model=8, state_dim=64, scan_mode=mode), "forward_differentiable")


def test_abi_refuses_bad_backward_arguments():
    from velocity_asr import _lib
    L = _lib.load()
    assert L.vasr_ssm_scan_checkpoint_floats(32, 501, 384, 64) == 32 * 32 * 384 * 64
    assert L.vasr_ssm_scan_bwd_workspace_floats(32, 501, 384, 64) == 2 * 32 * 501 * 24 * 64
    fake = 256  # aligned non-null pointer values: the checks return before any dereference
    rc = L.vasr_ssm_scan_save_f32(None, 0, None, 0, None, 0, None, None, None, 0, 1, 1, 16, 64, 1, None, 0, None)
    assert rc == -1 and b"null" in L.vasr_last_error()
    rc = L.vasr_ssm_scan_save_f32(fake, 32, fake, 16, fake, 128, fake, fake, fake, 16, 1, 20, 16, 64, 1, fake, 1024, None)
    assert rc == -1 and b"checkpoints of 1024 floats, 2048 needed" in L.vasr_last_error()
    rc = L.vasr_ssm_scan_save_f32(fake, 32, fake, 16, fake, 96, fake, fake, fake, 16, 1, 20, 16, 48, 1, fake, 4096, None)
    assert rc == -2 and b"state dim" in L.vasr_last_error()
    bwd = lambda z, dz, Di, ws: L.vasr_ssm_scan_bwd_f32(fake, Di, z, Di, fake, Di, fake, 128, fake, fake, fake, fake,  # noqa: E731
                                                        Di, fake, fake, fake, dz, fake, fake, fake, fake, fake, ws, 1, 20,
                                                        Di, 64, None)
    assert bwd(fake, None, 16, 1 << 20) == -1 and b"go together" in L.vasr_last_error()
    assert bwd(fake, fake, 24, 1 << 20) == -2 and b"multiple of 16" in L.vasr_last_error()
    assert bwd(fake, fake, 16, 100) == -1 and b"workspace" in L.vasr_last_error()
