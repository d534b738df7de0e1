"""Host-side tests of the differentiable CTC loss: the three new C entry points are declared,
exported and bound under ABI 20, their argument checks return before any launch (so no GPU is
needed), CTCLoss(differentiable=True) constructs, and the fp64 gradient of
tests/golden/gen_ctc_grad_goldens.py (ctc_grad_f64, the yardstick of the GPU tests) agrees with the
reference-made data of tests/golden/ctc_grad.npz."""

import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import gen_ctc_goldens as G  # noqa: E402
import gen_ctc_grad_goldens as GG  # noqa: E402  (our generator's helpers; the reference is not imported)

FAKE = 256  # aligned non-null pointer value: the checks return before any dereference
NEW = ("vasr_ctc_loss_alpha_f32", "vasr_ctc_occupancy_f32", "vasr_ctc_grad_logits_f32")


@pytest.fixture(scope="module")
def lib():
    from velocity_asr import _lib
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound_under_abi_20(lib):
    import velocity_asr as v
    from velocity_asr import _lib, ops

    assert _lib.ABI_VERSION == 21 and lib.vasr_version() == 21
    for name in NEW:
        assert name in _lib.header_functions() and name in _lib._SIGNATURES and hasattr(lib, name)
    for name in ("ctc_loss_alpha", "ctc_occupancy", "ctc_grad_logits"):
        assert callable(getattr(ops, name))
    assert "CTCLoss" not in v.__all__


def test_differentiable_loss_constructs():
    from velocity_asr.training import CTCLoss

    loss = CTCLoss(differentiable=True)
    assert (loss.blank_token, loss.reduction, loss.zero_infinity, loss.differentiable) == (0, "mean", True, True)
    assert CTCLoss().differentiable is False
    assert CTCLoss(0, "sum", False, differentiable=True).reduction == "sum"


def _alpha(lib, emis=FAKE, L=8, Smax=3, targets=FAKE, frames=FAKE, tlen=FAKE, out=FAKE, alpha=FAKE, elems=None):
    elems = L * (2 * Smax + 1) if elems is None else elems
    return lib.vasr_ctc_loss_alpha_f32(emis, 1, L, Smax, targets, frames, tlen, out, alpha, elems, None)


def _occupancy(lib, emis=FAKE, alpha=FAKE, nll=FAKE, L=8, Smax=3, targets=FAKE, frames=FAKE, tlen=FAKE, occ=FAKE,
               elems=None):
    elems = L * (2 * Smax + 1) if elems is None else elems
    return lib.vasr_ctc_occupancy_f32(emis, alpha, elems, nll, 1, L, Smax, targets, frames, tlen, occ, None)


def _grad(lib, logits=FAKE, L=8, V=10, targets=FAKE, Smax=3, frames=FAKE, tlen=FAKE, blank=0, occ=FAKE, scale=FAKE,
          ws=FAKE, elems=None, grad=FAKE):
    elems = Smax + 1 if elems is None else elems
    return lib.vasr_ctc_grad_logits_f32(logits, V, L * V, 1, L, V, targets, Smax, frames, tlen, blank, occ, scale, ws,
                                        elems, grad, None)


CALLS = ((_alpha, ("emis", "targets", "frames", "tlen", "out", "alpha")),
         (_occupancy, ("emis", "alpha", "nll", "targets", "frames", "tlen", "occ")),
         (_grad, ("logits", "targets", "frames", "tlen", "occ", "scale", "ws", "grad")))


def test_null_pointers_are_rejected(lib):
    for call, names in CALLS:
        for n in names:
            assert call(lib, **{n: None}) == -1, (call.__name__, n)
            assert b"null" in lib.vasr_last_error(), (call.__name__, n)


def test_more_than_8192_frames_is_rejected(lib):
    for call, _ in CALLS:
        assert call(lib, L=8193) == -1, call.__name__
        assert b"8192" in lib.vasr_last_error()


def test_targets_above_2048_are_unsupported(lib):
    for call, _ in CALLS:
        assert call(lib, Smax=2049) == -2, call.__name__  # VASR_EUNSUPPORTED
        assert b"2048" in lib.vasr_last_error()


def test_too_small_buffers_are_rejected(lib):
    for call, need in ((_alpha, 8 * 7), (_occupancy, 8 * 7), (_grad, 4)):
        for elems in (need - 1, 0):
            assert call(lib, elems=elems) == -1, (call.__name__, elems)
            assert b"needed" in lib.vasr_last_error()
    for blank in (-1, 10):
        assert _grad(lib, V=10, blank=blank) == -1
        assert b"blank" in lib.vasr_last_error()


@pytest.fixture(scope="module")
def gold():
    return golden("ctc_grad.npz")


@pytest.mark.parametrize("name", sorted(G.CASES))
def test_fp64_gradient_agrees_with_the_reference(name, gold):
    """ctc_grad_f64 against the fp64 reference gradient stored with the fixture, 1e-9 absolute
    (fp64 against fp64): every entry of the small cases; of the larger ones the blank-and-target
    columns and a sample of other columns at the stored frames, and every row's sum.  The
    non-finite entries are the reference's: none with zero_infinity, the infeasible utterance's
    20 without."""
    assert sorted(gold["names"].tolist()) == sorted(G.CASES)
    c = G.CASES[name]
    tg, ilen, tlen = G.make_targets(c)
    x = G.make_logits(c).numpy()
    own = GG.case_grad_f64(c, x, tg, ilen, tlen, "sum", True)
    raw = GG.case_grad_f64(c, x, tg, ilen, tlen, "sum", False)
    assert np.isfinite(own).all() and int(gold[f"{name}/nonfinite_zi1"]) == 0
    assert int((~np.isfinite(raw)).sum()) == int(gold[f"{name}/nonfinite_zi0"])
    assert 0 < float(gold[f"{name}/e_ref"]) < 2e-3
    for b in range(c["B"]):
        assert not own[b, int(ilen[b]):].any()
    if c["B"] * c["L"] * c["V"] <= GG.FULL_LIMIT:
        assert np.abs(own - gold[f"{name}/grad_sum"]).max() <= 1e-9
        mean = GG.case_grad_f64(c, x, tg, ilen, tlen, "mean", True)
        assert np.abs(mean - gold[f"{name}/grad_mean"]).max() <= 1e-9
        assert np.array_equal(~np.isfinite(raw), gold[f"{name}/mask_zi0"])
        return
    frames, cols = gold[f"{name}/frames"], gold[f"{name}/cols"]
    assert np.array_equal(frames, GG.sample_frames(c, ilen, c["seed"]))
    assert np.array_equal(cols, GG.sample_columns(c, tg, c["seed"]))
    assert np.abs(GG.by_slot(own, tg, frames) - gold[f"{name}/slots"]).max() <= 1e-9
    other = np.stack([own[b][frames[b]][:, cols] for b in range(c["B"])])
    assert np.abs(other - gold[f"{name}/other"]).max(initial=0.0) <= 1e-9  # V = 20 / 50: every column is a target's
    assert np.abs(own.sum(axis=2) - gold[f"{name}/rowsum"]).max() <= 1e-9


def test_infeasible_case_of_the_fixture(gold):
    """Without zero_infinity the reference's gradient of the infeasible utterance is non-finite in
    all of its 4 x 5 entries and the neighbour's is finite; with it, exactly 0."""
    mask = gold["infeasible/mask_zi0"]
    assert mask[0].all() and not mask[1].any() and int(gold["infeasible/nonfinite_zi0"]) == 20
    assert not gold["infeasible/grad_sum"][0].any() and gold["infeasible/grad_sum"][1].any()
