"""Host-side tests of the CTC loss / forced alignment feature: imports, argument checks of the new
C entry points (all before any launch, so no GPU is needed), the workspace formula, and the
fixture tests/golden/ctc_loss.npz itself (its fp64 lattice against the reference's fp32 values)."""

import sys

import numpy as np
import pytest

from conftest import GOLDEN, golden

sys.path.insert(0, GOLDEN)
import gen_ctc_goldens as G  # noqa: E402  (our generator's helpers; the reference is not imported)

FAKE = 256  # aligned non-null pointer value: the checks return before any dereference


@pytest.fixture(scope="module")
def lib():
    from velocity_asr import _lib
    return _lib.load()


def test_new_names_import_and_public_all_is_unchanged():
    import velocity_asr as v
    from velocity_asr.decode import CTCDecoder, ctc_forced_align
    from velocity_asr.training import CTCLoss

    assert callable(ctc_forced_align) and hasattr(CTCDecoder, "align")
    loss = CTCLoss()
    assert (loss.blank_token, loss.reduction, loss.zero_infinity) == (0, "mean", True)
    with pytest.raises(ValueError):
        CTCLoss(reduction="average")
    for name in ("CTCLoss", "ctc_forced_align"):
        assert name not in v.__all__


def test_abi_version_20_and_bindings(lib):
    from velocity_asr import _lib
    assert _lib.ABI_VERSION == 21 and lib.vasr_version() == 21
    for name in ("vasr_ctc_emissions_f32", "vasr_ctc_loss_f32", "vasr_ctc_align_f32",
                 "vasr_ctc_align_workspace_bytes"):
        assert name in _lib.header_functions() and name in _lib._SIGNATURES


def _emissions(lib, logits=FAKE, L=8, V=10, targets=FAKE, Smax=3, frames=FAKE, tlen=FAKE, blank=0, emis=FAKE):
    return lib.vasr_ctc_emissions_f32(logits, V, L * V, 1, L, V, targets, Smax, frames, tlen, blank, emis, None)


def _loss(lib, emis=FAKE, L=8, Smax=3, targets=FAKE, frames=FAKE, tlen=FAKE, out=FAKE):
    return lib.vasr_ctc_loss_f32(emis, 1, L, Smax, targets, frames, tlen, out, None)


def _align(lib, emis=FAKE, L=8, Smax=3, targets=FAKE, frames=FAKE, tlen=FAKE, ws=FAKE, ws_bytes=None, state=FAKE,
           st=FAKE, en=FAKE, score=FAKE):
    if ws_bytes is None:
        ws_bytes = lib.vasr_ctc_align_workspace_bytes(1, L, Smax)
    return lib.vasr_ctc_align_f32(emis, 1, L, Smax, targets, frames, tlen, ws, ws_bytes, state, st, en, score, None)


def test_null_pointers_are_rejected(lib):
    for call, names in ((_emissions, ("logits", "targets", "frames", "tlen", "emis")),
                        (_loss, ("emis", "targets", "frames", "tlen", "out")),
                        (_align, ("emis", "targets", "frames", "tlen", "ws", "state", "st", "en", "score"))):
        for n in names:
            assert call(lib, **{n: None}) == -1, (call.__name__, n)
            assert b"null" in lib.vasr_last_error(), (call.__name__, n)


def test_blank_outside_the_vocabulary_is_rejected(lib):
    for blank in (-1, 10, 11):
        assert _emissions(lib, V=10, blank=blank) == -1
        assert b"blank" in lib.vasr_last_error()


def test_more_than_8192_frames_is_rejected(lib):
    for call in (_emissions, _loss, _align):
        assert call(lib, L=8193) == -1
        assert b"8192" in lib.vasr_last_error()


def test_too_small_a_workspace_is_rejected(lib):
    need = lib.vasr_ctc_align_workspace_bytes(1, 8, 3)
    assert _align(lib, ws_bytes=need - 1) == -1
    assert b"workspace" in lib.vasr_last_error()
    assert _align(lib, ws_bytes=0) == -1


def test_targets_above_2048_are_unsupported(lib):
    for call in (_emissions, _loss, _align):
        assert call(lib, Smax=2049) == -2, call.__name__  # VASR_EUNSUPPORTED
        assert b"2048" in lib.vasr_last_error()


def test_align_workspace_formula(lib):
    """include/vasr.h: B * L * 4 * ceil((2 Smax + 1) / 16) bytes (2 bits per (t, s), rows padded to words)."""
    for B, L, S in ((1, 1, 0), (1, 8, 3), (2, 33, 12), (3, 140, 64), (32, 501, 100), (1, 8192, 2048), (2, 7, 7),
                    (2, 7, 8)):
        assert lib.vasr_ctc_align_workspace_bytes(B, L, S) == B * L * 4 * -(-(2 * S + 1) // 16)


def test_fixture_fp64_lattice_agrees_with_the_reference():
    """Pins tests/golden/ctc_loss.npz: the inputs regenerate from their seeds, the fp64 lattice
    recomputed here equals the stored one, and the reference's stored fp32 losses sit within fp32
    accuracy of it: 1.5e-6 relative, a few times the ~3e-7 the reference shows at these shapes."""
    g = golden("ctc_loss.npz")
    assert sorted(g["names"].tolist()) == sorted(G.CASES)
    worst = 0.0
    for name, c in G.CASES.items():
        tg, ilen, tlen = G.make_targets(c)
        assert np.array_equal(tg, g[f"{name}/targets"]) and np.array_equal(ilen, g[f"{name}/ilen"])
        assert np.array_equal(tlen, g[f"{name}/tlen"])
        f64 = G.case_f64(c, G.make_logits(c), tg, ilen, tlen)
        np.testing.assert_allclose(f64, g[f"{name}/f64"], rtol=1e-12)
        ref = g[f"{name}/ref_none_zi0"].astype(np.float64)
        ok = np.isfinite(f64)
        assert np.array_equal(np.isfinite(ref), ok)
        rel = np.abs(ref[ok] - f64[ok]) / np.abs(f64[ok])
        worst = max(worst, float(rel.max()))
        assert rel.max() <= 1.5e-6, (name, rel)
        for zi in (0, 1):
            for red in ("none", "mean", "sum"):
                want = G.reduce_f64(f64, tlen, red, bool(zi))
                got = g[f"{name}/ref_{red}_zi{zi}"].astype(np.float64)
                np.testing.assert_allclose(g[f"{name}/f64_{red}_zi{zi}"], want, rtol=1e-12)
                if np.isfinite(want).all():
                    np.testing.assert_allclose(got, want, rtol=1.5e-6, err_msg=f"{name} {red} zi{zi}")
                else:
                    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    print(f"reference fp32 vs fp64, largest relative error: {worst:.3e}")
    inf = g["infeasible/ref_none_zi0"]
    assert np.isposinf(inf[0]) and np.isfinite(inf[1]) and g["infeasible/ref_none_zi1"][0] == 0.0


def test_fixture_alignment_seeds_have_their_margin():
    g = golden("ctc_loss.npz")
    assert sorted(g["align_names"].tolist()) == sorted(G.ALIGN_CASES)
    for name, c in G.ALIGN_CASES.items():
        cc = dict(c, seed=int(g[f"align/{name}/seed"]))
        tg, _, _ = G.make_targets(cc)
        score, state, margin = G.viterbi_f64(G.make_logits(cc).numpy()[0], tg[0], c["L"])
        assert margin > G.ALIGN_MARGIN, (name, margin)
        assert np.array_equal(state, g[f"align/{name}/state"]) and abs(score - float(g[f"align/{name}/score"])) < 1e-9
