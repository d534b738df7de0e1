"""Evaluation-side pieces of reference velocity_asr/training.py: the CTC loss that
Trainer.eval_step scores a checkpoint with (training.py:47-104, :273-299) and the WER/CER
metrics scripts/evaluate.py imports (training.py:412-501).

CTCLoss here is the loss on the HIP path (vasr_ctc_emissions_f32 + vasr_ctc_loss_f32): by default
forward only, scoring a known transcript; with differentiable=True it also has a backward pass
(vasr_ctc_loss_alpha_f32 in the forward, vasr_ctc_occupancy_f32 + vasr_ctc_grad_logits_f32 in the
backward), so a PyTorch training loop can use it in place of F.log_softmax + nn.CTCLoss.

CTCHeadLoss is the same loss taken one layer earlier, on the CTC head's input: the head's GEMM keeps
each row's log-sum-exp in its epilogue (VASR_EPI_LSE) and only the blank's and the target tokens'
logits are formed (vasr_ctc_head_emissions_f32), so neither the (B, L, V) logits nor, with
differentiable=True, their gradient is ever allocated whole: the backward recomputes the logits a
chunk of utterances at a time, turns the chunk into its gradient in place
(vasr_ctc_grad_logits_stats_f32) and contracts it against the weight and the rows at once.  Its
memory is bounded by chunk_bytes, not by rows x vocabulary ("The loss on the head").
VELOCITYASR.ctc_loss, CTCOutputHead.ctc_emissions and CTCOutputHead.align are its forward-only users.

Of the model's own kernels both selective scans have a backward pass too (velocity_asr.ssm.selective_scan: the
recurrence of scan_mode "sequential" / "mamba", vasr_ssm_scan_save_f32 + vasr_ssm_scan_bwd_f32, and the default
"parallel" tree, the inference kernel + vasr_ssm_tree_bwd_f32), and SelectiveSSM, SSMBlock, LocalSSMProcessor and
GlobalSSM have a forward_differentiable built on them.  The global context's two non-GEMM kernels have one as
well (velocity_asr.attention.pooled_attention and adaptive_avg_pool: the inference kernels forwards,
vasr_pooled_attention_bwd_f32 and vasr_adaptive_pool_bwd_f32 backwards), and AdaptivePool, MultiHeadAttention,
GatedFusion and HierarchicalGlobalContext a forward_differentiable built on them (the attention's dropout on its
probabilities is not built: refused in train mode with dropout > 0).  The layers around these kernels are GEMM,
LayerNorm, conv and sigmoid, which torch.autograd differentiates as torch ops.  The rest of training (a
whole-model forward_differentiable, backward passes of the fused GEMM, tail and LayerNorm kernels, bf16,
schedulers, Trainer) stays outside this build's scope.

The metrics: compute_wer / compute_cer are the reference's (a Python Levenshtein loop) unless given a HIP
device, in which case error_counts scores all pairs in one launch of the batched edit-distance kernel
(vasr_edit_counts_i32) and they return the same float.  edit_counts_host is that kernel's specification:
substitution, deletion and insertion counts carried forward with the cost.
error_alignments returns the edit paths behind those counts (which item for which), on a HIP device from
vasr_edit_align_i32; edit_alignment_host is its specification, format_alignment and confusions read the
paths.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops


class _CTCNll(torch.autograd.Function):
    """Per-utterance nll (B,) of float32 device logits, with the gradient to them; targets and
    lengths in ops.ctc_emissions' device forms.  Forward: emissions + the lattice that keeps alpha.
    Backward: occupancy (beta walked over the same lattice) + one pass over the logits that writes
    scale[b] (softmax - occupancy); scale[b] is the upstream gradient of nll_b, replaced for an
    infeasible utterance (nll = +inf) by 0 under zero_infinity and by NaN otherwise, as the
    reference yields.  Everything is enqueued on the current stream: no host synchronisation."""

    @staticmethod
    def forward(ctx, logits, tg, frames, tlen, blank, zero_infinity):
        x = logits.detach()
        emis, tg, frames, tlen = ops.ctc_emissions(x, tg, frames, tlen, blank)
        nll, alpha = ops.ctc_loss_alpha(emis, tg, frames, tlen)
        ctx.save_for_backward(x, emis, alpha, nll, tg, frames, tlen)
        ctx.blank, ctx.zero_infinity = blank, zero_infinity
        return nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_nll):
        x, emis, alpha, nll, tg, frames, tlen = ctx.saved_tensors
        scale = grad_nll.to(dtype=torch.float32)
        infeasible = torch.full_like(scale, 0.0 if ctx.zero_infinity else float("nan"))
        scale = torch.where(torch.isinf(nll), infeasible, scale)
        occ = ops.ctc_occupancy(emis, alpha, nll, tg, frames, tlen)
        grad = ops.ctc_grad_logits(x, occ, tg, frames, tlen, scale.contiguous(), ctx.blank)
        return grad, None, None, None, None, None


class CTCLoss(nn.Module):
    """CTC loss with the reference's signature and values (training.py:47-104).

    The reference takes F.log_softmax of the (B, L, V) logits and calls nn.CTCLoss; here one pass
    over the logits keeps only the blank's and the target tokens' log-probabilities, and a lattice
    kernel sums the paths, so no (B, L, V) log-softmax tensor is ever allocated.  The result is a
    device tensor.  By default forward only: logits that require grad (outside torch.no_grad()) are
    refused.  With differentiable=True such logits get their gradient from the device backward
    pass (_CTCNll), in their own dtype and shape; the loss value is bitwise the forward-only one.

    Args:
        blank_token: index of the blank token
        reduction: 'mean' (mean over the batch of nll_b / max(target_length_b, 1)), 'sum', 'none'
        zero_infinity: replace the +inf loss of an infeasible target by 0 (and its gradient by 0)
        differentiable: give logits that require grad a backward pass instead of refusing them
    """

    def __init__(self, blank_token: int = 0, reduction: str = "mean", zero_infinity: bool = True, *,
                 differentiable: bool = False):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"CTCLoss: {reduction} is not a valid value for reduction")
        self.blank_token = blank_token
        self.reduction = reduction
        self.zero_infinity = zero_infinity
        self.differentiable = differentiable

    def forward(self, logits: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                target_lengths: torch.Tensor) -> torch.Tensor:
        """logits (B, L, V); targets (B, Smax), each row read up to its target length, or 1-D, all
        utterances' targets concatenated (entries equal to the blank are dropped first, as
        training.py:95-99); input_lengths, target_lengths (B,) on the device or the host."""
        from .decode import _on_device

        with_grad = logits.requires_grad and torch.is_grad_enabled()
        if with_grad and not self.differentiable:
            raise RuntimeError(
                "velocity_asr.training.CTCLoss is forward-only (evaluation): it has no backward pass. "
                "Call it under torch.no_grad() or on detached logits.")
        if logits.dim() != 3:
            raise ValueError("CTCLoss: logits must be (batch, seq_len, vocab_size)")
        B = logits.shape[0]
        if targets.dim() == 1:
            targets = self._pad_concatenated(targets, target_lengths, B)
        if with_grad:
            # the casts to the device and to float32 are autograd's: the gradient comes back in the
            # logits' own device, dtype and shape
            logits = _on_device(logits)
            dev = logits.device
            tg = ops._ctc_targets("CTCLoss", targets, B, dev)
            frames = ops._ctc_lengths("CTCLoss.input_lengths", input_lengths, B, dev, logits.shape[1])
            tlen = ops._ctc_lengths("CTCLoss.target_lengths", target_lengths, B, dev, tg.shape[1])
            nll = _CTCNll.apply(logits, tg, frames, tlen, self.blank_token, self.zero_infinity)
        else:
            logits = _on_device(logits.detach())
            emis, tg, frames, tlen = ops.ctc_emissions(logits, targets, input_lengths, target_lengths,
                                                       self.blank_token)
            nll = ops.ctc_loss(emis, tg, frames, tlen)
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        return (nll / tlen.clamp(min=1).to(nll.dtype)).mean()

    def _pad_concatenated(self, targets: torch.Tensor, target_lengths, B: int) -> torch.Tensor:
        return _pad_concatenated("CTCLoss", targets, target_lengths, B, self.blank_token)


def _pad_concatenated(who: str, targets: torch.Tensor, target_lengths, B: int, blank: int) -> torch.Tensor:
    """1-D concatenated targets -> (B, Smax) rows (host bookkeeping: this form reads the lengths)."""
    flat = targets[targets != blank].cpu()
    lens = [int(n) for n in torch.as_tensor(target_lengths).cpu().tolist()]
    if len(lens) != B or sum(lens) > flat.numel():
        raise ValueError(f"{who}: target_lengths {lens} do not fit {flat.numel()} concatenated targets")
    out = torch.zeros((B, max(lens, default=0)), dtype=torch.int32)
    pos = 0
    for b, n in enumerate(lens):
        out[b, :n] = flat[pos:pos + n]
        pos += n
    return out


class _CTCHeadNll(torch.autograd.Function):
    """Per-utterance nll (B,) of the head's normalised rows xn (B * L, K), its weight (V, K) and bias,
    with the gradient to all three and no (B, L, V) tensor.  Forward: ops.ctc_head_emissions + the
    lattice that keeps alpha.  Backward: the occupancy once, then chunks of whole utterances with
    rows * V * 4 <= chunk_bytes (at least one utterance; sizes come from shapes, never from
    lengths): the chunk's logits by the plain GEMM into one reused buffer, their gradient in place,
    and dX = G W, dW += G^T xn, db += sum G straight from the buffer, each only if its input asks
    for a gradient (a frozen head forms no dW, db).  No host synchronisation."""

    @staticmethod
    def forward(ctx, xn, w, bias, tg, frames, tlen, blank, zero_infinity, B, chunk_bytes):
        emis, stats, tg, frames, tlen = ops.ctc_head_emissions(xn, w, bias, tg, frames, tlen, blank, B=B)
        nll, alpha = ops.ctc_loss_alpha(emis, tg, frames, tlen)
        ctx.save_for_backward(xn, w, bias, emis, alpha, nll, stats, tg, frames, tlen)
        ctx.blank, ctx.zero_infinity, ctx.chunk_bytes = blank, zero_infinity, chunk_bytes
        return nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_nll):
        xn, w, bias, emis, alpha, nll, stats, tg, frames, tlen = ctx.saved_tensors
        B, Lq = emis.shape[0], emis.shape[1]
        V, K = w.shape
        scale = grad_nll.to(dtype=torch.float32)
        infeasible = torch.full_like(scale, 0.0 if ctx.zero_infinity else float("nan"))
        scale = torch.where(torch.isinf(nll), infeasible, scale).contiguous()
        occ = ops.ctc_occupancy(emis, alpha, nll, tg, frames, tlen)
        nb = min(B, max(1, int(ctx.chunk_bytes) // (Lq * V * 4)))
        buf = torch.empty((nb * Lq, V), device=xn.device, dtype=torch.float32)
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty((B * Lq, K), device=xn.device, dtype=torch.float32) if need_x else None
        dw = torch.zeros((V, K), device=xn.device, dtype=torch.float32) if need_w else None
        db = torch.zeros((V,), device=xn.device, dtype=torch.float32) if need_b and bias is not None else None
        # rows past frames[b] may hold anything (NaN included): they are zero in G, and zero here
        live = (torch.arange(Lq, device=xn.device, dtype=torch.int32)[None, :] < frames[:, None]).reshape(B * Lq, 1)
        wd, stats = w.detach(), stats.view(B * Lq, 2)
        for b0 in range(0, B, nb):
            b1 = min(b0 + nb, B)
            r0, r1 = b0 * Lq, b1 * Lq
            xc = xn[r0:r1]
            g = ops.gemm(xc, w, bias, out=buf[:r1 - r0])
            ops.ctc_grad_logits_stats(g.view(b1 - b0, Lq, V), stats[r0:r1], occ[b0:b1], tg[b0:b1], frames[b0:b1],
                                      tlen[b0:b1], scale[b0:b1], ctx.blank)
            if dx is not None:
                torch.mm(g, wd, out=dx[r0:r1])
            if dw is not None:
                dw.addmm_(g.t(), torch.where(live[r0:r1], xc, torch.zeros((), device=xn.device)))
            if db is not None:
                db += g.sum(0)
        return dx, dw, db, None, None, None, None, None, None, None


class CTCHeadLoss(nn.Module):
    """CTCLoss()(head(features), ...) without the logits: the loss straight from the CTC head's
    input `features` (B, L, d_model), with CTCLoss's signature semantics otherwise (2-D or 1-D
    concatenated targets, the three reductions, zero_infinity, and inputs that require grad refused
    unless differentiable=True).

    Forward-only, a plain fp32 head runs ops.ctc_head_emissions; a bf16 or QAT head goes through
    its logits.  The forward-only value is the eval-mode one: the head's dropout is not applied,
    whatever head.training says (the differentiable path applies it, as a torch op).  With differentiable=True (fp32 plain heads only; others are refused) the LayerNorm
    and the dropout are torch ops that autograd differentiates and one autograd.Function covers the
    Linear and the loss (_CTCHeadNll): gradients reach the features, both LayerNorm parameters, the
    weight and the bias.  The loss value is the forward-only one, bitwise when the rows it is given
    are already normalised.

    Args:
        head: the model's CTCOutputHead (not registered as a submodule)
        blank_token, reduction, zero_infinity: as CTCLoss
        differentiable: give inputs that require grad a backward pass instead of refusing them
        chunk_bytes: the backward's logits buffer, whole utterances, at least one
        fused: None = the module decides (fused from FUSED_MIN_VOCAB up, and whenever a gradient
            is asked for: its point is the bounded memory); True / False force a path
    """

    # forward-only crossover (profiles/ctc_head.md, rows = 16032, where both GEMMs run on the rows
    # engine): through the logits is faster at V = 1000 (57 vs 89 us) and 2000 (105 vs 122), the two
    # tie at 3000 (155.6 both), logit-free is faster at 4000 (189 vs 198), 5000 (226 vs 253), 10000
    # (395 vs 472) and, at 4008 rows on the tile kernels, 50000 (530 vs 710).  The rule reads V alone:
    # the two GEMMs share an engine at every shape (ops.gemm_tile), so what is left to decide is the
    # logits' traffic against the gather's fixed cost, measured at this one row count only.
    FUSED_MIN_VOCAB = 3072

    def __init__(self, head, blank_token: int = 0, reduction: str = "mean", zero_infinity: bool = True, *,
                 differentiable: bool = False, chunk_bytes: int = 256 << 20, fused=None):
        super().__init__()
        if reduction not in ("mean", "sum", "none"):
            raise ValueError(f"CTCHeadLoss: {reduction} is not a valid value for reduction")
        if fused not in (None, True, False):
            raise ValueError("CTCHeadLoss: fused must be None, True or False")
        if int(chunk_bytes) <= 0:
            raise ValueError("CTCHeadLoss: chunk_bytes must be positive")
        if not all(hasattr(head, a) for a in ("proj", "fusable", "ctc_emissions")):
            raise TypeError("CTCHeadLoss: head must be a CTCOutputHead")
        if differentiable and not head.fusable():
            raise TypeError("CTCHeadLoss: differentiable=True needs a plain float32 head (not bf16, not QAT)")
        if fused and not head.fusable():
            raise TypeError("CTCHeadLoss: fused=True needs a plain float32 head (not bf16, not QAT)")
        object.__setattr__(self, "head", head)  # the model owns it
        self.blank_token = blank_token
        self.reduction = reduction
        self.zero_infinity = zero_infinity
        self.differentiable = differentiable
        self.chunk_bytes = int(chunk_bytes)
        self.fused = fused

    def forward(self, features: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                target_lengths: torch.Tensor, normalized: bool = False) -> torch.Tensor:
        """features (B, L, d_model); targets, input_lengths, target_lengths as CTCLoss.forward.
        normalized (extension): features are already head.proj[0](fused features)."""
        from .decode import _on_device

        head = self.head
        lin, ln = head.proj[2], head.proj[0]
        params = [p for p in (lin.weight, lin.bias, ln.weight, ln.bias) if p is not None]
        wants = torch.is_grad_enabled() and features.requires_grad
        if wants and not self.differentiable:
            raise RuntimeError(
                "velocity_asr.training.CTCHeadLoss is forward-only unless differentiable=True. "
                "Call it under torch.no_grad() or on detached features.")
        # differentiable: also when only the head's own parameters ask for a gradient
        with_grad = wants or (self.differentiable and torch.is_grad_enabled() and any(p.requires_grad for p in params))
        if features.dim() != 3:
            raise ValueError("CTCHeadLoss: features must be (batch, seq_len, d_model)")
        B, Lq, D = features.shape
        if targets.dim() == 1:
            targets = _pad_concatenated("CTCHeadLoss", targets, target_lengths, B, self.blank_token)
        features = _on_device(features if with_grad else features.detach())
        dev = features.device
        fused = self.fused
        if with_grad:
            if not head.fusable():
                raise TypeError("CTCHeadLoss: differentiable=True needs a plain float32 head (not bf16, not QAT)")
            fused = True if fused is None else fused
            tg = ops._ctc_targets("CTCHeadLoss", targets, B, dev)
            frames = ops._ctc_lengths("CTCHeadLoss.input_lengths", input_lengths, B, dev, Lq)
            tlen = ops._ctc_lengths("CTCHeadLoss.target_lengths", target_lengths, B, dev, tg.shape[1])
            xn = features.to(torch.float32)
            xn = head.proj[1](xn if normalized else ln(xn))
            if fused:
                nll = _CTCHeadNll.apply(xn.reshape(B * Lq, D), lin.weight, lin.bias, tg, frames, tlen,
                                        self.blank_token, self.zero_infinity, B, self.chunk_bytes)
            else:
                nll = _CTCNll.apply(nn.functional.linear(xn, lin.weight, lin.bias), tg, frames, tlen,
                                    self.blank_token, self.zero_infinity)
        else:
            if fused is None:
                fused = head.fusable() and lin.weight.shape[0] >= self.FUSED_MIN_VOCAB
            emis, tg, frames, tlen = head.ctc_emissions(features.to(torch.float32), targets, input_lengths,
                                                        target_lengths, self.blank_token, normalized, fused=fused)
            nll = ops.ctc_loss(emis, tg, frames, tlen)
        if self.zero_infinity:
            nll = torch.where(torch.isinf(nll), torch.zeros_like(nll), nll)
        if self.reduction == "none":
            return nll
        if self.reduction == "sum":
            return nll.sum()
        return (nll / tlen.clamp(min=1).to(nll.dtype)).mean()


def _edit_distance(a: Sequence, b: Sequence) -> int:
    """Levenshtein distance, unit costs, two-row DP (same values as the reference's full table)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        ai = a[i - 1]
        for j in range(1, len(b) + 1):
            if ai == b[j - 1]:
                cur[j] = prev[j - 1]
            else:
                cur[j] = 1 + min(prev[j], cur[j - 1], prev[j - 1])
        prev = cur
    return prev[len(b)]


def compute_wer(predictions: List[str], references: List[str], device=None) -> float:
    """Word error rate: total word edits / total reference words (0.0 if no words).  device: a HIP
    device scores the pairs with the edit-distance kernel (error_counts); the float is the same."""
    if device is not None:
        return error_rate(error_counts(predictions, references, "word", device))
    errors = words = 0
    for pred, ref in zip(predictions, references):
        ref_words = ref.lower().split()
        errors += _edit_distance(pred.lower().split(), ref_words)
        words += len(ref_words)
    return errors / words if words > 0 else 0.0


def compute_cer(predictions: List[str], references: List[str], device=None) -> float:
    """Character error rate: total char edits / total reference chars (0.0 if none).  device: as
    compute_wer."""
    if device is not None:
        return error_rate(error_counts(predictions, references, "char", device))
    errors = chars = 0
    for pred, ref in zip(predictions, references):
        ref_chars = list(ref.lower())
        errors += _edit_distance(list(pred.lower()), ref_chars)
        chars += len(ref_chars)
    return errors / chars if chars > 0 else 0.0


def edit_counts_host(hyp: Sequence, ref: Sequence) -> Tuple[int, int, int]:
    """(substitutions, deletions, insertions) of hyp against ref: the specification the device kernel
    (vasr_edit_counts_i32) reproduces exactly.  c[i][j] are the counts of hyp[:i] against ref[:j]:
    c[i][0] is i insertions, c[0][j] j deletions; equal items copy c[i-1][j-1] unconditionally (as
    _edit_distance does), otherwise the candidate of the smallest S + D + I wins, ties going to the
    first of substitution (c[i-1][j-1]), deletion (c[i][j-1]: a reference item with no counterpart),
    insertion (c[i-1][j]: a hypothesis item with no counterpart).  The counts travel with the cost:
    one row of memory, no backtrace.  S + D + I == _edit_distance(hyp, ref)."""
    n = len(ref)
    prev = [(0, j, 0) for j in range(n + 1)]
    for i in range(1, len(hyp) + 1):
        cur = [(0, 0, i)] + [None] * n
        hi = hyp[i - 1]
        for j in range(1, n + 1):
            if hi == ref[j - 1]:
                cur[j] = prev[j - 1]
                continue
            s, d, ins = prev[j - 1]
            best, cost = (s + 1, d, ins), s + d + ins
            s2, d2, i2 = cur[j - 1]
            if s2 + d2 + i2 < cost:
                best, cost = (s2, d2 + 1, i2), s2 + d2 + i2
            s3, d3, i3 = prev[j]
            if s3 + d3 + i3 < cost:
                best = (s3, d3, i3 + 1)
            cur[j] = best
        prev = cur
    return prev[n]


@dataclass
class ErrorCounts:
    """Edit counts of one hypothesis against its reference."""

    substitutions: int
    deletions: int
    insertions: int
    ref_length: int
    hyp_length: int

    @property
    def hits(self) -> int:
        return self.ref_length - self.substitutions - self.deletions

    @property
    def errors(self) -> int:
        return self.substitutions + self.deletions + self.insertions

    @property
    def rate(self) -> float:
        return self.errors / self.ref_length if self.ref_length > 0 else 0.0


def error_rate(counts: List[ErrorCounts]) -> float:
    """Corpus rate of per-pair counts: summed errors over summed reference items, divided once (the
    float compute_wer / compute_cer return); 0.0 if the references are empty."""
    errors = sum(c.errors for c in counts)
    items = sum(c.ref_length for c in counts)
    return errors / items if items > 0 else 0.0


MAX_DEVICE_ITEMS = ops.EDIT_MAX_ITEMS  # a longer sequence is scored on the host
# error_counts(device=...) keeps a batch of fewer DP cells than this on the host: below it the upload,
# launch and download cost more than the Python loop (profiles/score.md).
MIN_DEVICE_CELLS = 1000


def _is_hip(device) -> bool:
    return device is not None and torch.device(device).type == "cuda"


def _item_pairs(what: str, predictions: List[str], references: List[str], unit: str):
    """The (hypothesis items, reference items) of each pair: compute_wer's or compute_cer's normalisation."""
    if unit not in ("word", "char"):
        raise ValueError(f"{what}: unit must be 'word' or 'char', got {unit!r}")
    split = (lambda s: s.lower().split()) if unit == "word" else (lambda s: list(s.lower()))
    return [(split(p), split(r)) for p, r in zip(predictions, references)]


def _device_pairs(pairs, device, min_cells: int) -> List[int]:
    """Indices of the pairs a HIP device scores: all that fit the kernel, unless they are fewer than min_cells cells."""
    if not _is_hip(device):
        return []
    on_device = [k for k, (h, r) in enumerate(pairs) if len(h) <= MAX_DEVICE_ITEMS and len(r) <= MAX_DEVICE_ITEMS]
    if sum(len(pairs[k][0]) * len(pairs[k][1]) for k in on_device) < min_cells:
        return []
    return on_device


def _interned(pairs, which: List[int]):
    """One host buffer for one upload: [hyp ids | ref ids | hyp length | ref length] per chosen pair, the items
    interned as int32 ids of one dictionary.  -> (buffer (P, mh + mr + 2), mh, mr)."""
    import numpy as np
    ids: dict = {}
    mh = max(1, max(len(pairs[k][0]) for k in which))
    mr = max(1, max(len(pairs[k][1]) for k in which))
    buf = np.zeros((len(which), mh + mr + 2), np.int32)
    for row, k in zip(buf, which):
        h, r = pairs[k]
        row[:len(h)] = [ids.setdefault(x, len(ids)) for x in h]
        row[mh:mh + len(r)] = [ids.setdefault(x, len(ids)) for x in r]
        row[mh + mr], row[mh + mr + 1] = len(h), len(r)
    return buf, mh, mr


def error_counts(predictions: List[str], references: List[str], unit: str = "word", device=None) -> List[ErrorCounts]:
    """Per-pair substitution / deletion / insertion counts.  The text normalisation is compute_wer's
    (unit "word": .lower().split()) or compute_cer's ("char": list(.lower())).  device None (or a
    non-HIP device) runs edit_counts_host.  A HIP device interns the items as int32 ids (one dictionary
    per call), uploads the padded id matrices and lengths once, runs vasr_edit_counts_i32 and downloads
    the (P, 3) counts once; a pair with a side longer than 65535 items is scored on the host in the
    same call, and so is a batch of fewer than MIN_DEVICE_CELLS cells."""
    pairs = _item_pairs("error_counts", predictions, references, unit)
    out: List[ErrorCounts] = [None] * len(pairs)  # type: ignore[list-item]
    on_device = _device_pairs(pairs, device, MIN_DEVICE_CELLS)
    if on_device:
        buf, mh, mr = _interned(pairs, on_device)
        dev = torch.from_numpy(buf).to(device)
        got = ops.edit_counts(dev[:, :mh], dev[:, mh:mh + mr], dev[:, mh + mr].contiguous(),
                              dev[:, mh + mr + 1].contiguous()).cpu().tolist()
        for k, (s, d, i) in zip(on_device, got):
            out[k] = ErrorCounts(s, d, i, len(pairs[k][1]), len(pairs[k][0]))
    for k, (h, r) in enumerate(pairs):
        if out[k] is None:
            s, d, i = edit_counts_host(h, r)
            out[k] = ErrorCounts(s, d, i, len(r), len(h))
    return out


def token_error_counts(hyp_tokens: torch.Tensor, hyp_lengths: torch.Tensor, ref_tokens: torch.Tensor,
                       ref_lengths: torch.Tensor) -> torch.Tensor:
    """Edit counts of token ids already on the device, e.g. decoded tokens against padded targets in an
    evaluation loop: (P, Lh) and (P, Lr) integer ids with (P,) lengths -> (P, 3) int32 (S, D, I) on the
    device, no host round trip."""
    def i32(t):
        return t if t.dtype == torch.int32 else t.to(torch.int32)
    return ops.edit_counts(i32(hyp_tokens), i32(ref_tokens), i32(hyp_lengths).contiguous(), i32(ref_lengths).contiguous())


# --------------------------------------------------------------------------- alignments
HIT, SUBSTITUTION, DELETION, INSERTION = range(4)  # operation codes of an edit path


def edit_alignment_host(hyp: Sequence, ref: Sequence) -> List[int]:
    """The edit path of hyp against ref in forward order, one code per operation (0 hit, 1 substitution,
    2 deletion: a reference item with no counterpart, 3 insertion: a hypothesis item with no counterpart):
    the specification the device kernels (vasr_edit_align_i32) reproduce exactly.  Every cell of
    edit_counts_host's DP gets one choice: cell (0, j > 0) deletion, cell (i > 0, 0) insertion,
    hyp[i-1] == ref[j-1] hit, unconditionally; otherwise the smallest of c[i-1][j-1], c[i][j-1], c[i-1][j]
    (c the cost S + D + I), ties to the first of substitution, deletion, insertion.  The path walks back from
    (len(hyp), len(ref)) along the choices and is reversed.  Its counts are edit_counts_host's, and its length
    is len(ref) + insertions."""
    m, n = len(hyp), len(ref)
    prev = list(range(n + 1))
    choice = []  # choice[i - 1][j], i >= 1, j >= 1
    for i in range(1, m + 1):
        cur = [i] + [0] * n
        ch = bytearray(n + 1)
        hi = hyp[i - 1]
        for j in range(1, n + 1):
            if hi == ref[j - 1]:
                cur[j] = prev[j - 1]
                continue
            best, cost = SUBSTITUTION, prev[j - 1]
            if cur[j - 1] < cost:
                best, cost = DELETION, cur[j - 1]
            if prev[j] < cost:
                best, cost = INSERTION, prev[j]
            cur[j], ch[j] = cost + 1, best
        choice.append(ch)
        prev = cur
    path = []
    i, j = m, n
    while i > 0 or j > 0:
        op = DELETION if i == 0 else INSERTION if j == 0 else choice[i - 1][j]
        path.append(op)
        i -= op != DELETION
        j -= op != INSERTION
    path.reverse()
    return path


def _path_counts(path: Sequence[int]) -> Tuple[int, int, int]:
    s = d = i = 0
    for op in path:
        s += op == SUBSTITUTION
        d += op == DELETION
        i += op == INSERTION
    return s, d, i


@dataclass
class Alignment:
    """One hypothesis aligned to its reference: the two item lists (words or characters, normalised as
    compute_wer / compute_cer do), the path's operation codes in forward order and its counts."""

    hyp: List
    ref: List
    ops: List[int]
    counts: ErrorCounts

    def pairs(self):
        """Yields (op, hyp item or None, ref item or None, hyp index, ref index) along the path; the index
        of a missing side is that of the next item on that side."""
        i = j = 0
        for op in self.ops:
            yield (op, None if op == DELETION else self.hyp[i], None if op == INSERTION else self.ref[j], i, j)
            i += op != DELETION
            j += op != INSERTION


# error_alignments(device=...) keeps a batch of fewer DP cells than this on the host: its device call also
# downloads the paths and builds the objects, so it breaks even later than error_counts (profiles/align.md:
# the host wins at 1770 cells, the device at 3597).
ALIGN_MIN_DEVICE_CELLS = 2500
ALIGN_TABLE_BYTES = ops.EDIT_ALIGN_TABLE_BYTES  # a pair whose choice table is larger is aligned on the host


def _length_buckets(pairs, which: List[int]) -> List[List[int]]:
    """`which` by rising size, cut where a pair is more than four times as long as its bucket's first (of at
    least 64 items): every bucket is one padded upload, and a few long pairs must not widen all the rows."""
    size = lambda k: len(pairs[k][0]) + len(pairs[k][1])  # noqa: E731
    out: List[List[int]] = []
    for k in sorted(which, key=size):
        if out and size(k) <= 4 * max(64, size(out[-1][0])):
            out[-1].append(k)
        else:
            out.append([k])
    return out


def error_alignments(predictions: List[str], references: List[str], unit: str = "word", device=None) -> List[Alignment]:
    """Per-pair edit paths: which item was substituted for which, which were dropped and which added.  Text
    normalisation and interning are error_counts'.  device None (or a non-HIP device) runs edit_alignment_host.
    A HIP device runs vasr_edit_align_i32 (ops.edit_alignment), one upload and one download per bucket of pairs
    of similar length; on the host stay a pair with a side longer than 65535 items or a choice table over
    ALIGN_TABLE_BYTES, and a batch of fewer than ALIGN_MIN_DEVICE_CELLS cells.  The paths and counts are the
    same either way."""
    pairs = _item_pairs("error_alignments", predictions, references, unit)
    paths: list = [None] * len(pairs)
    on_device = _device_pairs(pairs, device, ALIGN_MIN_DEVICE_CELLS)
    for bucket in _length_buckets(pairs, on_device):
        buf, mh, mr = _interned(pairs, bucket)
        dev = torch.from_numpy(buf).to(device)
        _, path, length = ops.edit_alignment(dev[:, :mh], dev[:, mh:mh + mr], buf[:, mh + mr].tolist(),
                                             buf[:, mh + mr + 1].tolist(), table_bytes=ALIGN_TABLE_BYTES)
        length = length.cpu().tolist()
        path = path[:, :max(1, max(length))].cpu().numpy()
        for k, row, n in zip(bucket, path, length):
            if n >= 0:
                paths[k] = row[:n].tolist()
    out = []
    for (h, r), path in zip(pairs, paths):
        if path is None:
            path = edit_alignment_host(h, r)
        s, d, i = _path_counts(path)
        out.append(Alignment(h, r, path, ErrorCounts(s, d, i, len(r), len(h))))
    return out


def format_alignment(a: Alignment, width: int = 100) -> str:
    """The three-line view of an alignment: a REF and a HYP line with each pair of items in a column of
    equal width, `***` on the side that has no item, and under them S, D or I below every error; wrapped into
    blocks of at most `width` characters a line (a single wider column is not cut)."""
    cols = []
    for op, h, r, _, _ in a.pairs():
        show = lambda x: "***" if x is None else (str(x) if str(x).strip() else "_" * len(str(x)))  # noqa: E731
        rs, hs = show(r), show(h)
        w = max(len(rs), len(hs))
        cols.append((rs.ljust(w), hs.ljust(w), " SDI"[op].ljust(w)))
    blocks, cur, used = [], [], 5
    for c in cols:
        if cur and used + len(c[0]) + 1 > width:
            blocks.append(cur)
            cur, used = [], 5
        cur.append(c)
        used += len(c[0]) + 1
    blocks.append(cur)
    lines = []
    for b in blocks:
        lines += [("REF: " + " ".join(c[0] for c in b)).rstrip(), ("HYP: " + " ".join(c[1] for c in b)).rstrip(),
                  ("     " + " ".join(c[2] for c in b)).rstrip()]
    return "\n".join(lines)


def confusions(alignments: Sequence[Alignment]):
    """(substitutions, deletions, insertions) of a set of alignments as three Counters: of (ref item, hyp item)
    pairs, of deleted reference items and of inserted hypothesis items."""
    from collections import Counter
    sub, dele, ins = Counter(), Counter(), Counter()
    for a in alignments:
        for op, h, r, _, _ in a.pairs():
            if op == SUBSTITUTION:
                sub[(r, h)] += 1
            elif op == DELETION:
                dele[r] += 1
            elif op == INSERTION:
                ins[h] += 1
    return sub, dele, ins
