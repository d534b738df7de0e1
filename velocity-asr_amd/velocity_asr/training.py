"""Evaluation-side pieces of reference velocity_asr/training.py: the CTC loss that
Trainer.eval_step scores a checkpoint with (training.py:47-104, :273-299) and the WER/CER
metrics scripts/evaluate.py imports (training.py:412-501).

CTCLoss here is the loss on the HIP path (vasr_ctc_emissions_f32 + vasr_ctc_loss_f32): by default
forward only, scoring a known transcript; with differentiable=True it also has a backward pass
(vasr_ctc_loss_alpha_f32 in the forward, vasr_ctc_occupancy_f32 + vasr_ctc_grad_logits_f32 in the
backward), so a PyTorch training loop can use it in place of F.log_softmax + nn.CTCLoss.  Of the
model's own kernels both selective scans have a backward pass too (velocity_asr.ssm.selective_scan: the
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
"""

from __future__ import annotations

from typing import List, Sequence

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
        """1-D concatenated targets -> (B, Smax) rows (host bookkeeping: this form reads the lengths)."""
        flat = targets[targets != self.blank_token].cpu()
        lens = [int(n) for n in torch.as_tensor(target_lengths).cpu().tolist()]
        if len(lens) != B or sum(lens) > flat.numel():
            raise ValueError(f"CTCLoss: target_lengths {lens} do not fit {flat.numel()} concatenated targets")
        out = torch.zeros((B, max(lens, default=0)), dtype=torch.int32)
        pos = 0
        for b, n in enumerate(lens):
            out[b, :n] = flat[pos:pos + n]
            pos += n
        return out


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


def compute_wer(predictions: List[str], references: List[str]) -> float:
    """Word error rate: total word edits / total reference words (0.0 if no words)."""
    errors = words = 0
    for pred, ref in zip(predictions, references):
        ref_words = ref.lower().split()
        errors += _edit_distance(pred.lower().split(), ref_words)
        words += len(ref_words)
    return errors / words if words > 0 else 0.0


def compute_cer(predictions: List[str], references: List[str]) -> float:
    """Character error rate: total char edits / total reference chars (0.0 if none)."""
    errors = chars = 0
    for pred, ref in zip(predictions, references):
        ref_chars = list(ref.lower())
        errors += _edit_distance(list(pred.lower()), ref_chars)
        chars += len(ref_chars)
    return errors / chars if chars > 0 else 0.0
