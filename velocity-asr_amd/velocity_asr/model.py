"""VELOCITY-ASR model (drop-in for reference velocity_asr/model.py) on MI355X kernels.

Module tree, parameter/buffer names, config dataclass and checkpoint format are the
reference's (model.py:23-467), so reference checkpoints load with strict=True and
scripts/transcribe.py / scripts/evaluate.py work unchanged.  The forward pass runs
entirely in libvasr_hip.so; CPU tensors are rejected with a clear error.
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import torch.nn as nn

from . import _lib, ops
from . import quantize as Q
from ._prep import cached
from .attention import HierarchicalGlobalContext
from .ssm import LocalSSMProcessor, ScanMode


@dataclass
class VelocityASRConfig:
    """Configuration for VELOCITY-ASR (reference model.py:23-68)."""

    mel_bins: int = 80
    d_model: int = 192
    ssm_layers: int = 8
    ssm_state_dim: int = 64
    ssm_expand_ratio: int = 2
    ssm_kernel_size: int = 4
    global_ssm_layers: int = 2
    global_ssm_state_dim: int = 32
    attention_heads: int = 4
    attention_dim: int = 48
    vocab_size: int = 1000
    dropout: float = 0.1
    gradient_checkpointing: bool = False
    scan_mode: ScanMode = "parallel"
    use_compile: bool = False

    @classmethod
    def from_dict(cls, config_dict: Dict[str, Any]) -> "VelocityASRConfig":
        return cls(**{k: v for k, v in config_dict.items() if k in cls.__dataclass_fields__})


class PositionalEncoding2D(nn.Module):
    """[sinusoidal time (D/2) | learned frequency (D/2)] encoding (reference model.py:71-127)."""

    def __init__(self, d_model: int = 192, max_len: int = 5000, mel_bins: int = 80):
        super().__init__()
        self.d_model = d_model
        pe_time = torch.zeros(max_len, d_model // 2)
        position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
        div_term = torch.exp(torch.arange(0, d_model // 2, 2).float() * (-math.log(10000.0) / (d_model // 2)))
        pe_time[:, 0::2] = torch.sin(position * div_term)
        pe_time[:, 1::2] = torch.cos(position * div_term)
        self.register_buffer("pe_time", pe_time)
        self.pe_freq = nn.Parameter(torch.randn(1, 1, d_model // 2) * 0.02)

    def table(self, seq_len: int) -> torch.Tensor:
        """(seq_len, d_model) rows [pe_time[t] | pe_freq] on the parameters' device."""
        if seq_len > self.pe_time.shape[0]:
            raise RuntimeError(f"sequence of {seq_len} tokens exceeds the positional table ({self.pe_time.shape[0]}); "
                               "the reference fails the same way (model.py:125)")

        def build():
            half = self.pe_time.shape[1]
            return torch.cat([self.pe_time[:seq_len], self.pe_freq.reshape(1, half).expand(seq_len, half)],
                             -1).float().contiguous()
        return cached(self, f"pe{seq_len}", (self.pe_time, self.pe_freq), build)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, L, D = x.shape
        return ops.add_table(x, self.table(L))


class TemporalBindingLayer(nn.Module):
    """Conv1d(k3, s2) -> GELU -> +2-D PE -> LayerNorm (reference model.py:130-202).

    One batched fp32-MFMA GEMM: the mel frames are zero-padded once so every conv output
    row is a plain strided row (stride 2 frames, K = 3 frames) of the padded buffer; bias,
    exact GELU and the positional table are fused in the epilogue.
    """

    def __init__(self, mel_bins: int = 80, d_model: int = 192, kernel_size: int = 3, stride: int = 2):
        super().__init__()
        self.conv = nn.Conv1d(in_channels=mel_bins, out_channels=d_model, kernel_size=kernel_size, stride=stride,
                              padding=kernel_size // 2)
        self.pos_encoding = PositionalEncoding2D(d_model=d_model, mel_bins=mel_bins)
        self.norm = nn.LayerNorm(d_model)
        self.activation = nn.GELU()

    def conv_padding(self) -> int:
        return Q.inner(self.conv).padding[0]

    def output_length(self, frames: int) -> int:
        c = Q.inner(self.conv)
        k, s, p = c.kernel_size[0], c.stride[0], c.padding[0]
        return (frames + 2 * p - k) // s + 1

    def forward(self, mel_spectrogram: torch.Tensor, raw: bool = False) -> torch.Tensor:
        """raw (extension): the rows before the final LayerNorm (the first SSM block applies it
        inside its own first launch, VELOCITYASR._local_global)."""
        D = Q.inner(self.conv).out_channels
        L = self.output_length(mel_spectrogram.shape[1])
        if Q.observing(self.conv):
            Q.record(self.conv, Q.conv1d_rows(self.conv, mel_spectrogram))
        # conv (+ activation fake-quant for QuantizedConv1d) -> GELU -> + PE, one GEMM
        x = Q.conv1d_rows(self.conv, mel_spectrogram, epilogue=_lib.EPI_GELU_PE, aux=self.pos_encoding.table(L),
                          ld_aux=D)
        if raw:
            return x
        return ops.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)


class CTCOutputHead(nn.Module):
    """LayerNorm -> Dropout -> Linear(d_model, vocab) (reference model.py:205-239)."""

    def __init__(self, d_model: int = 192, vocab_size: int = 50000, dropout: float = 0.1):
        super().__init__()
        self.proj = nn.Sequential(nn.LayerNorm(d_model), nn.Dropout(dropout), nn.Linear(d_model, vocab_size))

    def _ln(self, normalized: bool):
        ln = self.proj[0]
        return None if normalized else (ln.weight, ln.bias, ln.eps)

    def forward(self, x: torch.Tensor, normalized: bool = False) -> torch.Tensor:
        """normalized (extension, also argmax / greedy): x is already proj[0](fused features) -- the
        gated fusion's launch applied it (HierarchicalGlobalContext.forward head_norm=)."""
        B, L, D = x.shape
        w, b, qp = Q.linear_parts(self.proj[2])
        # the LayerNorm is its own launch before the GEMM (ops._ln_prologue)
        logits = ops.gemm(x.reshape(B * L, D), w, b, qparams=qp, ln=self._ln(normalized))
        Q.record(self.proj[2], logits)
        return logits.view(B, L, w.shape[0])

    def argmax(self, x: torch.Tensor, normalized: bool = False) -> torch.Tensor:
        """argmax over the vocabulary of forward(x), (B, L) int32, fused into the head GEMM: the
        (B, L, V) logits are never written (SURVEY §8 f, rank 1)."""
        B, L, D = x.shape
        w, b, qp = Q.linear_parts(self.proj[2])
        return ops.gemm_argmax(x.reshape(B * L, D), w, b, qparams=qp, ln=self._ln(normalized)).view(B, L)

    def greedy(self, x: torch.Tensor, blank: int = 0, out=None, rows=None, normalized: bool = False):
        """Greedy CTC decode of forward(x) -- argmax(x) then the collapse of decode.py:46-69 --
        with the argmax and the collapse in one launch after the head GEMM: (tokens (B, L),
        lengths (B,)) int32.  rows: per-utterance row counts (int32 (B,)) of a padded batch."""
        B, L, D = x.shape
        w, b, qp = Q.linear_parts(self.proj[2])
        toks, lens, _, _ = ops.gemm_ctc_greedy(x.reshape(B * L, D), w, b, B, blank, qparams=qp,
                                               ln=self._ln(normalized), out=out, frames=rows)
        return toks, lens

    def greedy_scored(self, x: torch.Tensor, blank: int = 0, rows=None, normalized: bool = False):
        """greedy(x) with time spans and confidences (extension): (tokens, lengths, start, end,
        logp_sum, logp_min, path_logp) as ops.ctc_collapse_conf -- per kept token the sum and the
        minimum over its run of frames of the log-softmax value at the argmax, per utterance the
        sum over its frames (the log-probability of the greedy path).  A fusable() head never writes
        the (B, L, V) logits: its GEMM leaves each row's argmax key and log-sum-exp pair
        (VASR_EPI_ARGMAX_LSE) and one launch folds and collapses them.  A bf16 or QAT head goes
        through forward() and ops.argmax_logp."""
        B, L, D = x.shape
        with torch.no_grad():
            if self.fusable():
                lin = self.proj[2]
                return ops.gemm_ctc_greedy_conf(x.reshape(B * L, D), lin.weight, lin.bias, B, blank,
                                                ln=self._ln(normalized), frames=rows)
            pred, lp = ops.argmax_logp(self.forward(x, normalized=normalized))
            return ops.ctc_collapse_conf(pred, lp, blank, frames=rows)

    def beam_search(self, x: torch.Tensor, beam_width: int, blank: int = 0, rows=None, shortlist="auto",
                    chunk_bytes: int = 256 << 20, normalized: bool = False):
        """decode.ctc_beam_search(forward(x), beam_width, blank, input_lengths=rows, shortlist=shortlist)
        without the (B, L, V) logits (extension): per utterance its beams as
        DecodingResults, bitwise those.  The logits exist a chunk of whole utterances at a time
        (rows * V * 4 <= chunk_bytes, at least one utterance; sizes come from shapes, never from
        lengths), formed by the head's own GEMM into one reused buffer and reduced at once to each
        frame's shortlist (ops.ctc_beam_shortlist) in the batch's (B, L, K) arrays; one search launch
        then covers the batch, and an utterance with an uncertified frame has its own logits formed
        again for the exact search.  shortlist: "auto" or 1..64.  A bf16 or QAT head, a one-token
        vocabulary and shortlist=None go through forward()."""
        from . import decode as dec

        B, L, D = x.shape
        W = int(beam_width)
        lin = self.proj[2]
        with torch.no_grad():
            if shortlist is None or not self.fusable() or lin.weight.shape[0] < 2:
                return dec.ctc_beam_search(self.forward(x, normalized=normalized), W, blank, input_lengths=rows,
                                           shortlist=shortlist)
            if int(chunk_bytes) <= 0:
                raise ValueError("CTCOutputHead.beam_search: chunk_bytes must be positive")
            dec._check_shortlist("CTCOutputHead.beam_search", shortlist, W, False)
            V = lin.weight.shape[0]
            K = dec.beam_shortlist_size(shortlist, V, W)
            frames = ops._beam_frames("CTCOutputHead.beam_search", rows, B, L, x.device)
            short, logits_of = self._shortlists(x, K, blank, frames, chunk_bytes, normalized)

            def again(bad, fr):  # an uncertified utterance's own logits, in the same buffer, one at a time
                parts = [dec._beam_search_exact(logits_of(b, b + 1), W, blank, None if fr is None else fr[i:i + 1])
                         for i, b in enumerate(bad)]
                return tuple(torch.cat(p) for p in zip(*parts))

            return dec._beam_results(*dec._beam_search_from_shortlist(short, V, W, blank, frames, again))

    def _shortlists(self, x: torch.Tensor, K: int, blank: int, frames, chunk_bytes: int, normalized: bool):
        """The batch's per-frame shortlists (ops.ctc_beam_shortlist's three (B, L, K) / (B, L) arrays)
        from the head's input, the (B, L, V) logits existing a chunk of whole utterances at a time in
        one reused buffer, and logits_of(b0, b1), which forms utterances b0 .. b1 - 1 in that buffer
        again (rows * V * 4 <= chunk_bytes > 0, at least one utterance).  A fusable() head, under no_grad."""
        B, L, D = x.shape
        lin = self.proj[2]
        V = lin.weight.shape[0]
        xn = ops._ln_prologue(x.reshape(B * L, D), self._ln(normalized))
        nb = min(B, max(1, int(chunk_bytes) // max(L * V * 4, 1)))
        buf = torch.empty((nb * L, V), device=x.device, dtype=torch.float32)

        def logits_of(b0: int, b1: int) -> torch.Tensor:
            return ops.gemm(xn[b0 * L:b1 * L], lin.weight, lin.bias, out=buf[:(b1 - b0) * L]).view(b1 - b0, L, V)

        short = (torch.empty((B, L, K), device=x.device, dtype=torch.int32),
                 torch.empty((B, L, K), device=x.device, dtype=torch.float32),
                 torch.empty((B, L), device=x.device, dtype=torch.float32))
        for b0 in range(0, B, nb):
            b1 = min(b0 + nb, B)
            ops.ctc_beam_shortlist(logits_of(b0, b1), K, blank, None if frames is None else frames[b0:b1],
                                   out=tuple(t[b0:b1] for t in short))
        return short, logits_of

    def prefix_beam_search(self, x: torch.Tensor, beam_width: int, blank: int = 0, rows=None, token_topk="auto", lm=None,
                           lm_weight: float = 0.0, length_bonus: float = 0.0, chunk_bytes: int = 256 << 20,
                           normalized: bool = False):
        """decode.ctc_prefix_beam_search(forward(x), beam_width, blank, lm, lm_weight, length_bonus,
        input_lengths=rows, token_topk=token_topk) without the (B, L, V) logits (extension, DESIGN.md
        §3.6h): chunked GEMM -> per-frame shortlists as beam_search forms them, then one launch of the
        pruned standard search, with a decode.BigramLM fused on the device.  token_topk: "auto" or
        1..64.  A bf16 or QAT head, a one-token vocabulary, token_topk=None, a beam above 32 and any
        other scorer go through forward()."""
        from . import decode as dec

        B, L, D = x.shape
        W = int(beam_width)
        lin = self.proj[2]
        lm_on = lm is not None and lm_weight > 0
        with torch.no_grad():
            if (token_topk is None or not self.fusable() or lin.weight.shape[0] < 2 or not 1 <= W <= 32
                    or (lm_on and not isinstance(lm, dec.BigramLM))):
                return dec.ctc_prefix_beam_search(self.forward(x, normalized=normalized), W, blank, lm, lm_weight,
                                                  length_bonus, input_lengths=rows, token_topk=token_topk)
            if int(chunk_bytes) <= 0:
                raise ValueError("CTCOutputHead.prefix_beam_search: chunk_bytes must be positive")
            V = lin.weight.shape[0]
            K = dec.beam_shortlist_size(token_topk, V, W)
            frames = ops._beam_frames("CTCOutputHead.prefix_beam_search", rows, B, L, x.device)
            short, _ = self._shortlists(x, K, blank, frames, chunk_bytes, normalized)
            return dec._prefix_beam_results(*ops.ctc_prefix_beam_search_shortlist(
                *short, V, W, blank, frames=frames, lm_table=lm.device_table(x.device) if lm_on else None,
                alpha=float(lm_weight) if lm_on else 0.0, beta=float(length_bonus)))

    def fusable(self) -> bool:
        """Whether the loss can run straight from the head's input (ops.ctc_head_emissions): a plain
        fp32 nn.Linear.  A bf16 or QAT head goes through its logits."""
        lin = self.proj[2]
        return type(lin) is nn.Linear and lin.weight.dtype == torch.float32

    def ctc_emissions(self, x: torch.Tensor, targets: torch.Tensor, input_lengths=None, target_lengths=None,
                      blank: int = 0, normalized: bool = False, fused=None):
        """ops.ctc_emissions(forward(x), ...) -> (emis (B, L, Smax + 1), targets, frames, tlen),
        forward-only.  On an fp32 head the (B, L, V) logits are never written: the head GEMM leaves
        each row's log-sum-exp (VASR_EPI_LSE) and only the blank's and the target tokens' logits are
        formed.  fused (extension): None = where the head allows it, False = through the logits."""
        B, L, D = x.shape
        if fused is None:
            fused = self.fusable()
        elif fused and not self.fusable():
            raise TypeError("CTCOutputHead.ctc_emissions: the logit-free path needs a plain float32 head")
        with torch.no_grad():
            if not fused:
                return ops.ctc_emissions(self.forward(x, normalized=normalized), targets, input_lengths,
                                         target_lengths, blank)
            lin = self.proj[2]
            emis, _, tg, frames, tlen = ops.ctc_head_emissions(x.reshape(B * L, D), lin.weight, lin.bias, targets,
                                                               input_lengths, target_lengths, blank, B=B,
                                                               ln=self._ln(normalized))
        return emis, tg, frames, tlen

    def align(self, x: torch.Tensor, targets, input_lengths=None, target_lengths=None, blank: int = 0,
              normalized: bool = False):
        """decode.ctc_forced_align(forward(x), ...) without the logits (ctc_emissions, then the same
        Viterbi lattice): per utterance (score, [(start_frame, end_frame), ...], frame_labels)."""
        from .decode import _align_emissions, _align_targets

        targets, target_lengths = _align_targets(targets, target_lengths, blank)
        return _align_emissions(*self.ctc_emissions(x, targets, input_lengths, target_lengths, blank, normalized))


class VELOCITYASR(nn.Module):
    """VELOCITY-ASR v2 (reference model.py:242-471)."""

    def __init__(self, config: Optional[VelocityASRConfig] = None):
        super().__init__()
        if config is None:
            config = VelocityASRConfig()
        self.config = config
        self.temporal_binding = TemporalBindingLayer(mel_bins=config.mel_bins, d_model=config.d_model)
        self.local_ssm = LocalSSMProcessor(d_model=config.d_model, num_layers=config.ssm_layers,
                                           state_dim=config.ssm_state_dim, expand_ratio=config.ssm_expand_ratio,
                                           kernel_size=config.ssm_kernel_size, dropout=config.dropout,
                                           use_checkpoint=config.gradient_checkpointing, scan_mode=config.scan_mode)
        self.global_context = HierarchicalGlobalContext(d_model=config.d_model, num_heads=config.attention_heads,
                                                        attention_dim=config.attention_dim,
                                                        global_ssm_layers=config.global_ssm_layers,
                                                        global_ssm_state_dim=config.global_ssm_state_dim,
                                                        dropout=config.dropout)
        self.ctc_head = CTCOutputHead(d_model=config.d_model, vocab_size=config.vocab_size, dropout=config.dropout)
        self._init_weights()
        # config.use_compile: the reference wraps submodules in torch.compile
        # (model.py:320-331); here the whole forward is already native HIP and can be
        # captured in a HIP graph (velocity_asr.pipeline.GraphedTranscriber) instead.

    def _init_weights(self):
        """Same initialisers, same order as the reference (model.py:305-318)."""
        for module in self.modules():
            if isinstance(module, nn.Linear):
                nn.init.xavier_uniform_(module.weight)
                if module.bias is not None:
                    nn.init.zeros_(module.bias)
            elif isinstance(module, nn.Conv1d):
                nn.init.kaiming_normal_(module.weight, mode="fan_out", nonlinearity="relu")
                if module.bias is not None:
                    nn.init.zeros_(module.bias)
            elif isinstance(module, nn.LayerNorm):
                nn.init.ones_(module.weight)
                nn.init.zeros_(module.bias)

    def _token_lengths(self, frames, n_frames: int):
        """Per-utterance token counts of a zero-padded batch (frames: its per-utterance mel frame
        counts, each <= n_frames, frames past them zero), or None for a uniform batch."""
        if frames is None:
            return None
        frames = [int(f) for f in frames]
        if not all(1 <= f <= n_frames for f in frames):
            raise ValueError(f"frames: each utterance needs 1..{n_frames} frames, got {frames}")
        return [self.temporal_binding.output_length(f) for f in frames]

    def _local_global(self, mel: torch.Tensor, lengths):
        """mel -> (local features, head rows, normalised): the temporal binding, the local stack, then
        the global context.  The stack's final LayerNorm and the context's query LayerNorm run as one
        launch (VASR_LN_PAIR=0: two), and the temporal binding's LayerNorm inside the first block's
        norm1 + conv launch (VASR_TB_PRENORM=0: its own launch); bitwise the same either way.  The
        CTC head's LayerNorm goes down to the gated fusion: where that takes it into its launch
        (fp32 model, VASR_FUSION_TAIL=0: never) the head rows are already normalised and the flag,
        which the head's methods take, is True; else they are the fused features."""
        gc, tb = self.global_context, self.temporal_binding
        hn = self.ctc_head.proj[0]
        pre = None
        if os.environ.get("VASR_TB_PRENORM", "1") != "0" and type(tb.norm) is nn.LayerNorm:
            x, pre = tb(mel, raw=True), tb.norm
        else:
            x = tb(mel)
        if os.environ.get("VASR_LN_PAIR", "1") != "0" and type(gc.norm2) is nn.LayerNorm \
                and type(self.local_ssm.norm) is nn.LayerNorm:
            local, query = self.local_ssm.forward_pair(x, gc.norm2, pre_norm=pre)
            return (local,) + gc(local, lengths=lengths, query=query, head_norm=hn)
        local = self.local_ssm(x, pre_norm=pre)
        return (local,) + gc(local, lengths=lengths, head_norm=hn)

    def forward(self, mel_spectrogram: torch.Tensor, return_features: bool = False, frames=None):
        """(B, frames, mel_bins) -> CTC logits (B, (frames + 1) // 2, vocab_size).

        frames (extension): per-utterance frame counts of a batch of utterances of different
        lengths, zero-padded to a common length (velocity_asr.audio.mel_on_device(...,
        lengths=) writes such a batch).  Every utterance's logits over its own
        get_output_length(frames[b]) rows are then those it gets alone; later rows are junk."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): move the model and input to the HIP device "
                               "(model.to('cuda'), mel.to('cuda')); there is no CPU execution path")
        mel = mel_spectrogram.to(torch.float32)
        lengths = self._token_lengths(frames, mel.shape[1])
        with torch.no_grad():
            normalized = False
            if return_features:  # the temporal binding's rows are returned, so they are formed on their own
                x = self.temporal_binding(mel)
                local_features = self.local_ssm(x)
                fused_features = self.global_context(local_features, lengths=lengths)
            else:
                local_features, fused_features, normalized = self._local_global(mel, lengths)
            logits = self.ctc_head(fused_features, normalized=normalized)
        if return_features:
            return logits, {"temporal_binding": x, "local_features": local_features,
                            "fused_features": fused_features}
        return logits

    def token_ids(self, mel_spectrogram: torch.Tensor, frames=None) -> torch.Tensor:
        """argmax(forward(mel), -1) as (B, L) int32 on the device, without materialising logits
        (the CTC head's GEMM reduces each row in its epilogue).  Identical to the argmax of
        forward()'s logits: same GEMM, same accumulation order."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): token_ids needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return self.ctc_head.argmax(x, normalized=normalized)

    def greedy_token_ids(self, mel_spectrogram: torch.Tensor, frames=None, blank: int = 0, out=None, rows=None):
        """Collapsed greedy CTC tokens of forward(mel) on the device, (tokens (B, L), lengths (B,))
        int32: token_ids + ops.ctc_collapse with the argmax and the collapse in one launch.
        rows: per-utterance token-row counts (int32 (B,) on the device) of a padded batch."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): greedy_token_ids needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return self.ctc_head.greedy(x, blank, out=out, rows=rows, normalized=normalized)

    def greedy_scored(self, mel_spectrogram: torch.Tensor, frames=None, blank: int = 0):
        """greedy_token_ids with time spans and confidences, on the device: (tokens, lengths, start,
        end, logp_sum, logp_min, path_logp) as CTCOutputHead.greedy_scored.  frames: per-utterance
        mel frame counts of a zero-padded batch, as forward() takes them."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): greedy_scored needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        rows = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=mel_spectrogram.device)
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return self.ctc_head.greedy_scored(x, blank, rows=rows, normalized=normalized)

    def beam_search(self, mel_spectrogram: torch.Tensor, frames=None, beam_width: int = 10, blank: int = 0,
                    shortlist="auto", chunk_bytes: int = 256 << 20):
        """decode.ctc_beam_search(forward(mel, frames=frames), beam_width, blank, input_lengths=token rows,
        shortlist=shortlist) without the (B, L, V) logits (CTCOutputHead.beam_search): per utterance
        its beams as DecodingResults, bitwise those.  frames: per-utterance mel frame counts of a
        zero-padded batch, as forward() takes them."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): beam_search needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return self.ctc_head.beam_search(x, beam_width, blank, rows=lengths, shortlist=shortlist,
                                             chunk_bytes=chunk_bytes, normalized=normalized)

    def prefix_beam_search(self, mel_spectrogram: torch.Tensor, frames=None, beam_width: int = 10, blank: int = 0,
                           token_topk="auto", lm=None, lm_weight: float = 0.0, length_bonus: float = 0.0,
                           chunk_bytes: int = 256 << 20):
        """The standard CTC prefix beam search (decode.ctc_prefix_beam_search: summed alignments, a
        per-token language-model term and length bonus) with token pruning, without the (B, L, V)
        logits (CTCOutputHead.prefix_beam_search): per utterance its beams as DecodingResults with
        score and logp.  frames: per-utterance mel frame counts of a zero-padded batch."""
        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): prefix_beam_search needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return self.ctc_head.prefix_beam_search(x, beam_width, blank, rows=lengths, token_topk=token_topk, lm=lm,
                                                    lm_weight=lm_weight, length_bonus=length_bonus,
                                                    chunk_bytes=chunk_bytes, normalized=normalized)

    def ctc_loss(self, mel_spectrogram: torch.Tensor, targets: torch.Tensor, input_lengths, target_lengths, *,
                 reduction: str = "mean", zero_infinity: bool = True, frames=None, blank: int = 0) -> torch.Tensor:
        """training.CTCLoss(blank, reduction, zero_infinity)(forward(mel, frames=frames), targets,
        input_lengths, target_lengths) without the (B, L, V) logits (training.CTCHeadLoss on the head's
        input): scoring a checkpoint.  Forward-only, eval mode as the inference kernels demand.
        input_lengths are token-row counts, as CTCLoss takes them."""
        from .training import CTCHeadLoss

        if mel_spectrogram.device.type != "cuda":
            _lib.require_device()
            raise RuntimeError("velocity_asr (MI355X build): ctc_loss needs HIP tensors")
        lengths = self._token_lengths(frames, mel_spectrogram.shape[1])
        loss = CTCHeadLoss(self.ctc_head, blank, reduction, zero_infinity)
        with torch.no_grad():
            _, x, normalized = self._local_global(mel_spectrogram.to(torch.float32), lengths)
            return loss(x, targets, input_lengths, target_lengths, normalized=normalized)

    def get_output_length(self, input_length: int) -> int:
        return (input_length + 1) // 2

    @classmethod
    def from_pretrained(cls, model_name_or_path: str, quantized: bool = False, **kwargs) -> "VELOCITYASR":
        """Load a checkpoint written by save_pretrained or Trainer (reference model.py:385-433)."""
        if not os.path.exists(model_name_or_path):
            raise NotImplementedError("Model hub download not yet implemented. "
                                      "Please provide a local path to the checkpoint.")
        checkpoint = torch.load(model_name_or_path, map_location="cpu", weights_only=True)
        if "config" in checkpoint:
            config = VelocityASRConfig.from_dict(checkpoint["config"])
        else:
            config = VelocityASRConfig()
        model = cls(config)
        if "model_state_dict" in checkpoint:
            model.load_state_dict(checkpoint["model_state_dict"])
        else:
            model.load_state_dict(checkpoint)
        return model

    def save_pretrained(self, save_path: str):
        """Same on-disk format as the reference (model.py:435-467)."""
        d = os.path.dirname(save_path)
        if d:
            os.makedirs(d, exist_ok=True)
        c = self.config
        checkpoint = {
            "config": {
                "mel_bins": c.mel_bins, "d_model": c.d_model, "ssm_layers": c.ssm_layers,
                "ssm_state_dim": c.ssm_state_dim, "ssm_expand_ratio": c.ssm_expand_ratio,
                "ssm_kernel_size": c.ssm_kernel_size, "global_ssm_layers": c.global_ssm_layers,
                "global_ssm_state_dim": c.global_ssm_state_dim, "attention_heads": c.attention_heads,
                "attention_dim": c.attention_dim, "vocab_size": c.vocab_size, "dropout": c.dropout,
                "gradient_checkpointing": c.gradient_checkpointing, "scan_mode": c.scan_mode,
                "use_compile": c.use_compile,
            },
            "model_state_dict": {k: v.detach().cpu() for k, v in self.state_dict().items()},
        }
        torch.save(checkpoint, save_path)

    def count_parameters(self) -> int:
        return sum(p.numel() for p in self.parameters() if p.requires_grad)
