"""Hierarchical pooled global context (drop-in for reference velocity_asr/attention.py).

Pooling, pooled cross-attention and the gated fusion run as HIP kernels: adaptive
average pooling, GEMMs for the projections, a per-(token, head) softmax kernel with the
pooled K/V set in LDS, and the gated fusion as two GEMMs whose second epilogue combines
gate, local and global branches in registers (no (B, L, 2D) concat, no gate tensor in HBM).
"""

from __future__ import annotations

import math
import os
from typing import Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from . import quantize as Q
from ._prep import cached
from .ssm import GlobalSSM


def _device_ints(values: Sequence[int], device) -> torch.Tensor:
    """Host sizes -> the int32 (B,) device array the _var kernels read."""
    return torch.tensor([int(v) for v in values], dtype=torch.int32).to(device)


def _sizes(values, B: int, device) -> Optional[torch.Tensor]:
    """None, a host sequence or an int32 device tensor -> the (B,) device array (or None)."""
    if values is None or isinstance(values, torch.Tensor):
        return values
    if len(values) != B:
        raise ValueError(f"expected {B} per-utterance sizes, got {len(values)}")
    return _device_ints(values, device)


class _PooledAttention(torch.autograd.Function):
    """out = softmax(q k^T / sqrt(hd)) v per (utterance, head).  Forward: ops.pooled_attention, the
    inference kernel itself; only q, kv (and the key counts) are saved.  Backward:
    ops.pooled_attention_bwd, which recomputes the softmax.  Enqueued on the current stream."""

    @staticmethod
    def forward(ctx, q, kv, heads, kps):
        B, Lq, A = q.shape
        Kp = kv.shape[1]
        with torch.no_grad():
            q2, kv2 = q.reshape(B * Lq, A), kv.reshape(B * Kp, 2 * A).contiguous()
            out = ops.pooled_attention(q2, kv2, B, Lq, Kp, heads, kps=kps)
        ctx.save_for_backward(q2, kv2, *(() if kps is None else (kps,)))
        ctx.dims = (B, Lq, Kp, A, heads)
        return out.view(B, Lq, A)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        q2, kv2, *rest = ctx.saved_tensors
        B, Lq, Kp, A, heads = ctx.dims
        dq, dkv = ops.pooled_attention_bwd(q2, kv2, g.to(torch.float32).reshape(B * Lq, A).contiguous(), B, Lq, Kp,
                                           heads, kps=rest[0] if rest else None)
        need = ctx.needs_input_grad
        return (dq.view(B, Lq, A) if need[0] else None, dkv.view(B, Kp, 2 * A) if need[1] else None, None, None)


def pooled_attention(q: torch.Tensor, kv: torch.Tensor, num_heads: int, key_lengths=None) -> torch.Tensor:
    """The pooled cross-attention core as a differentiable operator (reference attention.py:143-160,
    no mask, no dropout): per utterance and head, out = softmax(q k^T / sqrt(head_dim)) v.

    q: (B, Lq, A) and kv: (B, Kp, 2A) holding [K | V], float32 on a HIP device; A = num_heads *
    head_dim.  key_lengths (host sequence or int32 (B,) device tensor, each in [1, Kp]): utterance b
    attends over its own first key_lengths[b] keys; the rows of d kv past them are 0.  The value is
    bitwise ops.pooled_attention (the inference kernel); only q and kv are kept, and the gradients of
    both come from vasr_pooled_attention_bwd_f32 (no atomics: run-to-run bitwise, an utterance's
    gradients the same alone and in a batch).  When nothing requires grad the inference kernel runs
    alone.  Limits are the kernel's: Kp <= 64, head_dim <= 32, A <= 256 and a multiple of 4.

    Query rows are independent, so as with selective_scan the caller zeroes the upstream gradient on
    the padded frames of a padded batch: the gradients of the keys, values and parameters are then
    exact."""
    if q.dim() != 3 or kv.dim() != 3 or kv.shape[0] != q.shape[0] or kv.shape[2] != 2 * q.shape[2] \
            or q.shape[2] % num_heads:
        raise ValueError(f"pooled_attention: q {tuple(q.shape)} / kv {tuple(kv.shape)} / {num_heads} heads do not fit")
    _lib.require_device()
    B, Lq, A = q.shape
    kps = _sizes(key_lengths, B, q.device)
    if torch.is_grad_enabled() and (q.requires_grad or kv.requires_grad):
        return _PooledAttention.apply(q, kv, num_heads, kps)
    Kp = kv.shape[1]
    return ops.pooled_attention(q.detach().reshape(B * Lq, A), kv.detach().reshape(B * Kp, 2 * A), B, Lq, Kp,
                                num_heads, kps=kps).view(B, Lq, A)


class _AdaptiveAvgPool(torch.autograd.Function):
    """out = adaptive average pooling over time.  Forward: ops.adaptive_pool, the inference kernel;
    nothing but the sizes is saved (the pooling is linear).  Backward: ops.adaptive_pool_bwd."""

    @staticmethod
    def forward(ctx, x, K, lens, ks):
        with torch.no_grad():
            out = ops.adaptive_pool(x, K, lens=lens, ks=ks)
        ctx.save_for_backward(*(() if lens is None else (lens, ks)))
        ctx.L = x.shape[1]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lens, ks = ctx.saved_tensors if ctx.saved_tensors else (None, None)
        dx = ops.adaptive_pool_bwd(g.to(torch.float32), ctx.L, lens=lens, ks=ks) if ctx.needs_input_grad[0] else None
        return dx, None, None, None


def adaptive_avg_pool(x: torch.Tensor, K: int, lengths=None, sizes=None) -> torch.Tensor:
    """F.adaptive_avg_pool1d over time as a differentiable operator: (B, L, C) -> (B, K, C), bin i
    the mean of rows [floor(i L / K), ceil((i + 1) L / K)), 1 <= K <= L.  lengths / sizes (both or
    neither; host sequences or int32 (B,) device tensors): utterance b pools its first lengths[b]
    rows into sizes[b] bins, later bins 0, and d x is 0 past lengths[b].  The value is bitwise
    ops.adaptive_pool; the gradient is vasr_adaptive_pool_bwd_f32, a gather (each element written
    once, no atomics).  When x does not require grad the inference kernel runs alone."""
    if x.dim() != 3:
        raise ValueError(f"adaptive_avg_pool: expected (B, L, C), got {tuple(x.shape)}")
    if (lengths is None) != (sizes is None):
        raise ValueError("adaptive_avg_pool: lengths and sizes go together")
    _lib.require_device()
    lens, ks = _sizes(lengths, x.shape[0], x.device), _sizes(sizes, x.shape[0], x.device)
    if torch.is_grad_enabled() and x.requires_grad:
        return _AdaptiveAvgPool.apply(x, int(K), lens, ks)
    return ops.adaptive_pool(x.detach(), int(K), lens=lens, ks=ks)


class AdaptivePool(nn.Module):
    """Adaptive average pooling + learnable projection (reference attention.py:17-78)."""

    def __init__(self, level: int = 1, d_model: int = 192):
        super().__init__()
        self.level = level
        self.d_model = d_model
        self.pool_proj = nn.Linear(d_model, d_model)

    def _compute_pool_size(self, seq_len: int, prev_pool_size: Optional[int] = None) -> int:
        if self.level == 1:
            return max(64, seq_len // 8)
        k1 = prev_pool_size if prev_pool_size else max(64, seq_len // 8)
        return min(64, max(16, k1 // 4))

    def forward(self, x: torch.Tensor, prev_pool_size=None, lengths: Optional[Sequence[int]] = None,
                pre_norm: Optional[nn.LayerNorm] = None):
        """(B, L, D) -> ((B, K, D), K).  lengths: per-utterance valid rows of a zero-padded batch
        (prev_pool_size then per utterance too): each utterance is pooled to the size it gets
        alone, rows past it are junk nobody reads, and the sizes are returned as a list.
        pre_norm (extension): x is the row before that LayerNorm, applied inside the pooling launch
        (ops.ln_adaptive_pool), bitwise the same as pooling pre_norm(x)."""
        B, L, D = x.shape

        def pool(K, lens=None, ks=None):
            if pre_norm is None:
                return ops.adaptive_pool(x, K, lens=lens, ks=ks)
            return ops.ln_adaptive_pool(x, pre_norm.weight, pre_norm.bias, pre_norm.eps, K, lens=lens, ks=ks)
        if lengths is None:
            pool_size = min(self._compute_pool_size(L, prev_pool_size), L)
            pooled = pool(pool_size)
        else:
            prev = prev_pool_size if prev_pool_size is not None else [None] * B
            sizes = [min(self._compute_pool_size(n, p), n) for n, p in zip(lengths, prev)]
            pool_size = max(sizes)
            pooled = pool(pool_size, lens=_device_ints(lengths, x.device), ks=_device_ints(sizes, x.device))
        w, b, qp = Q.linear_parts(self.pool_proj)
        out = ops.gemm(pooled.view(B * pool_size, D), w, b, qparams=qp)
        Q.record(self.pool_proj, out)
        return out.view(B, pool_size, D), (pool_size if lengths is None else sizes)

    def forward_differentiable(self, x: torch.Tensor, prev_pool_size=None,
                               lengths: Optional[Sequence[int]] = None):
        """The reference's forward (attention.py:46-78) for training: adaptive_avg_pool (HIP forward
        and backward), then pool_proj as a torch op.  lengths / prev_pool_size per utterance as in
        forward; the pooled rows past an utterance's size are pool_proj's bias, which nobody reads."""
        B, L, D = x.shape
        if lengths is None:
            pool_size = min(self._compute_pool_size(L, prev_pool_size), L)
            pooled = adaptive_avg_pool(x, pool_size)
        else:
            prev = prev_pool_size if prev_pool_size is not None else [None] * B
            sizes = [min(self._compute_pool_size(n, p), n) for n, p in zip(lengths, prev)]
            pool_size = max(sizes)
            pooled = adaptive_avg_pool(x, pool_size, lengths=lengths, sizes=sizes)
        out = torch.nn.functional.linear(pooled, self.pool_proj.weight, self.pool_proj.bias)
        return out, (pool_size if lengths is None else sizes)


class MultiHeadAttention(nn.Module):
    """Multi-head attention with a small attention dim (reference attention.py:81-164).

    The HIP core supports the pooled-key regime the model uses (kv_len <= 64, head_dim
    <= 32) and mask=None, which is the only way the reference calls it.
    """

    def __init__(self, d_model: int = 192, num_heads: int = 4, attention_dim: int = 48, dropout: float = 0.1):
        super().__init__()
        self.d_model = d_model
        self.num_heads = num_heads
        self.attention_dim = attention_dim
        self.head_dim = attention_dim // num_heads
        self.q_proj = nn.Linear(d_model, attention_dim)
        self.k_proj = nn.Linear(d_model, attention_dim)
        self.v_proj = nn.Linear(d_model, attention_dim)
        self.out_proj = nn.Linear(attention_dim, d_model)
        self.dropout = nn.Dropout(dropout)
        self.scale = math.sqrt(self.head_dim)

    def _kv_weights(self):
        """[k_proj; v_proj] as one GEMM: weights, biases and (if either is quantized) the
        per-column activation fake-quant of both halves."""
        def build():
            A = self.attention_dim
            w = torch.cat([Q.effective_weight(self.k_proj), Q.effective_weight(self.v_proj)], 0).contiguous()
            b = torch.cat([Q.inner(self.k_proj).bias, Q.inner(self.v_proj).bias], 0).contiguous()
            qk, qv = Q.act_qparams(self.k_proj, A), Q.act_qparams(self.v_proj, A)
            qp = None
            if qk is not None or qv is not None:
                qp = torch.cat([Q.act_qparams_or_identity(self.k_proj, A, w.device),
                                Q.act_qparams_or_identity(self.v_proj, A, w.device)], 0).contiguous()
            return w, b, qp
        return cached(self, "kv", Q.deps(self.k_proj) + Q.deps(self.v_proj), build)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                mask: Optional[torch.Tensor] = None, key_lengths: Optional[Sequence[int]] = None,
                project_out: bool = True) -> torch.Tensor:
        """key_lengths: per-utterance valid keys of a padded (B, Kp, D) key set.  project_out=False:
        the (B * Lq, attention_dim) head outputs before out_proj (GatedFusion.forward_attention
        folds out_proj into its global-branch product)."""
        if mask is not None:
            raise NotImplementedError("velocity_asr (MI355X build): attention masks are not supported "
                                      "(the reference path never passes one)")
        B, Lq, D = query.shape
        Kp = key.shape[1]
        A = self.attention_dim
        wq, bq, qpq = Q.linear_parts(self.q_proj)
        q = ops.gemm(query.reshape(B * Lq, D), wq, bq, qparams=qpq)
        Q.record(self.q_proj, q)
        if key is value:
            w_kv, b_kv, qp_kv = self._kv_weights()
            kv = ops.gemm(key.reshape(B * Kp, D), w_kv, b_kv, qparams=qp_kv)
        else:
            kv = torch.empty((B * Kp, 2 * A), device=query.device, dtype=torch.float32)
            for mod, src, sl in ((self.k_proj, key, slice(0, A)), (self.v_proj, value, slice(A, 2 * A))):
                w, b, qp = Q.linear_parts(mod)
                ops.gemm(src.reshape(B * Kp, D), w, b, out=kv[:, sl], qparams=qp)
        Q.record(self.k_proj, kv[:, :A])
        Q.record(self.v_proj, kv[:, A:])
        o = ops.pooled_attention(q, kv, B, Lq, Kp, self.num_heads,
                                 kps=None if key_lengths is None else _device_ints(key_lengths, q.device))
        if not project_out:
            return o
        wo, bo, qpo = Q.linear_parts(self.out_proj)
        out = ops.gemm(o, wo, bo, qparams=qpo)
        Q.record(self.out_proj, out)
        return out.view(B, Lq, D)

    def forward_differentiable(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                               mask: Optional[torch.Tensor] = None,
                               key_lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The reference's forward (attention.py:116-164) for training: the four projections as
        torch ops on this module's parameters (K and V by one F.linear on [k_proj; v_proj] when key
        is value), the softmax core as pooled_attention (HIP forward and backward).  The reference
        drops attention probabilities, which happens inside the fused kernel and is not built:
        refused in train() with dropout > 0.  key_lengths as in forward; zero the upstream gradient
        on padded query frames (pooled_attention)."""
        if mask is not None:
            raise NotImplementedError("velocity_asr (MI355X build): attention masks are not supported "
                                      "(the reference path never passes one)")
        if self.training and self.dropout.p > 0:
            raise NotImplementedError(
                "MultiHeadAttention.forward_differentiable: dropout on the attention probabilities acts inside the "
                f"fused HIP kernel and is not implemented (dropout p={self.dropout.p} in train mode); call eval() on "
                "this module or build it with dropout=0")
        F = torch.nn.functional
        A = self.attention_dim
        q = F.linear(query, self.q_proj.weight, self.q_proj.bias)
        if key is value:
            kv = F.linear(key, torch.cat([self.k_proj.weight, self.v_proj.weight], 0),
                          torch.cat([self.k_proj.bias, self.v_proj.bias], 0))
        else:
            kv = torch.cat([F.linear(key, self.k_proj.weight, self.k_proj.bias),
                            F.linear(value, self.v_proj.weight, self.v_proj.bias)], -1)
        o = pooled_attention(q, kv, self.num_heads, key_lengths=key_lengths)
        return F.linear(o, self.out_proj.weight, self.out_proj.bias)


class GatedFusion(nn.Module):
    """g * local_proj(local) + (1 - g) * global_proj(global) -> out_proj (reference attention.py:167-220)."""

    def __init__(self, d_model: int = 192):
        super().__init__()
        self.gate_proj = nn.Sequential(nn.Linear(d_model * 2, d_model), nn.Sigmoid())
        self.local_proj = nn.Linear(d_model, d_model)
        self.global_proj = nn.Linear(d_model, d_model)
        self.out_proj = nn.Linear(d_model, d_model)

    def _paired(self):
        """Rows interleaved in 32-row pairs so one wave holds gate and branch of the same column
        (weights, biases and, for quantized layers, the epilogue's activation fake-quant)."""
        gate, loc, glob = self.gate_proj[0], self.local_proj, self.global_proj

        def build():
            D = Q.inner(loc).weight.shape[0]
            if D % 32:
                raise NotImplementedError("GatedFusion on HIP needs d_model % 32 == 0")
            Wg = Q.effective_weight(gate)
            bg = Q.inner(gate).bias

            def pair(a, b):
                return torch.stack([a.reshape(D // 32, 32, *a.shape[1:]), b.reshape(D // 32, 32, *b.shape[1:])],
                                   1).reshape(2 * D, *a.shape[1:]).contiguous()
            w_local = pair(Wg[:, :D], Q.effective_weight(loc))      # [gate_l | local_proj]
            w_glob = pair(Wg[:, D:], Q.effective_weight(glob))      # [gate_g | global_proj]
            b_glob = pair(bg, Q.inner(glob).bias)
            qp = None
            if any(Q.act_qparams(m, D) is not None for m in (gate, loc, glob)):
                dev = Wg.device
                qp = torch.cat([pair(Q.act_qparams_or_identity(gate, D, dev), Q.act_qparams_or_identity(glob, D, dev)),
                                Q.act_qparams_or_identity(loc, D, dev)], 0).contiguous()
            return w_local, w_glob, b_glob, qp
        return cached(self, "paired", Q.deps(gate) + Q.deps(loc) + Q.deps(glob), build)

    def _paired_attention(self, mha: "MultiHeadAttention"):
        """The global branch with the attention's out_proj folded in: global_context = o Wo^T + bo
        feeds only this product, so [gate_g | global_proj] (o Wo^T + bo) + b = o ([gate_g |
        global_proj] Wo)^T + ([gate_g | global_proj] bo + b), the composite formed in float64 and
        rounded once (as the SSM's composed projection): K = attention_dim (48) instead of d_model,
        and no (B * L, d_model) global_context in HBM."""
        _, w_glob, b_glob, _ = self._paired()

        def build():
            wo, bo = mha.out_proj.weight, mha.out_proj.bias
            w = (w_glob.detach().double() @ wo.detach().double()).to(w_glob.dtype).contiguous()
            b = (ops.f32(b_glob).double() + w_glob.detach().double() @ ops.f32(bo).detach().double()).float().contiguous()
            return w, b
        return cached(self, "paired_attn", (w_glob, b_glob, mha.out_proj.weight, mha.out_proj.bias), build)

    def composable(self, mha: "MultiHeadAttention") -> bool:
        """forward_attention applies: plain Linears (no QAT fake-quant on global_context or the
        fusion's inputs), one weight dtype; VASR_ATTN_COMPOSE=0 keeps the separate out_proj."""
        mods = (mha.out_proj, self.gate_proj[0], self.local_proj, self.global_proj, self.out_proj)
        return (os.environ.get("VASR_ATTN_COMPOSE", "1") != "0" and all(type(m) is nn.Linear for m in mods)
                and len({m.weight.dtype for m in mods}) == 1 and mha.out_proj.bias is not None)

    def fusable(self, mha: "MultiHeadAttention", head_norm) -> bool:
        """forward_attention can run as ops.fusion_tail with head_norm (the LayerNorm that follows)
        inside: the composed path, fp32 weights, the kernel's widths (d_model 192, attention dim 48), a
        plain fp32 LayerNorm.  VASR_FUSION_TAIL=0 keeps the three GEMMs and the LayerNorm launch."""
        return (os.environ.get("VASR_FUSION_TAIL", "1") != "0" and type(head_norm) is nn.LayerNorm
                and self.composable(mha) and self.out_proj.weight.dtype == torch.float32
                and head_norm.weight is not None and head_norm.weight.dtype == torch.float32
                and head_norm.bias is not None and tuple(self.out_proj.weight.shape) == (192, 192)
                and mha.attention_dim == 48 and self.out_proj.bias is not None and self.local_proj.bias is not None)

    def forward_attention(self, local_features: torch.Tensor, o: torch.Tensor,
                          mha: "MultiHeadAttention", head_norm: Optional[nn.LayerNorm] = None) -> torch.Tensor:
        """forward(local_features, mha's output) from the attention's head outputs o (B * L, A).
        head_norm (extension, only where fusable(mha, head_norm)): head_norm of that, the whole chain
        in one launch (ops.fusion_tail), bitwise the separate launches."""
        B, L, D = local_features.shape
        local2 = local_features.reshape(B * L, D)
        w_local, _, _, qp = self._paired()
        w_glob, b_glob = self._paired_attention(mha)
        if head_norm is not None:
            y, _ = ops.fusion_tail(local2, o, w_local, w_glob, b_glob, self.local_proj.bias, self.out_proj.weight,
                                   self.out_proj.bias, head_norm.weight, head_norm.bias, head_norm.eps)
            return y.view(B, L, D)
        t1 = ops.gemm(local2, w_local)
        fused = ops.gemm(o, w_glob, b_glob, epilogue=_lib.EPI_PAIR_FUSION, aux=t1,
                         aux2=self.local_proj.bias, n_out=D, qparams=qp)
        out = ops.gemm(fused, self.out_proj.weight, self.out_proj.bias)
        return out.view(B, L, D)

    def _observe(self, local2: torch.Tensor, glob2: torch.Tensor) -> None:
        """Calibration only: the raw (pre-quantizer) gate / local / global outputs, summed in
        the fused epilogue's order ((local part + global part) + bias for the gate)."""
        gate, loc, glob = self.gate_proj[0], self.local_proj, self.global_proj
        D = local2.shape[1]
        Wg = Q.effective_weight(gate)
        if Q.observing(gate):
            t = ops.gemm(local2, Wg[:, :D].contiguous())
            Q.record(gate, ops.gemm(glob2, Wg[:, D:].contiguous(), epilogue=_lib.EPI_RESIDUAL, aux=t)
                     + Q.inner(gate).bias.detach())
        for mod, src in ((loc, local2), (glob, glob2)):
            if Q.observing(mod):
                Q.record(mod, ops.gemm(src, Q.effective_weight(mod), Q.inner(mod).bias))

    def forward(self, local_features: torch.Tensor, global_features: torch.Tensor) -> torch.Tensor:
        B, L, D = local_features.shape
        local2, glob2 = local_features.reshape(B * L, D), global_features.reshape(B * L, D)
        self._observe(local2, glob2)
        w_local, w_glob, b_glob, qp = self._paired()
        t1 = ops.gemm(local2, w_local)
        fused = ops.gemm(glob2, w_glob, b_glob, epilogue=_lib.EPI_PAIR_FUSION, aux=t1,
                         aux2=Q.inner(self.local_proj).bias, n_out=D, qparams=qp)
        wo, bo, qpo = Q.linear_parts(self.out_proj)
        out = ops.gemm(fused, wo, bo, qparams=qpo)
        Q.record(self.out_proj, out)
        return out.view(B, L, D)

    def forward_differentiable(self, local_features: torch.Tensor, global_features: torch.Tensor) -> torch.Tensor:
        """The reference's forward (attention.py:191-220) for training, as torch ops on this module's
        parameters: gate = sigmoid(gate_proj([local | global])), out_proj(gate * local_proj(local) +
        (1 - gate) * global_proj(global))."""
        F = torch.nn.functional
        gate = self.gate_proj(torch.cat([local_features, global_features], dim=-1))
        local_t = F.linear(local_features, self.local_proj.weight, self.local_proj.bias)
        global_t = F.linear(global_features, self.global_proj.weight, self.global_proj.bias)
        return F.linear(gate * local_t + (1 - gate) * global_t, self.out_proj.weight, self.out_proj.bias)


class HierarchicalGlobalContext(nn.Module):
    """pool1 -> GlobalSSM -> pool2 -> norm -> cross-attention -> gated fusion (reference attention.py:223-319)."""

    def __init__(self, d_model: int = 192, num_heads: int = 4, attention_dim: int = 48, global_ssm_layers: int = 2,
                 global_ssm_state_dim: int = 32, dropout: float = 0.1):
        super().__init__()
        self.pool1 = AdaptivePool(level=1, d_model=d_model)
        self.global_ssm = GlobalSSM(d_model=d_model, num_layers=global_ssm_layers, state_dim=global_ssm_state_dim,
                                    dropout=dropout)
        self.pool2 = AdaptivePool(level=2, d_model=d_model)
        self.cross_attention = MultiHeadAttention(d_model=d_model, num_heads=num_heads, attention_dim=attention_dim,
                                                  dropout=dropout)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.fusion = GatedFusion(d_model=d_model)

    def forward(self, local_features: torch.Tensor, lengths: Optional[Sequence[int]] = None,
                query: Optional[torch.Tensor] = None, head_norm: Optional[nn.LayerNorm] = None):
        """lengths: per-utterance token counts of a zero-padded batch (None: all L).  Pooling
        sizes and attention keys then follow each utterance's own length; the global SSM is
        causal, so the junk rows past an utterance's pooled tokens never reach them.
        query (extension): norm2(local_features) when the caller already has it
        (LocalSSMProcessor.forward_pair).
        head_norm (extension): the LayerNorm the caller applies next (the CTC head's).  The result is
        then (rows, normalised): head_norm(fused features) and True where the gated fusion takes it
        into its own launch (GatedFusion.fusable), else the fused features and False."""
        x_pool1, pool_size1 = self.pool1(local_features, lengths=lengths)
        # VASR_POOL_PRENORM=1: the global stack's final LayerNorm inside the second pooling launch.
        # Bitwise the same, and 3.5 vs 5.3 us graph-timed alone at C2's 32 x 64 -> 16 rows, but C2
        # 0.3 % slower in the model's graph over three interleaved rounds (profiles/r06bh/, r06bi/):
        # off by default
        gnorm = self.global_ssm.norm
        fold = os.environ.get("VASR_POOL_PRENORM", "0") == "1" and type(gnorm) is nn.LayerNorm
        x_ssm = self.global_ssm(x_pool1, raw=fold)
        x_pool2, pool_size2 = self.pool2(x_ssm, prev_pool_size=pool_size1,
                                         lengths=None if lengths is None else pool_size1,
                                         pre_norm=gnorm if fold else None)
        x_pool2 = ops.layer_norm(x_pool2, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        if query is None:
            query = ops.layer_norm(local_features, self.norm2.weight, self.norm2.bias, self.norm2.eps)
        kl = None if lengths is None else pool_size2
        if self.fusion.composable(self.cross_attention):
            o = self.cross_attention(query=query, key=x_pool2, value=x_pool2, key_lengths=kl, project_out=False)
            if head_norm is not None and self.fusion.fusable(self.cross_attention, head_norm):
                return self.fusion.forward_attention(local_features, o, self.cross_attention, head_norm), True
            out = self.fusion.forward_attention(local_features, o, self.cross_attention)
        else:
            global_context = self.cross_attention(query=query, key=x_pool2, value=x_pool2, key_lengths=kl)
            out = self.fusion(local_features, global_context)
        return out if head_norm is None else (out, False)

    def forward_differentiable(self, local_features: torch.Tensor,
                               lengths: Optional[Sequence[int]] = None) -> torch.Tensor:
        """The reference's forward (attention.py:283-319) for training: every stage's
        forward_differentiable (the poolings and the attention core by their HIP forward and backward
        kernels, the global stack by GlobalSSM.forward_differentiable), the two LayerNorms as torch
        ops.  loss.backward() reaches every parameter and local_features.

        lengths: per-utterance token counts of a zero-padded batch; pool sizes and key counts then
        follow each utterance as in forward, and the global SSM is causal.  As with selective_scan,
        the caller zeroes the upstream gradient on the padded frames: the gradients of the valid
        frames and of the parameters are then those of each utterance run alone."""
        x_pool1, pool_size1 = self.pool1.forward_differentiable(local_features, lengths=lengths)
        x_ssm = self.global_ssm.forward_differentiable(x_pool1)
        x_pool2, pool_size2 = self.pool2.forward_differentiable(x_ssm, prev_pool_size=pool_size1,
                                                                lengths=None if lengths is None else pool_size1)
        x_pool2 = self.norm1(x_pool2)
        query = self.norm2(local_features)
        global_context = self.cross_attention.forward_differentiable(
            query=query, key=x_pool2, value=x_pool2, key_lengths=None if lengths is None else pool_size2)
        return self.fusion.forward_differentiable(local_features, global_context)
