"""MLP head (reference: src/model/model_utils/utils.py:6-17).  The dense head is plain GEMM work
and stays nn.Linear on rocBLAS/hipBLASLt -- it is adjacent to, not part of, the HIP hot path.
Module nesting (`.network` = nn.Sequential of Linear/ReLU) keeps the reference's state_dict keys.

Opt-in (`NRX_MLP_WGRAD=1`, or `utils.MLP_WGRAD = True` before the model is built): the layers' WEIGHT gradient runs on
nrx_linear_wgrad -- at batch 65 536 that GEMM contracts over the batch and is the largest single item of a full training step on
the vendor library (tools/bench_full_step_c2.py).  Forward, input gradient, parameters and state_dict keys are unchanged."""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

MLP_WGRAD = os.environ.get("NRX_MLP_WGRAD", "0") == "1"
# NRX_FUSED_ATTENTION=0 (or utils.FUSED_ATTENTION = False): MultiHeadSelfAttention keeps to its torch path on the GPU too (A/B runs)
FUSED_ATTENTION = os.environ.get("NRX_FUSED_ATTENTION", "1") != "0"


class _Linear(nn.Linear):
    """nn.Linear (same parameters / state_dict keys) whose backward computes g_W with nrx_linear_wgrad on fp32 CUDA inputs."""

    def forward(self, x):
        if x.is_cuda and x.dtype == self.weight.dtype and (x.requires_grad or self.weight.requires_grad):
            from ... import ops
            return ops.linear(x, self.weight, self.bias)
        return super().forward(x)


class MLP(nn.Module):
    def __init__(self, dims=(16, 32, 32, 1)):
        super().__init__()
        dims = list(dims)
        layers = []
        last = len(dims) - 2
        linear = _Linear if MLP_WGRAD else nn.Linear
        for i, (d_in, d_out) in enumerate(zip(dims[:-1], dims[1:])):
            layers.append(linear(d_in, d_out))
            if i < last:
                layers.append(nn.ReLU())
        self.network = nn.Sequential(*layers)

    def forward(self, x):
        return self.network(x)


def attention_math(qkv, num_heads, key_mask=None):
    """The definition of ops.seq_attention in plain torch, on any device and dtype: qkv [B, N, 3 C] -> [B, N, C].  Without a mask this is
    the reference's arithmetic (src/model/model_utils/utils.py:33-38): scores / sqrt(head_dim), softmax over the keys, probabilities @ v.
    key_mask [B, N]: key j takes part iff key_mask[b, j] != 0; a sample with no kept key gives zeros."""
    B, N, W = qkv.shape
    C = W // 3
    head_dim = C // num_heads
    q, k, v = qkv.reshape(B, N, 3, num_heads, head_dim).permute(2, 0, 3, 1, 4)          # each [B, H, N, head_dim]
    scores = (q @ k.transpose(-2, -1)) / (head_dim ** 0.5)
    if key_mask is None:
        probs = F.softmax(scores, dim=-1)
    else:
        keep = (key_mask != 0).reshape(B, 1, 1, N)
        some = keep.any(dim=-1, keepdim=True)
        # (a sample with nothing kept: a softmax over -inf alone is NaN, so its scores stay as they are and its probabilities are zeroed)
        probs = F.softmax(scores.masked_fill(~keep & some, float("-inf")), dim=-1) * some.to(scores.dtype)
    return (probs @ v).transpose(1, 2).reshape(B, N, C)


class MultiHeadSelfAttention(nn.Module):
    """Self-attention over [B, N, embed_dim] (reference: src/model/model_utils/utils.py:20-40; the same constructor, attributes and
    state_dict keys, so a reference checkpoint loads with strict=True).  forward(x, mask=None): mask is the [B, N] `<name>_mask` of the
    DataReader, used as the key mask.  On fp32 CUDA inputs of a shape ops.seq_attention takes, the core between the two projections is that
    fused op; everything else (CPU, other dtypes, N > 128, other head widths) runs attention_math, the same definition in torch."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError(f"embed_dim ({embed_dim}) must be divisible by num_heads ({num_heads})")
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_dim = embed_dim // num_heads
        self.qkv_proj = nn.Linear(embed_dim, embed_dim * 3)
        self.out_proj = nn.Linear(embed_dim, embed_dim)

    def _fused(self, qkv):
        if not (FUSED_ATTENTION and qkv.is_cuda and qkv.dtype == torch.float32):
            return False
        from ... import ops
        return ops.seq_attention_supported(qkv.shape[1], self.num_heads, self.head_dim)

    def forward(self, x, mask=None):
        qkv = self.qkv_proj(x)
        if self._fused(qkv):
            from ... import ops
            core = ops.seq_attention(qkv, self.num_heads, key_mask=mask)
        else:
            core = attention_math(qkv, self.num_heads, mask)
        return self.out_proj(core)


class TransformerBlock(nn.Module):
    """Post-norm encoder block (reference: src/model/model_utils/utils.py:43-61; the same constructor, attributes and state_dict keys):
    x = norm1(x + dropout(attention(x, mask))); x = norm2(x + dropout(ffn(x))).  The projections, LayerNorm, FFN and dropout are torch."""

    def __init__(self, embed_dim, num_heads, ff_dim, dropout=0.0):
        super().__init__()
        self.attention = MultiHeadSelfAttention(embed_dim, num_heads)
        self.norm1 = nn.LayerNorm(embed_dim)
        self.ffn = nn.Sequential(nn.Linear(embed_dim, ff_dim), nn.ReLU(), nn.Linear(ff_dim, embed_dim))
        self.norm2 = nn.LayerNorm(embed_dim)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, mask=None):
        x = self.norm1(x + self.dropout(self.attention(x, mask)))
        return self.norm2(x + self.dropout(self.ffn(x)))
