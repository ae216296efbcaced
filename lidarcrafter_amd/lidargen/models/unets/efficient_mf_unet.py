"""MFEfficientUNet: the MeanFlow range-image generator on the gfx950 kernels.

API / state_dict mirror of the reference's `lidargen/models/unets/efficient_mf_unet.py`, which differs from
efficient_unet.py in two places only:

  * the self-attention is timm's `Attention(dim, num_heads, qkv_bias=True, qk_norm=True, norm_layer=RMSNorm)` with
    `fused_attn=False` (RMSNorm :23-30): q and k of every head are L2-normalised and scaled by sqrt(head_dim) and one
    learnable gain each, then softmax(q k^T / sqrt(head_dim)) v and a `proj` Linear (not zero-initialised);
  * two time MLPs, `start_time_embedding(t) + end_time_embedding(r)` with t, r in [0, 1].

Everything else -- ResidualBlock, Block, ring convs, FIR resampling, GroupNorm / AdaGN, Fourier coordinates, the level
layout and every fold of the EfficientUNet hot path -- is efficient_unet.py's.  The attention runs as there (the qkv
projection as a 1x1 conv on the GroupNorm's output, channel-major attention, `proj` + residual + 1/sqrt(2) in the conv
epilogue) with one pass added between projection and attention: ops.qk_norm_cm (csrc/flow.hip).  Training (MeanFlow.loss)
runs autograd.mf_unet_forward_jvp: the differentiable forward with its tangent alongside (csrc/flow_jvp.hip).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from lidarcrafter_amd import autograd as AG
from lidarcrafter_amd import ops as K

from . import ops
from .efficient_unet import EfficientUNet


class RMSNorm(nn.Module):
    """Parameter container of the reference's RMSNorm (efficient_mf_unet.py:23-30): F.normalize(x, dim=-1) * scale * g.
    Applied by ops.qk_norm_cm on the channel-major qkv projection, never on its own."""

    def __init__(self, dim):
        super().__init__()
        self.scale = dim ** 0.5
        self.g = nn.Parameter(torch.ones(1))

    def forward(self, x):
        raise NotImplementedError("RMSNorm runs inside SelfAttentionBlock (ops.qk_norm_cm); there is no eager path")


class _TimmAttentionParams(nn.Module):
    """Parameter container with timm Attention's names / shapes (qkv_bias=True, qk_norm=True, norm_layer=RMSNorm).
    The qkv weight rows are packed (3, heads, head_dim), as nn.MultiheadAttention's in_proj_weight."""

    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.q_norm = RMSNorm(self.head_dim)
        self.k_norm = RMSNorm(self.head_dim)
        self.proj = nn.Linear(dim, dim)


class SelfAttentionBlock(nn.Module):
    def __init__(self, in_channels, num_heads, gn_eps=1e-6, gn_num_groups=8, scale=1 / np.sqrt(2)):
        super().__init__()
        self.norm = ops.GroupNorm(gn_num_groups, in_channels, gn_eps)
        self.attn = _TimmAttentionParams(in_channels, num_heads)
        self.register_buffer("scale", torch.tensor(scale).float())
        self._scale_f = float(scale)
        self._pk_in, self._pk_out = K.PackedConv(), K.PackedConv()

    def forward(self, x, out=None):
        B, C, H, W = x.shape
        a = self.attn
        # qkv on channel-major tokens == 1x1 conv on NCHW: the three routes of efficient_unet.SelfAttentionBlock
        w_in = a.qkv.weight[:, :, None, None]
        if K.fuse_gn(3 * C):
            qkv = K.conv2d_ring(x, self._pk_in, w_in, a.qkv.bias, gn_coeffs=self.norm.coeffs(x), gn_silu=False)
        elif K.presplit_1x1(C, 3 * C, self.norm.num_groups):
            qkv = K.conv2d_ring(self.norm(x, split_for=self._pk_in), self._pk_in, w_in, a.qkv.bias)
        else:
            qkv = K.conv2d_ring(self.norm(x), self._pk_in, w_in, a.qkv.bias)
        t = qkv.view(B, 3 * C, H * W)
        q, k = t[:, :C], t[:, C:2 * C]
        K.qk_norm_cm(q, k, a.num_heads, a.q_norm.g, a.k_norm.g)        # in place: q_norm(q), k_norm(k)
        o = K.attention_cm(q, k, t[:, 2 * C:], a.num_heads, scale=a.scale)
        # proj + residual + 1/sqrt(2) in the conv epilogue (+ octet statistics for the next block's first GroupNorm)
        return K.conv2d_ring(o.view(B, C, H, W), self._pk_out, a.proj.weight[:, :, None, None], a.proj.bias,
                             res=x, out=out, out_scale=self._scale_f, emit_stats=True)


class MFEfficientUNet(EfficientUNet):
    """forward(images, start_timesteps, end_timesteps, condition=None) -> the average velocity u(z, t, r)."""

    _attn_cls = SelfAttentionBlock

    def __init__(self, in_channels: int, resolution, out_channels: int | None = None,
                 base_channels: int = 128, temb_channels: int | None = None,
                 channel_multiplier=(1, 2, 4, 8), num_residual_blocks=(3, 3, 3, 3),
                 gn_num_groups: int = 32 // 4, gn_eps: float = 1e-6, attn_num_heads: int = 8,
                 coords_encoding="spherical_harmonics", ring: bool = True):
        super().__init__(in_channels, resolution, out_channels=out_channels, base_channels=base_channels,
                         temb_channels=temb_channels, channel_multiplier=channel_multiplier,
                         num_residual_blocks=num_residual_blocks, gn_num_groups=gn_num_groups, gn_eps=gn_eps,
                         attn_num_heads=attn_num_heads, coords_encoding=coords_encoding, ring=ring)
        temb_channels = base_channels * 4 if temb_channels is None else temb_channels
        del self.time_embedding

        def mlp():
            return nn.Sequential(ops.SinusoidalPositionalEmbedding(base_channels),
                                 nn.Linear(base_channels, temb_channels), nn.SiLU(),
                                 nn.Linear(temb_channels, temb_channels))

        self.start_time_embedding = mlp()
        self.end_time_embedding = mlp()
        self._temb_cache = None

    def _temb_weights(self):
        """[W3_start | W3_end] and b3_start + b3_end: the two output Linears as ONE launch on the concatenated hidden
        rows; rebuilt when a parameter changes (address / version), like EfficientUNet._ada_weights."""
        ls, le = self.start_time_embedding[3], self.end_time_embedding[3]
        key = tuple((p.data_ptr(), p._version) for p in (ls.weight, ls.bias, le.weight, le.bias))
        if self._temb_cache is None or self._temb_cache[0] != key:
            w = torch.cat([ls.weight.detach(), le.weight.detach()], 1).contiguous()
            b = (ls.bias.detach() + le.bias.detach()).contiguous()
            self._temb_cache = (key, w, b)
        return self._temb_cache[1], self._temb_cache[2]

    def time_features(self, t: torch.Tensor, r: torch.Tensor):
        """start times t [M], end times r [M] -> (temb [M, T] = start(t) + end(r), all AdaGN (scale|shift) rows)."""
        se, ee = self.start_time_embedding, self.end_time_embedding
        hs = K.linear(se[0](t), se[1].weight, se[1].bias, act_out=True)
        he = K.linear(ee[0](r), ee[1].weight, ee[1].bias, act_out=True)
        w, b = self._temb_weights()
        temb = K.linear(torch.cat([hs, he], 1), w, b)
        wa, ba = self._ada_weights()
        return temb, K.linear(temb, wa, ba, act_in=True)

    @torch.compiler.disable
    @K.range_checked
    def forward(self, images: torch.Tensor, start_timesteps: torch.Tensor, end_timesteps: torch.Tensor,
                condition=None, time_features=None):
        """images [B, C, H, W], start / end times [B] (or 0-d) -> [B, C_out, H, W].  `condition` is accepted and unused,
        as in the reference.  `time_features`: optional precomputed `self.time_features(t, r)` (MeanFlow.sample hoists
        them).  In grad mode on the GPU the result is the differentiable u of autograd.mf_unet_forward (MeanFlow
        training; its tangent comes from `forward_jvp`)."""
        if time_features is None and AG.training_active(self, images):
            if not images.is_cuda:
                raise NotImplementedError(
                    "MFEfficientUNet: the jvp / training forward runs on the GPU kernels only; there is no CPU path")
            return AG.mf_unet_forward(self, images, start_timesteps.to(images), end_timesteps.to(images))
        B = images.shape[0]
        if time_features is None:
            t, r = start_timesteps, end_timesteps
            if t.dim() == 0:
                t = t[None].repeat_interleave(B, dim=0)
            if r.dim() == 0:
                r = r[None].repeat_interleave(B, dim=0)
            time_features = self.time_features(t.to(images), r.to(images))
        return self._unet(images, time_features)

    @torch.compiler.disable
    @K.range_checked
    def forward_jvp(self, images, start_timesteps, end_timesteps, d_images, d_start, d_end):
        """(u, du) = (self(images, t, r), its directional derivative along (d_images, d_start, d_end)) -- what
        torch.func.jvp(model, (z, t, r), (v, 1, 0)) gives MeanFlow.loss.  u carries the autograd graph of the training
        forward when grad mode is on; du never does (the tangent runs under no_grad next to the primal: u's parameter
        gradients are all the MeanFlow loss needs, its target being stop-gradient).  GPU only."""
        if not images.is_cuda:
            raise NotImplementedError(
                "MFEfficientUNet.forward_jvp: the jvp / training forward runs on the GPU kernels only; there is no CPU path")
        f = lambda t_: torch.as_tensor(t_, dtype=torch.float32).to(images.device)
        return AG.mf_unet_forward_jvp(self, images, f(start_timesteps), f(end_timesteps), d_images.to(images),
                                      f(d_start), f(d_end))
