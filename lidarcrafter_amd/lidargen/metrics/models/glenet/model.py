"""Mirror of the reference's `lidargen/metrics/models/glenet/model.py`: `Encoder_x`, `Encoder_xy`, `Object_feat_encoder` and
`Generator(model_cfg, input_channels, scale)` with the reference's module names and all 110 state-dict keys (`global_step`
and the `xy_encoder.*` keys that inference never reads included), so `checkpoint['model_state']` loads with strict=True.
`model_cfg` is a plain mapping with the keys of exp20.yaml's MODEL block (`DEFAULT_MODEL_CFG`).

Eval mode only.  One plan: the two per-point trunks and their max per (draw, object) row in the fused
kernel of csrc/glenet.hip, which gathers every row's points through its index list; every dense layer behind them on the
exact-fp32 dense kernel of csrc/pointmlp.hip with the rows as its columns ([1, C, R], channel-major), BatchNorm folded on
the host in float64.  Not built (NotImplementedError by name): training mode, the losses, CPU tensors (RuntimeError)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from lidarcrafter_amd import ops_glenet as KG
from lidarcrafter_amd import ops_pointmlp as KM

from ...extractor.pointnet import _plain, fold_bn
from .point_net import PointNetfeat, SimPointNetfeat, _no_forward

DEFAULT_MODEL_CFG = {
    "INPUT_CHANNELS": 3, "LATENT_DIM": 8, "DIR_OFFSET": 0.78539, "DIR_LIMIT_OFFSET": 0.0, "NUM_DIR_BINS": 2,
    "LOSS_CONFIG": {"LOSS_WEIGHTS": {"latent_weight": 10, "loc_weight": 10.0, "dir_weight": 0.002,
                                     "code_weights": [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]}},
}
ROWS_PER_PASS = 16384        # rows (draw, object) per pass of sample_boxes: bounds the [1024, R] operand of the widest layer


def _not_built_loss(name):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"{name} is not built: GLENet training and its losses are out of scope, the sampler is "
                                  "inference only")
    fn.__name__ = name
    return fn


l2_regularisation = _not_built_loss("l2_regularisation")


class _LossNotBuilt(nn.Module):
    """Stands where the reference registers `reg_loss_func` / `dir_loss_func` (modules without state)."""

    def __init__(self, name):
        super().__init__()
        self._name = name

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{self._name} is not built: GLENet training and its losses are out of scope")


class Encoder_x(nn.Module):
    def __init__(self, input_channels, x=1, latent_size=3):
        super().__init__()
        self.input_channels = input_channels
        self.fe = PointNetfeat(input_channels, x)
        fe_out_channels = 512 * x
        self.fc1 = nn.Linear(fe_out_channels, latent_size)
        self.fc2 = nn.Linear(fe_out_channels, latent_size)

    forward = _no_forward


class Encoder_xy(nn.Module):
    def __init__(self, input_channels, x=1, latent_size=3):
        super().__init__()
        self.input_channels = input_channels
        self.fe = PointNetfeat(input_channels, x)
        fe_out_channels = 512 * x
        self.fc1 = nn.Linear(fe_out_channels + 8, latent_size)
        self.fc2 = nn.Linear(fe_out_channels + 8, latent_size)

    def forward(self, *args, **kwargs):
        raise NotImplementedError("Encoder_xy.forward is not built: the posterior encoder is used in training only")


class Object_feat_encoder(nn.Module):
    def __init__(self, input_channels, x=1, latent_dim=3, num_bins=2):
        super().__init__()
        x = 0.5                                # as the reference: the argument is overwritten
        self.fe = SimPointNetfeat(input_channels, x)
        fe_out_channels = int(16 * x)
        fc_scale = 0.25
        w = int(256 * fc_scale)
        self.fc1 = nn.Linear(fe_out_channels + latent_dim, w)
        self.fc2 = nn.Linear(w, w)
        self.bn1 = nn.BatchNorm1d(w)
        self.bn2 = nn.BatchNorm1d(w)
        self.fc_s1 = nn.Linear(w, w)
        self.fc_s2 = nn.Linear(w, 3, bias=False)
        self.fc_ce1 = nn.Linear(w, w)
        self.fc_ce2 = nn.Linear(w, 3, bias=False)
        self.fc_hr1 = nn.Linear(w, w)
        self.fc_hr2 = nn.Linear(w, 1, bias=False)
        self.fc_dir1 = nn.Linear(w, w)
        self.fc_dir2 = nn.Linear(w, num_bins, bias=False)

    forward = _no_forward


def _cfg(cfg, key, default=None):
    if isinstance(cfg, dict) or hasattr(cfg, "keys"):
        return cfg[key] if key in cfg else default
    return getattr(cfg, key, default)


def heading_postprocess(box: torch.Tensor, dir_offset: float, dir_limit_offset: float, num_bins: int) -> torch.Tensor:
    """The reference's post-processing of the sampled box [.., 9], in place: label = argmax of the two direction logits (1 iff
    dir[1] > dir[0]); v = box[6] - dir_offset; rot = v - floor(v / period + dir_limit_offset) period (limit_period), period =
    2 pi / num_bins; box[6] = rot + dir_offset + period label."""
    labels = torch.max(box[..., -2:], dim=-1)[1]
    period = 2 * np.pi / num_bins
    v = box[..., 6] - dir_offset
    rot = v - torch.floor(v / period + dir_limit_offset) * period
    box[..., 6] = rot + dir_offset + period * labels.to(box.dtype)
    return box


class Generator(nn.Module):
    def __init__(self, model_cfg, input_channels, scale):
        super().__init__()
        self.model_cfg = model_cfg
        self.latent_dim = int(_cfg(model_cfg, "LATENT_DIM"))
        self.obj_encoder = Object_feat_encoder(input_channels, scale, latent_dim=self.latent_dim)
        self.xy_encoder = Encoder_xy(input_channels, scale, self.latent_dim)
        self.x_encoder = Encoder_x(input_channels, scale, self.latent_dim)
        self.add_module("reg_loss_func", _LossNotBuilt("reg_loss_func"))
        self.add_module("dir_loss_func", _LossNotBuilt("dir_loss_func"))
        self.register_buffer("global_step", torch.LongTensor(1).zero_())
        self.last_batch_dict = None
        self.last_tb_dict = None

    def update_global_step(self):
        self.global_step += 1

    kl_divergence = staticmethod(_not_built_loss("Generator.kl_divergence"))
    reg_loss = staticmethod(_not_built_loss("Generator.reg_loss"))
    get_training_loss = staticmethod(_not_built_loss("Generator.get_training_loss"))
    add_sin_difference = staticmethod(_not_built_loss("Generator.add_sin_difference"))
    get_direction_target = staticmethod(_not_built_loss("Generator.get_direction_target"))

    @staticmethod
    def reparametrize(mu, logvar, eps):
        """z = eps exp(0.5 logvar) + mu, the reference's expression with `eps` given (its own draw comes from the global CUDA
        stream, which cannot be reproduced)."""
        std = logvar.mul(0.5).exp_()
        return eps.mul(std).add_(mu)

    # ---- the fold --------------------------------------------------------------------------------------------------------
    def _fingerprint(self):
        return tuple((t.data_ptr(), t._version, str(t.device), t.dtype)
                     for t in list(self.parameters()) + list(self.buffers()))

    def plan_weights(self) -> dict:
        """The float32 weights of the plan, BatchNorm folded in float64 (scale inside the weights: a negative scale does not
        commute with the max): 'main' / 'side' the two trunks as (w1, b1, w2, b2, w3, b3); every dense layer as (w, b) --
        x_fc stacks fc1 | fc2 (mu | logvar), o_h1 stacks the four heads' first layers (centre, size, heading, direction) and
        o_h2 is their second layers as one block-diagonal [9, 256] matrix (head i reads its own 64 hidden channels; the
        zero blocks add exact zeros)."""
        with torch.no_grad():
            xe, oe = self.x_encoder, self.obj_encoder

            def trunk(fe):
                out = []
                for conv, bn in ((fe.conv1, fe.bn1), (fe.conv2, fe.bn2), (fe.conv3, fe.bn3)):
                    out += list(fold_bn(conv.weight, conv.bias, bn))
                return tuple(out)

            def lin(m):
                return _plain(m.weight, m.bias)

            w = oe.fc1.weight.shape[0]
            heads1 = (oe.fc_ce1, oe.fc_s1, oe.fc_hr1, oe.fc_dir1)
            heads2 = (oe.fc_ce2, oe.fc_s2, oe.fc_hr2, oe.fc_dir2)
            rows = sum(m.weight.shape[0] for m in heads2)
            w2 = torch.zeros((rows, 4 * w), dtype=torch.float32, device=oe.fc1.weight.device)
            r0 = 0
            for i, m in enumerate(heads2):
                w2[r0:r0 + m.weight.shape[0], i * w:(i + 1) * w] = m.weight.detach().float()
                r0 += m.weight.shape[0]
            return {
                "main": trunk(xe.fe), "side": trunk(oe.fe),
                "x_seq0": lin(xe.fe.output_sequential[0]), "x_seq2": lin(xe.fe.output_sequential[2]),
                "x_fc": _plain(torch.cat([xe.fc1.weight, xe.fc2.weight]), torch.cat([xe.fc1.bias, xe.fc2.bias])),
                "o_seq0": lin(oe.fe.output_sequential[0]), "o_seq2": lin(oe.fe.output_sequential[2]),
                "o_fc1": fold_bn(oe.fc1.weight, oe.fc1.bias, oe.bn1),
                "o_fc2": fold_bn(oe.fc2.weight, oe.fc2.bias, oe.bn2),
                "o_h1": _plain(torch.cat([m.weight for m in heads1]), torch.cat([m.bias for m in heads1])),
                "o_h2": (w2, torch.zeros(rows, device=w2.device)),
            }

    def folded(self) -> dict:
        """`plan_weights()` as the kernels take them -- the trunks as they are, every dense layer as (packed weight, bias, Co)
        -- on the parameters' device; made again when any parameter or buffer changed."""
        key = self._fingerprint()
        hit = self.__dict__.get("_lc_folded")
        if hit is not None and hit[0] == key:
            return hit[1]
        f = {}
        for name, t in self.plan_weights().items():
            if name in ("main", "side"):
                f[name] = t
            else:
                w, b = t
                f[name] = (KM.pack_weight(w.cpu().contiguous()).to(w.device), b.contiguous(), w.shape[0])
        self.__dict__["_lc_folded"] = (key, f)
        return f

    # ---- the plan --------------------------------------------------------------------------------------------------------
    def _check_mode(self, who):
        if self.training:
            raise NotImplementedError(f"{who}: training mode is not built (the posterior encoder, the KL and regression losses, "
                                      "BatchNorm batch statistics) -- call .eval() first")

    @staticmethod
    def _check_cuda(who, **tensors):
        for name, t in tensors.items():
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError(f"{who}: `{name}` must be a CUDA(HIP) tensor -- the sampler has no CPU fallback")

    def _rows(self, norm, offsets, text_cm, choice, eps, postprocess=True):
        """[D,B,9] for one pass: norm [total,3] normalised points, text_cm [512,B], choice int32 [D,B,K], eps [D,B,latent]."""
        f = self.folded()
        D, B, _ = choice.shape
        R, L = D * B, self.latent_dim
        dev = norm.device
        xcat = torch.empty((1, 1024, R), device=dev, dtype=torch.float32)
        ocat = torch.empty((1, 8 + 512, R), device=dev, dtype=torch.float32)
        KG.glenet_trunk(norm, offsets, choice, f["main"], f["side"], out=(xcat[0, :512], ocat[0, :8]))
        text = text_cm.repeat(1, D)                               # column r = d B + b holds object b's text feature
        xcat[0, 512:] = text
        ocat[0, 8:] = text

        def run(t, name, act):
            wpk, b, Co = f[name]
            return KM.conv(t, wpk, b, Co, act)

        ml = run(run(run(xcat, "x_seq0", True), "x_seq2", False), "x_fc", False)      # [1, 2 L, R]: mu | logvar
        z = self.reparametrize(ml[0, :L], ml[0, L:], eps.reshape(R, L).t())
        o = run(run(ocat, "o_seq0", True), "o_seq2", False)
        h = torch.cat([o[0], z], dim=0).unsqueeze(0).contiguous()                      # [1, 8 + L, R]
        feat = run(run(h, "o_fc1", True), "o_fc2", True)
        box = run(run(feat, "o_h1", True), "o_h2", False)[0].t().contiguous()          # [R, 9]
        if postprocess:
            cfg = self.model_cfg
            heading_postprocess(box, _cfg(cfg, "DIR_OFFSET"), _cfg(cfg, "DIR_LIMIT_OFFSET"), _cfg(cfg, "NUM_DIR_BINS"))
        return box.reshape(D, B, 9)

    def sample_boxes(self, points, offsets, text_feat, choice, eps, postprocess=True):
        """[D,B,9]: D draws for each of the B objects of a ragged batch.  points float32 [total,3] (raw object points),
        offsets int32 [B+1], text_feat [B,512], choice int32 [D,B,K] (indices into each object's own rows: the reference's
        np.random.choice(n, 512, replace=True), made by the caller), eps [D,B,latent].  The points are centred and scaled
        once per object (ops_glenet.segment_center), not once per draw.  postprocess=False returns obj_encoder's output
        without the heading post-process.  An object without points raises ValueError."""
        self._check_mode("Generator.sample_boxes")
        self._check_cuda("Generator.sample_boxes", points=points, offsets=offsets, text_feat=text_feat, choice=choice,
                         eps=eps)
        B = offsets.numel() - 1
        if B < 1 or bool((offsets[1:] <= offsets[:-1]).any()):
            raise ValueError("Generator.sample_boxes: an object without points (the reference's dataset builds a 4-channel "
                             "zero cloud for it, which its 3-channel network cannot take)")
        if choice.dim() != 3 or choice.shape[1] != B or tuple(eps.shape) != (choice.shape[0], B, self.latent_dim) \
                or tuple(text_feat.shape) != (B, 512):
            raise ValueError(f"Generator.sample_boxes: choice {tuple(choice.shape)}, eps {tuple(eps.shape)}, text_feat "
                             f"{tuple(text_feat.shape)} for {B} objects and latent {self.latent_dim}")
        with torch.cuda.device(points.device), torch.no_grad():
            norm, _ = KG.segment_center(points.float().contiguous(), offsets)
            return self._passes(norm, offsets, text_feat, choice, eps, postprocess)

    def _passes(self, norm, offsets, text_feat, choice, eps, postprocess=True):
        D, B, _ = choice.shape
        text_cm = text_feat.float().t().contiguous()
        step = max(1, ROWS_PER_PASS // B)
        out = [self._rows(norm, offsets, text_cm, choice[d:d + step].contiguous(), eps[d:d + step].float().contiguous(),
                          postprocess) for d in range(0, D, step)]
        return out[0] if len(out) == 1 else torch.cat(out, dim=0)

    def forward(self, batch_dict):
        """The reference's eval-mode forward: batch_dict['points'] [B,3,K] (normalised, sampled), ['text_feat'] [B,512] ->
        the box [B,9].  eps from batch_dict['eps'] [B,latent] when present, else torch.randn with
        batch_dict.get('generator')."""
        self._check_mode("Generator.forward")
        x, text_feat = batch_dict["points"], batch_dict["text_feat"]
        self._check_cuda("Generator.forward", points=x, text_feat=text_feat)
        if x.dim() != 3 or x.shape[1] != 3 or x.shape[0] < 1 or x.shape[2] < 1:
            raise ValueError(f"Generator.forward: `points` must be [B,3,K], got {tuple(x.shape)}")
        B, _, K = x.shape
        dev = x.device
        eps = batch_dict.get("eps")
        if eps is None:
            gen = batch_dict.get("generator")
            gdev = gen.device if gen is not None else dev
            eps = torch.randn((B, self.latent_dim), generator=gen, device=gdev, dtype=torch.float32)
        eps = eps.to(dev).float().reshape(1, B, self.latent_dim)
        with torch.cuda.device(dev), torch.no_grad():
            norm = x.float().permute(0, 2, 1).reshape(B * K, 3).contiguous()
            offsets = torch.arange(B + 1, device=dev, dtype=torch.int32) * K
            choice = torch.arange(K, device=dev, dtype=torch.int32).reshape(1, 1, K).expand(1, B, K).contiguous()
            self.box_pred = self._passes(norm, offsets, text_feat, choice, eps)[0]
        return self.box_pred

    def load_params_from_file(self, filename, logger=None, to_cpu=False):
        import os

        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        state = torch.load(filename, map_location="cpu", weights_only=False)["model_state"]
        self.load_state_dict(state)

