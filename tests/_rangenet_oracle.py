"""CPU restatement of RangeNet++ for the tests: both module trees' forwards from their state dicts on
torch.nn.functional.conv2d / conv_transpose2d / batch_norm at a chosen dtype (BatchNorm is NOT folded here), the single
layer with the product's epilogue, the fold's float64 formula, the three aggregations and the Frechet distance of the
evaluator.  Nothing here touches the product's kernels."""
import math
import random

import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = {21: [1, 1, 2, 2, 1], 53: [1, 2, 8, 8, 4]}
EPS = 1e-5
TOL_CONV = 2e-6
"""Per-sample relative L2 bound of the HIP path against float64.  The kernel is an exact-fp32 fma chain of at most 144
terms per chunk plus at most 64 chunk additions: per layer its error is that of any float32 convolution, about
eps_32 = 6e-8 times a small factor.  The float32 CPU oracle of the whole 53-layer network measures 3e-7 against
float64 on the decoder map; a float32 implementation with another summation order may differ from it by a few times that.
2e-6 = 32 eps_32 is about 6 x the float32 oracle's own error; a wrong tap, pad or fold shows as 1e-2 or more."""

CONFIG = {"backbone": {"input_depth": {"range": True, "xyz": True, "remission": False}, "dropout": 0.01, "bn_d": 0.01,
                       "OS": 32, "extra": {"layers": 53}},
          "decoder": {"dropout": 0.01, "bn_d": 0.01}}


def config(layers=53, range_=True, xyz=True, remission=False, OS=32):
    c = {"backbone": dict(CONFIG["backbone"]), "decoder": dict(CONFIG["decoder"])}
    c["backbone"]["input_depth"] = {"range": range_, "xyz": xyz, "remission": remission}
    c["backbone"]["extra"] = {"layers": layers}
    c["backbone"]["OS"] = OS
    return c


def out_width(mode, W):
    return (W - 1) // 2 + 1 if mode == 2 else (2 * W if mode == 3 else W)


def raw_conv(x, w, mode):
    if mode == 0:
        return F.conv2d(x, w)
    if mode == 1:
        return F.conv2d(x, w, padding=1)
    if mode == 2:
        return F.conv2d(x, w, stride=(1, 2), padding=1)
    return F.conv_transpose2d(x, w, stride=(1, 2), padding=(0, 1))


def conv_layer(x, w, bias, mode, act, res1=None, res2=None, dtype=torch.float64):
    """The product's layer: conv + bias, LeakyReLU(0.1), then the addends."""
    y = raw_conv(x.to(dtype), w.to(dtype), mode) + bias.to(dtype).view(1, -1, 1, 1)
    if act:
        y = F.leaky_relu(y, 0.1)
    for r in (res1, res2):
        if r is not None:
            y = y + r.to(dtype)
    return y


def fold64(w, conv_bias, gamma, beta, mean, var, eps, mode):
    """The fold's formula in float64: (w * g / sqrt(var + eps), beta - mean * g / sqrt(var + eps) + conv_bias * g / ...)."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    w64 = w.double() * (s.view(1, -1, 1, 1) if mode == 3 else s.view(-1, 1, 1, 1))
    b = beta.double() - mean.double() * s
    if conv_bias is not None:
        b = b + conv_bias.double() * s
    return w64, b


def _cbl(sd, conv, bn, x, mode, dtype):
    """conv -> eval BatchNorm -> LeakyReLU(0.1) from the keys `conv` and `bn`."""
    y = raw_conv(x, sd[conv + ".weight"].to(dtype), mode)
    if conv + ".bias" in sd:
        y = y + sd[conv + ".bias"].to(dtype).view(1, -1, 1, 1)
    y = F.batch_norm(y, sd[bn + ".running_mean"].to(dtype), sd[bn + ".running_var"].to(dtype), sd[bn + ".weight"].to(dtype),
                     sd[bn + ".bias"].to(dtype), False, 0.0, EPS)
    return F.leaky_relu(y, 0.1)


def _network(sd, x, dtype, layers, names):
    """names(kind, level, block, conv_index) -> (conv key, bn key).  Returns (encoder map, decoder map)."""
    h = _cbl(sd, *names("stem", 0, 0, 0), x, 1, dtype)
    skips = [h]
    for i, n in enumerate(BLOCKS[layers], start=1):
        h = _cbl(sd, *names("enc", i, -1, 0), h, 2, dtype)
        for r in range(n):
            t = _cbl(sd, *names("enc", i, r, 1), h, 0, dtype)
            h = _cbl(sd, *names("enc", i, r, 2), t, 1, dtype) + h
        skips.append(h)
    enc = skips.pop()
    for i in range(5, 0, -1):
        h = _cbl(sd, *names("dec", i, -1, 0), h, 3, dtype)
        t = _cbl(sd, *names("dec", i, 0, 1), h, 0, dtype)
        h = (_cbl(sd, *names("dec", i, 0, 2), t, 1, dtype) + h) + skips.pop()
    return enc, h


def _model_names(kind, i, r, c):
    if kind == "stem":
        return "backbone.conv1", "backbone.bn1"
    if kind == "enc":
        base = f"backbone.enc{i}"
        return (f"{base}.conv", f"{base}.bn") if r < 0 else (f"{base}.residual_{r}.conv{c}", f"{base}.residual_{r}.bn{c}")
    base = f"decoder.dec{i}"
    return (f"{base}.upconv", f"{base}.bn") if r < 0 else (f"{base}.residual.conv{c}", f"{base}.residual.bn{c}")


def _extractor_names(kind, i, r, c):
    if kind == "stem":
        return "stem.0", "stem.1"
    base = f"{kind}{i}"
    if r < 0:
        return f"{base}.conv.0", f"{base}.conv.1"
    return f"{base}.residual_blocks.{r}.residual.{c - 1}.0", f"{base}.residual_blocks.{r}.residual.{c - 1}.1"


def input_idxs(cfg):
    d = cfg["backbone"]["input_depth"]
    return ([0] if d["range"] else []) + ([1, 2, 3] if d["xyz"] else []) + ([4] if d["remission"] else [])


def model_forward(sd, cfg, x, dtype=torch.float64):
    """(encoder map, decoder map) of models.rangenet.model.Model from its state dict."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    return _network(sd, x[:, input_idxs(cfg)].to(dtype), dtype, cfg["backbone"]["extra"]["layers"], _model_names)


def extractor_forward(sd, backbone, x, dtype=torch.float64):
    """(decoder map, head logits) of extractor.rangenet.RangeNet from its state dict."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    _, dec = _network(sd, x.to(dtype), dtype, backbone, _extractor_names)
    logits = F.conv2d(dec, sd["head.1.weight"].to(dtype), sd["head.1.bias"].to(dtype), padding=1)
    return dec, logits


def aggregate(y, kind):
    B, C, H, W = y.shape
    if kind == "all":
        return y.mean([2, 3])
    if kind == "sector":
        return y.reshape(B, C, H, 16, W // 16).mean([2, 4]).reshape(B, -1)
    return y.reshape(B, C, 16, H // 16, W).mean([3, 4]).reshape(B, -1)


def subsample(y, k=4096):
    B = y.shape[0]
    n = y[0].numel()
    return y.reshape(B, n)[:, random.Random(0).sample(range(n), k)]


def rel_l2_per_sample(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    B = ref.shape[0]
    e = (got - ref).reshape(B, -1).norm(dim=1) / ref.reshape(B, -1).norm(dim=1)
    return [float(v) for v in e]


def compute_fd(a, b):
    """eval_utils.compute_fd restated: np.mean / np.cov / sqrtm."""
    from scipy import linalg

    mu1, mu2 = np.mean(a, axis=0), np.mean(b, axis=0)
    s1, s2 = np.cov(a, rowvar=False), np.cov(b, rowvar=False)
    root, _ = linalg.sqrtm(s1.dot(s2), disp=False)
    if np.iscomplexobj(root):
        root = root.real
    d = mu1 - mu2
    return float(d.dot(d) + np.trace(s1) + np.trace(s2) - 2 * np.trace(root))


def metre_cloud(seed, n=600):
    """A synthetic sweep in metres: points at 3 .. 40 m over the full azimuth, elevations inside nuScenes' fov."""
    g = np.random.default_rng(seed)
    d = g.uniform(3.0, 40.0, n)
    yaw = g.uniform(-math.pi, math.pi, n)
    pitch = np.radians(g.uniform(-29.0, 9.0, n))
    return np.stack([d * np.cos(pitch) * np.cos(yaw), d * np.cos(pitch) * np.sin(yaw), d * np.sin(pitch)], 1).astype(np.float32)
