"""Sparse building blocks -- mirror of the reference's `lidargen/metrics/models/ts/basic_blocks.py`
(`BasicConvolutionBlock` :16-30, `BasicDeconvolutionBlock` :33-47, `ResidualBlock` :50-79) and of the three torchsparse
1.4.0 layers they are made of (`spnn.Conv3d`, `spnn.BatchNorm`, `spnn.ReLU`), with the same module tree and parameter names,
so the reference's checkpoints load: a conv holds `kernel` ([ks^3, inc, outc], or [inc, outc] when ks = 1; no bias), a norm
is `nn.BatchNorm1d` on the rows.

The modules hold parameters only.  They are run by the model that owns them (minkowskinet/model.py), which folds every
BatchNorm into the conv in front of it and launches lidarcrafter_amd.ops_spconv.sparse_conv; calling one on its own
raises."""
import math

import torch
import torch.nn as nn


class Conv3d(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, dilation=1, bias=False, transposed=False):
        super().__init__()
        if bias or dilation != 1:
            raise NotImplementedError("Conv3d: bias and dilation are not built (the extractors use neither)")
        if (kernel_size, stride, transposed) not in ((1, 1, False), (3, 1, False), (2, 2, False), (2, 2, True)):
            raise NotImplementedError(f"Conv3d: kernel_size={kernel_size}, stride={stride}, transposed={transposed} is not "
                                      "built: ks 1 and ks 3 at stride 1, ks 2 at stride 2 and its transpose are")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation, self.transposed = kernel_size, stride, dilation, transposed
        self.kernel_volume = kernel_size ** 3
        shape = (self.kernel_volume, in_channels, out_channels) if self.kernel_volume > 1 else (in_channels, out_channels)
        self.kernel = nn.Parameter(torch.zeros(*shape))
        self.bias = None
        self.reset_parameters()

    def reset_parameters(self):
        std = 1.0 / math.sqrt((self.out_channels if self.transposed else self.in_channels) * self.kernel_volume)
        self.kernel.data.uniform_(-std, std)

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, stride={self.stride}"
                + (", transposed=True" if self.transposed else ""))

    def forward(self, x):
        raise RuntimeError("Conv3d holds parameters only: run the model that owns it (its forward folds the BatchNorm "
                           "behind this layer and launches the HIP kernel)")


BatchNorm = nn.BatchNorm1d


class ReLU(nn.ReLU):
    pass


def _conv_bn(inc, outc, ks, stride, transposed=False):
    return [Conv3d(inc, outc, kernel_size=ks, stride=stride, transposed=transposed), BatchNorm(outc)]


class BasicConvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        self.net = nn.Sequential(*_conv_bn(inc, outc, ks, stride), ReLU(True))


class BasicDeconvolutionBlock(nn.Module):
    def __init__(self, inc, outc, ks=3, stride=1):
        super().__init__()
        self.net = nn.Sequential(*_conv_bn(inc, outc, ks, stride, transposed=True), ReLU(True))


class ResidualBlock(nn.Module):
    """relu(net(x) + downsample(x)); `downsample` is empty (the identity) or a ks = 1 conv and its BatchNorm."""

    def __init__(self, inc, outc, ks=3, stride=1, dilation=1):
        super().__init__()
        if stride != 1:
            raise NotImplementedError("ResidualBlock: stride != 1 is not built")
        self.net = nn.Sequential(*_conv_bn(inc, outc, ks, stride), ReLU(True), *_conv_bn(outc, outc, ks, 1))
        self.downsample = nn.Sequential() if inc == outc else nn.Sequential(*_conv_bn(inc, outc, 1, 1))
        self.ReLU = ReLU(True)
