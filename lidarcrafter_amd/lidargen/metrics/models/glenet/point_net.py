"""Mirror of the reference's `lidargen/metrics/models/glenet/point_net.py`: `PointNetfeat` and `SimPointNetfeat`, the same
constructor arguments, module names and state-dict keys.  The modules hold parameters; the per-point trunks and the max run
for both at once, per (draw, object) row, in csrc/glenet.hip (ops_glenet.glenet_trunk) under `model.Generator`, and the
`output_sequential` layers on the dense kernel of csrc/pointmlp.hip.  Only the widths the kernel is built for are taken."""
import torch
import torch.nn as nn


def _no_forward(self, *args, **kwargs):
    raise NotImplementedError(f"{type(self).__name__}.forward is not built on its own: the sampler runs as one plan through "
                              "Generator.forward / Generator.sample_boxes")


class PointNetfeat(nn.Module):
    def __init__(self, pts_dim, x=1):
        super().__init__()
        if pts_dim != 3 or int(512 * x) != 512:
            raise NotImplementedError(f"PointNetfeat: pts_dim = {pts_dim}, x = {x} is not built; the trunk kernel is 3 -> 64 -> "
                                      "128 -> 512 (exp20.yaml: INPUT_CHANNELS 3, scale 1)")
        self.output_channel = int(512 * x)
        self.conv1 = torch.nn.Conv1d(pts_dim, int(64 * x), 1)
        self.conv2 = torch.nn.Conv1d(int(64 * x), int(128 * x), 1)
        self.conv3 = torch.nn.Conv1d(int(128 * x), self.output_channel, 1)
        self.bn1 = nn.BatchNorm1d(int(64 * x))
        self.bn2 = nn.BatchNorm1d(int(128 * x))
        self.bn3 = nn.BatchNorm1d(self.output_channel)
        self.output_sequential = nn.Sequential(
            nn.Linear(self.output_channel + 512, 768),
            nn.ReLU(),
            nn.Linear(768, 512),
        )

    forward = _no_forward


class SimPointNetfeat(nn.Module):
    def __init__(self, pts_dim, x=1):
        super().__init__()
        if pts_dim != 3 or int(16 * x) != 8:
            raise NotImplementedError(f"SimPointNetfeat: pts_dim = {pts_dim}, x = {x} is not built; the side trunk is 3 -> 8 -> "
                                      "8 -> 8 (Object_feat_encoder passes x = 0.5)")
        self.output_channel = int(16 * x)
        self.conv1 = torch.nn.Conv1d(pts_dim, int(16 * x), 1)
        self.conv2 = torch.nn.Conv1d(int(16 * x), int(16 * x), 1)
        self.conv3 = torch.nn.Conv1d(int(16 * x), self.output_channel, 1)
        self.bn1 = nn.BatchNorm1d(int(16 * x))
        self.bn2 = nn.BatchNorm1d(int(16 * x))
        self.bn3 = nn.BatchNorm1d(self.output_channel)
        self.output_sequential = nn.Sequential(
            nn.Linear(self.output_channel + 512, 256),
            nn.ReLU(),
            nn.Linear(256, self.output_channel),
        )

    forward = _no_forward
