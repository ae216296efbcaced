"""Mirror of the reference's `lidargen/ops/pointnet2`: the batch variant's farthest point sampling (csrc/pointmlp.hip)."""
