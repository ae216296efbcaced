"""Mirror of the reference's `lidargen/ops/pointnet2`: the batch variant's farthest point sampling (csrc/pointmlp.hip) and
the stacked variant `pointnet2_stack` (csrc/pointnet2_stack.hip) without its vector-pool family."""
