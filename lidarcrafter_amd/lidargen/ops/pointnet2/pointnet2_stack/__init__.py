"""Mirror of the reference's `lidargen/ops/pointnet2/pointnet2_stack`: the ragged-batch (stacked) set-abstraction
operators on the HIP kernels of csrc/pointnet2_stack.hip -- ball query, grouping, stacked farthest
point sampling, three-NN, interpolation, voxel query, `StackSAModuleMSG`, `StackPointnetFPModule`,
`NeighborVoxelSAModuleMSG`.  The vector-pool family is not built and says so by name."""
