"""`pointnet2_utils.furthest_point_sample` on the HIP kernel of csrc/pointmlp.hip; the other operators of the batch variant
are not built (the stacked variant, `..pointnet2_stack`, has ball query, grouping, three-NN and interpolation)."""
