"""`pointnet2_utils.furthest_point_sample` on the HIP kernel of csrc/pointmlp.hip; the other operators are not built."""
