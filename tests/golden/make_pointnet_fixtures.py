"""Golden vectors of the PointNet extractor and of the feature-set distances -> tests/golden/pointnet.npz.

Loads the reference's `lidargen/metrics/extractor/pointnet.py` and `lidargen/metrics/distribution.py` by file path
(both import torch / numpy / scipy only) from the read-only reference tree (`_ref_import.REF`, or argv[1]) and records

  names / shapes / checksums   the state dict of the reference's PointNet1(k=16) after testing.seeded_fill_pointnet(salt=1):
                               key, shape and float64 (sum, sum of squares) per tensor.  The weights themselves (1.6 M
                               values) are not stored: the tests draw them again from the same generator and prove it
                               with the checksums.
  x_<i> / feat_<i> / trans_<i> inputs [B,3,N] (testing.pointnet_clouds: a third of the points zeroed), the reference
                               module's float32 CPU features [B,1808] and its STN's transform [B,3,3]
  dist_a / dist_b / frechet / squared_mmd
                               two seeded feature matrices and the reference's two numbers on them (the MMD after
                               np.random.seed(0), num_subsets=5, max_subset_size=30)

Run from the repository root: python tests/golden/make_pointnet_fixtures.py"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

SALT = 1
CASES = ((2, 37, 11), (3, 1000, 12), (1, 131, 13))     # (B, N, seed)
MMD_ARGS = dict(num_subsets=5, max_subset_size=30)


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from _ref_import import REF

    from lidarcrafter_amd.testing import pointnet_clouds, seeded_fill_pointnet

    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    P = _load(os.path.join(ref, "lidargen", "metrics", "extractor", "pointnet.py"), "_ref_pointnet")
    D = _load(os.path.join(ref, "lidargen", "metrics", "distribution.py"), "_ref_distribution")

    model = seeded_fill_pointnet(P.PointNet1(k=16), SALT).eval()
    sd = model.state_dict()
    out = {
        "names": np.array(list(sd.keys())),
        "shapes": np.array([",".join(str(d) for d in v.shape) for v in sd.values()]),
        "checksums": np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()], np.float64),
        "salt": np.int64(SALT),
        "cases": np.array(CASES, np.int64),
    }
    with torch.no_grad():
        for i, (B, N, seed) in enumerate(CASES):
            x = pointnet_clouds(B, N, seed)
            out[f"x_{i}"] = x.numpy()
            out[f"feat_{i}"] = model(x).numpy()
            out[f"trans_{i}"] = model.feat.stn(x).numpy()
    g = np.random.default_rng(5)
    a = g.normal(0.0, 1.0, (40, 24)) * g.uniform(0.5, 2.0, 24)
    b = g.normal(0.2, 1.1, (50, 24)) * g.uniform(0.5, 2.0, 24)
    out["dist_a"], out["dist_b"] = a, b
    out["frechet"] = np.float64(D.compute_frechet_distance(a, b))
    np.random.seed(0)
    out["squared_mmd"] = np.float64(D.compute_squared_mmd(a, b, **MMD_ARGS))
    path = os.path.join(HERE, "pointnet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(sd), "state tensors; frechet", out["frechet"], "mmd",
          out["squared_mmd"])


if __name__ == "__main__":
    main()
