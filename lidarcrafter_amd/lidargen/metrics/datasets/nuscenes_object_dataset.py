"""Foreground-object dataset of the object scores and CGF -- mirror of the reference's
`lidargen/metrics/datasets/nuscenes_object_dataset.py` (`NuscObject`): the `pkl_path` form (generated objects: a dict
class -> infos, points stored as float32 x 4) and the 'ori' form (the nuScenes infos list, points stored as float32 x 5).
All numpy.  Unlike the reference, which shuffles with the global numpy state, the shuffle takes an explicit generator."""
import os
import pickle

import numpy as np


def rotate_points_along_z(points, angle):
    """points [B,N,3+C], angle [B] -> the points rotated about z (x towards y), float32: points[..., :3] @ [[c, s, 0],
    [-s, c, 0], [0, 0, 1]] as the reference's dataset.utils.rotate_points_along_z forms it (float32 matrix product)."""
    points = np.asarray(points, np.float32)
    angle = np.asarray(angle, np.float32)
    cosa, sina = np.cos(angle), np.sin(angle)
    zeros, ones = np.zeros_like(angle), np.ones_like(angle)
    rot = np.stack([cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones], axis=1).reshape(-1, 3, 3).astype(np.float32)
    return np.concatenate([np.matmul(points[:, :, :3], rot), points[:, :, 3:]], axis=-1)


class NuscObject:
    def __init__(self, num_points=1024, partition="train", class_name=("car", "truck", "bus"), pkl_path=None,
                 data_root=None, info_path=None, generator=None):
        """pkl_path: the generated objects' info dict; None: the 'ori' form, the info list at `info_path` (default
        ../data/infos/nuscenes_object_classification_<partition>.pkl) with point files under `data_root` (default
        ../data/nuscenes).  generator: a numpy Generator for the shuffle (default: np.random.default_rng(0))."""
        self.class_name = list(class_name)
        self.pkl_path = pkl_path
        self.num_points = num_points
        self.partition = partition
        self.data_root = "../data/nuscenes" if data_root is None else data_root
        self.info_path = info_path
        self.generator = np.random.default_rng(0) if generator is None else generator
        self.data_infos = self.load_data(partition)

    def load_data(self, partition):
        if self.pkl_path is not None:
            self.dataset_type = "custom"
            self.data_root = ""
            path = self.pkl_path
        else:
            self.dataset_type = "ori"
            path = self.info_path or f"../data/infos/nuscenes_object_classification_{partition}.pkl"
        if not os.path.isfile(path):
            raise FileNotFoundError(f"NuscObject: no info file at {path}")
        with open(path, "rb") as f:
            infos = pickle.load(f)
        if self.dataset_type == "ori":
            return infos
        out = []
        for key, value in infos.items():
            if key in self.class_name:
                out.extend(value)
        return out

    def load_points(self, fg_path):
        if self.dataset_type == "custom":
            return np.fromfile(fg_path, dtype=np.float32).reshape(-1, 4)[:, :3]
        return np.fromfile(os.path.join(self.data_root, fg_path), dtype=np.float32).reshape(-1, 5)[:, :3]

    def norm_fg_points(self, fg_points, box3d):
        """Rotate by -heading and scale every axis by the box extent into [0, 1] (+ 0.5)."""
        fg_points = rotate_points_along_z(fg_points[np.newaxis, :, :], -np.array([box3d[-1]]))[0]
        fg_points[:, 0] = fg_points[:, 0] / box3d[3] + 0.5
        fg_points[:, 1] = fg_points[:, 1] / box3d[4] + 0.5
        fg_points[:, 2] = fg_points[:, 2] / box3d[5] + 0.5
        return fg_points

    def __getitem__(self, item):
        info = self.data_infos[item]
        fg_points = self.norm_fg_points(self.load_points(info["path"]), info["box3d_lidar"][:7])
        self.generator.shuffle(fg_points)
        if fg_points.shape[0] < self.num_points:
            fg_points = np.pad(fg_points, ((0, self.num_points - fg_points.shape[0]), (0, 0)), mode="constant")
        else:
            fg_points = fg_points[:self.num_points]
        if info["name"] not in self.class_name:
            label = np.array(0)
        else:
            label = np.array(self.class_name.index(info["name"]) + 1)
        return fg_points, label, np.array(info["num_points_in_gt"])

    def __len__(self):
        return len(self.data_infos)
