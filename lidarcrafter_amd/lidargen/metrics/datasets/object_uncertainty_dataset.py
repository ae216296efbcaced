"""Dataset of the RGF object metric -- mirror of the reference's `lidargen/metrics/datasets/object_uncertainty_dataset.py`
(`Object_Uncertainty_Dataset` in its eval split) for what `fg_object.compute_rgf_fold` reads.  All numpy.

Unlike the reference, which re-reads and re-subsamples every object file once per draw and takes its 512 indices from the
global numpy state, an object is read once, stays ragged (all of its points), and the indices of all draws come from an
explicit `np.random.Generator` (`choice`).  The centring and scaling of the points is left to the device
(ops_glenet.segment_center); the gt box is normalised here, with the same mean definition (a float64 sum rounded once)."""
import os
import pickle

import numpy as np

POINT_ANCHOR_SIZE = (3.9, 1.6, 1.56)
KEEP_NUM = 512


def kfold_indices(n, n_splits=10, seed=42):
    """[(train_idx, val_idx)] of sklearn's KFold(n_splits, shuffle=True, random_state=seed).split(np.arange(n)), restated:
    the indices are shuffled by RandomState(seed), the first n % n_splits folds take n // n_splits + 1 of them, and both
    halves are returned in ascending order (sklearn selects them with a boolean mask)."""
    n, n_splits = int(n), int(n_splits)
    if n_splits < 2 or n < n_splits:
        raise ValueError(f"kfold_indices: {n_splits} folds of {n} samples")
    indices = np.arange(n)
    np.random.RandomState(seed).shuffle(indices)
    sizes = np.full(n_splits, n // n_splits, dtype=int)
    sizes[:n % n_splits] += 1
    out, start = [], 0
    for size in sizes:
        mask = np.zeros(n, dtype=bool)
        mask[indices[start:start + size]] = True
        out.append((np.nonzero(~mask)[0], np.nonzero(mask)[0]))
        start += size
    return out


def object_mean(points):
    """float32 [3]: the mean of the object's points as ops_glenet.segment_center forms it, a float64 sum rounded once."""
    return np.asarray(points, np.float32)[:, :3].mean(axis=0, dtype=np.float64).astype(np.float32)


def normalise_gt_box(box3d_lidar, mean, anchor=POINT_ANCHOR_SIZE):
    """float32 [7]: the reference's eval-split `gt_boxes` (box3d_lidar_dim7): the centre as minus the points' mean over
    (diagonal, diagonal, dza), the sizes as log(size / anchor), the heading unchanged."""
    dxa, dya, dza = anchor
    diagonal = np.sqrt(dxa ** 2 + dya ** 2)
    box = np.array(box3d_lidar, dtype=np.float64)[:7].copy()
    x_mean, y_mean, z_mean = (np.float32(v) for v in mean)
    box[0] = (-x_mean) / diagonal
    box[1] = (-y_mean) / diagonal
    box[2] = (-z_mean) / dza
    box[3] = np.log(box[3] / dxa)
    box[4] = np.log(box[4] / dya)
    box[5] = np.log(box[5] / dza)
    return box.astype(np.float32)


class NuscObjUncertainty:
    def __init__(self, infos, text_feat, fold_idx=None, class_names=("car", "truck", "bus"), data_root="",
                 point_columns=4, generator=None, n_splits=10, seed=42):
        """infos: the list of object infos ('path' or 'points', 'name', 'box3d_lidar', 'num_points_in_gt'), a dict class ->
        list (the generated objects' pkl form, flattened over `class_names` in that order) or the path of such a pickle.
        text_feat: {class name: [1,512] or [512]} (the reference's obj_text_feat.pkl) or its path.  fold_idx: the eval half of
        that fold of kfold_indices(len(infos), n_splits, seed); None keeps every object.  generator: np.random.Generator of
        `choice` (default np.random.default_rng(0))."""
        if isinstance(infos, (str, os.PathLike)):
            with open(infos, "rb") as f:
                infos = pickle.load(f)
        if isinstance(infos, dict):
            infos = [v for name in infos if name in class_names for v in infos[name]]
        else:
            infos = [x for x in infos if x["name"] in class_names]
        if isinstance(text_feat, (str, os.PathLike)):
            with open(text_feat, "rb") as f:
                text_feat = pickle.load(f)
        self.text_feat = {k: np.asarray(v, np.float32).reshape(-1, 512)[0] for k, v in text_feat.items()}
        self.class_names = list(class_names)
        self.data_root = data_root
        self.point_columns = point_columns
        self.generator = np.random.default_rng(0) if generator is None else generator
        if fold_idx is None:
            self.frame_ids = np.arange(len(infos))
        else:
            self.frame_ids = kfold_indices(len(infos), n_splits, seed)[fold_idx][1]
        self.infos = [infos[i] for i in self.frame_ids]

    def __len__(self):
        return len(self.infos)

    def points_of(self, info):
        if "points" in info:
            return np.ascontiguousarray(np.asarray(info["points"], np.float32)[:, :3])
        path = os.path.join(self.data_root, info["path"]) if self.data_root else info["path"]
        return np.ascontiguousarray(np.fromfile(path, dtype=np.float32).reshape(-1, self.point_columns)[:, :3])

    def __getitem__(self, index):
        """{'points' float32 [n,3] (raw, ragged), 'gt_boxes' float32 [7] (normalised), 'text_feat' [512],
        'num_points_in_gt', 'key'} -- key '<frame>_<gt>' with both the object's index in the fold's source list, as the
        reference forms it."""
        info = self.infos[index]
        points = self.points_of(info)
        if points.shape[0] == 0:
            raise ValueError(f"NuscObjUncertainty: object {index} has no points")
        fid = int(self.frame_ids[index])
        return {"points": points, "gt_boxes": normalise_gt_box(info["box3d_lidar"], object_mean(points)),
                "text_feat": self.text_feat[info["name"]], "num_points_in_gt": info["num_points_in_gt"],
                "key": f"{fid}_{fid}"}

    def batches(self, batch_size):
        """Ragged batches: {'points' [total,3], 'offsets' int32 [B+1], 'gt_boxes' [B,7], 'text_feat' [B,512],
        'num_points_in_gt' [B], 'key' [B]}."""
        for start in range(0, len(self), batch_size):
            items = [self[i] for i in range(start, min(start + batch_size, len(self)))]
            counts = [it["points"].shape[0] for it in items]
            yield {"points": np.concatenate([it["points"] for it in items], axis=0),
                   "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
                   "gt_boxes": np.stack([it["gt_boxes"] for it in items]),
                   "text_feat": np.stack([it["text_feat"] for it in items]),
                   "num_points_in_gt": [it["num_points_in_gt"] for it in items],
                   "key": [it["key"] for it in items]}

    def choice(self, counts, draws, keep_num=KEEP_NUM):
        """int32 [draws, B, keep_num]: per draw and object `keep_num` indices into the object's own rows, with replacement
        (the reference's np.random.choice(n, 512, replace=True)), from the dataset's generator."""
        counts = np.asarray(counts, np.int64).reshape(1, -1, 1)
        u = self.generator.random((draws, counts.shape[1], keep_num))
        return np.minimum((u * counts).astype(np.int64), counts - 1).astype(np.int32)
