"""Temporal metrics of generated 4-D sequences (the reference's lidargen/metrics/temporal.py):

  TTCE  translation error of a point-to-point ICP registration between frames 3 and 4 apart against the ego poses;
  TCD   chamfer distance between frames 1 to 4 apart in world coordinates.

The reference registers with Open3D (registration_icp, identity start, TransformationEstimationPointToPoint, default
criteria) on a thread pool; here every pair of a sequence goes to the device in one ops.icp_point_to_point call
(csrc/icp.hip, DESIGN.md section 5p -- Open3D's semantics restated from its sources, it is not a dependency).  TCD is
ops.chamfer3d on the float32 world points, the kernel the reference's chamfer_3DDist maps to.  natsort and pyquaternion are
replaced by the few lines they amount to here.

Names, arguments, defaults and printed lines are the reference's; `num_threads` is accepted and ignored (there is no
thread pool to size).  calculate_TCD prints the reference's own "TTCE:" label -- kept, scripts parse these lines.

python -m lidargen.metrics.temporal --method_name NAME [--metric ttce|tcd] [--infos PKL] [--results_root DIR]
"""
import argparse
import os
import pickle
import re
from collections import defaultdict

import numpy as np
import torch

from lidarcrafter_amd import ops

_INFOS = "../data/infos/nuscenes_infos_val.pkl"
_RESULTS = "../generated_results"


def natural_sorted(names):
    """natsort.natsorted for file names: runs of digits compare as integers (frame_9 before frame_10)."""
    def key(s):
        return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", s) if t != ""]

    return sorted(names, key=key)


def quaternion_rotation_matrix(q):
    """(w, x, y, z), normalised first (pyquaternion's Quaternion(q).rotation_matrix)."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _token(frame_filename):
    # the reference's rule, literally: str.strip removes CHARACTERS of '.txt' from both ends, not the suffix
    return frame_filename.split('_')[-1].strip('.txt')


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("lidargen.metrics.temporal: the registration and the chamfer distance run on the GPU only")
    return torch.device("cuda")


def _icp_batch(clouds, pairs, threshold):
    """clouds: list of [n,3] float64 arrays, pairs: list of (source, target) -> [P,4,4] float64 array, identity start."""
    sizes = [len(c) for c in clouds]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    out = np.tile(np.eye(4), (len(pairs), 1, 1))
    if not pairs or offsets[-1] == 0:
        return out
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds, axis=0), dtype=np.float64)).to(_device())
    T, _, _, _ = ops.icp_point_to_point(pts, torch.from_numpy(offsets), torch.tensor(pairs, dtype=torch.int64),
                                        float(threshold))
    return T.cpu().numpy()


def _chamfer_mean(pts_a, pts_b):
    """(dist1.mean() + dist2.mean()) / 2 of the float32 chamfer kernel (compute_pairwise_cd_batch + the caller's mean)."""
    dev = _device()
    a = torch.from_numpy(np.ascontiguousarray(pts_a)).to(dev).unsqueeze(0).float()
    b = torch.from_numpy(np.ascontiguousarray(pts_b)).to(dev).unsqueeze(0).float()
    d1, d2, _, _ = ops.chamfer3d(a, b)
    return ((d1.mean() + d2.mean()) / 2).item()


def estimate_transform_icp(pts_source, pts_target, threshold=1.0):
    """-> (transformation [4,4], rotation [3,3], translation [3]) as numpy float64."""
    T = _icp_batch([np.asarray(pts_source, dtype=np.float64).reshape(-1, 3),
                    np.asarray(pts_target, dtype=np.float64).reshape(-1, 3)], [(0, 1)], threshold)[0]
    return T, T[:3, :3], T[:3, 3]


def load_points(frame_filepath, data_infos, to_global=False):
    info = data_infos[_token(os.path.basename(frame_filepath))]
    points = np.loadtxt(frame_filepath)[:, :3]
    points = points[np.linalg.norm(points, axis=1) > 0.2]   # drop the returns at the sensor itself
    if not to_global:
        return points
    lidar2ego = quaternion_rotation_matrix(info['lidar2ego_rotation'])
    ego2global = quaternion_rotation_matrix(info['ego2global_rotation'])
    R = ego2global @ lidar2ego
    T = np.asarray(info['ego2global_translation']) + ego2global @ np.asarray(info['lidar2ego_translation'])
    return (R @ points.T).T + T


def get_gt_transformation(source_frame_filename, target_frame_filename, data_infos):
    """-> (R [3,3], t [3]): source lidar coordinates -> target lidar coordinates from the four pose fields of the two
    frames (the reference's row-vector algebra; its inv(.).T of a rotation matrix is the matrix itself)."""
    src, tgt = data_infos[_token(source_frame_filename)], data_infos[_token(target_frame_filename)]
    Ls, Es = quaternion_rotation_matrix(src['lidar2ego_rotation']), quaternion_rotation_matrix(src['ego2global_rotation'])
    Lt, Et = quaternion_rotation_matrix(tgt['lidar2ego_rotation']), quaternion_rotation_matrix(tgt['ego2global_rotation'])
    back = Et @ Lt                                      # row vectors: global -> target lidar
    R = (Ls.T @ Es.T) @ back
    t = (np.asarray(src['lidar2ego_translation']) @ Es.T + np.asarray(src['ego2global_translation'])) @ back
    t = t - (np.asarray(tgt['ego2global_translation']) @ back + np.asarray(tgt['lidar2ego_translation']) @ Lt)
    return R.T, t


def _frames(seq_path):
    return [os.path.join(seq_path, f) for f in natural_sorted(os.listdir(seq_path))]


def calculate_single_sequence_TTCE(seq_path, data_infos):
    seq_results = defaultdict(list)
    frame_files = _frames(seq_path)
    frame_num = len(frame_files)
    order = [(split, i) for split in [3, 4] for i in range(frame_num - split)]
    if not order:
        return seq_results
    clouds = [load_points(f, data_infos, to_global=False) for f in frame_files]
    T = _icp_batch(clouds, [(i, i + split) for split, i in order], 2.0)
    for (split, i), T_est in zip(order, T):
        _, t_gt = get_gt_transformation(os.path.basename(frame_files[i]), os.path.basename(frame_files[i + split]),
                                        data_infos)
        seq_results[split].append(np.mean(np.abs(T_est[:3, 3] - t_gt)))
    return seq_results


def calculate_single_sequence_TCD(seq_path, data_infos):
    seq_results = defaultdict(list)
    frame_files = _frames(seq_path)
    frame_num = len(frame_files)
    clouds = None
    for split in [1, 2, 3, 4]:
        for i in range(frame_num - split):
            if clouds is None:
                clouds = [load_points(f, data_infos, to_global=True) for f in frame_files]
            seq_results[split].append(_chamfer_mean(clouds[i], clouds[i + split]))
    return seq_results


def _calculate(single, splits, method_name, infos_path, results_root):
    with open(_INFOS if infos_path is None else infos_path, 'rb') as f:
        data_infos = pickle.load(f)
    data_infos_dict = {info['token']: info for info in data_infos['infos']}
    folder = os.path.join(_RESULTS if results_root is None else results_root, method_name, 'temporal_points')
    method_results = defaultdict(list)
    for seq in os.listdir(folder):
        for split, errors in single(os.path.join(folder, seq), data_infos_dict).items():
            method_results[split].extend(errors)
    out = {}
    for split in splits:
        mean_error = np.mean(method_results[split]) if method_results[split] else float('nan')
        print(f'Method: {method_name}, Split: {split}, TTCE: {mean_error:.4f} m')
        out[split] = float(mean_error)
    return out


def calculate_TTCE(method_name, num_threads=None, *, infos_path=None, results_root=None):
    """Prints one line per split (3, 4) and returns {split: mean error in metres}."""
    return _calculate(calculate_single_sequence_TTCE, [3, 4], method_name, infos_path, results_root)


def calculate_TCD(method_name, num_threads=None, *, infos_path=None, results_root=None):
    """Prints one line per split (1 ... 4) -- labelled "TTCE:" like the reference's -- and returns {split: mean}."""
    return _calculate(calculate_single_sequence_TCD, [1, 2, 3, 4], method_name, infos_path, results_root)


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Temporal metrics (TTCE / TCD) of generated sequences.')
    parser.add_argument('--method_name', type=str, default='our', help='Name of the method to evaluate.')
    parser.add_argument('--num_threads', type=int, default=4, help='Accepted for compatibility; unused.')
    parser.add_argument('--metric', choices=('ttce', 'tcd'), default='tcd')
    parser.add_argument('--infos', type=str, default=None, help=f'infos pickle (default {_INFOS})')
    parser.add_argument('--results_root', type=str, default=None, help=f'default {_RESULTS}')
    args = parser.parse_args()
    fn = calculate_TTCE if args.metric == 'ttce' else calculate_TCD
    fn(args.method_name, args.num_threads, infos_path=args.infos, results_root=args.results_root)
