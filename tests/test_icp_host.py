"""Host side of the temporal metrics (lidargen/metrics/temporal.py) and the CPU restatement of the registration they
rest on (tests/_icp_oracle.py); no GPU: the device calls of the front-end are replaced by stubs where a test reaches them."""
import os
import pickle
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _icp_oracle as O  # noqa: E402


def _info(rng, token):
    q1, q2 = rng.normal(size=4), rng.normal(size=4)   # NOT unit: the front-end normalises like pyquaternion
    return {"token": token, "lidar2ego_rotation": list(q1 * 1.7), "lidar2ego_translation": list(rng.normal(size=3)),
            "ego2global_rotation": list(q2 * 0.4), "ego2global_translation": list(rng.normal(size=3) * 300.0)}


def _pose(info):
    def rot(q):   # scipy takes (x, y, z, w) and normalises
        return Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()

    L, E = rot(info["lidar2ego_rotation"]), rot(info["ego2global_rotation"])
    P = np.eye(4)
    P[:3, :3] = E @ L
    P[:3, 3] = np.asarray(info["ego2global_translation"]) + E @ np.asarray(info["lidar2ego_translation"])
    return P


def test_quaternion_matrix_matches_scipy():
    from lidargen.metrics import temporal as TM

    rng = np.random.default_rng(0)
    for _ in range(8):
        q = rng.normal(size=4) * rng.uniform(0.1, 5.0)
        want = Rotation.from_quat([q[1], q[2], q[3], q[0]]).as_matrix()
        assert np.abs(TM.quaternion_rotation_matrix(q) - want).max() < 1e-12


def test_gt_transformation_is_relative_pose():
    from lidargen.metrics import temporal as TM

    rng = np.random.default_rng(1)
    infos = {"aaa": _info(rng, "aaa"), "bbb": _info(rng, "bbb")}
    R, t = TM.get_gt_transformation("seq_0_aaa.txt", "seq_1_bbb.txt", infos)
    rel = np.linalg.inv(_pose(infos["bbb"])) @ _pose(infos["aaa"])
    # translations of ~300 m enter: 1e-12 absolute is ~15 ulp of the operands
    assert np.abs(R - rel[:3, :3]).max() < 1e-12
    assert np.abs(t - rel[:3, 3]).max() < 1e-12


def test_load_points_filter_token_and_world_transform(tmp_path):
    from lidargen.metrics import temporal as TM

    rng = np.random.default_rng(2)
    # "x7.txt".strip('.txt') == "7": the rule strips CHARACTERS ('x' and 't' too), not the suffix
    infos = {"7": _info(rng, "7")}
    pts = np.array([[0.2, 0.0, 0.0],      # norm exactly 0.2 in float64: dropped, the filter is strict
                    [0.0, 0.25, 0.0],
                    [0.1, 0.1, 0.1],      # 0.173: dropped
                    [3.0, -4.0, 12.0],
                    [0.0, 0.0, np.nextafter(0.2, 1.0)]])
    path = tmp_path / "frame_3_x7.txt"
    np.savetxt(path, np.concatenate([pts, np.full((5, 1), 9.0)], axis=1), fmt="%.17g")   # a 4th column is ignored
    assert np.linalg.norm(pts[0]) == 0.2
    local = TM.load_points(str(path), infos, to_global=False)
    assert local.dtype == np.float64 and np.array_equal(local, pts[[1, 3, 4]])
    world = TM.load_points(str(path), infos, to_global=True)
    P = _pose(infos["7"])
    assert np.abs(world - (pts[[1, 3, 4]] @ P[:3, :3].T + P[:3, 3])).max() < 1e-10   # |t| ~ 300
    with pytest.raises(KeyError):
        TM.load_points(str(tmp_path / "frame_3_x8.txt"), infos)


def test_natural_sort():
    from lidargen.metrics import temporal as TM

    names = ["frame_10_a.txt", "frame_9_b.txt", "frame_1_c.txt", "frame_100_d.txt", "frame_2_e.txt"]
    assert TM.natural_sorted(names) == ["frame_1_c.txt", "frame_2_e.txt", "frame_9_b.txt", "frame_10_a.txt",
                                        "frame_100_d.txt"]
    assert sorted(names).index("frame_10_a.txt") < sorted(names).index("frame_9_b.txt")   # what a plain sort does


def test_oracle_identical_clouds_stop_after_one_iteration():
    src, _, _ = O.scene_pair(300, 300, 5)
    r = O.icp(src, src, 2.0)
    assert r.iterations == 1 and r.fitness == 1.0
    assert r.records[0]['rmse'] == 0.0 and r.inlier_rmse < 1e-13   # the update is the identity up to rounding
    assert np.abs(r.T - np.eye(4)).max() < 1e-14


def test_oracle_far_source_finds_nothing():
    src, _, _ = O.scene_pair(300, 300, 5)
    r = O.icp(src + np.array([500.0, 0.0, 0.0]), src, 2.0)
    assert r.iterations == 1 and r.fitness == 0.0 and r.inlier_rmse == 0.0
    assert np.array_equal(r.T, np.eye(4))
    assert (r.records[-1]["idx"] == -1).all()


def test_oracle_recovers_a_small_rigid_motion():
    """The loop converges to the motion when correspondences are exact: the target is the moved source itself."""
    src, _, _ = O.scene_pair(400, 400, 9)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("zyx", [1.0, 0.3, -0.2], degrees=True).as_matrix()
    T[:3, 3] = [0.05, -0.03, 0.02]
    r = O.icp(src, O.apply_transform(T, src), 2.0, max_iteration=200, relative_fitness=0.0, relative_rmse=1e-14)
    assert np.abs(r.T - T).max() < 1e-9


def test_oracle_brute_force_ties_and_radius():
    tgt = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 9.0, 0.0]])
    idx, d2 = O.nn_brute(src, tgt, 2.0)
    assert idx.tolist() == [0, 0, 0, -1]                 # ties: the smallest index; (0,1,0) -> d2 = 2 three ways
    assert d2[:3].tolist() == [1.0, 0.0, 2.0] and np.isinf(d2[3])
    idx, d2 = O.nn_brute(np.array([[0.0, 5.0, 0.0]]), tgt, 2.0)  # exactly on the radius counts
    assert idx.tolist() == [3] and d2.tolist() == [4.0]


def _write_sequence(root, method, rng, frames=5):
    seq = root / method / "temporal_points" / "scene_0"
    seq.mkdir(parents=True)
    infos = []
    for k in range(frames):
        token = f"{k:02d}ab"
        infos.append(_info(rng, token))
        np.savetxt(seq / f"frame_{k}_{token}.txt", rng.normal(size=(6, 4)) * 5.0)
    pkl = root / "infos.pkl"
    with open(pkl, "wb") as f:
        pickle.dump({"infos": infos}, f)
    return pkl


def test_printed_lines_and_return_values(tmp_path, monkeypatch, capsys):
    """The reference's lines character for character (TCD's carries its "TTCE:" label), {split: mean} returned; the two
    device calls are stubs: the registration answers a fixed translation, the chamfer mean a constant."""
    from lidargen.metrics import temporal as TM

    rng = np.random.default_rng(3)
    pkl = _write_sequence(tmp_path, "mine", rng, frames=5)
    seen = {}

    def fake_icp(clouds, pairs, threshold):
        seen["pairs"], seen["threshold"], seen["n"] = list(pairs), threshold, len(clouds)
        T = np.tile(np.eye(4), (len(pairs), 1, 1))
        T[:, :3, 3] = [1.0, 2.0, 3.0]
        return T

    monkeypatch.setattr(TM, "_icp_batch", fake_icp)
    monkeypatch.setattr(TM, "_chamfer_mean", lambda a, b: 0.125)
    out = TM.calculate_TTCE("mine", 7, infos_path=str(pkl), results_root=str(tmp_path))
    lines = capsys.readouterr().out.splitlines()
    assert seen == {"pairs": [(0, 3), (1, 4), (0, 4)], "threshold": 2.0, "n": 5}   # one call for the whole sequence
    assert sorted(out) == [3, 4]
    infos = {i["token"]: i for i in pickle.load(open(pkl, "rb"))["infos"]}
    names = TM.natural_sorted(os.listdir(tmp_path / "mine" / "temporal_points" / "scene_0"))
    want = {}
    for split, prs in ((3, [(0, 3), (1, 4)]), (4, [(0, 4)])):
        errs = [np.mean(np.abs(np.array([1.0, 2.0, 3.0]) - TM.get_gt_transformation(names[a], names[b], infos)[1]))
                for a, b in prs]
        want[split] = np.mean(errs)
        assert out[split] == pytest.approx(want[split], rel=1e-14)
    assert lines == [f"Method: mine, Split: {s}, TTCE: {want[s]:.4f} m" for s in (3, 4)]
    out = TM.calculate_TCD("mine", infos_path=str(pkl), results_root=str(tmp_path))
    lines = capsys.readouterr().out.splitlines()
    assert out == {1: 0.125, 2: 0.125, 3: 0.125, 4: 0.125}
    assert lines == [f"Method: mine, Split: {s}, TTCE: 0.1250 m" for s in (1, 2, 3, 4)]


def test_short_sequence_gives_nan_lines(tmp_path, monkeypatch, capsys):
    from lidargen.metrics import temporal as TM

    pkl = _write_sequence(tmp_path, "short", np.random.default_rng(4), frames=3)
    monkeypatch.setattr(TM, "_icp_batch", lambda *a: pytest.fail("nothing to register"))
    out = TM.calculate_TTCE("short", infos_path=str(pkl), results_root=str(tmp_path))
    assert np.isnan(out[3]) and np.isnan(out[4])
    assert capsys.readouterr().out.splitlines() == ["Method: short, Split: 3, TTCE: nan m",
                                                    "Method: short, Split: 4, TTCE: nan m"]


def test_ops_refuse_cpu_tensors_and_bad_operands():
    import torch

    from lidarcrafter_amd import ops

    pts = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.nn_radius(pts, [0, 2, 4], [[0, 1]], torch.eye(4, dtype=torch.float64)[None], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.icp_point_to_point(pts, [0, 2, 4], [[0, 1]], 1.0)


def test_entry_points_check_arguments_before_any_launch():
    from lidarcrafter_amd import _lib

    h = _lib.lib()
    p = 4096
    EINVAL, EUNSUP = -1, -2
    assert h.lc_nn_grid_bytes(0, 10) == 0 and h.lc_nn_grid_bytes(70000, 10) == 0 and h.lc_nn_grid_bytes(2, 100) > 0
    assert h.lc_icp_scratch_bytes(0, 10) == 0 and h.lc_icp_scratch_bytes(3, 1000) > 0
    assert h.lc_nn_grid_build(None, p, 1, 10, 10, 1.0, p, None) == EINVAL
    assert h.lc_nn_grid_build(p, p, 1, 10, 10, 0.0, p, None) == EINVAL            # h0
    assert h.lc_nn_grid_build(p, p, 1, 0, 1, 1.0, p, None) == EINVAL              # no points
    assert h.lc_nn_grid_build(p, p, 70000, 10, 10, 1.0, p, None) == EUNSUP        # clouds beyond gridDim.y
    assert h.lc_nn_radius(p, p, 1, 10, p, p, p, 1, 10, -1.0, p, p, None) == EINVAL
    assert h.lc_nn_radius(p, p, 1, 10, p, None, p, 1, 10, 1.0, p, p, None) == EINVAL
    assert h.lc_nn_radius(p, p, 1, 10, p, p, p, 70000, 10, 1.0, p, p, None) == EUNSUP
    assert h.lc_icp_run(p, p, 1, 10, p, p, 1, 10, 1.0, -1, 1e-6, 1e-6, p, p, p, p, p, None) == EINVAL
    assert h.lc_icp_run(p, p, 1, 10, p, p, 0, 10, 1.0, 30, 1e-6, 1e-6, p, p, p, p, p, None) == EINVAL
    assert h.lc_icp_run(p, p, 1, 10, p, p, 1, 10, 1.0, 30, 1e-6, 1e-6, p, p, p, p, None, None) == EINVAL
    assert h.lc_icp_run(p, p, 1, 10, p, p, 70000, 10, 1.0, 30, 1e-6, 1e-6, p, p, p, p, p, None) == EUNSUP


def test_module_runs_as_a_script():
    """`python -m lidargen.metrics.temporal` (the reference's __main__) resolves through the package alias."""
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "lidargen.metrics.temporal", "--help"], cwd=root, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--method_name", "--metric", "--infos", "--results_root", "--num_threads"):
        assert flag in r.stdout
