"""Golden vectors of the GLENet box sampler and the rotated IoU of the RGF metric -> tests/golden/glenet.npz.

Loads the reference's `lidargen/metrics/models/glenet/{point_net,model,loss_utils}.py` and `eval_utils/eval_utils.py` by path
from the read-only reference tree (`_ref_import.REF`, or argv[1]) as a synthetic package, with stub modules for what they
import and never use on this path (`pcdet.*`: two loss classes without state, `limit_period`; `torchvision`).  Records:

  names / shapes                 the 110 state-dict keys of the reference's Generator(exp20 MODEL block, 3, 1) and their shapes
  obj_points / obj_offsets       6 ragged raw objects of 1, 2, 127, 128, 129 and 700 points; obj_mean their float32 means
  obj_choice [3,6,512]           the index lists of 3 draws (index 0 and n - 1 and repeats in every list)
  obj_class / obj_text / obj_eps the class of every object, the 3 class text vectors, the latent noise [3,6,8]
  ref_mu / ref_logvar / ref_box  the reference float32 module's x_encoder and obj_encoder outputs (row r = d 6 + b) after
                                 testing.seeded_fill_glenet(salt 7) -- weights are not stored, the seed is; ref_box_post the
                                 box after the reference's heading post-process
  gen_g / gen_q [2000,7]         seeded generic pairs (gt sizes around (3.9, 1.6, 1.56), the prediction jittered by 0.3 m /
                                 0.3 rad / 10 % size); gen_cg / gen_cq the reference's corners; gen_pts / gen_cnt / gen_area /
                                 gen_iou its compute_vertex output, polygon area and iou3d
  named / nam_*                  the same for the named cases (json list of names, in row order)

Run from the repository root: python tests/golden/make_glenet_fixtures.py"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SALT = 7
PI = float(np.pi)
G0 = (1.3, -0.7, 0.2, 3.9, 1.6, 1.56, 0.3)
A0 = (0.0, 0.0, 0.0, 3.9, 1.6, 1.56, 0.0)
NAMED = (
    ("axis_aligned_overlap", A0, (1.0, 0.5, 0.2, 3.9, 1.6, 1.56, 0.0)),
    ("cross_90", A0, (0.0, 0.0, 0.0, 3.9, 1.6, 1.56, PI / 2)),
    ("contained", A0, (0.1, 0.05, 0.0, 2.0, 0.8, 1.0, 0.0)),
    ("contained_rotated", A0, (0.1, 0.05, 0.0, 1.5, 0.6, 1.0, 0.5)),
    ("disjoint", A0, (10.0, 10.0, 0.0, 3.9, 1.6, 1.56, 0.3)),
    ("edge_touching", A0, (3.9, 0.0, 0.0, 3.9, 1.6, 1.56, 0.0)),
    ("corner_touching", A0, (3.9, 1.6, 0.0, 3.9, 1.6, 1.56, 0.0)),
    ("z_disjoint", A0, (0.5, 0.2, 5.0, 3.9, 1.6, 1.56, 0.2)),
    ("rot45_common_centre", A0, (0.0, 0.0, 0.0, 3.9, 1.6, 1.56, PI / 4)),
    ("thin_1mm", A0, (0.3, 0.1, 0.0, 3.9, 0.001, 1.56, 0.4)),
    ("identical", G0, G0),
    ("turned_by_pi", A0[:6] + (0.3,), A0[:6] + (0.3 + PI,)),        # the reference scores about 4e-8 here, not 1
    ("negative_size", A0, (0.5, 0.2, 0.0, -3.0, 1.4, 1.5, 0.2)),
    ("centre_at_150m", (150.0, -150.0, 1.0, 4.2, 1.8, 1.6, 0.7), (150.2, -149.9, 1.1, 4.0, 1.7, 1.5, 0.8)),
)


class _Cfg(dict):
    """A mapping with attribute access, what the reference reads its yaml into."""
    __getattr__ = dict.__getitem__


def load_reference(ref):
    """(model module, loss_utils module, eval_utils module) of the reference, as the synthetic package `_ref_glenet`."""
    stubs = {}

    def stub(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        stubs[name] = m
        return m

    class _Loss(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    def limit_period(val, offset=0.5, period=np.pi):
        return val - torch.floor(val / period + offset) * period

    lu = stub("pcdet.utils.loss_utils", WeightedSmoothL1Loss=_Loss, WeightedCrossEntropyLoss=_Loss)
    cu = stub("pcdet.utils.common_utils", limit_period=limit_period)
    bu = stub("pcdet.utils.box_utils")
    stub("pcdet.utils", loss_utils=lu, common_utils=cu, box_utils=bu)
    stub("pcdet.models", load_data_to_gpu=lambda d: None)
    stub("pcdet")
    stub("torchvision.models")
    stub("torchvision", models=stubs["torchvision.models"])
    if importlib.util.find_spec("tqdm") is None:
        stub("tqdm", tqdm=lambda *a, **k: None)
    pkg = types.ModuleType("_ref_glenet")
    pkg.__path__ = [os.path.join(ref, "lidargen", "metrics", "models", "glenet")]
    saved = {k: sys.modules.get(k) for k in stubs}
    sys.modules.update(stubs)
    sys.modules["_ref_glenet"] = pkg
    try:
        model = importlib.import_module("_ref_glenet.model")
        loss_utils = importlib.import_module("_ref_glenet.loss_utils")
        eval_utils = importlib.import_module("_ref_glenet.eval_utils.eval_utils")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return model, loss_utils, eval_utils, limit_period


def reference_iou(L, E, g, q):
    """The reference on paired boxes: corners, compute_vertex, polygon area, iou3d."""
    g, q = torch.from_numpy(g), torch.from_numpy(q)
    gc, qc = torch.clamp(g, -200.0, 200.0), torch.clamp(q, -200.0, 200.0)
    cg = L.rbbox_to_corners()(gc[:, [0, 1, 3, 4, 6]])
    cq = L.rbbox_to_corners()(qc[:, [0, 1, 3, 4, 6]])
    pts, cnt = L.compute_vertex.apply(cg, cq)
    area = L.rinter_area_compute()(cg, cq)
    iou = E.iou3d(g, q)
    return {"cg": cg.numpy(), "cq": cq.numpy(), "pts": pts.numpy(), "cnt": cnt.numpy().astype(np.int32),
            "area": area.numpy(), "iou": iou.numpy()}


def generic_pairs(n, seed):
    r = np.random.default_rng(seed)
    g = np.empty((n, 7), np.float32)
    g[:, 0:2] = r.uniform(-40, 40, (n, 2))
    g[:, 2] = r.uniform(-1, 1, n)
    g[:, 3:6] = np.array([3.9, 1.6, 1.56]) * np.exp(r.normal(0, 0.15, (n, 3)))
    g[:, 6] = r.uniform(-np.pi, np.pi, n)
    q = g.copy()
    q[:, 0:3] += r.normal(0, 0.3, (n, 3)).astype(np.float32)
    q[:, 3:6] *= (1 + r.normal(0, 0.1, (n, 3))).astype(np.float32)
    q[:, 6] += r.normal(0, 0.3, n).astype(np.float32)
    return g, q


def objects(seed):
    import _glenet_oracle as O

    r = np.random.default_rng(seed)
    sizes = O.OBJECT_SIZES
    pts = [(r.uniform(-0.5, 0.5, (n, 3)) * np.array([3.9, 1.6, 1.56]) + np.array([20.0, -8.0, 0.5])).astype(np.float32)
           for n in sizes]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    mean = np.stack([p.mean(axis=0, dtype=np.float64).astype(np.float32) for p in pts])
    D, K = 3, 512
    choice = np.stack([np.stack([r.integers(0, n, K) for n in sizes]) for _ in range(D)]).astype(np.int32)
    for b, n in enumerate(sizes):
        choice[:, b, 0], choice[:, b, 1], choice[:, b, 2], choice[:, b, 3] = 0, n - 1, n - 1, 0
    text = r.normal(0, 1, (3, 512))
    text = (text / np.linalg.norm(text, axis=1, keepdims=True)).astype(np.float32)
    return {"obj_points": np.concatenate(pts), "obj_offsets": off, "obj_mean": mean, "obj_choice": choice,
            "obj_class": np.array([0, 1, 2, 0, 1, 2], np.int32), "obj_text": text,
            "obj_eps": r.normal(0, 1, (D, len(sizes), 8)).astype(np.float32)}


def main():
    import _glenet_oracle as O
    from _ref_import import REF
    from lidarcrafter_amd.testing import seeded_fill_glenet

    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    M, L, E, limit_period = load_reference(ref)
    out = {}

    cfg = _Cfg(O.CFG)
    cfg["LOSS_CONFIG"] = _Cfg(LOSS_WEIGHTS={"latent_weight": 10, "loc_weight": 10.0, "dir_weight": 0.002,
                                            "code_weights": [1.0] * 7})
    net = seeded_fill_glenet(M.Generator(cfg, input_channels=3, scale=1), SALT).eval()
    sd = net.state_dict()
    out["names"] = np.array(json.dumps(list(sd)))
    out["shapes"] = np.array(json.dumps([list(v.shape) for v in sd.values()]))
    assert len(sd) == 110, len(sd)

    out.update(objects(11))
    x, text, eps, _, _ = O.gathered(out)
    with torch.no_grad():
        x_dict = {"x": torch.from_numpy(x), "text_feat": torch.from_numpy(text)}
        _, mu, logvar = net.x_encoder(x_dict)
        z = torch.from_numpy(eps).mul(logvar.mul(0.5).exp()).add(mu)
        box = net.obj_encoder(x_dict, z)
        post = box.clone()
        labels = torch.max(post[:, -2:], dim=-1)[1]
        period = 2 * np.pi / cfg.NUM_DIR_BINS
        rot = limit_period(post[..., 6] - cfg.DIR_OFFSET, cfg.DIR_LIMIT_OFFSET, period)
        post[..., 6] = rot + cfg.DIR_OFFSET + period * labels.to(post.dtype)
    out.update(ref_mu=mu.numpy(), ref_logvar=logvar.numpy(), ref_box=box.numpy(), ref_box_post=post.numpy())

    g, q = generic_pairs(2000, 5)
    out.update(gen_g=g, gen_q=q, **{"gen_" + k: v for k, v in reference_iou(L, E, g, q).items()})
    g = np.array([c[1] for c in NAMED], np.float32)
    q = np.array([c[2] for c in NAMED], np.float32)
    out.update(nam_g=g, nam_q=q, named=np.array(json.dumps([c[0] for c in NAMED])),
               **{"nam_" + k: v for k, v in reference_iou(L, E, g, q).items()})

    path = os.path.join(HERE, "glenet.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", "named iou:",
          dict(zip([c[0] for c in NAMED], out["nam_iou"].tolist())))


if __name__ == "__main__":
    main()
