"""SPVCNN feature extractor of the Frechet Point-Voxel Distance -- mirror of the reference's
`lidargen/metrics/models/spvcnn/model.py` (`Model` :13-179) and of the three point <-> voxel functions of its
`models/ts/utils.py` (`initial_voxelize`, `point_to_voxel`, `voxel_to_point`): the MinkUNet of minkowskinet/model.py (the
same module tree and state-dict names) plus the point branch, `point_transforms.{0,1,2}` = Linear + BatchNorm1d + ReLU, so
`ckpt['state_dict']` of the reference's `model.ckpt` loads.

Inference only.  The convolutions run as in the MinkUNet; the seven exchanges between points and voxels run in
csrc/spvoxel.hip (ops_spvoxel: `query` once per stride, `devoxelize`, `voxelize`); a point transform is the dense form of
the sparse convolution kernel (w [1, Ci, Co], Linear bias and BatchNorm folded in float64 through `_Folded`), its result is
the addend of the devoxelize pass that follows, which writes in place.  The points' float coordinate, the coordinate
levels, hashes, query results and point orders belong to one forward only.  DESIGN.md section 5m."""
from __future__ import annotations

import torch
import torch.nn as nn

from lidarcrafter_amd import ops_spconv as KS
from lidarcrafter_amd import ops_spvoxel as KV

from ...extractor.pointnet import fold_bn
from ..minkowskinet.model import Model as _MinkUNet


def float_coords(coords: torch.Tensor, pres: float, vres: float) -> torch.Tensor:
    """[N, 4] float32 = ((xyz * pres) / vres, batch): the points' coordinate after the reference's initial_voxelize, by
    its own expression on the tensors' device.  In float32 it is not the identity: some c come back as c + 1 ulp."""
    c = coords.float()
    return torch.cat([(c[:, :3] * pres) / vres, c[:, -1].view(-1, 1)], 1).contiguous()


class Model(_MinkUNet):
    def __init__(self, config):
        super().__init__(config)
        cs = self.cs
        self.point_transforms = nn.ModuleList([
            nn.Sequential(nn.Linear(cs[0], cs[4]), nn.BatchNorm1d(cs[4]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[4], cs[6]), nn.BatchNorm1d(cs[6]), nn.ReLU(True)),
            nn.Sequential(nn.Linear(cs[6], cs[8]), nn.BatchNorm1d(cs[8]), nn.ReLU(True))])
        for c in (self.stem[0].in_channels, cs[0], cs[4], cs[6], cs[8]):
            if (c != self.stem[0].in_channels and c not in KV.WIDTHS_DEVOX) or (c != cs[8] and c not in KV.WIDTHS_VOX):
                raise NotImplementedError(f"Model: the point branch's width {c} is not one the point <-> voxel kernels are "
                                          f"built for (devoxelize {KV.WIDTHS_DEVOX}, voxelize {KV.WIDTHS_VOX})")
        self.weight_initialization()

    # ---- folded weights -------------------------------------------------------------------------------------------
    def _pairs(self):
        """The MinkUNet's (conv, norm) pairs, then (Linear, BatchNorm1d) of the three point transforms."""
        return super()._pairs() + [(seq[0], seq[1]) for seq in self.point_transforms]

    def _fold_pair(self, layer, bn):
        if isinstance(layer, nn.Linear):                     # w [1, Ci, Co] = (W^T s), b = (bias - mean) s + beta
            w, b = fold_bn(layer.weight, layer.bias, bn)
            return w.t().contiguous()[None], b
        return super()._fold_pair(layer, bn)

    # ---- forward --------------------------------------------------------------------------------------------------
    def forward(self, feats: torch.Tensor, coords: torch.Tensor, return_logits=False, return_final_logits=True):
        """feats [N, input_dims] float32 and coords [N, 4] = (x, y, z, batch) of the collated batch, on the GPU ->
        {'logits' [N, cs[8]] per input point in input order, 'coords' [N, 3] (the points' float coordinate, as the
        reference returns it), 'batch_indices' [N]} (the reference's `return_final_logits=True`); `return_logits=True`:
        the bottleneck voxels' features after the second exchange and their batch indices."""
        self._check_inputs(feats, coords, return_logits, return_final_logits)
        cs, dev = self.cs, feats.device
        with torch.cuda.device(dev), torch.no_grad():
            feats = feats.float().contiguous()
            coords = coords.to(torch.int32).contiguous()
            top = coords.max(dim=0).values.tolist()          # one read: the limits are checked on the host
            if int(coords.min().item()) < 0:
                raise ValueError("Model: negative coordinates (pcd2voxel subtracts the minimum)")
            conv, block = self._layer_ops()
            # initial_voxelize: the level-0 voxels are the unique floors of the float coordinate
            pts = float_coords(coords, self.pres, self.vres)
            cells = torch.floor(pts).to(torch.int32)
            vox = KS.unpack_keys(torch.unique(KS.pack_keys(cells), sorted=True))
            L = KS.CoordLevels(vox, n_batch=top[3] + 1)
            maps = {}

            def at(lvl):
                """(idx, w, perm, offsets) of the stride of level `lvl`: built once per forward."""
                if lvl not in maps:
                    idx, w = KV.query(pts, 1 << lvl, L.table(lvl), L.rows(lvl))
                    maps[lvl] = (idx, w) + KV.voxel_order(idx[:, 0].contiguous(), L.rows(lvl))
                return maps[lvl]

            def to_points(x, lvl, addend=None):
                idx, w, _, _ = at(lvl)
                return KV.devoxelize(x, idx, w, addend=addend, out=addend)

            def to_voxels(f, lvl):
                _, _, perm, offsets = at(lvl)
                return KV.voxelize(f, perm, offsets)

            def transform(i, f):
                return conv(self.point_transforms[i][0], f, None, True)

            cat = self._cat_buffers(L, dev)
            same0 = L.same(0)
            x = conv(self.stem[0], to_voxels(feats, 0), same0, True)
            x0 = conv(self.stem[3], x, same0, True, out=cat[4], col=cs[8])
            z0 = to_points(x0, 0)
            x4 = self._stages(to_voxels(z0, 0), L, cat, conv, block)
            z1 = to_points(x4, 4, addend=transform(0, z0))
            y = to_voxels(z1, 4)
            if return_logits:
                return {"logits": y, "batch_indices": L.coords[4][:, 3]}
            y = self._up(1, y, L, cat, conv, block)
            y = self._up(2, y, L, cat, conv, block)
            z2 = to_points(y, 2, addend=transform(1, z1))
            y = self._up(3, to_voxels(z2, 2), L, cat, conv, block)
            y = self._up(4, y, L, cat, conv, block)
            z3 = to_points(y, 0, addend=transform(2, z2))
        return {"logits": z3, "coords": pts[:, :3], "batch_indices": coords[:, 3].long()}
