"""Scene-graph convolution -- module tree and `state_dict` keys of the reference's lidargen/models/unets/graph.py:89-250
(`GraphTripleConv`, `GraphTripleConvNet`) and layers.py:21-38 (`build_mlp`).

The `forward` here is plain torch ops on whatever device the operands live on: it serves the condition model
(`SceneGraph`, once per `sample()` call on tiny operands).  The copy of this network INSIDE the denoiser
(`UNet1DModel.box_graph_cov`, re-run every step) does not go through it: `unet_1d.pack_layout_gen` turns it into skinny
dense layers and a CSR pooling for csrc/layout_gen.hip."""
from __future__ import annotations

import torch
from torch import nn


def build_mlp(dim_list, activation="relu", batch_norm="none", dropout=0, final_nonlinearity=True):
    layers = []
    for i in range(len(dim_list) - 1):
        layers.append(nn.Linear(dim_list[i], dim_list[i + 1]))
        if i != len(dim_list) - 2 or final_nonlinearity:
            if batch_norm == "batch":
                layers.append(nn.BatchNorm1d(dim_list[i + 1]))
            if activation == "relu":
                layers.append(nn.ReLU())
            elif activation == "leakyrelu":
                layers.append(nn.LeakyReLU())
        if dropout > 0:
            layers.append(nn.Dropout(p=dropout))
    return nn.Sequential(*layers)


def _init_weights(module):
    if isinstance(module, nn.Linear):
        nn.init.kaiming_normal_(module.weight)


def edge_csr(s_idx, o_idx, num_objs):
    """CSR of the pooling (host side, once per call): for every object the slots `2 * triple + role` of the triples it
    takes part in -- first as subject (role 0), then as object (role 1), each in ascending triple order, which is the
    order two sequential `scatter_add` calls visit them in.  -> (row_ptr [O+1], slots [2T]) int32 CPU tensors."""
    s = torch.as_tensor(s_idx, dtype=torch.int64).cpu()
    o = torch.as_tensor(o_idx, dtype=torch.int64).cpu()
    T = s.numel()
    if T and (int(min(s.min(), o.min())) < 0 or int(max(s.max(), o.max())) >= num_objs):
        raise ValueError("edge_csr: a triple names an object outside [0, num_objs)")
    owner = torch.cat([s, o])
    slot = torch.cat([torch.arange(T) * 2, torch.arange(T) * 2 + 1])
    order = torch.sort(owner, stable=True).indices
    counts = torch.bincount(owner, minlength=num_objs)
    row_ptr = torch.zeros(num_objs + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(counts, 0)
    return row_ptr.to(torch.int32), slot[order].to(torch.int32)


class GraphTripleConv(nn.Module):
    def __init__(self, input_dim_obj, input_dim_pred, output_dim=None, hidden_dim=512, pooling="avg",
                 mlp_normalization="none", residual=True):
        super().__init__()
        if pooling != "avg":
            raise NotImplementedError(f"GraphTripleConv: pooling={pooling!r} is not built (only 'avg')")
        output_dim = input_dim_obj if output_dim is None else output_dim
        self.input_dim_obj, self.input_dim_pred = input_dim_obj, input_dim_pred
        self.output_dim, self.hidden_dim = output_dim, hidden_dim
        self.residual, self.pooling = residual, pooling
        self.net1 = build_mlp([2 * input_dim_obj + input_dim_pred, hidden_dim, 2 * hidden_dim + input_dim_pred],
                              batch_norm=mlp_normalization)
        self.net1.apply(_init_weights)
        self.net2 = build_mlp([hidden_dim, hidden_dim, output_dim], batch_norm=mlp_normalization)
        self.net2.apply(_init_weights)
        if residual:
            self.linear_projection = nn.Linear(input_dim_obj, output_dim)
            self.linear_projection_pred = nn.Linear(input_dim_pred, input_dim_pred)

    def forward(self, obj_vecs, pred_vecs, edges):
        O, T, H, Dp = obj_vecs.size(0), pred_vecs.size(0), self.hidden_dim, self.input_dim_pred
        s_idx, o_idx = edges[:, 0].contiguous(), edges[:, 1].contiguous()
        t = self.net1(torch.cat([obj_vecs[s_idx], pred_vecs, obj_vecs[o_idx]], dim=1))
        new_s, new_p, new_o = t[:, :H], t[:, H:H + Dp], t[:, H + Dp:]
        pooled = torch.zeros(O, H, dtype=obj_vecs.dtype, device=obj_vecs.device)
        pooled = pooled.index_add(0, s_idx, new_s).index_add(0, o_idx, new_o)
        ones = torch.ones(T, dtype=obj_vecs.dtype, device=obj_vecs.device)
        counts = torch.zeros(O, dtype=obj_vecs.dtype, device=obj_vecs.device)
        counts = counts.index_add(0, s_idx, ones).index_add(0, o_idx, ones).clamp(min=1)
        new_obj = self.net2(pooled / counts.view(-1, 1))
        if self.residual:
            new_obj = new_obj + self.linear_projection(obj_vecs)
            new_p = new_p + self.linear_projection_pred(pred_vecs)
        return new_obj, new_p


class GraphTripleConvNet(nn.Module):
    def __init__(self, input_dim_obj, input_dim_pred, num_layers=2, hidden_dim=512, residual=False, pooling="avg",
                 mlp_normalization="none", output_dim=None):
        super().__init__()
        self.num_layers = num_layers
        self.gconvs = nn.ModuleList()
        kw = dict(input_dim_obj=input_dim_obj, input_dim_pred=input_dim_pred, hidden_dim=hidden_dim, pooling=pooling,
                  residual=residual, mlp_normalization=mlp_normalization)
        for i in range(num_layers):
            last = output_dim is not None and i >= num_layers - 1
            self.gconvs.append(GraphTripleConv(**kw, output_dim=output_dim) if last else GraphTripleConv(**kw))

    def forward(self, obj_vecs, pred_vecs, edges):
        for gconv in self.gconvs:
            obj_vecs, pred_vecs = gconv(obj_vecs, pred_vecs, edges)
        return obj_vecs, pred_vecs
