"""Condition model of the layout generator -- module tree, `state_dict` keys and outputs of the reference's
lidargen/models/unets/scene_graph.py:6-149 (`SceneGraph`): an encoder GCN on the encoder graph, zero rows at the added
nodes, a 64-value change marker per node (zeros for untouched nodes, `np.random.normal` for added / manipulated ones,
drawn in node order from numpy's global generator exactly as the reference draws them), the manipulation GCN on the
decoder graph.

It runs ONCE per `sample()` call on a few hundred rows, in plain torch ops on the device of its operands (the
reference hard-codes `.cuda()`; here every new tensor follows `latent_obj_vecs.device`)."""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .graph import GraphTripleConvNet


class SceneGraph(nn.Module):
    def __init__(self, vocab, embedding_dim=128, batch_size=32, gconv_pooling="avg", gconv_num_layers=5,
                 mlp_normalization="none", separated=False, replace_latent=False, residual=False, use_angles=False,
                 use_clip=True):
        super().__init__()
        gconv_dim = embedding_dim
        hidden = gconv_dim * 4
        self.replace_all_latent = replace_latent
        self.batch_size = batch_size
        self.embedding_dim = gconv_dim
        self.vocab = vocab
        self.use_angles = use_angles
        self.clip = use_clip
        add_dim = 512 if use_clip else 0
        self.edge_list = list(set(vocab["pred_idx_to_name"]))
        self.obj_classes_list = list(set(vocab["object_idx_to_name"]))
        self.classes = dict(zip(sorted(self.obj_classes_list), range(len(self.obj_classes_list))))
        self.classes_r = dict(zip(self.classes.values(), self.classes.keys()))
        num_objs, num_preds = len(self.obj_classes_list), len(self.edge_list)

        self.obj_embeddings_ec = nn.Embedding(num_objs + 1, gconv_dim * 2)
        self.pred_embeddings_ec = nn.Embedding(num_preds, gconv_dim * 2)
        self.obj_embeddings_dc = nn.Embedding(num_objs + 1, gconv_dim * 2)
        self.pred_embeddings_man_dc = nn.Embedding(num_preds, gconv_dim * 2)

        self.out_dim_ini_encoder = gconv_dim * 2 + add_dim
        self.out_dim_manipulator = gconv_dim * 2 + add_dim
        common = dict(input_dim_pred=gconv_dim * 2 + add_dim, hidden_dim=hidden, pooling=gconv_pooling,
                      mlp_normalization=mlp_normalization, residual=residual)
        self.gconv_net_ec = GraphTripleConvNet(input_dim_obj=gconv_dim * 2 + add_dim, num_layers=gconv_num_layers,
                                               output_dim=self.out_dim_ini_encoder, **common)
        self.gconv_net_manipulation = GraphTripleConvNet(
            input_dim_obj=self.out_dim_ini_encoder + gconv_dim + gconv_dim * 2 + add_dim,
            num_layers=min(gconv_num_layers, 5), output_dim=self.out_dim_manipulator, **common)
        self.s_l_separated = separated
        if separated:       # never called by forward; its parameters are part of the checkpoint
            self.gconv_net_ec_rel_l = GraphTripleConvNet(
                input_dim_obj=self.out_dim_manipulator + gconv_dim * 2 + add_dim, num_layers=gconv_num_layers,
                output_dim=self.out_dim_manipulator, **common)

    @staticmethod
    def _edges(triples):
        s, p, o = [x.squeeze(1) for x in triples.chunk(3, dim=1)]
        return p, torch.stack([s, o], dim=1)

    def init_encoder(self, objs, triples, enc_text_feat, enc_rel_feat):
        p, edges = self._edges(triples)
        obj_embed, pred_embed = self.obj_embeddings_ec(objs), self.pred_embeddings_ec(p)
        if self.clip:
            obj_embed = torch.cat([enc_text_feat, obj_embed], dim=1)
            pred_embed = torch.cat([enc_rel_feat, pred_embed], dim=1)
        latent_obj_f, latent_pred_f = self.gconv_net_ec(obj_embed, pred_embed, edges)
        return obj_embed, pred_embed, latent_obj_f, latent_pred_f

    def manipulate(self, latent_f, objs, triples, dec_text_feat, dec_rel_feat):
        p, edges = self._edges(triples)
        obj_embed, pred_embed = self.obj_embeddings_ec(objs), self.pred_embeddings_man_dc(p)
        if self.clip:
            obj_embed = torch.cat([dec_text_feat, obj_embed], dim=1)
            pred_embed = torch.cat([dec_rel_feat, pred_embed], dim=1)
        obj_vecs_, pred_vecs_ = self.gconv_net_manipulation(torch.cat([latent_f, obj_embed], dim=1), pred_embed, edges)
        return obj_vecs_, pred_vecs_, obj_embed, pred_embed

    def forward(self, enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat, dec_objs, dec_triples,
                dec_boxes, encoded_dec_text_feat, encoded_dec_rel_feat, dec_objs_to_scene, dec_triples_to_scene,
                missing_nodes, manipulated_nodes):
        _, _, latent, _ = self.init_encoder(enc_objs, enc_triples, encoded_enc_text_feat, encoded_enc_rel_feat)
        nodes_added = []
        for i in range(len(missing_nodes)):
            ad_id = int(missing_nodes[i]) + i
            nodes_added.append(ad_id)
            zeros = torch.zeros(1, self.out_dim_ini_encoder, dtype=latent.dtype, device=latent.device)
            latent = torch.cat([latent[:ad_id], zeros, latent[ad_id:]], dim=0)
        manipulated = [int(m) for m in manipulated_nodes]
        change = np.zeros((len(latent), self.embedding_dim))
        for i in range(len(latent)):
            if i in nodes_added or i in manipulated:
                change[i] = np.random.normal(0, 1, self.embedding_dim)
        change = torch.from_numpy(change).float().to(device=latent.device, dtype=latent.dtype)
        latent_, _, obj_embed_, _ = self.manipulate(torch.cat([latent, change], dim=1), dec_objs, dec_triples,
                                                    encoded_dec_text_feat, encoded_dec_rel_feat)
        if self.replace_all_latent:
            return latent_, obj_embed_
        for node in sorted(nodes_added + manipulated):
            latent = torch.cat([latent[:node], latent_[node:node + 1], latent[node + 1:]], dim=0)
        return latent, obj_embed_
