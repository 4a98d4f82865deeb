"""DIN ranker: the click history pooled by target attention -- the candidate's own embedding is the query, the history rows are keys and
values (ops.din_pool: fused into the gather) -- next to the fused embedding concat of every other feature -> MLP -> sigmoid.
No reference counterpart: the reference's rankers see the history through array_feature_pooling's masked mean, the same user vector whatever
candidate is scored.  The head, the training step and the optimizers are Deep's (src/model/sort/deep/model.py:24-70).

New optional config block (defaults in brackets):
    din_cfg:
      history_feature_names: [user_history]   # array features pooled by target attention [every array feature of the model whose table a
                                              #   single-valued feature of the model owns]
      query_feature: item_id                  # [the single-valued feature that owns the histories' table]
      scale: null                             # [dim ** -0.5]
Array features not listed keep the masked mean.  Query and keys live in one space -- the shipped configs share the history's table with item_id
(share_emb_table_features) -- so there is no projection and the model has no parameters beyond Deep's."""
import os

import torch

from .... import ops
from ...BaseModel.base_model import BaseModel
from ..deep.model import DeepModel


def fused_din_enabled() -> bool:
    """NRX_FUSED_DIN=0: pool with ops.din_pool_math over get_feature_embedding instead of the fused kernels (A/B runs)."""
    return os.environ.get("NRX_FUSED_DIN", "1") != "0"


class DIN(BaseModel):
    def __init__(self, config_path):
        super().__init__(config_path)
        self._load_din_cfg()
        self.score_fc = DeepModel(input_dim=self.user_input_dim + self.item_input_dim, hidden_dims=[128, 128, 128, 64, 1])

    def _load_din_cfg(self):
        cfg = self.config.get("din_cfg", {}) or {}
        feats = self.user_feature_names | self.item_feature_names
        single = (self.sparse_feature_names - self.array_feature_names) & feats
        names = cfg.get("history_feature_names")
        if names is None:
            names = [n for n in sorted(self.array_feature_names & feats) if self._get_emb_feature_name(n) in single]
        names = sorted(names)
        if not names:
            raise ValueError("din_cfg.history_feature_names: no array feature to pool (none is listed, and no array feature of the model shares "
                             "its table with a single-valued feature)")
        for n in names:
            if n not in self.array_feature_names:
                raise ValueError(f"din_cfg.history_feature_names: '{n}' is not an array feature (features.array_feature_names)")
            if n not in feats:
                raise ValueError(f"din_cfg.history_feature_names: '{n}' is not among the model's user / item features")
            if self._get_emb_feature_name(n) not in self.embedding_tables:
                raise ValueError(f"din_cfg.history_feature_names: '{n}' has no embedding table")
        query = cfg.get("query_feature")
        if query is None:
            owners = {self._get_emb_feature_name(n) for n in names}
            if len(owners) != 1 or next(iter(owners)) not in single:
                raise ValueError(f"din_cfg.query_feature: set it -- no single-valued feature of the model owns the table(s) of {names} ({sorted(owners)})")
            query = next(iter(owners))
        if query not in single or query in self.dense_feature_names:
            raise ValueError(f"din_cfg.query_feature: '{query}' is not a single-valued sparse feature of the model")
        if self._get_emb_feature_name(query) not in self.embedding_tables:
            raise ValueError(f"din_cfg.query_feature: '{query}' has no embedding table")
        qd = self.embedding_tables[self._get_emb_feature_name(query)].embedding_dim
        for n in names:
            hd = self.embedding_tables[self._get_emb_feature_name(n)].embedding_dim
            if hd != qd:
                raise ValueError(f"din_cfg: query_feature '{query}' has dim {qd} but history feature '{n}' has dim {hd}: query and keys must "
                                 "share one embedding dim (there is no projection)")
        scale = cfg.get("scale")
        self.din_cfg = dict(history_feature_names=names, query_feature=query, scale=None if scale is None else float(scale))
        self._din_other = frozenset(feats - set(names))

    def _history(self, batch, name):
        """(ids [B, L], mask [B, L] or None) of a history feature; a CSR batch (<name>_offsets) is converted to the padded form."""
        offsets = batch.get(f"{name}_offsets")
        if offsets is not None:
            L = self.array_max_length.get(name)
            if L is None:
                raise ValueError(f"Max length for array feature '{name}' missing in config.")
            return ops.csr_to_padded(batch[name], offsets, int(L))
        return batch[name], batch.get(f"{name}_mask")

    def get_inp_embedding(self, batch):
        cfg = self.din_cfg
        # one fused launch over every other feature; the row stride is padded to 4 floats so that the query's column slice can be read in place
        concat, _, _, dims, names = self._embed(batch, self._din_other, out_ld=-4)
        if concat is None or cfg["query_feature"] not in names:
            raise ValueError(f"din_cfg.query_feature: '{cfg['query_feature']}' is missing from the batch")
        col = sum(dims[:names.index(cfg["query_feature"])])
        query = concat[:, col:col + dims[names.index(cfg["query_feature"])]]
        sg = self.sparse_grad
        if sg in ("fused", "exact"):
            if self._sparse_sink is None:
                self._sparse_sink = ops.SparseGradSink()
            sg = self._sparse_sink if torch.is_grad_enabled() else False
        parts = [concat]
        for n in cfg["history_feature_names"]:
            ids, mask = self._history(batch, n)
            weight = self._table_weight(n)
            if fused_din_enabled() and ops.din_pool_supported(ids.shape[1], weight.shape[1]):
                parts.append(ops.din_pool(weight, ids, query, mask, scale=cfg["scale"], sparse_grad=sg, index_check=self.index_check))
            else:
                parts.append(ops.din_pool_math(None, None, query, mask, scale=cfg["scale"], rows=self.get_feature_embedding(n, ids)))
        return torch.cat(parts, dim=1)

    def forward(self, x):
        return self.score_fc(self.get_inp_embedding(x))

    def training_step(self, batch, batch_idx):
        return self._ranking_training_step(batch)

    def configure_optimizers(self):
        return self._ranking_optimizers()

    @torch.no_grad()
    def inference(self, batch):
        return self.score_fc(self.get_inp_embedding(batch))
