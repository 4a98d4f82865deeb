"""PNN ranker (inner-product PNN; with every field taking part, the interaction of DLRM): every pair of field embeddings multiplied out to its
own feature -- z[(i, j)] = <e_i, e_j>, i > j (ops.dot_interaction_cat_: on the matrix cores, written next to the concat it reads)
-- and handed to the MLP beside the fused embedding concat -> MLP -> sigmoid.
No reference counterpart: the reference has neither PNN nor DLRM (its FM only ever forms the SUM of these products), so the model is
parity-unpinned.  The head, the training step and the optimizers are Deep's (src/model/sort/deep/model.py:24-70).

New optional config block (defaults in brackets):
    pnn_cfg:
      product_feature_names: [user_id, item_id]   # the fields that interact [every sparse / array feature of the model]
      self_interaction: false                     # also <e_i, e_i>  [false]
The fields must share one embedding dim.  Array features take part with their pooled vector.  Dense features, and embedding features that are
not listed, stay plain concat columns and do not interact (a DLRM bottom MLP for the dense features is out of scope).  The model has no
parameters beyond Deep's with a wider first layer: user_input_dim + item_input_dim + P columns, P = F (F - 1) / 2 (F (F + 1) / 2 with
self_interaction)."""
import logging
import os

import torch

from .... import ops
from ...BaseModel.base_model import BaseModel
from ..deep.model import DeepModel


logger = logging.getLogger(__name__)


def fused_pnn_enabled() -> bool:
    """NRX_FUSED_PNN=0: interact with ops.dot_interaction_math over the concat instead of the fused kernels (A/B runs)."""
    return os.environ.get("NRX_FUSED_PNN", "1") != "0"


class PNN(BaseModel):
    def __init__(self, config_path):
        super().__init__(config_path)
        self._load_pnn_cfg()
        self._pnn_warned = False
        self.score_fc = DeepModel(input_dim=self.user_input_dim + self.item_input_dim + self.pnn_pairs, hidden_dims=[128, 128, 128, 64, 1])

    def _load_pnn_cfg(self):
        cfg = self.config.get("pnn_cfg", {}) or {}
        feats = self.user_feature_names | self.item_feature_names
        names = cfg.get("product_feature_names")
        if names is None:
            names = [n for n in feats if n in (self.sparse_feature_names | self.array_feature_names) and n not in self.dense_feature_names]
        names = sorted(set(names))
        for n in names:
            if n not in feats:
                raise ValueError(f"pnn_cfg.product_feature_names: '{n}' is not among the model's user / item features")
            if n in self.dense_feature_names:
                raise ValueError(f"pnn_cfg.product_feature_names: '{n}' is a dense feature (dense features stay concat columns and do not interact)")
            if self._get_emb_feature_name(n) not in self.embedding_tables:
                raise ValueError(f"pnn_cfg.product_feature_names: '{n}' has no embedding table")
        if len(names) < 2:
            raise ValueError(f"pnn_cfg.product_feature_names: an interaction needs at least 2 fields (got {names})")
        dims = {n: self.embedding_tables[self._get_emb_feature_name(n)].embedding_dim for n in names}
        if len(set(dims.values())) != 1:
            raise ValueError(f"pnn_cfg.product_feature_names: the fields must share one embedding dim, got {dims} -- list the features of one "
                             "dim, or give them one embeddings.embedding_size")
        self_i = bool(cfg.get("self_interaction", False))
        self.pnn_cfg = dict(product_feature_names=names, self_interaction=self_i)
        self.pnn_dim = next(iter(dims.values()))
        self.pnn_pairs = ops.dot_interaction_pairs(len(names), self_i)

    def get_inp_embedding(self, batch):
        cfg = self.pnn_cfg
        feats = self.user_feature_names | self.item_feature_names
        plan, _, dims, names = self._plan(batch, feats, False, ())
        missing = [n for n in cfg["product_feature_names"] if n not in names]
        if missing:
            raise ValueError(f"pnn_cfg.product_feature_names: {missing} missing from the batch")
        width, D, P, self_i = plan.out_width, self.pnn_dim, self.pnn_pairs, cfg["self_interaction"]
        offs = tuple(sum(dims[:names.index(n)]) for n in cfg["product_feature_names"])
        # fused: ONE embedding launch writes the concat into the wide buffer, ONE interaction launch writes the pairs next to it.  The
        # kernels read 16-byte aligned field rows: a 1-column dense feature sorted in front of a field takes that away (-> the torch form)
        aligned = all(o % 4 == 0 for o in offs)
        if not aligned and fused_pnn_enabled() and ops.dot_interaction_supported(len(offs), D) and not self._pnn_warned:
            self._pnn_warned = True
            logger.warning("PNN: the product fields start at columns %s of the concat, not all multiples of 4 (a dense feature sorts in front of "
                           "one): the fused interaction needs 16-byte aligned fields, so this model runs ops.dot_interaction_math + torch.cat",
                           list(offs))
        if aligned and fused_pnn_enabled() and ops.dot_interaction_supported(len(offs), D):
            ld = (width + P + 3) // 4 * 4
            buf, _, _, _, _ = self._embed(batch, feats, out_ld=ld)
            buf = ops.dot_interaction_cat_(buf, width, offs, D, self_i)
            return buf if ld == width + P else buf[:, :width + P]          # (the pad columns are never written and never read)
        concat, _, _, _, _ = self._embed(batch, feats)
        return torch.cat([concat, ops.dot_interaction_math(concat, offs, D, self_i)], dim=1)

    def forward(self, x):
        return self.score_fc(self.get_inp_embedding(x))

    def training_step(self, batch, batch_idx):
        return self._ranking_training_step(batch)

    def configure_optimizers(self):
        return self._ranking_optimizers()

    @torch.no_grad()
    def inference(self, batch):
        return self.score_fc(self.get_inp_embedding(batch))
