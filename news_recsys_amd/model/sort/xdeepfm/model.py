"""xDeepFM ranker (Lian et al., KDD 2018): a Compressed Interaction Network over the field embeddings -- explicit, vector-wise, higher-order
interaction with learned weights; layer k forms X^k[h] = sum_{i, j} W_k[h, i, j] X^{k-1}[i] * X^0[j] (element-wise over the embedding dim) and
contributes its sum over the embedding dim (ops.cin: each layer a GEMM on the matrix cores, read in place from the fused embedding concat, no
[B, Hp, m, D] tensor) -- beside Deep's MLP over the concat:  sigmoid(bias + Linear(sum H_k -> 1, no bias)(cin) + MLP(concat)).
No reference counterpart: the reference has no xDeepFM, so the model is parity-unpinned.  The MLP, the training step and the optimizers are
Deep's (src/model/sort/deep/model.py:24-70).

New optional config block (defaults in brackets):
    xdeepfm_cfg:
      cin_feature_names: [user_id, item_id]   # the fields of X^0 [every sparse / array feature of the model]
      cin_layer_sizes: [32, 32]               # H_1 .. H_T, the feature maps per layer  [[32, 32]]
The fields must share one embedding dim.  Array features take part with their pooled vector.  Dense features, and embedding features that are
not listed, stay plain concat columns the MLP sees and the CIN does not.  The paper's identity form: no bias or activation inside the CIN, no
split_half / direct connections, no first-order term over raw features.
Parameters beyond Deep's: cin.weights.{k} [H_k, H_{k-1}, m] (H_0 = m; uniform in +-sqrt(3 / fan_in), fan_in = H_{k-1} m: the variance Xavier's
rule gives a layer of that fan-in, drawn from torch's generator like every other parameter), cin_out.weight [1, sum H_k], bias [1]."""
import logging
import math
import os

import torch

from .... import ops
from ...BaseModel.base_model import BaseModel
from ..deep.model import DeepModel


logger = logging.getLogger(__name__)


def fused_cin_enabled() -> bool:
    """NRX_FUSED_CIN=0: interact with ops.cin_math over the concat instead of the fused kernels (A/B runs)."""
    return os.environ.get("NRX_FUSED_CIN", "1") != "0"


class CIN(torch.nn.Module):
    """The layer weights W_k [H_k, H_{k-1}, m]."""

    def __init__(self, n_fields, layer_sizes):
        super().__init__()
        self.weights = torch.nn.ParameterList()
        Hp = n_fields
        for H in layer_sizes:
            a = math.sqrt(3.0 / (Hp * n_fields))
            self.weights.append(torch.nn.Parameter(torch.empty(H, Hp, n_fields).uniform_(-a, a)))
            Hp = H


class xDeepFM(BaseModel):
    def __init__(self, config_path):
        super().__init__(config_path)
        self._load_xdeepfm_cfg()
        self._cin_warned = False
        sizes = self.xdeepfm_cfg["cin_layer_sizes"]
        self.cin = CIN(len(self.xdeepfm_cfg["cin_feature_names"]), sizes)
        self.cin_out = torch.nn.Linear(ops.cin_out_width(sizes), 1, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        self.score_fc = DeepModel(input_dim=self.user_input_dim + self.item_input_dim, hidden_dims=[128, 128, 128, 64, 1])

    def _load_xdeepfm_cfg(self):
        cfg = self.config.get("xdeepfm_cfg", {}) or {}
        feats = self.user_feature_names | self.item_feature_names
        names = cfg.get("cin_feature_names")
        if names is None:
            names = [n for n in feats if n in (self.sparse_feature_names | self.array_feature_names) and n not in self.dense_feature_names]
        names = sorted(set(names))
        for n in names:
            if n not in feats:
                raise ValueError(f"xdeepfm_cfg.cin_feature_names: '{n}' is not among the model's user / item features")
            if n in self.dense_feature_names:
                raise ValueError(f"xdeepfm_cfg.cin_feature_names: '{n}' is a dense feature (dense features stay concat columns and do not interact)")
            if self._get_emb_feature_name(n) not in self.embedding_tables:
                raise ValueError(f"xdeepfm_cfg.cin_feature_names: '{n}' has no embedding table")
        if len(names) < 2:
            raise ValueError(f"xdeepfm_cfg.cin_feature_names: an interaction needs at least 2 fields (got {names})")
        dims = {n: self.embedding_tables[self._get_emb_feature_name(n)].embedding_dim for n in names}
        if len(set(dims.values())) != 1:
            raise ValueError(f"xdeepfm_cfg.cin_feature_names: the fields must share one embedding dim, got {dims} -- list the features of one "
                             "dim, or give them one embeddings.embedding_size")
        sizes = cfg.get("cin_layer_sizes", [32, 32])
        if not isinstance(sizes, (list, tuple)) or len(sizes) == 0 or any(isinstance(h, bool) or not isinstance(h, int) or h < 1 for h in sizes):
            raise ValueError(f"xdeepfm_cfg.cin_layer_sizes: a non-empty list of positive feature-map counts H_1 .. H_T (got {sizes!r})")
        self.xdeepfm_cfg = dict(cin_feature_names=names, cin_layer_sizes=[int(h) for h in sizes])
        self.cin_dim = next(iter(dims.values()))

    def _cin_shapes_supported(self, m):
        Hp = m
        for H in self.xdeepfm_cfg["cin_layer_sizes"]:
            if not ops.cin_supported(m, Hp, H, self.cin_dim):
                return False
            Hp = H
        return True

    def _logit(self, batch):
        cfg = self.xdeepfm_cfg
        feats = self.user_feature_names | self.item_feature_names
        plan, _, dims, names = self._plan(batch, feats, False, ())
        missing = [n for n in cfg["cin_feature_names"] if n not in names]
        if missing:
            raise ValueError(f"xdeepfm_cfg.cin_feature_names: {missing} missing from the batch")
        offs = tuple(sum(dims[:names.index(n)]) for n in cfg["cin_feature_names"])
        D, weights = self.cin_dim, list(self.cin.weights)
        # fused: ONE embedding launch writes the concat, the CIN layers read its fields in place.  The kernels read 16-byte aligned field rows:
        # a 1-column dense feature sorted in front of a field takes that away (-> the torch form)
        aligned = all(o % 4 == 0 for o in offs)
        supported = self._cin_shapes_supported(len(offs))
        if fused_cin_enabled() and supported and not aligned and not self._cin_warned:
            self._cin_warned = True
            logger.warning("xDeepFM: the CIN fields start at columns %s of the concat, not all multiples of 4 (a dense feature sorts in front of "
                           "one): the fused interaction needs 16-byte aligned fields, so this model runs ops.cin_math", list(offs))
        concat, _, _, _, _ = self._embed(batch, feats)
        if fused_cin_enabled() and supported and aligned:
            pooled = ops.cin(concat, offs, D, weights)
        else:
            pooled = ops.cin_math(concat, offs, D, weights)
        return self.bias + self.cin_out(pooled) + self.score_fc.network(concat)

    def forward(self, x):
        return torch.sigmoid(self._logit(x))

    def training_step(self, batch, batch_idx):
        return self._ranking_training_step(batch)

    def configure_optimizers(self):
        return self._ranking_optimizers()

    @torch.no_grad()
    def inference(self, batch):
        return torch.sigmoid(self._logit(batch))
