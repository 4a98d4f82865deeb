"""AFM ranker (Attentional Factorization Machine; Xiao et al., IJCAI 2017): every pair of field embeddings keeps its element-wise product
h_(i,j) = e_i * e_j as a vector, a small attention network scores it, a_(i,j) = w2 . relu(w1 h_(i,j) + b1), the scores are softmax-normalised over
the pairs of the sample and the pair vectors pooled by those weights (ops.afm_pool: the scores a GEMM on the matrix cores, read in place from
the fused embedding concat, no [B, P, D] or [B, P, A] tensor, forward or backward) -- beside Deep's MLP over the concat when
use_deep:  sigmoid(bias + Linear(dim -> 1, no bias)(pooled) [+ MLP(concat)]).
No reference counterpart: the reference has no AFM, so the model is parity-unpinned.  The MLP, the training step and the optimizers are
Deep's (src/model/sort/deep/model.py:24-70).

New optional config block (defaults in brackets):
    afm_cfg:
      afm_feature_names: [user_id, item_id]   # the interacting fields [every sparse / array feature of the model]
      attention_factor: 16                    # A, the hidden units of the attention network  [16]
      use_deep: true                          # add Deep's MLP over the concat to the logit  [true]
The fields must share one embedding dim.  Array features take part with their pooled vector.  Dense features, and embedding features that are
not listed, stay plain concat columns the MLP sees and the interaction does not.  No dropout on the attention weights, no L2 on w1, no
first-order term over raw features, no self pairs.
Parameters beyond Deep's: attention.w1 [A, dim] and attention.w2 [A] (uniform in +-sqrt(3 / fan_in), fan_in = dim and A: the variance Xavier's
rule gives a layer of that fan-in, drawn from torch's generator like every other parameter), attention.b1 [A] (zeros), afm_out.weight [1, dim],
bias [1]; score_fc.* only when use_deep."""
import logging
import math
import os

import torch

from .... import ops
from ...BaseModel.base_model import BaseModel
from ..deep.model import DeepModel


logger = logging.getLogger(__name__)


def fused_afm_enabled() -> bool:
    """NRX_FUSED_AFM=0: pool with ops.afm_pool_math over the concat instead of the fused kernels (A/B runs)."""
    return os.environ.get("NRX_FUSED_AFM", "1") != "0"


class Attention(torch.nn.Module):
    """The attention network's parameters: w1 [A, dim], b1 [A], w2 [A]."""

    def __init__(self, dim, factor):
        super().__init__()
        a1, a2 = math.sqrt(3.0 / dim), math.sqrt(3.0 / factor)
        self.w1 = torch.nn.Parameter(torch.empty(factor, dim).uniform_(-a1, a1))
        self.b1 = torch.nn.Parameter(torch.zeros(factor))
        self.w2 = torch.nn.Parameter(torch.empty(factor).uniform_(-a2, a2))


class AFM(BaseModel):
    def __init__(self, config_path):
        super().__init__(config_path)
        self._load_afm_cfg()
        self._afm_warned = False
        self.attention = Attention(self.afm_dim, self.afm_cfg["attention_factor"])
        self.afm_out = torch.nn.Linear(self.afm_dim, 1, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        if self.afm_cfg["use_deep"]:
            self.score_fc = DeepModel(input_dim=self.user_input_dim + self.item_input_dim, hidden_dims=[128, 128, 128, 64, 1])

    def _load_afm_cfg(self):
        cfg = self.config.get("afm_cfg", {}) or {}
        feats = self.user_feature_names | self.item_feature_names
        names = cfg.get("afm_feature_names")
        if names is None:
            names = [n for n in feats if n in (self.sparse_feature_names | self.array_feature_names) and n not in self.dense_feature_names]
        names = sorted(set(names))
        for n in names:
            if n not in feats:
                raise ValueError(f"afm_cfg.afm_feature_names: '{n}' is not among the model's user / item features")
            if n in self.dense_feature_names:
                raise ValueError(f"afm_cfg.afm_feature_names: '{n}' is a dense feature (dense features stay concat columns and do not interact)")
            if self._get_emb_feature_name(n) not in self.embedding_tables:
                raise ValueError(f"afm_cfg.afm_feature_names: '{n}' has no embedding table")
        if len(names) < 2:
            raise ValueError(f"afm_cfg.afm_feature_names: an interaction needs at least 2 fields (got {names})")
        dims = {n: self.embedding_tables[self._get_emb_feature_name(n)].embedding_dim for n in names}
        if len(set(dims.values())) != 1:
            raise ValueError(f"afm_cfg.afm_feature_names: the fields must share one embedding dim, got {dims} -- list the features of one "
                             "dim, or give them one embeddings.embedding_size")
        factor = cfg.get("attention_factor", 16)
        if isinstance(factor, bool) or not isinstance(factor, int) or factor < 1:
            raise ValueError(f"afm_cfg.attention_factor: a positive integer count of attention units (got {factor!r})")
        use_deep = cfg.get("use_deep", True)
        if not isinstance(use_deep, bool):
            raise ValueError(f"afm_cfg.use_deep: true or false (got {use_deep!r})")
        self.afm_cfg = dict(afm_feature_names=names, attention_factor=int(factor), use_deep=use_deep)
        self.afm_dim = next(iter(dims.values()))

    def _logit(self, batch):
        cfg = self.afm_cfg
        feats = self.user_feature_names | self.item_feature_names
        plan, _, dims, names = self._plan(batch, feats, False, ())
        missing = [n for n in cfg["afm_feature_names"] if n not in names]
        if missing:
            raise ValueError(f"afm_cfg.afm_feature_names: {missing} missing from the batch")
        offs = tuple(sum(dims[:names.index(n)]) for n in cfg["afm_feature_names"])
        D, att = self.afm_dim, self.attention
        # fused: ONE embedding launch writes the concat, the operator reads its fields in place.  The kernels read 16-byte aligned field rows:
        # a 1-column dense feature sorted in front of a field takes that away (-> the torch form)
        aligned = all(o % 4 == 0 for o in offs)
        supported = ops.afm_supported(len(offs), D, cfg["attention_factor"])
        if fused_afm_enabled() and supported and not aligned and not self._afm_warned:
            self._afm_warned = True
            logger.warning("AFM: the interacting fields start at columns %s of the concat, not all multiples of 4 (a dense feature sorts in front "
                           "of one): the fused pooling needs 16-byte aligned fields, so this model runs ops.afm_pool_math", list(offs))
        concat, _, _, _, _ = self._embed(batch, feats)
        if fused_afm_enabled() and supported and aligned:
            pooled = ops.afm_pool(concat, offs, D, att.w1, att.b1, att.w2)
        else:
            pooled = ops.afm_pool_math(concat, offs, D, att.w1, att.b1, att.w2)
        logit = self.bias + self.afm_out(pooled)
        if cfg["use_deep"]:
            logit = logit + self.score_fc.network(concat)
        return logit

    def forward(self, x):
        return torch.sigmoid(self._logit(x))

    def training_step(self, batch, batch_idx):
        return self._ranking_training_step(batch)

    def configure_optimizers(self):
        return self._ranking_optimizers()

    @torch.no_grad()
    def inference(self, batch):
        return torch.sigmoid(self._logit(batch))
