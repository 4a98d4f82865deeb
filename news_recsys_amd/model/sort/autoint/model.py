"""AutoInt ranker (Song et al., CIKM 2019): the field embeddings pass through a stack of interacting layers -- multi-head self-attention over
the fields with a residual projection and a ReLU (ops.interacting_layer: projections and attention on the matrix cores, the first layer reading
the fused embedding concat in place, no q / k / v tensor and nothing of size B x F x F in global memory, forward or backward) --
beside Deep's MLP over the concat when use_deep:  sigmoid(bias + Linear(F * C -> 1, no bias)(last layer) [+ MLP(concat)]).
No reference counterpart: the reference has no AutoInt, so the model is parity-unpinned.  The MLP, the training step and the optimizers are
Deep's (src/model/sort/deep/model.py:24-70).

New optional config block (defaults in brackets):
    autoint_cfg:
      autoint_feature_names: [user_id, item_id]   # the interacting fields [every sparse / array feature of the model]
      att_layers: 3                               # stacked interacting layers  [3]
      att_heads: 2                                # heads per layer  [2]
      att_head_dim: 16                            # width of each head  [16]
      use_residual: true                          # add the residual projection Wres  [true]
      scaling: false                              # false: the paper's unscaled scores; true: head_dim ** -0.5  [false]
      use_deep: true                              # add Deep's MLP over the concat to the logit  [true]
The fields must share one embedding dim.  Array features take part with their pooled vector.  Dense features, and embedding features that are
not listed, stay plain concat columns the MLP sees and the interaction does not.  No dropout on the attention weights, no biases in the
projections, no layer norm.
Parameters beyond Deep's: att.{l}.wq / wk / wv [/ wres] [C, din_l] (C = att_heads * att_head_dim, din_0 = the embedding dim, din_l = C after;
uniform in +-sqrt(3 / din_l): the variance Xavier's rule gives a layer of that fan-in, drawn from torch's generator like every other
parameter), autoint_out.weight [1, F * C], bias [1]; score_fc.* only when use_deep."""
import logging
import math
import os

import torch

from .... import ops
from ...BaseModel.base_model import BaseModel
from ..deep.model import DeepModel


logger = logging.getLogger(__name__)


def fused_autoint_enabled() -> bool:
    """NRX_FUSED_AUTOINT=0: run ops.interacting_layer_math instead of the fused kernels (A/B runs)."""
    return os.environ.get("NRX_FUSED_AUTOINT", "1") != "0"


class InteractingLayer(torch.nn.Module):
    """One layer's parameters: wq, wk, wv [C, din] and, with the residual, wres [C, din]."""

    def __init__(self, din, width, residual):
        super().__init__()
        a = math.sqrt(3.0 / din)
        self.wq = torch.nn.Parameter(torch.empty(width, din).uniform_(-a, a))
        self.wk = torch.nn.Parameter(torch.empty(width, din).uniform_(-a, a))
        self.wv = torch.nn.Parameter(torch.empty(width, din).uniform_(-a, a))
        if residual:
            self.wres = torch.nn.Parameter(torch.empty(width, din).uniform_(-a, a))
        else:
            self.wres = None


class AutoInt(BaseModel):
    def __init__(self, config_path):
        super().__init__(config_path)
        self._load_autoint_cfg()
        self._autoint_warned = False
        cfg = self.autoint_cfg
        C = cfg["att_heads"] * cfg["att_head_dim"]
        self.att = torch.nn.ModuleList(InteractingLayer(self.autoint_dim if l == 0 else C, C, cfg["use_residual"]) for l in range(cfg["att_layers"]))
        self.autoint_out = torch.nn.Linear(len(cfg["autoint_feature_names"]) * C, 1, bias=False)
        self.bias = torch.nn.Parameter(torch.zeros(1))
        if cfg["use_deep"]:
            self.score_fc = DeepModel(input_dim=self.user_input_dim + self.item_input_dim, hidden_dims=[128, 128, 128, 64, 1])

    def _load_autoint_cfg(self):
        cfg = self.config.get("autoint_cfg", {}) or {}
        feats = self.user_feature_names | self.item_feature_names
        names = cfg.get("autoint_feature_names")
        if names is None:
            names = [n for n in feats if n in (self.sparse_feature_names | self.array_feature_names) and n not in self.dense_feature_names]
        names = sorted(set(names))
        for n in names:
            if n not in feats:
                raise ValueError(f"autoint_cfg.autoint_feature_names: '{n}' is not among the model's user / item features")
            if n in self.dense_feature_names:
                raise ValueError(f"autoint_cfg.autoint_feature_names: '{n}' is a dense feature (dense features stay concat columns and do not interact)")
            if self._get_emb_feature_name(n) not in self.embedding_tables:
                raise ValueError(f"autoint_cfg.autoint_feature_names: '{n}' has no embedding table")
        if len(names) < 2:
            raise ValueError(f"autoint_cfg.autoint_feature_names: an interaction needs at least 2 fields (got {names})")
        dims = {n: self.embedding_tables[self._get_emb_feature_name(n)].embedding_dim for n in names}
        if len(set(dims.values())) != 1:
            raise ValueError(f"autoint_cfg.autoint_feature_names: the fields must share one embedding dim, got {dims} -- list the features of one "
                             "dim, or give them one embeddings.embedding_size")
        out = dict(autoint_feature_names=names)
        for key, default, what in (("att_layers", 3, "count of stacked interacting layers"), ("att_heads", 2, "count of heads per layer"),
                                   ("att_head_dim", 16, "width of each head")):
            v = cfg.get(key, default)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"autoint_cfg.{key}: a positive integer {what} (got {v!r})")
            out[key] = int(v)
        for key, default in (("use_residual", True), ("scaling", False), ("use_deep", True)):
            v = cfg.get(key, default)
            if not isinstance(v, bool):
                raise ValueError(f"autoint_cfg.{key}: true or false (got {v!r})")
            out[key] = v
        self.autoint_cfg = out
        self.autoint_dim = next(iter(dims.values()))

    def _logit(self, batch):
        cfg = self.autoint_cfg
        feats = self.user_feature_names | self.item_feature_names
        plan, _, dims, names = self._plan(batch, feats, False, ())
        missing = [n for n in cfg["autoint_feature_names"] if n not in names]
        if missing:
            raise ValueError(f"autoint_cfg.autoint_feature_names: {missing} missing from the batch")
        offs = tuple(sum(dims[:names.index(n)]) for n in cfg["autoint_feature_names"])
        concat, _, _, _, _ = self._embed(batch, feats)
        logit = self.bias + self.autoint_out(self._interact(concat, offs))
        if cfg["use_deep"]:
            logit = logit + self.score_fc.network(concat)
        return logit

    def _interact(self, concat, offs):
        """The stack of interacting layers over the fields at the columns `offs` of concat -> [B, F * C]."""
        cfg = self.autoint_cfg
        F, H, hd = len(offs), cfg["att_heads"], cfg["att_head_dim"]
        C = H * hd
        scale = hd ** -0.5 if cfg["scaling"] else 1.0
        # fused: ONE embedding launch writes the concat, the first layer reads its fields in place.  The kernels read 16-byte aligned field
        # rows: a 1-column dense feature sorted in front of a field takes that away (-> the torch form)
        aligned = all(o % 4 == 0 for o in offs)
        supported = ops.interacting_layer_supported(F, self.autoint_dim, H, hd) and ops.interacting_layer_supported(F, C, H, hd)
        if fused_autoint_enabled() and supported and not aligned and not self._autoint_warned:
            self._autoint_warned = True
            logger.warning("AutoInt: the interacting fields start at columns %s of the concat, not all multiples of 4 (a dense feature sorts in "
                           "front of one): the fused layer needs 16-byte aligned fields, so this model runs ops.interacting_layer_math", list(offs))
        layer = ops.interacting_layer if fused_autoint_enabled() and supported and aligned else ops.interacting_layer_math
        h, h_offs, din = concat, offs, self.autoint_dim
        for att in self.att:
            h = layer(h, h_offs, din, att.wq, att.wk, att.wv, att.wres, heads=H, scale=scale)
            h_offs, din = tuple(range(0, F * C, C)), C
        return h

    def forward(self, x):
        return torch.sigmoid(self._logit(x))

    def training_step(self, batch, batch_idx):
        return self._ranking_training_step(batch)

    def configure_optimizers(self):
        return self._ranking_optimizers()

    @torch.no_grad()
    def inference(self, batch):
        return torch.sigmoid(self._logit(batch))
