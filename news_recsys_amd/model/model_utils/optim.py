"""Optimizer for the row-sparse gradient mode (`embeddings.sparse_grad: true`).

The reference trains everything with one dense `AdamW(self.parameters())` (sort/deep/model.py:55): on a
100M-row table that is a full-table read-modify-write of weights and both moments every step.  With
row-sparse table grads the tables are updated by `torch.optim.SparseAdam` (moments touched only for the
looked-up rows; no weight decay) and the dense parameters keep AdamW.  This wrapper presents both as
one `Optimizer` so `configure_optimizers()` keeps its reference shape (one optimizer + one scheduler)."""
import ctypes as C
import math

import torch

from ... import _lib, ops


def dense_adamw(params, **kw):
    """torch.optim.AdamW as the reference builds it (sort/deep/model.py:55, recall/DSSM/model.py) -- with torch's ONE-PASS multi-tensor kernel
    (`fused=True`) when every parameter lives on the GPU: same update rule, one read and one write of (p, grad, m, v) instead of the ~10
    elementwise passes of the default foreach form.  On the 26 x 100 k-row tables of a C2-shaped model the step (embedding forward, backward,
    optimizer) goes 1110 -> 396 us at B = 512 (tools/probe_small_train_modes.py); NRX_ADAMW_FUSED=0 keeps torch's default."""
    import os
    params = list(params)
    if os.environ.get("NRX_ADAMW_FUSED", "1") != "0" and params and all(torch.is_tensor(p) and p.is_cuda and p.is_floating_point() for p in params):
        try:
            return torch.optim.AdamW(params, fused=True, **kw)
        except (RuntimeError, TypeError, ValueError):
            pass
    return torch.optim.AdamW(params, **kw)


class _SinkTableOptimizer:
    """What the optimizers that drain an ops.SparseGradSink share: tables identified by tensor identity and registered on first appearance (or, bf16, in
    the order of `params`), the launch-local -> optimizer-wide renumbering of an entry's keys, the merge of a table fed by several backward groups into ONE
    update per row, the row maps of bf16 arenas, and the step / seed bookkeeping of a checkpoint.  A subclass supplies `_add_state(t)` (the state of a
    newly registered table) and its `step()`."""
    _NAME = "FusedSparseAdam"        # the class an error message names

    def _init_common(self, sink, lr, capturable, params, sr_seed, row_maps):
        self.sink, self.lr = sink, lr
        self.capturable = bool(capturable)
        self.params = list(params) if params is not None else None
        self._t_dev = None
        self.t = 0
        self.tables = []         # every table seen so far; position = the table's index in the optimizer's key space
        self._index = {}         # id(tensor) -> position
        self._gmaps = {}         # table-list identity -> device map (launch-local table index -> position)
        self._identity = {}      # table-list identity -> that map is the identity
        self._maps = []          # per-table slot maps of the two-list merge (made on first use)
        self.pair_merge = True   # two backward groups of one width: merge by marking (False: the sort-based _merge)
        self.sr_seed = int(sr_seed) & ((1 << 64) - 1)     # stochastic rounding of bf16 tables
        self.row_maps = None
        if row_maps is not None:
            self.set_row_maps(row_maps)
        # global-norm clipping of the sink's lists (nrx_rows_sqnorm / _finish / nrx_rows_scale; see prepare / finish_norm / apply)
        self.max_grad_norm = None
        self.norm_group = None   # a torch.distributed group: the ranks' bins are summed (int64) before the finish launch
        self.norm_skip = None    # table tensors this rank must not count (a replicated table on the ranks other than 0)
        self.grad_norm = None    # device double[1] / float[1] of the last clipped step: logging without a host read
        self.clip_coef = None
        self._norm_bins = None
        self._prepared = None
        if self.params is not None and any(t.dtype is torch.bfloat16 for t in self.params):
            # the rounding hash names a table by its position here: pinned to the params order, so a run resumed from a checkpoint
            # (whose load registers the tables in that order) hashes every table as the uninterrupted run does
            for t in self.params:
                self._register(t)

    def set_row_maps(self, row_maps):
        """(row_mul, row_add) per entry of `params` (see __init__); None: the identity for every table."""
        if row_maps is None:
            self.row_maps = None
            return
        row_maps = [(int(m), int(a)) for m, a in row_maps]
        if self.params is None or len(row_maps) != len(self.params):
            raise ValueError(f"{self._NAME}: row_maps needs params=<the table list> and one (row_mul, row_add) per table of it")
        self.row_maps = row_maps

    def _register(self, t: torch.Tensor) -> int:
        i = self._index.get(id(t))
        if i is None:
            if t.dtype is torch.bfloat16 and (self.params is None or not any(p is t for p in self.params)):
                # positions by first appearance in the sink would make the rounding stream depend on the batch order of a run
                raise ValueError(f"{self._NAME}: bf16 tables need params=<the table list>: their positions in it name them in the "
                                 "stochastic-rounding hash, which a resumed run must reproduce")
            i = len(self.tables)
            self._index[id(t)] = i
            self.tables.append(t)
            self._add_state(t)
        return i

    def _global_keys(self, e):
        """Re-express an entry's keys (table index = position in that launch's table list) in the optimizer's own
        table numbering; filler past the device-side count becomes INT64_MAX (ignored by the kernel)."""
        BIG = torch.iinfo(torch.int64).max
        MASK = (1 << 40) - 1
        dev = e["uniq"].device
        ck = tuple(id(t) for t in e["tables"])
        gmap = self._gmaps.get(ck)
        if gmap is None:        # built once per table list (a host-to-device copy: must not happen inside a graph capture)
            pos = [self._register(t) for t in e["tables"]]
            gmap = torch.tensor(pos, dtype=torch.int64, device=dev)
            self._gmaps[ck] = gmap
            self._identity[ck] = pos == list(range(len(pos)))
        k = e["uniq"]
        if e.get("filler"):             # the one-launch small form: unused slots are keyed -1 wherever they are
            if self._identity.get(ck):
                return k                # launch-local table numbers ARE the optimizer's: the kernel skips negative keys itself
            valid = k >= 0
        else:
            valid = torch.arange(e["cap"], device=dev) < e["counts"][0]
        local = torch.where(valid, k >> 40, torch.zeros_like(k))
        return torch.where(valid, (gmap[local] << 40) | (k & MASK), torch.full_like(k, BIG))

    @staticmethod
    def _merge(keys, vals):
        """(keys, values) lists with possibly repeated (table,row) keys -> one entry per key.  Device-only torch
        ops; INT64_MAX filler sorts last and stays filler."""
        BIG = torch.iinfo(torch.int64).max
        skeys, order = torch.sort(keys, stable=True)
        head = torch.ones_like(skeys, dtype=torch.bool)
        head[1:] = skeys[1:] != skeys[:-1]
        seg = torch.cumsum(head, 0) - 1
        merged_vals = torch.zeros_like(vals).index_add_(0, seg, vals[order])
        merged_keys = torch.full_like(skeys, BIG)
        merged_keys[seg] = skeys
        return merged_keys, merged_vals

    def _pending_by_dim(self):
        """The sink's entries as {dim: [(keys in the optimizer's numbering, values)]} (registers the tables an entry names)."""
        by_dim = {}
        for e in self.sink.pending:
            by_dim.setdefault(e["dim"], []).append((self._global_keys(e), e["values"]))
        return by_dim

    def _merge_lists(self, lib, by_dim):
        """(dim, keys, values) for every list of by_dim, after making the lists of one dim disjoint: a table fed by several backward groups in one
        step gets ONE gradient per row.  A generator: a dim's merge launches run when the consumer reaches that dim."""
        n = len(self.tables)
        for dim, lst in by_dim.items():
            if len(lst) == 1:
                yield (dim, *lst[0])
            elif len(lst) == 2 and self.pair_merge:
                # one table fed by two backward groups (DSSM's towers share the news table): ONE update per row.  List A is marked in per-table
                # slot maps, the pairs of B that A also holds are added into A's rows and blanked (nrx_rows_merge), A is unmarked; the two lists
                # are then disjoint: three small launches instead of a device sort + segment sums over the concatenation
                (ka, va), (kb, vb) = lst
                stream = torch.cuda.current_stream(ka.device).cuda_stream
                maps = self._slot_maps()
                rows = (C.c_int64 * n)(*[t.shape[0] for t in self.tables])
                ops.check(lib.nrx_rows_mark(ka.data_ptr(), ka.numel(), None, maps, rows, n, 0, stream), "nrx_rows_mark")
                ops.check(lib.nrx_rows_merge(kb.data_ptr(), vb.data_ptr(), kb.numel(), None, va.data_ptr(), maps, rows, n, dim, stream), "nrx_rows_merge")
                ops.check(lib.nrx_rows_mark(ka.data_ptr(), ka.numel(), None, maps, rows, n, 1, stream), "nrx_rows_mark")
                yield dim, ka, va
                yield dim, kb, vb
            else:
                yield (dim, *self._merge(torch.cat([k for k, _ in lst]), torch.cat([v for _, v in lst])))

    def _update_merged(self, lib, by_dim, update):
        """update(dim, keys, values) on every list of by_dim (made disjoint: _merge_lists)."""
        for dim, keys, vals in self._merge_lists(lib, by_dim):
            update(dim, keys, vals)

    # ---- global-norm clipping.  step() = prepare() -> finish_norm() -> apply() when max_grad_norm is set, and exactly the unclipped sequence of
    # library calls when it is None.  SparseDenseAdam drives the three phases itself, with the dense parameters' part in between.
    def _init_clip(self, max_grad_norm, norm_group, norm_skip):
        self.set_max_grad_norm(max_grad_norm)
        self.norm_group = norm_group
        self.norm_skip = list(norm_skip) if norm_skip is not None else None

    def set_max_grad_norm(self, v):
        """The global-norm bound of the next step() (None: no clipping, no norm).  A captured step keeps the value it was captured with."""
        if v is not None and not float(v) > 0:
            raise ValueError(f"{self._NAME}: max_grad_norm must be positive (got {v!r})")
        self.max_grad_norm = None if v is None else float(v)

    def _clip_buffers(self, dev):
        if self._norm_bins is None:
            self._norm_bins = torch.zeros(258, dtype=torch.int64, device=dev)     # (re-armed by every finish launch)
            self.grad_norm = torch.zeros(1, dtype=torch.float64, device=dev)
            self.clip_coef = torch.ones(1, dtype=torch.float32, device=dev)

    def _prepare_lists(self, lib):
        return list(self._merge_lists(lib, self._pending_by_dim()))

    def _skip_mask(self):
        """The norm_skip tables as a mask over the optimizer's table positions.  A table is found by identity or by its storage (a bound sharded step
        holds `weight.data` of an fp32 model: another Python object over the same memory).  One that this step's lists did not register yet is
        legitimately absent -- as long as `params` knows it; a tensor that is neither registered nor in `params` names no table of this optimizer:
        counting it on every rank would be silent and wrong, so that is an error."""
        skip = 0
        for t in self.norm_skip or ():
            i = self._index.get(id(t))
            if i is None:
                i = next((k for k, reg in enumerate(self.tables) if reg.data_ptr() == t.data_ptr() and reg.shape == t.shape), None)
            if i is not None:
                skip |= 1 << i
            elif self.params is None or not any(p.data_ptr() == t.data_ptr() and p.shape == t.shape for p in self.params):
                raise ValueError(f"{self._NAME}: a norm_skip tensor {tuple(t.shape)} is none of the tables this optimizer has registered or was "
                                 "given in `params`: it would be counted on every rank")
        return skip

    @torch.no_grad()
    def prepare(self, device=None):
        """Phase 1 of a clipped step: the sink's lists made disjoint (the norm is the MERGED gradient's: a row fed by two backward groups counts
        once), and every list's live rows added into the bins.  device: where the bins live when the sink is empty."""
        lib = _lib.load()
        lists = self._prepare_lists(lib)
        self._prepared = lists
        dev = lists[0][1].device if lists else (device if device is not None else (self.tables[0].device if self.tables else
                                                                                    (self.params[0].device if self.params else None)))
        if dev is None:
            if self.norm_group is not None:     # (the other ranks wait in the bins' all-reduce: this rank must reach it too)
                raise RuntimeError(f"{self._NAME}: a clipped step over several ranks found no gradient and no table to place the norm's bins by; "
                                   "construct the optimizer with params=<the table list>")
            return
        self._clip_buffers(dev)
        n = len(self.tables)
        if lists and n > _lib.NRX_MAX_FEATURES:
            raise NotImplementedError(f"{self._NAME}: more than 64 distinct tables")
        skip = self._skip_mask()
        for dim, keys, vals in lists:
            ops.check(lib.nrx_rows_sqnorm(keys.data_ptr(), vals.data_ptr(), keys.numel(), None, n, dim, skip, self._norm_bins.data_ptr(),
                                          torch.cuda.current_stream(keys.device).cuda_stream), "nrx_rows_sqnorm")

    @torch.no_grad()
    def finish_norm(self, extra_sq=None):
        """Phase 2: the bins (summed over norm_group as int64 when set) + extra_sq (device double[1]: the dense parameters' squared norm) ->
        grad_norm and clip_coef on the device; the bins are re-armed.  No host read."""
        if self._norm_bins is None:
            return
        if self.norm_group is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self._NAME}: a clipped step over several ranks cannot be captured in a graph (the all-reduce of the norm's "
                                   "bins is not captured); capture at world 1 or step eagerly")
            import torch.distributed as dist
            dist.all_reduce(self._norm_bins, op=dist.ReduceOp.SUM, group=self.norm_group)
        ops.check(_lib.load().nrx_rows_sqnorm_finish(self._norm_bins.data_ptr(), extra_sq.data_ptr() if extra_sq is not None else None,
                                                     float(self.max_grad_norm), self.grad_norm.data_ptr(), self.clip_coef.data_ptr(), 1,
                                                     torch.cuda.current_stream(self._norm_bins.device).cuda_stream), "nrx_rows_sqnorm_finish")

    @torch.no_grad()
    def apply(self):
        """Phase 3: every list scaled by clip_coef (a launch that returns at once where the coefficient is 1), then the update launches."""
        lists, self._prepared = self._prepared, None
        if lists is None:
            raise RuntimeError(f"{self._NAME}.apply() without prepare()")
        if self._norm_bins is not None:
            lib = _lib.load()
            for dim, _, vals in lists:
                ops.check(lib.nrx_rows_scale(vals.data_ptr(), vals.shape[0], dim, self.clip_coef.data_ptr(),
                                             torch.cuda.current_stream(vals.device).cuda_stream), "nrx_rows_scale")
        self._step(lists)

    @torch.no_grad()
    def step(self):
        if self.max_grad_norm is None:
            return self._step(None)
        self.prepare()
        self.finish_norm()
        self.apply()

    def _hash_row_maps(self, n):
        """(row_mul, row_add) host arrays in the optimizer's table order for the rounding hash of bf16 tables, or (None, None): the identity."""
        if self.row_maps is None or all(m == (1, 0) for m in self.row_maps):
            return None, None
        maps = [self.row_maps[self._stable_index(t)] for t in self.tables]      # (bf16 tables are all in params: _register)
        return (C.c_int64 * n)(*[m for m, _ in maps]), (C.c_int64 * n)(*[a for _, a in maps])

    def _slot_maps(self):
        """int32 [rows] per table, all -1 between uses (nrx_rows_mark / nrx_rows_merge): made when a step first needs them."""
        while len(self._maps) < len(self.tables):
            t = self.tables[len(self._maps)]
            self._maps.append(torch.full((t.shape[0],), -1, dtype=torch.int32, device=t.device))
        return (C.c_void_p * len(self._maps))(*[m.data_ptr() for m in self._maps])

    def zero_grad(self, set_to_none: bool = True):
        self.sink.clear()

    def _stable_index(self, t):
        if self.params is not None:
            for i, p in enumerate(self.params):
                if p is t:
                    return i
        return None

    def _check_saved_key(self, key, what):
        """A checkpoint names a table by its position in `params`: refuse the ones it could not name, and a `params` that does not cover the key."""
        if isinstance(key, str):
            raise ValueError(f"{self._NAME}.load_state_dict: the checkpoint holds {what} of a table that was not in "
                             "`params` when it was saved; construct the optimizer with params=<the table list>")
        if self.params is None or not 0 <= key < len(self.params):
            raise ValueError(f"{self._NAME}.load_state_dict needs params=<the same table list as at save time>")


class FusedSparseAdam(_SinkTableOptimizer):
    """Adam(W) for the embedding tables, fused with the row-sparse backward.  The backward
    leaves (unique (table,row) keys, summed row gradients, counts) on the device in an ops.SparseGradSink; step()
    updates exactly those rows of weights and moments with one `nrx_sparse_adam_step` launch per group -- no
    COO tensors, no host synchronisation, no traffic proportional to the table size.  Update rule =
    torch.optim.SparseAdam (tested against it) + optional decoupled weight decay on the touched rows.
    A table that received gradients from several backward groups in one step (DSSM's towers share the news
    table) gets them merged first, so the step is still ONE Adam update per row.  Tables are identified by tensor
    identity; their moments are created (zeros) the first time a table shows up in the sink.

    bf16 tables (torch.bfloat16; all tables of the optimizer then) keep fp32 moments and step through
    `nrx_sparse_adam_step_bf16`: the fp32 update of the widened row, rounded back to bf16 stochastically with bits that
    depend on (sr_seed, step, table, row, column) only -- sr_seed and the step count are in state_dict(), so a resumed run
    continues the same rounding stream.  `table` is the table's position in `params`, which bf16 tables therefore require.
    `row` is the key's row, or -- row_maps -- an affine function of it: a row-sharded bf16 arena (shard_step.make_arena) names a row by
    its local index, the hash takes the global one (shard_step.arena_row_map), so a sharded run leaves the unsharded run's bit patterns."""

    def __init__(self, sink: "ops.SparseGradSink", lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False,
                 params=None, sr_seed=0, row_maps=None, max_grad_norm=None, norm_group=None, norm_skip=None):
        """capturable=True keeps the step counter and the bias-corrected step size on the device (like
        torch.optim.Adam(capturable=True)) so step() can be captured in a HIP graph (graph.GraphedStep); lr is
        then fixed at capture time.  params (optional): the table tensors in a stable order -- state_dict() then
        keys the moments by position in that list, so a checkpoint restores into a freshly built model.
        row_maps (optional, bf16 tables): one (row_mul, row_add) per entry of `params` -- the stochastic rounding hashes
        row * row_mul + row_add; None, or (1, 0) for a table: the key's row itself.
        max_grad_norm (optional): step() first scales the sink's gradients so that their global norm (the merged lists' live rows; summed over the
        ranks of norm_group, without the tables of norm_skip) is at most this -- torch.nn.utils.clip_grad_norm_'s rule, computed on the device
        (include/nrx_embed.h: nrx_rows_sqnorm); grad_norm / clip_coef hold the last step's values on the device."""
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.moments = []        # (exp_avg, exp_avg_sq) per table
        self._init_common(sink, lr, capturable, params, sr_seed, row_maps)
        self._init_clip(max_grad_norm, norm_group, norm_skip)

    def _add_state(self, t):
        # both moments of a row side by side ([rows, 2, D]; exp_avg / exp_avg_sq are its two views): the update is a random
        # read-modify-write of (w, m, v) and every 64-byte access costs a 128-byte fetch -- adjacent, m and v share one
        mv = torch.zeros((t.shape[0], 2, t.shape[1]), dtype=torch.float32 if t.dtype is torch.bfloat16 else t.dtype, device=t.device)
        self.moments.append((mv[:, 0], mv[:, 1]))

    @torch.no_grad()
    def _step(self, lists):
        """lists: None -- the unclipped step, straight from the sink -- or prepare()'s disjoint (dim, keys, values) lists."""
        if not self.sink.pending:
            return
        lib = _lib.load()
        self.t += 1
        b1, b2 = self.betas
        step_size = self.lr * math.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)
        ss_dev = None
        if self.capturable:
            dev = self.sink.pending[0]["uniq"].device
            if self._t_dev is None:
                self._t_dev = torch.zeros((), dtype=torch.float64, device=dev)
            self._t_dev += 1
            ss_dev = (self.lr * torch.sqrt(1.0 - b2 ** self._t_dev) / (1.0 - b1 ** self._t_dev)).to(torch.float32).reshape(1)
        by_dim = self._pending_by_dim() if lists is None else None
        n = len(self.tables)
        if n > _lib.NRX_MAX_FEATURES:
            raise NotImplementedError("FusedSparseAdam: more than 64 distinct tables")
        tp = (C.c_void_p * n)(*[t.data_ptr() for t in self.tables])
        mp = (C.c_void_p * n)(*[m.data_ptr() for m, _ in self.moments])
        vp = (C.c_void_p * n)(*[v.data_ptr() for _, v in self.moments])
        n_bf16 = sum(t.dtype is torch.bfloat16 for t in self.tables)
        if 0 < n_bf16 < n:
            raise NotImplementedError("FusedSparseAdam: bf16 and fp32 tables in one optimizer")
        # the rounding stream's step index: the host count, or (capturable) the device count a captured loop advances
        step_dev = self._t_dev.to(torch.int64).reshape(1) if (n_bf16 and self._t_dev is not None) else None
        rmul, radd = self._hash_row_maps(n) if n_bf16 else (None, None)
        def adam(dim, keys, vals):
            if rmul is not None:
                ops.check(lib.nrx_sparse_adam_step_bf16_rows(tp, mp, vp, n, dim, keys.data_ptr(), vals.data_ptr(), keys.numel(), None,
                                                             step_size, ss_dev.data_ptr() if ss_dev is not None else None, b1, b2, self.eps,
                                                             self.lr * self.weight_decay, self.sr_seed, self.t,
                                                             step_dev.data_ptr() if step_dev is not None else None, rmul, radd,
                                                             torch.cuda.current_stream(keys.device).cuda_stream), "nrx_sparse_adam_step_bf16_rows")
                return
            if n_bf16:
                ops.check(lib.nrx_sparse_adam_step_bf16(tp, mp, vp, n, dim, keys.data_ptr(), vals.data_ptr(), keys.numel(), None,
                                                        step_size, ss_dev.data_ptr() if ss_dev is not None else None, b1, b2, self.eps,
                                                        self.lr * self.weight_decay, self.sr_seed, self.t,
                                                        step_dev.data_ptr() if step_dev is not None else None,
                                                        torch.cuda.current_stream(keys.device).cuda_stream), "nrx_sparse_adam_step_bf16")
                return
            ops.check(lib.nrx_sparse_adam_step(tp, mp, vp, n, dim, keys.data_ptr(), vals.data_ptr(), keys.numel(), None,
                                               step_size, ss_dev.data_ptr() if ss_dev is not None else None, b1, b2, self.eps,
                                               self.lr * self.weight_decay,
                                               torch.cuda.current_stream(keys.device).cuda_stream), "nrx_sparse_adam_step")

        if lists is None:
            self._update_merged(lib, by_dim, adam)
        else:
            for dim, keys, vals in lists:
                adam(dim, keys, vals)
        self.sink.clear()

    # ---- checkpointing: step count + both moments of every table that has been updated so far
    def state_dict(self):
        tables = {}
        for pos, t in enumerate(self.tables):
            key = self._stable_index(t)
            m, v = self.moments[pos]
            tables[key if key is not None else f"unlisted:{pos}"] = {"exp_avg": m, "exp_avg_sq": v}
        steps = {}
        for pos, c in getattr(self, "_steps", {}).items():          # (ExactDenseAdamW: a table's own step count)
            key = self._stable_index(self.tables[pos])
            steps[key if key is not None else f"unlisted:{pos}"] = c
        return {"t": self.t, "t_dev": None if self._t_dev is None else float(self._t_dev.item()), "tables": tables, "steps": steps,
                "sr_seed": self.sr_seed}

    def load_state_dict(self, sd):
        self.t = int(sd["t"])
        if "sr_seed" in sd:
            self.sr_seed = int(sd["sr_seed"])
        self._t_dev = None
        if sd.get("t_dev") is not None and self.capturable and self.params:
            self._t_dev = torch.tensor(sd["t_dev"], dtype=torch.float64, device=self.params[0].device)
        for key, mv in sd["tables"].items():
            self._check_saved_key(key, "moments")
            pos = self._register(self.params[key])
            m, v = self.moments[pos]
            m.copy_(mv["exp_avg"])
            v.copy_(mv["exp_avg_sq"])
        unlisted = [key for key in (sd.get("steps") or {}) if isinstance(key, str)]
        if unlisted:
            raise ValueError("load_state_dict: the checkpoint holds step counts of tables that were not in `params` when it was saved "
                             f"({unlisted}); construct the optimizer with params=<the table list>")
        if sd.get("steps"):
            self._steps = {self._register(self.params[key]): int(c) for key, c in sd["steps"].items()}
        elif hasattr(self, "maps"):
            # (ExactDenseAdamW) a checkpoint written before the per-table step counts existed: every table had moved on every one of the `t`
            # steps -- restarting the tables at step 1 would apply lr / (1 - beta1) to the restored moments and leave torch.optim.AdamW's path
            self._steps = {pos: self.t for pos in range(len(self.tables))}


class FusedSparseAdagrad(_SinkTableOptimizer):
    """Adagrad for the embedding tables, fused with the row-sparse backward like FusedSparseAdam and with its contract (the sink is drained in
    step(); tables by tensor identity, registered on first appearance; a table fed by two backward groups gets ONE update per row; bf16 tables need
    `params=` and round stochastically from (sr_seed, step, table, row, column); row_maps for bf16 arenas) -- with ONE fp32 accumulator per row
    (rowwise=True: `s += mean(g^2)` over the row, state [rows]) or per element (rowwise=False: torch.optim.Adagrad on sparse gradients with
    lr_decay = 0 and initial_accumulator_value = 0, state [rows, dim]) where Adam keeps two moments per element:  `w -= lr * g / (sqrt(s) + eps)`,
    after the optional decoupled decay `w -= w * lr * weight_decay` of the touched rows.  One `nrx_sparse_adagrad_step` launch per list.
    The reference trains the tables with dense AdamW: like `sparse_grad: fused` itself this is an opt-in, documented deviation."""
    _NAME = "FusedSparseAdagrad"

    def __init__(self, sink: "ops.SparseGradSink", lr=1e-2, eps=1e-10, weight_decay=0.0, rowwise=True, capturable=False, params=None, sr_seed=0,
                 row_maps=None, max_grad_norm=None, norm_group=None, norm_skip=None):
        """capturable=True keeps the step count (the rounding stream of bf16 tables) and the lr on the device, so step() can be captured in a HIP
        graph (graph.GraphedStep): a replay advances the count itself, and reads the lr from `lr_dev` -- set_lr() between replays follows a
        schedule (the decay factor lr * weight_decay is a launch argument, fixed at capture time).  params / sr_seed / row_maps and
        max_grad_norm / norm_group / norm_skip: FusedSparseAdam's."""
        self.eps, self.weight_decay, self.rowwise = eps, weight_decay, bool(rowwise)
        self.sums = []           # per table: [rows] (rowwise) or [rows, dim], fp32, zeros at registration
        self.lr_dev = None
        self._init_common(sink, lr, capturable, params, sr_seed, row_maps)
        self._init_clip(max_grad_norm, norm_group, norm_skip)

    def _add_state(self, t):
        self.sums.append(torch.zeros((t.shape[0],) if self.rowwise else tuple(t.shape), dtype=torch.float32, device=t.device))

    def set_lr(self, lr):
        """The step of the next step(): the host value and (capturable) the device word a captured step() reads.  Not to be called inside a capture."""
        self.lr = float(lr)
        if self.lr_dev is not None:
            self.lr_dev.fill_(self.lr)

    @torch.no_grad()
    def _step(self, lists):
        """lists: None -- the unclipped step, straight from the sink -- or prepare()'s disjoint (dim, keys, values) lists."""
        if not self.sink.pending:
            return
        lib = _lib.load()
        self.t += 1
        if self.capturable:
            dev = self.sink.pending[0]["uniq"].device
            if self._t_dev is None:
                self._t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            if self.lr_dev is None:
                self.lr_dev = torch.full((1,), float(self.lr), dtype=torch.float32, device=dev)
            elif not torch.cuda.is_current_stream_capturing():
                self.lr_dev.fill_(float(self.lr))        # (an eager step follows the host value; a captured one reads the word as a replay finds it)
            self._t_dev += 1
        by_dim = self._pending_by_dim() if lists is None else None
        n = len(self.tables)
        if n > _lib.NRX_MAX_FEATURES:
            raise NotImplementedError("FusedSparseAdagrad: more than 64 distinct tables")
        n_bf16 = sum(t.dtype is torch.bfloat16 for t in self.tables)
        if 0 < n_bf16 < n:
            raise NotImplementedError("FusedSparseAdagrad: bf16 and fp32 tables in one optimizer")
        tp = (C.c_void_p * n)(*[t.data_ptr() for t in self.tables])
        sp = (C.c_void_p * n)(*[s.data_ptr() for s in self.sums])
        flags = (_lib.NRX_ADAGRAD_ROWWISE if self.rowwise else 0) | (_lib.NRX_ADAGRAD_TABLE_BF16 if n_bf16 else 0)
        rmul, radd = self._hash_row_maps(n) if n_bf16 else (None, None)
        lr_dev = self.lr_dev.data_ptr() if self.capturable else None
        step_dev = self._t_dev.data_ptr() if self.capturable else None

        def adagrad(dim, keys, vals):
            ops.check(lib.nrx_sparse_adagrad_step(tp, sp, n, dim, keys.data_ptr(), vals.data_ptr(), keys.numel(), None, self.lr, lr_dev, self.eps,
                                                  self.lr * self.weight_decay, flags, self.sr_seed, self.t, step_dev, rmul, radd,
                                                  torch.cuda.current_stream(keys.device).cuda_stream), "nrx_sparse_adagrad_step")

        if lists is None:
            self._update_merged(lib, by_dim, adagrad)
        else:
            for dim, keys, vals in lists:
                adagrad(dim, keys, vals)
        self.sink.clear()

    # ---- checkpointing: step count, rounding seed and the accumulators of every table that has been updated so far, by position in `params`
    def state_dict(self):
        tables = {}
        for pos, t in enumerate(self.tables):
            key = self._stable_index(t)
            tables[key if key is not None else f"unlisted:{pos}"] = {"sum": self.sums[pos]}
        return {"t": self.t, "t_dev": None if self._t_dev is None else int(self._t_dev.item()), "tables": tables, "sr_seed": self.sr_seed,
                "rowwise": self.rowwise}

    def load_state_dict(self, sd):
        if "rowwise" in sd and bool(sd["rowwise"]) != self.rowwise:
            raise ValueError(f"FusedSparseAdagrad.load_state_dict: the checkpoint was written with rowwise={bool(sd['rowwise'])}, this optimizer has "
                             f"rowwise={self.rowwise}")
        self.t = int(sd["t"])
        if "sr_seed" in sd:
            self.sr_seed = int(sd["sr_seed"])
        self._t_dev = None
        if sd.get("t_dev") is not None and self.capturable and self.params:
            self._t_dev = torch.tensor([int(sd["t_dev"])], dtype=torch.int64, device=self.params[0].device)
        for key, st in sd["tables"].items():
            self._check_saved_key(key, "accumulators")
            self.sums[self._register(self.params[key])].copy_(st["sum"])


class ExactDenseAdamW(FusedSparseAdam):
    """The reference's optimizer for the tables -- ONE dense torch.optim.AdamW over model.parameters() (sort/deep/model.py:54-65: every row of
    every table moves every step: decoupled weight decay, decaying moments) -- fed from the row-sparse sink instead of dense .grad tensors:
    `nrx_rows_mark` notes which rows have a gradient this step, `nrx_dense_adamw_rows` streams over every row of every table once (SURVEY 8f
    row 2, "exact-dense mode").  Same numbers as torch.optim.AdamW on the dense gradients (tests/test_fused_sparse_adam_gpu.py); no dense
    gradient is formed, zero-filled or read.  As torch.optim.AdamW skips a parameter whose .grad is None, a step() updates the tables that a
    backward launch of the step looked up (the sink entries name them) -- all of their rows -- and leaves the others alone, each table with
    its own step count (capturable=True: one device-side count for all tables, every registered table is streamed every step).
    exp_avg / exp_avg_sq are plain [rows, dim] tensors (torch's layout)."""

    def __init__(self, sink, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=False, max_grad_norm=None,
                 norm_group=None, norm_skip=None):
        super().__init__(sink, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable, params=list(params),
                         max_grad_norm=max_grad_norm, norm_group=norm_group, norm_skip=norm_skip)
        self.maps = []
        for t in self.params:
            self._register(t)

    def _register(self, t: torch.Tensor) -> int:
        i = self._index.get(id(t))
        if i is None:
            if t.dtype is torch.bfloat16:
                raise TypeError("ExactDenseAdamW: bf16 tables train with FusedSparseAdam (embeddings.sparse_grad: fused)")
            i = len(self.tables)
            self._index[id(t)] = i
            self.tables.append(t)
            self.moments.append((torch.zeros_like(t), torch.zeros_like(t)))
            self.maps.append(torch.full((t.shape[0],), -1, dtype=torch.int32, device=t.device))
        return i

    def _collect(self):
        """The sink's entries as {dim: [(keys, values)]}, and the positions of the tables a backward launch of the step looked up."""
        by_dim = {}
        touched = set()
        for e in self.sink.pending:
            by_dim.setdefault(e["dim"], []).append((self._global_keys(e), e["values"]))
            for tid in e.get("table_ids", range(len(e["tables"]))):      # the tables this backward launch looked up
                i = self._index.get(id(e["tables"][tid]))
                if i is not None:
                    touched.add(i)
        return by_dim, touched

    def _one_list(self, lst):
        if len(lst) == 1:
            return lst[0]
        # one table fed by several backward groups: ONE gradient per row
        return self._merge(torch.cat([kk for kk, _ in lst]), torch.cat([v for _, v in lst]))

    def _prepare_lists(self, lib):
        by_dim, touched = self._collect()
        merged = {dim: self._one_list(lst) for dim, lst in by_dim.items()}
        self._collected = (merged, touched)
        return [(dim, k, v) for dim, (k, v) in merged.items()]

    @torch.no_grad()
    def _step(self, lists):
        """lists: None -- the unclipped step, straight from the sink -- or prepare()'s lists (one per dim, already merged and scaled)."""
        lib = _lib.load()
        self.t += 1
        merged = None
        if lists is None:
            by_dim, touched = self._collect()
        else:
            merged, touched = self._collected
            by_dim, self._collected = merged, None
        if self.capturable:
            touched = set(range(len(self.tables)))       # (one device-side step count: every table moves every step)
        steps = getattr(self, "_steps", None)
        if steps is None:
            steps = self._steps = {}
        for i in touched:
            steps[i] = steps.get(i, 0) + 1
        n = len(self.tables)
        if n > _lib.NRX_MAX_FEATURES:
            raise NotImplementedError("ExactDenseAdamW: more than 64 distinct tables")
        b1, b2 = self.betas
        hyper = None
        if self.capturable:             # the step count lives on the device: a captured loop advances the bias corrections between replays
            dev0 = self.tables[0].device
            if self._t_dev is None:
                self._t_dev = torch.zeros((), dtype=torch.float64, device=dev0)
            self._t_dev += 1
            hyper = torch.stack([self.lr / (1.0 - b1 ** self._t_dev), 1.0 / torch.sqrt(1.0 - b2 ** self._t_dev)]).to(torch.float32)
        elif torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ExactDenseAdamW: construct with capturable=True to capture step() in a graph (the step count is baked in otherwise)")
        marked = {}
        for dim, tstep in sorted({(self.tables[i].shape[1], steps[i]) for i in touched}):
            idx = [i for i in sorted(touched) if self.tables[i].shape[1] == dim and steps[i] == tstep]
            dev = self.tables[idx[0]].device
            stream = torch.cuda.current_stream(dev).cuda_stream
            k = len(idx)
            rows = (C.c_int64 * n)(*[t.shape[0] for t in self.tables])
            maps_all = (C.c_void_p * n)(*[m.data_ptr() for m in self.maps])
            if dim not in marked:                    # a dim's rows are marked once; tables of the dim at another step count read the same marks
                vals = None
                lst = by_dim.get(dim)
                if lst:
                    keys, vals = lst if merged is not None else self._one_list(lst)
                    ops.check(lib.nrx_rows_mark(keys.data_ptr(), keys.numel(), None, maps_all, rows, n, 0, stream), "nrx_rows_mark")
                marked[dim] = vals
            vals = marked[dim]
            tp = (C.c_void_p * k)(*[self.tables[i].data_ptr() for i in idx])
            mp = (C.c_void_p * k)(*[self.moments[i][0].data_ptr() for i in idx])
            vp = (C.c_void_p * k)(*[self.moments[i][1].data_ptr() for i in idx])
            sp = (C.c_void_p * k)(*[self.maps[i].data_ptr() for i in idx])
            rk = (C.c_int64 * k)(*[self.tables[i].shape[0] for i in idx])
            ops.check(lib.nrx_dense_adamw_rows(tp, mp, vp, sp, rk, k, dim, vals.data_ptr() if vals is not None else None, tstep, self.lr, b1, b2,
                                               self.eps, self.weight_decay, hyper.data_ptr() if hyper is not None else None, stream),
                      "nrx_dense_adamw_rows")
        self.sink.clear()


TABLE_OPTIMIZERS = ("adam", "adagrad", "rowwise_adagrad")


class SparseDenseAdam(torch.optim.Optimizer):
    def __init__(self, sparse_params, dense_params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, fused_sink=None,
                 capturable=False, exact=False, sr_seed=0, row_maps=None, table_optimizer="adam", table_lr=None, adagrad_eps=1e-10,
                 max_grad_norm=None, norm_group=None, norm_skip=None):
        """fused_sink: an ops.SparseGradSink -> the tables are updated by FusedSparseAdam from the sink instead of
        torch.optim.SparseAdam from COO .grad tensors.  exact (with fused_sink): by ExactDenseAdamW -- the reference's dense AdamW over every
        row, weight decay included, fed from the sink.  row_maps: FusedSparseAdam's (bf16 arenas of the bound sharded step).
        table_optimizer: "adam" (the above), or "adagrad" / "rowwise_adagrad" -- FusedSparseAdagrad(rowwise=...) on the tables (needs fused_sink, not
        exact; eps = adagrad_eps); the dense parameters keep AdamW.  table_lr: the tables' step where it differs from lr (Adagrad wants a larger one
        than the dense AdamW): a scheduler's lr is forwarded to the tables scaled by table_lr / lr.
        max_grad_norm (needs fused_sink): step() clips the GLOBAL gradient norm -- the tables' row-sparse lists in the sink and the dense .grads together
        -- to it, on the device and without a host read: tables' bins (prepare), the dense part (torch._foreach_norm, squared and summed in double),
        the all-reduce of the bins over norm_group when set (the dense gradients are already all-reduced: every rank adds the same dense part),
        finish, the dense .grads and the lists scaled by clip_coef, then both updates.  norm_skip: tables this rank must not count (replicated ones
        on the ranks other than 0).  grad_norm / clip_coef: device tensors of the last clipped step."""
        sparse_params, dense_params = list(sparse_params), list(dense_params)
        if max_grad_norm is not None and fused_sink is None:
            raise ValueError("SparseDenseAdam: max_grad_norm needs fused_sink (embeddings.sparse_grad: fused | exact): the COO and dense-gradient "
                             "modes hold .grad tensors, which torch.nn.utils.clip_grad_norm_ clips")
        if table_optimizer not in TABLE_OPTIMIZERS:
            raise ValueError(f"SparseDenseAdam: table_optimizer must be one of {TABLE_OPTIMIZERS} (got {table_optimizer!r})")
        if table_optimizer != "adam" and (fused_sink is None or exact):
            raise ValueError(f"SparseDenseAdam: table_optimizer={table_optimizer!r} needs fused_sink and exact=False (the Adagrad forms drain the "
                             "row-sparse sink: embeddings.sparse_grad: fused)")
        if table_lr is not None and not (float(table_lr) > 0 and lr > 0):
            raise ValueError("SparseDenseAdam: table_lr and lr must be positive")
        self._table_scale = 1.0 if table_lr is None else float(table_lr) / float(lr)
        groups = [{"params": sparse_params, "sparse": True}]
        if dense_params:
            groups.append({"params": dense_params, "sparse": False})
        super().__init__(groups, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if exact and fused_sink is None:
            raise ValueError("SparseDenseAdam(exact=True) needs fused_sink")
        if row_maps is not None and (exact or fused_sink is None):
            raise ValueError("SparseDenseAdam: row_maps belong to FusedSparseAdam (fused_sink, not exact)")
        if fused_sink is None and any(p.dtype is torch.bfloat16 for p in sparse_params):
            raise TypeError("SparseDenseAdam: bf16 tables train only with the fused sink (torch.optim.SparseAdam needs COO gradients, "
                            "which bf16 tables do not form); use embeddings.sparse_grad: fused")
        self._sparse = (ExactDenseAdamW(fused_sink, sparse_params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable) if exact else
                        FusedSparseAdagrad(fused_sink, lr=lr * self._table_scale, eps=adagrad_eps, rowwise=table_optimizer == "rowwise_adagrad",
                                           capturable=capturable, params=sparse_params, sr_seed=sr_seed, row_maps=row_maps)
                        if table_optimizer != "adam" else
                        FusedSparseAdam(fused_sink, lr=lr * self._table_scale, betas=betas, eps=eps, capturable=capturable, params=sparse_params, sr_seed=sr_seed,
                                        row_maps=row_maps)
                        if fused_sink is not None
                        else torch.optim.SparseAdam(sparse_params, lr=lr, betas=betas, eps=eps))
        self._dense = (torch.optim.AdamW(dense_params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable)
                       if dense_params else None)
        self._dense_params = dense_params
        if fused_sink is not None:
            self._sparse._init_clip(max_grad_norm, norm_group, norm_skip)

    @property
    def max_grad_norm(self):
        return getattr(self._sparse, "max_grad_norm", None)

    def set_max_grad_norm(self, v):
        if not isinstance(self._sparse, _SinkTableOptimizer):
            raise ValueError("SparseDenseAdam: max_grad_norm needs fused_sink (embeddings.sparse_grad: fused | exact)")
        self._sparse.set_max_grad_norm(v)

    @property
    def grad_norm(self):
        return getattr(self._sparse, "grad_norm", None)

    @property
    def clip_coef(self):
        return getattr(self._sparse, "clip_coef", None)

    def _clipped_step(self):
        sp = self._sparse
        grads = [p.grad for p in self._dense_params if p.grad is not None]
        if not grads and not sp.sink.pending and sp.norm_group is None:
            return                          # (with a norm_group the step goes on: the other ranks wait in the bins' all-reduce)
        sp.prepare(device=grads[0].device if grads else None)
        extra = None
        if grads:
            extra = torch.stack(torch._foreach_norm(grads)).to(torch.float64).square_().sum().reshape(1)
        sp.finish_norm(extra)
        if grads:
            torch._foreach_mul_(grads, sp.clip_coef[0])
        sp.apply()
        if self._dense is not None:
            self._dense.step()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():         # the closure runs forward + backward
                loss = closure()
        for g in self.param_groups:           # a scheduler edits self.param_groups: forward the lr
            if g["sparse"] and isinstance(self._sparse, _SinkTableOptimizer):
                self._sparse.lr = g["lr"] * self._table_scale
                continue
            for inner in ((self._sparse,) if g["sparse"] else ((self._dense,) if self._dense else ())):
                for ig in inner.param_groups:
                    ig["lr"] = g["lr"]
        if self.max_grad_norm is not None:
            self._clipped_step()
            return loss
        self._sparse.step()
        if self._dense is not None:
            self._dense.step()
        return loss

    def zero_grad(self, set_to_none: bool = True):
        self._sparse.zero_grad(set_to_none)
        if self._dense is not None:
            self._dense.zero_grad(set_to_none)

    # ---- checkpointing (Lightning saves optimizer.state_dict()): all Adam state lives in the inner optimizers
    def state_dict(self):
        return {"sparse_dense_adam": 1,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups],
                "sparse": self._sparse.state_dict(),
                "dense": self._dense.state_dict() if self._dense is not None else None}

    def load_state_dict(self, sd):
        if "sparse_dense_adam" not in sd:
            raise ValueError("not a SparseDenseAdam state dict")
        for g, saved in zip(self.param_groups, sd["param_groups"]):
            g.update(saved)
        self._sparse.load_state_dict(sd["sparse"])
        if self._dense is not None and sd.get("dense") is not None:
            self._dense.load_state_dict(sd["dense"])
