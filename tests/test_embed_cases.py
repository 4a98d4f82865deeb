"""CPU checks of the generated embedding cases (tests/embed_cases.py): the float64 restatement against the oracle's fp32 definitions
(oracle/ref_np.py), the error scale A against the actual fp32 error, the bound's power to see one lost lookup, and the seed list's coverage."""
import numpy as np
import pytest

from oracle import ref_np as R
from tests import embed_cases as E
from news_recsys_amd._lib import NRX_BAG_MASKED_MEAN, NRX_BAG_MEAN, NRX_BAG_SUM, NRX_DENSE, NRX_FEAT_BAG_CSR, NRX_SPARSE

F32 = np.float32


def _cheap_seeds(k, styles=None):
    out = []
    for sd in E.SEEDS:
        c = E.make_case(sd)
        if (styles is None or c.style in styles) and sum(c.B * max(1, s.bag_len) * s.dim for s in c.slots) <= 1 << 20 and \
                all(t.size <= 1 << 20 for t in c.tables):
            out.append(sd)
        if len(out) == k:
            break
    return out


CPU_SEEDS = sorted(set(_cheap_seeds(6) + _cheap_seeds(2, ("many_fm",)) + _cheap_seeds(1, ("fm_wide",)) + _cheap_seeds(1, ("bf16",))))


def _oracle_fp32(case, order_seed=0):
    """The launch in numpy fp32 through the oracle's functions: embed_concat_ex for the reference's kinds (tables named per feature by
    `share`), a plain fp32 sum for NRX_BAG_SUM, wide_split, fm_split + fm_logit; the gradients by array_pool_bwd / fm_logit_bwd and an fp32
    scatter-add of the lookups in a shuffled order."""
    B = case.B
    names = [s.name for s in case.slots]
    tabs = {f"T{t}": tab for t, tab in enumerate(case.tables)}
    batch, share, sparse, dense, array = {}, {}, [], [], []
    padded = {}
    for s, x, w in zip(case.slots, case.inputs, case.weights):
        if s.kind == NRX_DENSE:
            dense.append(s.name)
            batch[s.name] = x
            continue
        share[s.name] = f"T{s.table}"
        if s.flags & NRX_FEAT_BAG_CSR:
            ids, mask = R.csr_bag_to_padded(x, w, s.bag_len)
            w = None if s.kind == NRX_BAG_MEAN else mask
        else:
            ids = x
        padded[s.name] = (ids, w)
        if s.kind == NRX_BAG_SUM:
            continue
        batch[s.name] = ids
        if s.kind == NRX_SPARSE:
            sparse.append(s.name)
        else:
            array.append(s.name)
            if s.kind == NRX_BAG_MASKED_MEAN:
                batch[s.name + "_mask"] = w
    space = R.FeatureSpace(sparse, dense, array, share)
    feats, dims, _, used = R.embed_concat_ex(space, tabs, batch, set(batch) - {k for k in batch if k.endswith("_mask")})
    vec, c0 = {}, 0
    for n, d in zip(used, dims):
        vec[n] = feats[:, c0:c0 + d]
        c0 += d
    for s in case.slots:
        if s.kind == NRX_BAG_SUM:
            ids, w = padded[s.name]
            emb = R.gather_rows(case.tables[s.table], ids)
            vec[s.name] = (emb.sum(1, dtype=F32) if w is None else (emb * w.astype(F32)[:, :, None]).sum(1, dtype=F32))
    ordered = [vec[n] for n in names]
    wide_names = {s.name for s in case.slots if s.wide_col >= 0}
    out = np.zeros((B, case.out_width), F32)
    wide = None
    if wide_names:
        wide, _ = R.wide_split(np.concatenate(ordered, 1), [v.shape[1] for v in ordered], names, wide_names)
    for s, v in zip(case.slots, ordered):
        d = v[:, 1:] if s.wide_col >= 0 else v
        out[:, s.out_col:s.out_col + d.shape[1]] = d
    fm = None
    fm_slots = [i for i, s in enumerate(case.slots) if s.fm_field]
    if case.use_fm:
        w_, v_ = R.fm_split(np.concatenate([ordered[i] for i in fm_slots], 1), [case.slots[i].dim for i in fm_slots])
        fm = R.fm_logit(w_, v_, 0.0)[:, 0]
    # gradients
    ge = {}
    for s in case.slots:
        g = np.zeros((B, s.dim), F32)
        if s.wide_col >= 0:
            g[:, 0] = case.g_wide[:, s.wide_col]
            g[:, 1:] = case.g_out[:, s.out_col:s.out_col + s.dim - 1]
        else:
            g[:] = case.g_out[:, s.out_col:s.out_col + s.dim]
        ge[s.name] = g
    if case.use_fm:
        gw, gv, _ = R.fm_logit_bwd(w_, v_, case.g_fm[:, None].astype(F32))
        for j, i in enumerate(fm_slots):
            n = case.slots[i].name
            ge[n] = ge[n] + np.concatenate([gw[:, j:j + 1], gv[:, j]], 1)
    rows_all, vals_all = [[] for _ in case.tables], [[] for _ in case.tables]
    for s in case.slots:
        if s.kind == NRX_DENSE:
            continue
        ids, w = padded[s.name]
        g = ge[s.name]
        if s.kind == NRX_SPARSE:
            per = g
        elif s.kind == NRX_BAG_SUM:
            per = np.broadcast_to(g[:, None, :], ids.shape + (s.dim,)) if w is None else g[:, None, :] * w.astype(F32)[:, :, None]
        else:
            per = R.array_pool_bwd(R.gather_rows(case.tables[s.table], ids), w if s.kind == NRX_BAG_MASKED_MEAN else None, g)
        rows_all[s.table].append(np.asarray(ids, np.int64).reshape(-1))
        vals_all[s.table].append(np.asarray(per, F32).reshape(-1, s.dim))
    rng = np.random.default_rng(order_seed)
    grads = []
    for t, tab in enumerate(case.tables):
        g = np.zeros(tab.shape, F32)
        if rows_all[t]:
            r = np.concatenate(rows_all[t])
            v = np.concatenate(vals_all[t])
            p = rng.permutation(len(r))
            np.add.at(g, r[p], v[p])                 # fp32 accumulation, one addition at a time, in a shuffled order
        g[0] = 0
        grads.append(g)
    return out, wide, fm, grads


def _check(got, ref, A, n, what):
    import torch
    ex, i = E.excess(torch.from_numpy(np.asarray(got)), ref, A, n)
    assert ex <= 0, f"{what}: element {i} beyond the bound by {ex:.3g}"


@pytest.mark.parametrize("seed", CPU_SEEDS)
def test_restatement_matches_the_oracle_within_the_bound(seed):
    """The float64 restatement against the oracle's fp32 definitions: copies bit for bit, every other element (concat, wide, fm, table
    gradients summed in a shuffled fp32 order) within C * n * 2^-24 * A -- so A bounds an actual fp32 evaluation's error."""
    import torch
    case = E.make_case(seed)
    ref = E.restate(case)
    out, wide, fm, grads = _oracle_fp32(case, order_seed=seed)
    cc = ref.copy_cols
    assert np.array_equal(out[:, cc], ref.out[:, cc].numpy().astype(F32)), case.spec()
    _check(out, ref.out, ref.A_out, ref.n_out, "concat")
    if case.wide_width:
        wc = ref.wide_copy_cols
        assert np.array_equal(wide[:, wc], ref.wide[:, wc].numpy().astype(F32)), "wide columns of single ids are copies"
        _check(wide, ref.wide, ref.A_wide, ref.n_out, "wide")
    if case.use_fm:
        _check(fm, ref.fm, ref.A_fm, ref.n_fm, "fm")
    for t, g in enumerate(grads):
        _check(g, ref.grads[t], ref.A_grads[t], ref.n_grads[t], f"grad of table {t}")
        assert float(ref.grads[t][0].abs().max()) == 0.0
        assert torch.all((ref.A_grads[t] == 0) <= (ref.grads[t] == 0))


def test_the_bound_sees_one_lost_lookup():
    """One single-valued lookup's upstream row taken out of its table gradient (what a backward that drops a lookup leaves) exceeds the bound
    wherever that row's rounding chain is short -- the bound is not a flat tolerance that swallows a lost term."""
    import torch
    hits = []
    for seed in CPU_SEEDS:
        case = E.make_case(seed)
        ref = E.restate(case)
        for s, x in zip(case.slots, case.inputs):
            x = np.asarray(x)
            if s.kind != NRX_SPARSE or ref.n_grads[s.table] > 2000 or s.wide_col >= 0 or s.fm_field or not (x != 0).any():
                continue
            b = int(np.flatnonzero(x != 0)[0])
            up = torch.from_numpy(case.g_out[b, s.out_col:s.out_col + s.dim].astype(np.float64))
            if float(up.abs().max()) < 0.05:
                continue
            g = ref.grads[s.table].clone()
            g[int(x[b])] -= up
            ex, _ = E.excess(g, ref.grads[s.table], ref.A_grads[s.table], ref.n_grads[s.table])
            assert ex > 0, (seed, s.name)
            hits.append((seed, s.name))
            break
    assert len(hits) >= 3, hits


def test_seed_list_covers_the_generator():
    cov = E.coverage()
    need = ["kind:sparse", "kind:dense", "kind:masked_mean", "kind:mean", "kind:sum", "masked_mean:non_binary", "sum:weighted", "sum:unweighted",
            "padded_bag", "csr", "csr:empty_bag", "csr:longer_than_L", "padded:empty_bag", "table_shared_by_id_and_bag", "rows:2", "rows:100k+",
            "ids:int32", "ids:int64", "ids:mixed_in_launch", "fm:on", "fm:off", "wide", "out_ld:wide", "out_ld:narrow", "col_not_multiple_of_4",
            "feats:<=64", "feats:>64", "bf16",
            "knob:PLAN_LDS=0", "knob:PLAN_LDS=1", "knob:PAD_SPLIT=0", "knob:PAD_SPLIT=1", "knob:SPARSE_PLACE=False",
            "knob:DENSE_SORTED_MIN=lowered", "knob:DENSE_LDS_MIN=lowered", "knob:PLAN_AHEAD_MIN=lowered", "knob:PAD_SPLIT_MIN=lowered",
            "path:dense_small", "path:dense_sorted", "path:dense_atomic", "path:fwd_split", "path:fm_bwd_concat", "path:csr_sink",
            "path:adam_two_groups"]
    need += [f"width:{w}" for w in E.WIDTHS]
    # batch sizes on both sides of the block (64), the small-kernel / per-table limits (4096) and a few thousand samples
    need += [f"batch:{b}" for b in (1, 63, 64, 65, 257, 2048, 2049, 4096, 4097, 9000, 30000)]
    missing = [k for k in need if k not in cov]
    assert not missing, missing
    assert all(E.make_case(s).lookups() <= E.MAX_LOOKUPS for s in E.SEEDS)


def test_cases_are_reproducible_and_printable():
    a, b = E.make_case(7), E.make_case(7)
    assert a.spec() == b.spec()
    assert all(np.array_equal(x, y) for x, y in zip(a.inputs, b.inputs))
    assert all(np.array_equal(x, y) for x, y in zip(a.tables, b.tables))
    assert "seed 7" in a.spec()
