"""float64 numpy restatements of the row-optimizer kernels of nrx_row_optim.hip (include/nrx_embed.h), and the hand-made key lists their tests run on.
No GPU, no torch: tests/test_row_optim_ref.py holds these against torch's float64 optimizers on the CPU, tests/test_row_optimizer_kernels_gpu.py
holds the kernels against these.

  adam_rows        nrx_sparse_adam_step (and the fp32 side of the bf16 forms): torch.optim.SparseAdam's rule on the live keys of a list
  adamw_all_rows   nrx_dense_adamw_rows: torch's single-tensor AdamW over every row, a zero gradient where a row has no slot
  mark_slots       nrx_rows_mark: which key of a list owns which (table, row)
  merge_lists      nrx_rows_mark + nrx_rows_merge: list B folded into the marked list A, in fp32 (one addition per shared row: exact)

Hyperparameters enter as the float32 values the C entries receive: beta -> float(np.float32(beta)), and 1 - beta is formed in float64 from that
(the difference is exact in fp32 for betas in [0.5, 1), so it is the kernel's `1.0f - beta`); the step size, eps, lr and lr * weight_decay are
rounded to float32 first.  With float64 hyperparameters `1 - 0.999` alone is 1.3e-5 (relative) away from the kernel's `1.0f - 0.999f`."""
import numpy as np

BIG = np.iinfo(np.int64).max
ROW_MASK = (1 << 40) - 1


def f32(x):
    """The double a C `float` argument holds."""
    return float(np.float32(x))


def split_key(k):
    k = int(k)
    return k >> 40, k & ROW_MASK


def key_list(n, rng, rows=40):
    """n entries over three tables of `rows` rows: real keys (consecutive rows of table 1 first: one 128-byte line of a per-row state is written by
    several lane groups), -1 and INT64_MAX fillers interleaved, a key with row 0, a key with table 3 (>= n_tables).  From n >= 3 on the LAST entry is a
    real key that a device-side count of n - 1 must hide.  Returns (keys int64 [n], that count or None).  There are 2.5 * (rows - 1) real keys; a
    longer list is filled up with -1."""
    real = [(1 << 40) | r for r in range(1, rows)] + [(0 << 40) | r for r in range(rows - 1, 0, -2)] + [(2 << 40) | int(r) for r in rng.permutation(np.arange(1, rows))]
    last = real.pop(3)                       # (table 1, row 4): in the middle of the run of consecutive rows
    keys, it = [], iter(real)
    for i in range(n):
        if n >= 3 and i == n - 1:
            keys.append(last)
        elif n > 1 and i % 5 == 1:
            keys.append(-1)
        elif i % 7 == 3:
            keys.append(BIG)
        elif i == 2:
            keys.append((1 << 40) | 0)       # the padding row
        elif i == 4:
            keys.append((3 << 40) | 5)       # a table the call does not have
        else:
            keys.append(next(it, -1))
    return np.array(keys, dtype=np.int64), (n - 1 if n >= 3 else None)


def rows_for(n):
    """The smallest table (rows, at least 6) whose key_list of n entries runs out of no real keys: the list then names rows of all three tables."""
    need = 1 + sum(1 for i in range(n) if not ((n >= 3 and i == n - 1) or (n > 1 and i % 5 == 1) or i % 7 == 3 or i in (2, 4)))
    rows = 6
    while (rows - 1) + rows // 2 + (rows - 1) < need:
        rows += 1
    return rows


def is_live(k, n_tables):
    """nrx_sparse_adam_step / nrx_sparse_adagrad_step: not negative, not INT64_MAX, a table of the call, not the padding row."""
    t, r = split_key(k)
    return k >= 0 and k != BIG and t < n_tables and r != 0


def adam_rows(w, m, v, keys, g, n_tables, step_size, beta1, beta2, eps, decay):
    """w, m, v: per table float64 [rows, dim]; keys [n] with g [n, dim] (entries past a device-side count already cut off by the caller).
    For every live key:  m += (g - m)(1 - beta1);  v += (g g - v)(1 - beta2);  w -= w * decay;  w -= step_size * m / (sqrt(v) + eps).
    Returns (w, m, v, named): new arrays and per table the set of rows a live key names."""
    w, m, v = [x.astype(np.float64) for x in w], [x.astype(np.float64) for x in m], [x.astype(np.float64) for x in v]
    ss, eps, decay = f32(step_size), f32(eps), f32(decay)
    omb1, omb2 = 1.0 - f32(beta1), 1.0 - f32(beta2)
    named = [set() for _ in w]
    for i, k in enumerate(keys):
        if not is_live(k, n_tables):
            continue
        t, r = split_key(k)
        assert r not in named[t], "a unique-key list names a row once"
        gi = np.asarray(g[i], dtype=np.float64)
        m[t][r] = m[t][r] + (gi - m[t][r]) * omb1
        v[t][r] = v[t][r] + (gi * gi - v[t][r]) * omb2
        wd = w[t][r] - w[t][r] * decay
        w[t][r] = wd - ss * (m[t][r] / (np.sqrt(v[t][r]) + eps))
        named[t].add(r)
    return w, m, v, named


def mark_slots(keys, rows, n_tables):
    """nrx_rows_mark: per table {row: i} for every key i = (t << 40 | row) with t < n_tables and 0 < row < rows[t]."""
    maps = [dict() for _ in range(n_tables)]
    for i, k in enumerate(keys):
        t, r = split_key(k)
        if k < 0 or t >= n_tables or r == 0 or r >= rows[t]:
            continue
        assert r not in maps[t], "a unique-key list names a row once"
        maps[t][r] = i
    return maps


def adamw_all_rows(w, m, v, slot_grads, step, lr, beta1, beta2, eps, weight_decay):
    """torch.optim.AdamW's single-tensor step `step` (>= 1) over EVERY row of every table, row 0 included.  slot_grads: per table {row: gradient [dim]};
    a row that is not in it takes a zero gradient (it still decays, and its moments shrink).  Returns the new (w, m, v)."""
    lr, b1, b2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    keep = 1.0 - f32(lr * f32(weight_decay))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    out_w, out_m, out_v = [], [], []
    for t in range(len(w)):
        wt, mt, vt = np.asarray(w[t], np.float64), np.asarray(m[t], np.float64), np.asarray(v[t], np.float64)
        g = np.zeros_like(wt)
        for r, gr in slot_grads[t].items():
            g[r] = gr
        wt = wt * keep                                           # param.mul_(1 - lr * weight_decay)
        mt = mt + (g - mt) * (1.0 - b1)                          # exp_avg.lerp_(grad, 1 - beta1)
        vt = vt * b2 + g * g * (1.0 - b2)                        # exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        denom = np.sqrt(vt) / np.sqrt(bc2) + eps
        out_w.append(wt - (lr / bc1) * (mt / denom))             # param.addcdiv_(exp_avg, denom, value=-lr / bias_correction1)
        out_m.append(mt)
        out_v.append(vt)
    return out_w, out_m, out_v


def merge_lists(keys_a, vals_a, keys_b, vals_b, rows, n_tables):
    """List A marked (mark_slots), then every pair of B whose row A holds is added to A's row in fp32 and its key becomes -1; the rest of B and
    every other row of A stay.  The lists are the entries a device-side count leaves visible.  Returns (new keys_b, new vals_a float32)."""
    maps = mark_slots(keys_a, rows, n_tables)
    keys_b, vals_a = np.array(keys_b, dtype=np.int64), np.array(vals_a, dtype=np.float32)
    vals_b = np.asarray(vals_b, dtype=np.float32)
    for j, k in enumerate(keys_b.tolist()):
        t, r = split_key(k)
        if k < 0 or t >= n_tables or r == 0 or r >= rows[t] or r not in maps[t]:
            continue
        sa = maps[t][r]
        vals_a[sa] = vals_a[sa] + vals_b[j]                      # one fp32 addition per element
        keys_b[j] = -1
    return keys_b, vals_a
