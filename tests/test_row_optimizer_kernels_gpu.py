"""The row-optimizer kernels of nrx_row_optim.hip ALONE, through ctypes, against the float64 restatements of tests/row_optim_ref.py (themselves held to
torch's float64 optimizers by tests/test_row_optim_ref.py):

  nrx_sparse_adam_step                 every lane-group width, the dim > 256 column loop, the float4 and the element-by-element form, both moment
                                       layouts ([rows, 2, dim] and separate arrays), lists of one entry up to three blocks, a device-side count
  nrx_sparse_adam_step_bf16 / _rows    moments = the fp32 call's bits, patterns = tests/sr_bf16_ref.py's rounding of the fp32 call's weights: every
                                       lane-group width, lists of one to five entries, the element-by-element form at a four-column dim
  nrx_rows_mark + nrx_dense_adamw_rows several blocks per table, a one-row table, a ragged last block, two steps, hyper_dev
  nrx_rows_mark + nrx_rows_merge       bit for bit (one fp32 addition per shared row), then the whole merged step against float64
  nrx_rows_to_dense                    store and accumulate forms on long lists and on lists shorter than a lane group's four entries

Every buffer a kernel may write sits inside a larger buffer of guard bytes that must come back untouched, and every row no live key names must keep
its bits (compared as integers) -- the padding row, the row of the entry past the device-side count, the neighbours of a named row.

Shapes.  rows_per_block(dim) = 4 * (256 >> ql) rows (ql as the entry points compute it: 1024 rows at dim <= 4, 16 at dim > 128); a "long" list has
2 * rows_per_block + 5 entries: three blocks, the last one ragged.  Tables have just enough rows to supply that many distinct keys.

Tolerances.  RTOL / ATOL = 2e-5 / 2e-6, tests/test_sparse_adagrad_gpu.py's values for an fp32 update against float64.  Inputs: w, g ~ N(0, 1),
m ~ 0.3 N(0, 1), v in [0.1, 1.1] (so m / (sqrt(v) + eps) is well conditioned); a numpy float32 emulation of one Adam and one AdamW step on such
inputs, with float32-rounded hyperparameters, stays under 3 % of that tolerance for w, m and v, which leaves room for the GPU's fma contraction."""
import ctypes as C

import numpy as np
import pytest
import torch

from news_recsys_amd import _lib, ops
from tests import row_optim_ref as R
from tests import sr_bf16_ref as SR
from tests.test_sparse_adagrad_gpu import ATOL, RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADB = 256                      # guard bytes on either side (a multiple of 16: the payload keeps the allocator's alignment)
GUARD = 0xA5
B1, B2, EPS = 0.9, 0.999, 1e-8
LR, WD, STEP = 0.05, 0.01, 3
SS = LR * np.sqrt(1 - B2 ** STEP) / (1 - B1 ** STEP)        # SparseAdam's step size at step 3
DECAY = LR * WD
ALL_DIMS = [1, 4, 6, 8, 16, 32, 64, 112, 128, 320, 516]


def rows_per_block(dim):
    ql = 0
    while (4 << ql) < dim and ql < 6:
        ql += 1
    return 4 * (256 >> ql)


def long_n(dim):
    return 2 * rows_per_block(dim) + 5


def test_rows_per_block_is_the_entry_points_arithmetic():
    assert [rows_per_block(d) for d in (1, 4, 5, 8, 9, 16, 32, 64, 112, 128, 129, 320, 516)] == [1024, 1024, 512, 512, 256, 256, 128, 64, 32, 32, 16, 16, 16]
    assert long_n(1) == 2053 and long_n(516) == 37


class Guarded:
    """A numpy array on the device inside a larger buffer of guard bytes: PADB before and after, and `off` more in front (a misaligned start)."""

    def __init__(self, arr, off=0):
        arr = np.ascontiguousarray(arr)
        self.shape, self.dtype, self.nbytes, self.lo = arr.shape, arr.dtype, arr.nbytes, PADB + off
        self.buf = torch.full((self.lo + self.nbytes + PADB,), GUARD, dtype=torch.uint8, device=DEV)
        self.buf[self.lo:self.lo + self.nbytes] = torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()).to(DEV)
        self.ptr = self.buf.data_ptr() + self.lo
        assert self.buf.data_ptr() % 16 == 0 and self.ptr % 16 == off % 16

    def get(self):
        return self.buf[self.lo:self.lo + self.nbytes].cpu().numpy().copy().view(self.dtype).reshape(self.shape)

    def intact(self):
        return bool((self.buf[:self.lo] == GUARD).all()) and bool((self.buf[self.lo + self.nbytes:] == GUARD).all())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _ptrs(ps):
    return (C.c_void_p * len(ps))(*ps)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _close(got, want):
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=RTOL, atol=ATOL)


def _bf16_values(x):
    """float32 values a bf16 holds exactly (the low 16 bits cut)."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


# ------------------------------------------------------------------------------------------------ nrx_sparse_adam_step and its bf16 forms
class AdamCase:
    """Three tables of rows_for(n) rows with their moments, tests/row_optim_ref.py's key list of n entries and its gradients; the inputs depend on
    (seed, dim, n) only -- not on the layout, the table type or the alignment -- so two cases can be compared bit for bit.
    inter: the moments of table t are ONE [rows, 2, dim] array (exp_avg_sq = exp_avg + dim) instead of two arrays.
    mis: "g" -- the gradients start 4 bytes off a 16-byte boundary; "m" -- table 1's exp_avg_sq does (separate arrays)."""
    MAPS = [(3, -1), (1, 0), (2, 5)]

    def __init__(self, dim, n, inter, bf16_values=False, store_bf16=False, mis=None, seed=1):
        rng = np.random.default_rng([seed, dim, n])
        self.dim, self.n, self.inter, self.store_bf16 = dim, n, inter, store_bf16
        self.rows = R.rows_for(n)
        self.keys, self.n_dev = R.key_list(n, rng, self.rows)
        self.g = rng.standard_normal((n, dim)).astype(np.float32)
        self.w0 = [rng.standard_normal((self.rows, dim)).astype(np.float32) for _ in range(3)]
        self.m0 = [(0.3 * rng.standard_normal((self.rows, dim))).astype(np.float32) for _ in range(3)]
        self.v0 = [(0.1 + rng.random((self.rows, dim))).astype(np.float32) for _ in range(3)]
        if bf16_values or store_bf16:
            self.w0 = [_bf16_values(x) for x in self.w0]
        self.d_keys, self.d_g = Guarded(self.keys), Guarded(self.g, off=4 if mis == "g" else 0)
        self.d_n = Guarded(np.array([self.n_dev], dtype=np.int64)) if self.n_dev is not None else None
        self.d_w = [Guarded((x.view(np.uint32) >> np.uint32(16)).astype(np.uint16) if store_bf16 else x) for x in self.w0]
        if inter:
            assert mis != "m"
            self.d_mv = [Guarded(np.stack([m, v], axis=1)) for m, v in zip(self.m0, self.v0)]
            self.pm, self.pv = [d.ptr for d in self.d_mv], [d.ptr + 4 * dim for d in self.d_mv]
            self.guards = [self.d_keys, self.d_g] + self.d_w + self.d_mv
        else:
            self.d_m = [Guarded(m) for m in self.m0]
            self.d_v = [Guarded(v, off=4 if mis == "m" and t == 1 else 0) for t, v in enumerate(self.v0)]
            self.pm, self.pv = [d.ptr for d in self.d_m], [d.ptr for d in self.d_v]
            self.guards = [self.d_keys, self.d_g] + self.d_w + self.d_m + self.d_v
        if mis is not None:                 # one 4-byte-off pointer: the entry point must take the element-by-element form
            assert sum(p % 16 == 4 for p in [self.d_g.ptr] + self.pm + self.pv) == 1

    def run(self, fn="nrx_sparse_adam_step", ss=SS, ss_dev=None, seed=0, step=0, step_dev=None, maps=None):
        lib = _lib.load()
        args = [_ptrs([d.ptr for d in self.d_w]), _ptrs(self.pm), _ptrs(self.pv), 3, self.dim, self.d_keys.ptr, self.d_g.ptr, self.n,
                self.d_n.ptr if self.d_n is not None else None, ss, ss_dev.ptr if ss_dev is not None else None, B1, B2, EPS, DECAY]
        if fn != "nrx_sparse_adam_step":
            assert self.store_bf16
            args += [seed, step, step_dev.ptr if step_dev is not None else None]
        if fn == "nrx_sparse_adam_step_bf16_rows":
            args += [None, None] if maps is None else [(C.c_int64 * 3)(*[a for a, _ in maps]), (C.c_int64 * 3)(*[b for _, b in maps])]
        else:
            assert maps is None
        ops.check(getattr(lib, fn)(*args, _stream()), fn)
        torch.cuda.synchronize()
        return self

    def read(self):
        w = [d.get() for d in self.d_w]
        if self.inter:
            mv = [d.get() for d in self.d_mv]
            return w, [np.ascontiguousarray(x[:, 0]) for x in mv], [np.ascontiguousarray(x[:, 1]) for x in mv]
        return w, [d.get() for d in self.d_m], [d.get() for d in self.d_v]

    def named(self):
        live = self.keys if self.n_dev is None else self.keys[:self.n_dev]
        named = [set() for _ in range(3)]
        for k in live:
            if R.is_live(k, 3):
                named[int(k) >> 40].add(int(k) & R.ROW_MASK)
        return named

    def check_guards_and_inputs(self):
        assert all(d.intact() for d in self.guards), "a word next to a buffer moved"
        assert _same(self.d_keys.get(), self.keys) and _same(self.d_g.get(), self.g)

    def check_against_float64(self):
        live_n = self.n if self.n_dev is None else self.n_dev
        W, M, V, named = R.adam_rows(self.w0, self.m0, self.v0, self.keys[:live_n], self.g[:live_n], 3, SS, B1, B2, EPS, DECAY)
        assert named == self.named()
        n_named = sum(len(x) for x in named)
        assert n_named >= (self.n // 2 if self.n >= 37 else 1)
        assert self.n < 37 or all(len(x) >= 3 for x in named)          # a long list names rows of all three tables
        if self.n_dev is not None:            # the entry past the device-side count is live, and names a row no visible entry names
            t, r = R.split_key(self.keys[-1])
            assert R.is_live(self.keys[-1], 3) and r not in named[t]
        got_w, got_m, got_v = self.read()
        for t in range(3):
            rows = np.array(sorted(named[t]), dtype=np.int64)
            rest = np.ones(self.rows, bool)
            rest[rows] = False
            assert rest[0]
            for what, got, was in (("table", got_w, self.w0), ("exp_avg", got_m, self.m0), ("exp_avg_sq", got_v, self.v0)):
                assert _same(got[t][rest], was[t][rest]), (t, f"{what}: rows that no live key names moved")
            if rows.size:
                _close(got_w[t][rows], W[t][rows])
                _close(got_m[t][rows], M[t][rows])
                _close(got_v[t][rows], V[t][rows])
                for got, was in ((got_w, self.w0), (got_m, self.m0), (got_v, self.v0)):
                    assert (_bits(got[t][rows]) != _bits(was[t][rows])).any(axis=1).all(), (t, "a named row did not move")
        self.check_guards_and_inputs()


ADAM_CASES = [(d, "long", i) for d in ALL_DIMS for i in (True, False)] + [(d, n, i) for d in (6, 16, 320) for n in (1, 3, 4, 5) for i in (True, False)]


@pytest.mark.parametrize("dim,n,inter", ADAM_CASES, ids=[f"d{d}-n{n}-{'inter' if i else 'sep'}" for d, n, i in ADAM_CASES])
def test_sparse_adam_step_matches_float64_and_leaves_every_other_row_alone(dim, n, inter):
    n = long_n(dim) if n == "long" else n
    AdamCase(dim, n, inter).run().check_against_float64()


@pytest.mark.parametrize("mis", ["g", "m"])
@pytest.mark.parametrize("dim", [16, 320])
def test_sparse_adam_step_on_misaligned_buffers_matches_float64(dim, mis):
    """The element-by-element form (one pointer 4 bytes off a 16-byte boundary): against float64 at the same tolerance, not against the float4 form's
    bits -- the rule is not written with explicit fma, so the two forms may contract differently."""
    AdamCase(dim, long_n(dim), inter=(mis == "g"), mis=mis).run().check_against_float64()


@pytest.mark.parametrize("dim", [6, 16])
def test_sparse_adam_step_size_on_the_device_overrides_the_host_value(dim):
    a = AdamCase(dim, long_n(dim), True).run()
    b = AdamCase(dim, long_n(dim), True)
    ss_dev = Guarded(np.array([SS], dtype=np.float32))
    b.run(ss=0.0, ss_dev=ss_dev)
    assert not _same(a.read()[0][1], a.w0[1])
    for x, y in zip(a.read(), b.read()):
        assert all(_same(p, q) for p, q in zip(x, y))
    assert ss_dev.intact() and _same(ss_dev.get(), np.array([SS], dtype=np.float32))
    b.check_guards_and_inputs()


def _bf16_adam_is_the_fp32_call_rounded(dim, n, inter, maps, mis=None):
    """The fp32 call on the widened table is held to float64 (same inputs up to the widening, same `mis`: both calls take the same form of the
    kernel); the bf16 call must leave its moments bit for bit and sr_round of its weights, the rounding stream hashed on the MAPPED row.
    A long list (n >= 37) names at least three rows of every table; a short one names what check_against_float64 finds from the reference alone,
    at least one row."""
    seed, step = 0xDEADBEEF12345, 7
    mapped = maps is not None
    ref = AdamCase(dim, n, inter, bf16_values=True, mis=mis).run()
    ref.check_against_float64()
    w32, m32, v32 = ref.read()
    first = AdamCase(dim, n, inter, store_bf16=True, mis=mis)
    step_dev = Guarded(np.array([step], dtype=np.int64))
    if mapped:
        first.run("nrx_sparse_adam_step_bf16_rows", seed=seed, step=step, maps=maps)
    else:
        first.run("nrx_sparse_adam_step_bf16", seed=seed, step=step)
    # the device-side step overrides a wrong host step; the row-mapped entry with NULL maps is the identity
    second = AdamCase(dim, n, inter, store_bf16=True, mis=mis).run("nrx_sparse_adam_step_bf16_rows", seed=seed, step=step + 1000, step_dev=step_dev, maps=maps)
    named, cols = ref.named(), np.arange(dim)
    assert sum(len(x) for x in named) >= 1
    for case in (first, second):
        got_w, got_m, got_v = case.read()
        for t in range(3):
            assert _same(got_m[t], m32[t]) and _same(got_v[t], v32[t]), (t, "moments != the fp32 call's on the widened table")
            rows = np.array(sorted(named[t]), dtype=np.int64)
            rest = np.ones(case.rows, bool)
            rest[rows] = False
            before = (case.w0[t].view(np.uint32) >> np.uint32(16)).astype(np.uint16)
            assert got_w[t].dtype == np.uint16 and np.array_equal(got_w[t][rest], before[rest]), (t, "bf16 rows that no live key names moved")
            mul, add = maps[t] if mapped else (1, 0)
            want = SR.sr_round(w32[t][rows], SR.sr_bits(seed, step, t, rows * mul + add, cols))
            assert SR.matches(got_w[t][rows], want), f"table {t}: bf16 patterns != (f32_bits(w_new) + bits16) >> 16"
            assert rows.size >= (3 if n >= 37 else 0)
            if rows.size:
                assert not np.array_equal(got_w[t][rows], before[rows])
            # (so the test sees the map: the unmapped stream gives other patterns -- asked where there are enough elements, 256 and more, that
            # two streams cannot round them all alike: every table of a long list)
            if mapped and (mul, add) != (1, 0) and rows.size * dim >= 256:
                assert not SR.matches(got_w[t][rows], SR.sr_round(w32[t][rows], SR.sr_bits(seed, step, t, rows, cols)))
            assert n < 37 or not mapped or t == 1 or rows.size * dim >= 256
        case.check_guards_and_inputs()
    assert step_dev.intact()


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("inter", [True, False])
@pytest.mark.parametrize("dim", [1, 6, 32, 112, 320])
def test_sparse_adam_bf16_is_the_fp32_call_rounded_by_the_restated_stream(dim, inter, mapped):
    _bf16_adam_is_the_fp32_call_rounded(dim, long_n(dim), inter, AdamCase.MAPS if mapped else None)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("n", [1, 3, 4, 5])
@pytest.mark.parametrize("dim", [6, 16, 320])
def test_sparse_adam_bf16_on_short_lists(dim, n, mapped):
    """A partial group of four entries in the element-by-element (dim 6) and the four-column body; at n = 5 the last lane group holds one key.  A
    short list names rows of table 1 only, so its map is not the identity here."""
    _bf16_adam_is_the_fp32_call_rounded(dim, n, False, [(3, -1), (2, 7), (2, 5)] if mapped else None)


@pytest.mark.parametrize("dim", [4, 8, 16, 64, 128, 516])
def test_sparse_adam_bf16_at_the_remaining_lane_group_widths(dim):
    """With the dims of the test above: 1, 2, 4, ... 64 lanes per row, and at 516 a second trip of the column loop."""
    _bf16_adam_is_the_fp32_call_rounded(dim, long_n(dim), True, None)


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("dim", [16, 320])
def test_sparse_adam_bf16_on_misaligned_gradients_takes_the_element_form_of_the_fp32_call(dim, mapped):
    """Gradients 4 bytes off a 16-byte boundary, in the fp32 call too: both take the element-by-element form at a dim the four-column form serves."""
    _bf16_adam_is_the_fp32_call_rounded(dim, long_n(dim), True, AdamCase.MAPS if mapped else None, mis="g")


# ------------------------------------------------------------------------------------------------ nrx_rows_mark + nrx_dense_adamw_rows
def _mark(keys_ptr, n, n_dev_ptr, maps, rows, unmark=0):
    lib = _lib.load()
    ops.check(lib.nrx_rows_mark(keys_ptr, n, n_dev_ptr, _ptrs([m.ptr for m in maps]), (C.c_int64 * len(rows))(*rows), len(rows), unmark, _stream()),
              "nrx_rows_mark")
    torch.cuda.synchronize()


def _adamw_keys(rows, rpb, rng):
    """A third of every table's rows (the first, the last and the rows around the block boundaries among them), fillers, the padding row of two
    tables, rows past the end of their table, a table the call does not have -- shuffled -- and a last live entry the device-side count hides."""
    ks = []
    for t, r in enumerate(rows):
        if r > 1:
            pick = set(int(x) for x in rng.choice(np.arange(1, r), size=max(1, (r - 1) // 3), replace=False))
            pick |= {x for x in (1, rpb - 1, rpb, rpb + 1, 2 * rpb - 1, 2 * rpb, r - 1) if 1 <= x < r}
            if t == 0:
                pick.discard(2)
            ks += [(t << 40) | x for x in sorted(pick)]
    ks += [-1, -1, R.BIG, (0 << 40) | 0, (1 << 40) | 0, (1 << 40) | 1, (0 << 40) | rows[0], (2 << 40) | (rows[2] + 7), (3 << 40) | 1]
    ks = [ks[i] for i in rng.permutation(len(ks))] + [(0 << 40) | 2]
    return np.array(ks, dtype=np.int64), len(ks) - 1


class AdamWCase:
    def __init__(self, dim, rows, seed=5, mis=False):
        rng = self.rng = np.random.default_rng([seed, dim])
        self.dim, self.rows = dim, rows
        self.w = [rng.standard_normal((r, dim)).astype(np.float32) for r in rows]
        self.m = [(0.3 * rng.standard_normal((r, dim))).astype(np.float32) for r in rows]
        self.v = [(0.1 + rng.random((r, dim))).astype(np.float32) for r in rows]
        self.d_w = [Guarded(x) for x in self.w]
        self.d_m = [Guarded(x, off=4 if mis and t == 0 else 0) for t, x in enumerate(self.m)]
        self.d_v = [Guarded(x) for x in self.v]
        self.d_map = [Guarded(np.full((r,), -1, dtype=np.int32)) for r in rows]
        self.W, self.M, self.V = self.w, self.m, self.v          # the float64 restatement's state

    def step(self, step, keys=None, n_dev=None, g=None, lr=LR, wd=WD, restate=True, hyper=None, host_lr=None, host_step=None):
        """mark (when there is a list) + one AdamW step; the float64 state moves along unless restate is False."""
        lib = _lib.load()
        k = len(self.rows)
        d_g = None
        slots = [dict() for _ in self.rows]
        if keys is not None:
            d_keys, d_g, d_n = Guarded(keys), Guarded(g), Guarded(np.array([n_dev], dtype=np.int64))
            _mark(d_keys.ptr, keys.size, d_n.ptr, self.d_map, self.rows)
            slots = R.mark_slots(keys[:n_dev], self.rows, k)
            for t in range(k):                # the maps hold exactly the visible list's slots
                want = np.full((self.rows[t],), -1, dtype=np.int32)
                for r, i in slots[t].items():
                    want[r] = i
                assert np.array_equal(self.d_map[t].get(), want), (t, "nrx_rows_mark")
            assert d_keys.intact() and _same(d_keys.get(), keys)
        ops.check(lib.nrx_dense_adamw_rows(_ptrs([d.ptr for d in self.d_w]), _ptrs([d.ptr for d in self.d_m]), _ptrs([d.ptr for d in self.d_v]),
                                           _ptrs([d.ptr for d in self.d_map]), (C.c_int64 * k)(*self.rows), k, self.dim, d_g.ptr if d_g is not None else None,
                                           step if host_step is None else host_step, lr if host_lr is None else host_lr, B1, B2, EPS, wd,
                                           hyper.ptr if hyper is not None else None, _stream()), "nrx_dense_adamw_rows")
        torch.cuda.synchronize()
        if d_g is not None:
            assert d_g.intact() and _same(d_g.get(), g)
        if restate:
            self.W, self.M, self.V = R.adamw_all_rows(self.W, self.M, self.V, [{r: g[i] for r, i in s.items()} for s in slots], step, lr, B1, B2, EPS, wd)
        return slots

    def read(self):
        return [d.get() for d in self.d_w], [d.get() for d in self.d_m], [d.get() for d in self.d_v]

    def check(self):
        got = self.read()
        for t in range(len(self.rows)):
            for what, x, want in zip(("table", "exp_avg", "exp_avg_sq"), got, (self.W, self.M, self.V)):
                np.testing.assert_allclose(x[t].astype(np.float64), want[t], rtol=RTOL, atol=ATOL, err_msg=f"table {t}: {what}")
            assert (self.d_map[t].get() == -1).all(), (t, "the slot map is all -1 again after the step")
        for d in self.d_w + self.d_m + self.d_v + self.d_map:
            assert d.intact(), "a word next to a table, a moment or a map moved"
        return got


def _adamw_shape(dim):
    rpb = rows_per_block(dim)
    return rpb, [2 * rpb + 3, 1, rpb + 1]          # several blocks with a ragged last one; a one-row table; one row past a block boundary


@pytest.mark.parametrize("dim,mis", [(d, False) for d in (1, 6, 16, 32, 112, 320)] + [(16, True)])
def test_dense_adamw_rows_matches_float64_over_two_steps(dim, mis):
    """mis: table 0's exp_avg starts 4 bytes off a 16-byte boundary -- the element-by-element form."""
    rpb, rows = _adamw_shape(dim)
    case = AdamWCase(dim, rows, mis=mis)
    for step in (1, 2):
        keys, n_dev = _adamw_keys(rows, rpb, case.rng)
        g = case.rng.standard_normal((keys.size, dim)).astype(np.float32)
        before = case.read()
        slots = case.step(step, keys, n_dev, g)
        assert len(slots[0]) >= rpb // 2 and not slots[1] and len(slots[2]) >= rpb // 3 and 2 not in slots[0] and (rows[0] - 1) in slots[0]
        got = case.check()
        for t, r in enumerate(rows):          # rows without a slot (row 0 among them) decay, and their moments shrink
            rest = np.array(sorted(set(range(r)) - set(slots[t])), dtype=np.int64)
            assert 0 in rest
            assert (np.abs(got[1][t][rest]) < np.abs(before[1][t][rest])).all() and (got[2][t][rest] < before[2][t][rest]).all()
            assert (got[0][t][rest] != before[0][t][rest]).all()


def test_dense_adamw_rows_without_gradients_is_pure_decay():
    dim = 16
    rpb, rows = _adamw_shape(dim)
    case = AdamWCase(dim, rows, seed=6)
    before = case.read()
    case.step(1)                              # grads == NULL, nothing marked
    got = case.check()
    keep = 1.0 - R.f32(R.f32(LR) * R.f32(WD))
    for t in range(3):
        w, m, v = (x[t].astype(np.float64) for x in before)          # step 1 on a zero gradient, in closed form
        _close(got[0][t], w * keep - (R.f32(LR) / (1 - R.f32(B1))) * (m * R.f32(B1)) / (np.sqrt(v * R.f32(B2)) / np.sqrt(1 - R.f32(B2)) + R.f32(EPS)))
        _close(got[1][t], m * R.f32(B1))
        _close(got[2][t], v * R.f32(B2))


@pytest.mark.parametrize("wd,wrong_lr", [(WD, False), (0.0, True)], ids=["wrong-step", "wrong-step-and-lr"])
@pytest.mark.parametrize("dim", [6, 16])
def test_dense_adamw_rows_hyper_dev_overrides_the_host_step_and_lr(dim, wd, wrong_lr):
    """hyper_dev = {lr / bias_correction1, 1 / sqrt(bias_correction2)} is read in the place of what the entry point derives from `step` and `lr`.
    The decoupled decay 1 - lr * weight_decay stays a host value (include/nrx_embed.h), so the host lr may be wrong only where weight_decay is 0."""
    rpb, rows = _adamw_shape(dim)
    step = 2
    a, b = AdamWCase(dim, rows, seed=7), AdamWCase(dim, rows, seed=7)
    keys, n_dev = _adamw_keys(rows, rpb, a.rng)
    g = a.rng.standard_normal((keys.size, dim)).astype(np.float32)
    a.step(step, keys, n_dev, g, wd=wd)
    a.check()
    b1, b2 = R.f32(B1), R.f32(B2)
    hyper = Guarded(np.array([R.f32(LR) / (1.0 - b1 ** step), 1.0 / np.sqrt(1.0 - b2 ** step)], dtype=np.float32))
    b.step(step, keys, n_dev, g, wd=wd, restate=False, hyper=hyper, host_step=1000, host_lr=7.0 if wrong_lr else None)
    for x, y in zip(a.read(), b.read()):
        assert all(_same(p, q) for p, q in zip(x, y))
    assert hyper.intact() and all((d.get() == -1).all() and d.intact() for d in b.d_map)


# ------------------------------------------------------------------------------------------------ nrx_rows_mark + nrx_rows_merge
MERGE_ROWS = [50, 30, 40]       # what nrx_rows_mark / nrx_rows_merge are told
ADAM_ROWS = 104                 # the tables of the merged step: nrx_sparse_adam_step takes no row counts, so they hold every row the lists name


def _merge_lists(rng):
    """A: 45 entries (fillers, the padding row, a row past its table, table 3 among them; the last, (0, 9), hidden by a count of 44).
    B: 90 entries -- rows A holds, rows A lacks, A's hidden row, both fillers, row 0, table 3, a row past its table -- shuffled, and a last SHARED
    entry hidden by a count of 89."""
    a_rows = [[1, 2, 3, 5, 8, 13, 21, 34, 49, 48, 20, 22], list(range(1, 30, 2)), [39, 1, 7, 6, 5, 30]]
    ka = [(t << 40) | r for t in range(3) for r in a_rows[t]] + [-1, -1, R.BIG, (0 << 40) | 0, (1 << 40) | 30, (2 << 40) | 99, (3 << 40) | 4]
    ka = [ka[i] for i in rng.permutation(len(ka))]
    ka += [-1] * (44 - len(ka)) + [(0 << 40) | 9]
    shared = [(0, r) for r in (1, 3, 8, 21, 49, 20)] + [(1, r) for r in (1, 5, 9, 29, 15)] + [(2, r) for r in (39, 7, 30)]
    lacks = [(0, r) for r in (4, 6, 7, 10, 11, 12, 47, 9)] + [(1, r) for r in range(2, 30, 2)] + [(2, r) for r in range(8, 30)]
    kb = [(t << 40) | r for t, r in shared + lacks] + [-1] * 6 + [R.BIG] * 3 + [(0 << 40) | 0, (2 << 40) | 0, (3 << 40) | 1, (3 << 40) | 4,
                                                                               (1 << 40) | 31, (0 << 40) | 50, (2 << 40) | 40]
    kb = [kb[i] for i in rng.permutation(len(kb))]
    kb += [-1] * (89 - len(kb)) + [(0 << 40) | 2]
    assert len(ka) == 45 and len(kb) == 90 and len(shared) == 14
    return np.array(ka, dtype=np.int64), 44, np.array(kb, dtype=np.int64), 89


@pytest.mark.parametrize("dim", [1, 6, 16, 17, 32, 320])
def test_rows_mark_and_merge_fold_list_b_into_list_a_bit_for_bit(dim):
    lib = _lib.load()
    rng = np.random.default_rng([8, dim])
    ka, na, kb, nb = _merge_lists(rng)
    va, vb = rng.standard_normal((ka.size, dim)).astype(np.float32), rng.standard_normal((kb.size, dim)).astype(np.float32)
    d_ka, d_va, d_kb, d_vb = Guarded(ka), Guarded(va), Guarded(kb), Guarded(vb)
    d_na, d_nb = Guarded(np.array([na], dtype=np.int64)), Guarded(np.array([nb], dtype=np.int64))
    maps = [Guarded(np.full((r,), -1, dtype=np.int32)) for r in MERGE_ROWS]
    everything = [d_ka, d_va, d_kb, d_vb, d_na, d_nb] + maps
    rows_c = (C.c_int64 * 3)(*MERGE_ROWS)
    _mark(d_ka.ptr, ka.size, d_na.ptr, maps, MERGE_ROWS)
    ops.check(lib.nrx_rows_merge(d_kb.ptr, d_vb.ptr, kb.size, d_nb.ptr, d_va.ptr, _ptrs([m.ptr for m in maps]), rows_c, 3, dim, _stream()), "nrx_rows_merge")
    torch.cuda.synchronize()
    want_kb_head, want_va_head = R.merge_lists(ka[:na], va[:na], kb[:nb], vb[:nb], MERGE_ROWS, 3)
    want_kb, want_va = np.concatenate([want_kb_head, kb[nb:]]), np.concatenate([want_va_head, va[na:]])
    assert int((want_kb != kb).sum()) == 14 and (want_kb[want_kb != kb] == -1).all()          # the 14 visible shared keys, and only they
    assert np.array_equal(d_kb.get(), want_kb), "shared keys of B become -1, every other key of B stays"
    assert _same(d_vb.get(), vb) and _same(d_ka.get(), ka)
    got_va = d_va.get()
    moved = (_bits(want_va) != _bits(va)).any(axis=1)
    assert int(moved.sum()) == 14
    assert _same(got_va, want_va), "values_a: numpy's fp32 sums on the shared slots, the same bits elsewhere"
    slots = R.mark_slots(ka[:na], MERGE_ROWS, 3)
    assert sum(len(s) for s in slots) == 33 and 9 not in slots[0]
    for t in range(3):
        want = np.full((MERGE_ROWS[t],), -1, dtype=np.int32)
        for r, i in slots[t].items():
            want[r] = i
        assert np.array_equal(maps[t].get(), want), (t, "the maps hold exactly A's visible slots")
    _mark(d_ka.ptr, ka.size, d_na.ptr, maps, MERGE_ROWS, unmark=1)
    assert all((m.get() == -1).all() for m in maps)
    assert all(d.intact() for d in everything)

    # the whole merged step: two nrx_sparse_adam_step calls on the now disjoint lists == the rule on the float64-summed union list
    assert max(R.split_key(k)[1] for k in ka.tolist() + kb.tolist() if R.is_live(k, 3)) < ADAM_ROWS
    w0 = [rng.standard_normal((ADAM_ROWS, dim)).astype(np.float32) for _ in range(3)]
    m0 = [(0.3 * rng.standard_normal((ADAM_ROWS, dim))).astype(np.float32) for _ in range(3)]
    v0 = [(0.1 + rng.random((ADAM_ROWS, dim))).astype(np.float32) for _ in range(3)]
    d_w, d_mv = [Guarded(x) for x in w0], [Guarded(np.stack([m, v], axis=1)) for m, v in zip(m0, v0)]
    tp, mp, vp = _ptrs([d.ptr for d in d_w]), _ptrs([d.ptr for d in d_mv]), _ptrs([d.ptr + 4 * dim for d in d_mv])
    for dk, dv, n, dn in ((d_ka, d_va, ka.size, d_na), (d_kb, d_vb, kb.size, d_nb)):
        ops.check(lib.nrx_sparse_adam_step(tp, mp, vp, 3, dim, dk.ptr, dv.ptr, n, dn.ptr, SS, None, B1, B2, EPS, DECAY, _stream()), "nrx_sparse_adam_step")
    torch.cuda.synchronize()
    union = {}
    for k, val in list(zip(ka[:na].tolist(), va[:na])) + list(zip(kb[:nb].tolist(), vb[:nb])):
        t, r = R.split_key(k)
        if R.is_live(k, 3):
            union[k] = union.get(k, 0.0) + val.astype(np.float64)
    assert len(union) == 33 + 2 + 44 + 3          # A's rows (two of them past the marked range), the rows only B names (three past it)
    W, M, V, named = R.adam_rows(w0, m0, v0, np.array(list(union), dtype=np.int64), np.stack(list(union.values())), 3, SS, B1, B2, EPS, DECAY)
    for t in range(3):
        rows = np.array(sorted(named[t]), dtype=np.int64)
        rest = np.ones(ADAM_ROWS, bool)
        rest[rows] = False
        mv = d_mv[t].get()
        got_w, got_m, got_v = d_w[t].get(), mv[:, 0], mv[:, 1]
        _close(got_w[rows], W[t][rows])
        _close(got_m[rows], M[t][rows])
        _close(got_v[rows], V[t][rows])
        assert _same(got_w[rest], w0[t][rest]) and _same(np.ascontiguousarray(got_m[rest]), m0[t][rest]) and _same(np.ascontiguousarray(got_v[rest]), v0[t][rest])
    assert all(d.intact() for d in everything + d_w + d_mv)


# ------------------------------------------------------------------------------------------------ nrx_rows_to_dense
def _rows_to_dense_stores_and_accumulates(dim, n, mis):
    """Every key with a table of the call names its target, row 0 included (the dense gradient of the padding row is formed, and never applied).
    A long list (n >= 37) writes rows of all three tables; key_list's short ones write (table 1, row 1) and, from n = 4 on, (table 1, row 0)."""
    lib = _lib.load()
    rng = np.random.default_rng([9, dim, int(mis)] + ([n] if n < 37 else []))
    rows = R.rows_for(n)
    keys, n_dev = R.key_list(n, rng, rows)
    vals = rng.standard_normal((n, dim)).astype(np.float32)
    t0 = [rng.standard_normal((rows, dim)).astype(np.float32) for _ in range(3)]
    d_keys, d_vals = Guarded(keys), Guarded(vals, off=4 if mis else 0)
    d_n = Guarded(np.array([n_dev], dtype=np.int64)) if n_dev is not None else None
    live = keys if n_dev is None else keys[:n_dev]
    targets = [(i,) + R.split_key(k) for i, k in enumerate(live.tolist()) if k >= 0 and (k >> 40) < 3]
    assert len(targets) >= max(n // 2, 1) and len({(t, r) for _, t, r in targets}) == len(targets)
    assert n < 4 or any(r == 0 for _, _, r in targets)
    written = {t for _, t, _ in targets}
    assert n < 37 or written == {0, 1, 2}
    for acc in (0, 1):
        d_t = [Guarded(x) for x in t0]
        want = [x.copy() for x in t0]
        for _ in range(1 + acc):
            ops.check(lib.nrx_rows_to_dense(_ptrs([d.ptr for d in d_t]), 3, dim, d_keys.ptr, d_vals.ptr, n, d_n.ptr if d_n is not None else None, acc,
                                            _stream()), "nrx_rows_to_dense")
            for i, t, r in targets:
                want[t][r] = want[t][r] + vals[i] if acc else vals[i]          # numpy's fp32 addition
        torch.cuda.synchronize()
        for t in range(3):
            assert _same(d_t[t].get(), want[t]), (t, "accumulate" if acc else "store")
            assert _same(want[t], t0[t]) == (t not in written)
        if n_dev is not None:
            hid_t, hid_r = R.split_key(keys[-1])                                 # the entry past the count left its target alone
            assert _same(d_t[hid_t].get()[hid_r], t0[hid_t][hid_r])
        assert all(d.intact() for d in d_t + [d_keys, d_vals] + ([d_n] if d_n is not None else []))
        assert _same(d_keys.get(), keys) and _same(d_vals.get(), vals)


@pytest.mark.parametrize("dim,mis", [(d, False) for d in (1, 6, 16, 17, 32, 320)] + [(16, True)])
def test_rows_to_dense_stores_and_accumulates_the_lists_rows_bit_for_bit(dim, mis):
    _rows_to_dense_stores_and_accumulates(dim, long_n(dim), mis)


@pytest.mark.parametrize("n", [1, 3, 4, 5])
@pytest.mark.parametrize("dim", [6, 16])
def test_rows_to_dense_on_short_lists(dim, n):
    """A partial group of four entries in both forms; at n = 4 and 5 one of the keys names row 0, which this kernel -- unlike the optimizers -- writes."""
    _rows_to_dense_stores_and_accumulates(dim, n, False)
