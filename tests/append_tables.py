"""Leaf tables for the tests of dsmgp_append_rows (tests/test_append_gpu.py, tests/test_append_host.py): the old table, the rows
added, the grown table a from-scratch context is given, and the drivers of both contexts.  Test infrastructure only."""
import numpy as np

SHARE_FULL, SHARE_COPY, SHARE_PREFIX = 0, 1, 2
TB = 128

KINDS = {                   # name -> (DSMGP_KIND_*, D, [logl..., logs, logNoise])
    "iso": (0, 2, np.array([np.log(0.3), 0.0, np.log(0.1)])),
    "ard": (8, 3, np.array([np.log(0.3), np.log(0.4), np.log(0.5), 0.0, np.log(0.1)])),       # ArdMatern52
}


class Table:
    """lists: the old observation lists; adds: per leaf the positions (rows of Xn) it receives; op / src / plen: the old sharing
    schedule; mean / mean_new: the leaves' means before and after (mean_new None: unchanged)."""

    def __init__(self, kind, X, y, lists, op, src, plen, mean, Xn, yn, adds, mean_new):
        self.kind_id, self.D, self.hyp = KINDS[kind]
        self.X, self.y, self.lists, self.op, self.src, self.plen, self.mean = X, y, lists, op, src, plen, mean
        self.Xn, self.yn, self.adds, self.mean_new = Xn, yn, adds, mean_new
        self.L = len(lists)
        self.kid = [0] * self.L

    # ---- what append_rows is given
    def add_csr(self):
        ptr = np.zeros(self.L + 1, dtype=np.int64)
        np.cumsum([len(a) for a in self.adds], out=ptr[1:])
        return ptr, np.concatenate([np.asarray(a, dtype=np.int64) for a in self.adds]) if ptr[-1] else np.zeros(0, np.int64)

    # ---- the grown table, as the issue's equivalent sequence spells it
    def grown(self):
        N0 = self.X.shape[0]
        lists = [np.concatenate([o, N0 + np.asarray(a, dtype=np.int64)]) for o, a in zip(self.lists, self.adds)]
        op = [SHARE_COPY if self.op[l] == SHARE_COPY and list(self.adds[l]) == list(self.adds[self.src[l]]) else SHARE_FULL
              for l in range(self.L)]
        src = [self.src[l] if op[l] == SHARE_COPY else -1 for l in range(self.L)]
        mean = list(self.mean if self.mean_new is None else self.mean_new)
        return np.vstack([self.X, self.Xn]), np.concatenate([self.y, self.yn]), lists, op, src, mean

    def kept_blocks(self, info_old=None):
        """Per leaf the block rows and columns the call keeps: floor(n_old / 128) for an owner that receives rows, every block of
        a leaf that receives none, 0 where the old factor failed."""
        out = []
        for l in range(self.L):
            n0 = len(self.lists[l])
            kb = -(-n0 // TB) if len(self.adds[l]) == 0 else n0 // TB
            out.append(0 if info_old is not None and info_old[l] != 0 else kb)
        return out


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(o) for o in lists], out=ptr[1:])
    return ptr, np.concatenate(lists)


def _data(kind, N, m, seed):
    _, D, _ = KINDS[kind]
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.uniform(size=(N, D)))
    Xn = np.asfortranarray(rng.uniform(size=(m, D)))
    f = lambda Z: np.sin(3.0 * Z[:, 0]) * np.cos(2.0 * Z[:, 1]) + 0.5       # noqa: E731
    return X, f(X) + 0.1 * rng.standard_normal(N), Xn, f(Xn) + 0.1 * rng.standard_normal(m)


def seven_leaves(kind="iso", variant="relocate"):
    """The table of the feature: old sizes and rows added
         0: 300 + 20   kb = 2, the partial block is rewritten, npad stays 384
         1: 128 + 1    kb = 1 exactly on a boundary, npad grows          (in_place: + 0, an untouched leaf)
         2: 100 + 5    kb = 0, a full restart
         3: 700 + 30   classic steps with K > 512
         4: 200 + 0    no additions
         5: COPY of 0  identical additions: stays COPY                    (split: one row fewer: the relation dissolves)
         6: PREFIX of 1 (its 128 rows + 172 more) + 15: becomes an owner, kb = 2
       Row 59 of the new rows goes to no leaf."""
    X, y, Xn, yn = _data(kind, 1600, 60, 20261019 + len(kind))
    lists = [np.arange(300, 600), np.arange(0, 128), np.arange(600, 700), np.arange(700, 1400), np.arange(1400, 1600),
             np.arange(300, 600), np.arange(0, 300)]
    op = [SHARE_FULL] * 5 + [SHARE_COPY, SHARE_PREFIX]
    src = [-1] * 5 + [0, 1]
    plen = [0] * 6 + [128]
    adds = [np.arange(0, 20), np.array([20]), np.arange(21, 26), np.arange(26, 56), np.zeros(0, np.int64), np.arange(0, 20),
            np.concatenate([[20], np.arange(30, 44)])]
    mean = [0.5, 0.4, 0.6, 0.5, 0.45, 0.55, 0.5]
    mean_new = [0.52, 0.41, 0.6, 0.48, 0.45, 0.5, 0.53]       # leaf 4 keeps its mean: nothing about it changes
    if variant == "in_place":
        adds[1] = np.zeros(0, np.int64)
        adds[6] = np.arange(30, 45)
        mean_new[1] = mean[1]
    elif variant == "split":
        adds[5] = np.arange(0, 19)
    else:
        assert variant == "relocate"
    return Table(kind, X, y, lists, op, src, plen, mean, Xn, yn, adds, mean_new)


def many_small_leaves(variant):
    """40 leaves of 150 rows: enough of them in block steps 0 and 1 that the steps run fused (DSMGP_OPT_FUSED_STEPS: 32 leaves or
    more in a shallow step), in the old fit and in the continuation: the kept Dinv_0 blocks hold their 16x16 inverses only when
    the call begins.  in_place: + 10 rows each (npad stays 256); relocate: + 120 (npad 256 -> 384); leaf 39 receives none."""
    L, n0 = 40, 150
    add = 10 if variant == "in_place" else 120
    X, y, Xn, yn = _data("iso", L * n0, L * add, 77 + add)
    lists = [np.arange(l * n0, (l + 1) * n0) for l in range(L)]
    adds = [np.arange(l * add, (l + 1) * add) for l in range(L)]
    adds[39] = np.zeros(0, np.int64)
    return Table("iso", X, y, lists, [SHARE_FULL] * L, [-1] * L, [0] * L, [0.5] * L, Xn, yn, adds, None)


def failed_owner_table(with_it=True):
    """Leaf 0 (kernel id 1, IsoLinear, l = 1, noise + jitter absorbed by rounding): rows 2^27 e_i with row 3 a copy of row 0 --
    the recipe of test_first_bad_minor_is_reported_exactly: every operation is exact, the pivot of row 3 is exactly 0, info = 4
    in LAPACK and here, before and after the rows are added.  Leaves 1..3: IsoSE leaves of 300, 200 and 400 rows that all
    receive rows.  No leaf reaches a block step with K >= 512, where an update tile may be cut along K by a rule that counts the
    tiles of the whole launch: no leaf's bits depend on which other leaves the table holds."""
    rng = np.random.default_rng(99)
    n0, D = 140, 3
    X0 = np.zeros((n0, D))
    for i in range(3):
        X0[i, i] = 2.0 ** 27
    X0[3, 0] = 2.0 ** 27
    for i in range(4, n0):
        X0[i, (i * 7) % D] = 2.0 ** 27
    X = np.asfortranarray(np.vstack([X0, rng.uniform(size=(900, D))]))
    y = np.concatenate([np.zeros(n0), np.sin(3.0 * X[n0:, 0]) + 0.1 * rng.standard_normal(900)])
    Xn = np.asfortranarray(np.vstack([X0[5:8], rng.uniform(size=(30, D))]))
    yn = np.concatenate([np.zeros(3), np.sin(3.0 * Xn[3:, 0])])
    lists = [np.arange(0, n0), np.arange(n0, n0 + 300), np.arange(n0 + 300, n0 + 500), np.arange(n0 + 500, n0 + 900)]
    adds = [np.arange(0, 3), np.arange(3, 13), np.arange(13, 23), np.arange(23, 33)]
    kid, mean = [1, 0, 0, 0], [0.0, 0.1, 0.2, 0.3]
    if not with_it:
        lists, adds, kid, mean = lists[1:], adds[1:], kid[1:], mean[1:]
    return X, y, Xn, yn, lists, adds, kid, mean


FAILED_HYP = {0: (0, np.array([np.log(0.3), np.log(0.4), np.log(0.1)])), 1: (2, np.array([0.0, 0.0, -30.0]))}



# ---- drivers

def fit_old(ctx, T, options=()):
    for o, v in options:
        ctx.set_option(o, v)
    ctx.set_train(T.X, T.y)
    ctx.set_leaves(*_csr(T.lists), T.kid, T.mean)
    ctx.set_hyper(0, T.kind_id, T.hyp)
    ctx.set_sharing(T.op, T.src, T.plen)
    return ctx.fit()


def append(ctx, T):
    ptr, idx = T.add_csr()
    return ctx.append_rows(T.Xn, T.yn, ptr, idx, T.mean_new)


def fit_grown(ctx, T, options=()):
    """The issue's equivalent sequence on a fresh context: set_train / set_leaves / set_sharing / fit on the grown table."""
    for o, v in options:
        ctx.set_option(o, v)
    Xg, yg, lists, op, src, mean = T.grown()
    ctx.set_train(Xg, yg)
    ctx.set_leaves(*_csr(lists), T.kid, mean)
    ctx.set_hyper(0, T.kind_id, T.hyp)
    ctx.set_sharing(op, src, [0] * T.L)
    return ctx.fit()


def factors(ctx, sizes):
    return [ctx.download_factor(l, int(n)) for l, n in enumerate(sizes)]
