"""CPU checks of deepstructuredmixtures_amd/leafset.py and of the three layers that slice the leaf table through it:
`hipabi.MultiContext`, `hipabi.StreamingContext` (both driven with the oracle context in place of the device) and
`dist.Shard`.  The references of part 1 are the loops the module replaced, transcribed as they stood."""
import json
import os

import numpy as np
import pytest

import deepstructuredmixtures_amd as dsm
from deepstructuredmixtures_amd import tree as ptree, hipabi, dist as pdist
from deepstructuredmixtures_amd.leafset import LeafSubset, share_roots
from oracle_context import OracleContext

FULL, COPY, PREFIX = ptree.SHARE_FULL, ptree.SHARE_COPY, ptree.SHARE_PREFIX


# ---------------------------------------------------------------------------- 1. helpers against the loops they replace

def loop_take_csr(ptr, idx, loc):
    lptr = np.concatenate([[0], np.cumsum(ptr[loc + 1] - ptr[loc])])
    lidx = np.concatenate([idx[ptr[g]:ptr[g + 1]] for g in loc]) if len(loc) else np.zeros(0, np.int64)
    return lptr, lidx


def loop_put_entries(out, ptr, loc, part):
    pos = 0
    for g in loc:
        c = int(ptr[g + 1] - ptr[g])
        out[ptr[g]:ptr[g + 1]] = part[pos:pos + c]
        pos += c


def loop_sharing_model(op, src, plen, loc):
    """Model._upload: a leaf whose source is held elsewhere is factorised in full."""
    g2l = {g: i for i, g in enumerate(loc)}
    lop = np.zeros(len(loc), dtype=np.int32)
    lsrc = np.full(len(loc), -1, dtype=np.int32)
    lpl = np.zeros(len(loc), dtype=np.int64)
    for i, g in enumerate(loc):
        if op[g] != FULL and int(src[g]) in g2l:
            lop[i], lsrc[i], lpl[i] = op[g], g2l[int(src[g])], plen[g]
    return lop, lsrc, lpl


def loop_sharing_wrapper(op, src, plen, loc):
    """MultiContext._upload and StreamingContext._pass: right only for unions of whole sharing groups."""
    g2l = {int(g): i for i, g in enumerate(loc)}
    return op[loc], np.array([g2l.get(int(src[g]), -1) for g in loc], dtype=np.int32), plen[loc]


def loop_group(op, src, L):
    """MultiContext._partition (`group`) and StreamingContext._make_groups (`unit`)."""
    group = np.arange(L)
    if op is not None:
        for j in range(L):
            if op[j] != 0 and src[j] >= 0:
                group[j] = src[j]
    return group


def loop_group_chained(op, src, L):
    """Shard.lpt."""
    group = np.arange(L)
    for j in range(L):
        if op[j] != 0 and src[j] >= 0:
            group[j] = src[j]
    for j in range(L):
        group[j] = group[group[j]]
    return group


def random_table(rng, L):
    """CSR table with empty rows, and a schedule whose sources are FULL and distinct from their leaf."""
    cnt = rng.integers(0, 6, L) * (rng.random(L) < 0.7)
    ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    idx = rng.integers(0, 1000, int(ptr[-1])).astype(np.int64)
    op = np.zeros(L, dtype=np.int32)
    src = np.full(L, -1, dtype=np.int32)
    plen = np.zeros(L, dtype=np.int64)
    full = np.flatnonzero(rng.random(L) < 0.5)
    if full.size == 0:
        full = np.array([int(rng.integers(0, L))])
    for j in np.setdiff1d(np.arange(L), full):
        if rng.random() < 0.7:
            op[j], src[j] = int(rng.integers(1, 3)), int(rng.choice(full))
            plen[j] = int(rng.integers(1, 50)) if op[j] == PREFIX else 0
    return ptr, idx, op, src, plen


def random_subsets(rng, L):
    yield np.zeros(0, dtype=np.int64)
    yield np.arange(L)
    for _ in range(4):
        yield np.flatnonzero(rng.random(L) < rng.random())


def test_helpers_equal_the_loops_they_replace():
    rng = np.random.default_rng(20240)
    n_sub = 0
    for L in range(1, 31):
        for _ in range(3):
            ptr, idx, op, src, plen = random_table(rng, L)
            roots = share_roots(op, src, L)
            assert roots.dtype == np.int64 and np.array_equal(roots, loop_group(op, src, L))
            assert np.array_equal(roots, loop_group_chained(op, src, L))
            assert np.array_equal(share_roots(None, None, L), np.arange(L))
            for loc in random_subsets(rng, L):
                sub = LeafSubset(loc, L)
                n_sub += 1
                lptr, lidx = sub.take_csr(ptr, idx)
                rptr, ridx = loop_take_csr(ptr, idx, loc)
                assert np.array_equal(lptr, rptr) and np.array_equal(lidx, ridx) and lidx.dtype == np.int64
                for shape in ((int(ptr[-1]),), (int(ptr[-1]), 3)):
                    part = rng.random((int(rptr[-1]),) + shape[1:])
                    got, want = np.full(shape, -1.0), np.full(shape, -1.0)
                    sub.put_entries(got, ptr, part)
                    loop_put_entries(want, ptr, loc, part)
                    assert np.array_equal(got, want)
                    vals = rng.random((loc.size,) + shape[1:])
                    got, want = np.full((L,) + shape[1:], -1.0), np.full((L,) + shape[1:], -1.0)
                    sub.put_leaves(got, vals)
                    want[loc] = vals
                    assert np.array_equal(got, want)
                g2l = sub.global_to_local()
                assert g2l.dtype == np.int64 and g2l.shape == (L,)
                assert np.array_equal(np.flatnonzero(g2l >= 0), loc) and np.array_equal(g2l[loc], np.arange(loc.size))
                got = sub.take_sharing(op, src, plen)
                assert [a.dtype for a in got] == [np.int32, np.int32, np.int64]
                assert all(np.array_equal(a, b) for a, b in zip(got, loop_sharing_model(op, src, plen, loc)))
                assert sub.take_sharing(None, None, None) == (None, None, None)
                # a union of whole sharing groups (what the two wrappers hand their contexts): their rule says the same
                whole = np.flatnonzero(np.isin(roots, roots[loc]))
                got = LeafSubset(whole, L).take_sharing(op, src, plen)
                assert all(np.array_equal(a, b) for a, b in zip(got, loop_sharing_wrapper(op, src, plen, whole)))
    assert n_sub == 30 * 3 * 6


def test_explicit_subsets():
    ptr = np.array([0, 2, 2, 5, 6], dtype=np.int64)
    idx = np.array([7, 8, 1, 2, 3, 9], dtype=np.int64)
    lptr, lidx = LeafSubset(np.arange(4), 4).take_csr(ptr, idx)
    assert lptr is ptr and lidx is idx                                # every leaf in order: the inputs themselves
    lptr, lidx = LeafSubset(np.array([1]), 4).take_csr(ptr, idx)      # one leaf without entries
    assert np.array_equal(lptr, [0, 0]) and lidx.size == 0 and lidx.dtype == np.int64
    lptr, lidx = LeafSubset(np.zeros(0, dtype=np.int64), 4).take_csr(ptr, idx)
    assert np.array_equal(lptr, [0]) and lidx.size == 0 and lidx.dtype == np.int64
    lptr, lidx = LeafSubset(np.array([0, 1, 3]), 4).take_csr(ptr, idx)
    assert np.array_equal(lptr, [0, 2, 2, 3]) and np.array_equal(lidx, [7, 8, 9])
    out = np.zeros(6)
    LeafSubset(np.array([1]), 4).put_entries(out, ptr, np.zeros(0))
    assert not out.any()
    # leaf 2 extends leaf 0 and leaf 3 copies it: without leaf 0 both are factorised in full
    op, src, plen = np.array([FULL, FULL, PREFIX, COPY]), np.array([-1, -1, 0, 0]), np.array([0, 0, 2, 0])
    lop, lsrc, lpl = LeafSubset(np.array([1, 2, 3]), 4).take_sharing(op, src, plen)
    assert lop.tolist() == [0, 0, 0] and lsrc.tolist() == [-1, -1, -1] and lpl.tolist() == [0, 0, 0]
    lop, lsrc, lpl = LeafSubset(np.array([0, 2]), 4).take_sharing(op, src, plen)
    assert lop.tolist() == [FULL, PREFIX] and lsrc.tolist() == [-1, 0] and lpl.tolist() == [0, 2]
    assert share_roots(op, src, 4).tolist() == [0, 1, 0, 0]


# ---------------------------------------------------------------------------- the model of parts 2 and 3

STRIDE = 3          # IsoSE: log length scale, log signal, log noise


def _build(ctx):
    X, y, Xt = dsm.regression_data(240, 2, n_test=40, seed=107)
    m = dsm.buildDSMGP(X, y, 2, 3, M=15, D=2, kernel=dsm.IsoSE(np.log(0.4), 0.0), logNoise=np.log(0.2), seed=7, ctx=ctx)
    return m, np.asfortranarray(Xt[:12])      # few rows: some leaves get none


@pytest.fixture(scope="module")
def resident():
    """The model on one plain oracle context: what every wrapper has to reproduce bit for bit (left unchanged)."""
    m, Xt = _build(OracleContext())
    ptr, idx = ptree.route(m.root, Xt)
    mu, var = m.ctx.predict_leaves(Xt, ptr, idx)
    op, src, plen = ptree.share_schedule(m.leaves, m.D, 0.05)
    return dict(m=m, Xt=Xt, ptr=ptr, idx=idx, mu=mu.copy(), var=var.copy(), grad=m.ctx.gradients(STRIDE),
                op=op, src=src, plen=plen)


def test_the_model_has_copy_and_prefix_leaves(resident):
    op, src = resident["op"], resident["src"]
    assert np.count_nonzero(op == COPY) >= 1 and np.count_nonzero(op == PREFIX) >= 1
    assert np.array_equal(resident["m"].share_op, op) and np.all(op[src[op != FULL]] == FULL)
    assert np.diff(resident["ptr"]).min() == 0 < np.diff(resident["ptr"]).max()       # leaves without a routed row too


# ---------------------------------------------------------------------------- 2. MultiContext on the CPU

def test_multicontext_equals_the_resident_run(resident):
    m, Xt = _build(hipabi.MultiContext(n=3, make_context=lambda d: OracleContext()))
    mc, r = m.ctx, resident
    assert np.array_equal(m.leaf_mll, r["m"].leaf_mll) and np.array_equal(m.leaf_info, r["m"].leaf_info)
    assert len(mc.act) == len(mc.part) == len(mc.subsets) == 3
    assert np.array_equal(np.sort(np.concatenate(mc.part)), np.arange(m.L))
    part_of = np.empty(m.L, dtype=np.int64)
    for k, (loc, sub, s) in enumerate(zip(mc.part, mc.subsets, mc.act)):
        part_of[loc] = k
        assert sub.loc is loc and s.L == loc.size
        assert all(np.array_equal(s.obs[i], m.leaves[g].obs) for i, g in enumerate(loc))
    shared = np.flatnonzero(r["op"] != FULL)
    assert np.array_equal(part_of[shared], part_of[r["src"][shared]])          # every shared leaf beside its source
    for loc, s in zip(mc.part, mc.act):                                         # ... and pointing at it, in local numbers
        assert np.array_equal(s.op, r["op"][loc]) and np.array_equal(loc[s.src[s.op != FULL]], r["src"][loc][s.op != FULL])
    mu, var = mc.predict_leaves(Xt, r["ptr"], r["idx"])
    assert np.array_equal(mu, r["mu"]) and np.array_equal(var, r["var"])
    assert np.array_equal(mc.gradients(STRIDE), r["grad"])
    assert sum(s.grad_evaluations for s in mc.subs) == m.L
    mask = np.arange(m.L) % 3 == 1
    mc.set_gradient_leaves(mask)
    g = mc.gradients(STRIDE)
    assert sum(s.grad_evaluations for s in mc.subs) == m.L + np.count_nonzero(mask)
    assert np.array_equal(g[mask], r["grad"][mask]) and not g[~mask].any() and r["grad"][mask].all(axis=1).all()
    for loc, s in zip(mc.part, mc.act):
        assert np.array_equal(s._grad_active, mask[loc])
    mc.pool.shutdown()


# ---------------------------------------------------------------------------- 3. StreamingContext on the CPU

class OracleStreamContext(OracleContext):
    """OracleContext with what a streaming pass asks of its context besides the numbers."""
    fits = 0

    def fit(self):
        self.fits += 1
        return super().fit()

    def memory(self):
        return 1 << 40, 1 << 40

    def reserve(self, nbytes):
        self.reserved = int(nbytes)

    def release(self):
        self.gps = []

    def timings(self):
        return {"fit": 1.0}

    def work(self):
        return float(self.L), 1

    def work_fused(self):
        return 0.0, 0

    def download_factor(self, leaf, n, factor=True):
        assert not factor and self.gps[leaf].alpha.shape == (n,)
        return None, self.gps[leaf].alpha.copy()


def test_streamingcontext_equals_the_resident_run(resident):
    r = resident
    n = np.array([lf.nobs for lf in r["m"].leaves])
    budget = sum(hipabi.estimate_bytes(n[j:j + 1], np.zeros(1, dtype=np.int64), 2) for j in range(n.size)) // 4   # of a bare fit
    m, Xt = _build(hipabi.StreamingContext(budget_bytes=budget, make_context=lambda d: OracleStreamContext()))
    sc = m.ctx
    assert np.array_equal(m.leaf_mll, r["m"].leaf_mll) and np.array_equal(m.leaf_info, r["m"].leaf_info)
    assert len(sc.groups) >= 3 and sc.passes == 1 and sc.ctx.fits == len(sc.groups)
    assert np.array_equal(np.sort(np.concatenate(sc.groups)), np.arange(m.L))
    group_of = np.empty(m.L, dtype=np.int64)
    for k, loc in enumerate(sc.groups):
        group_of[loc] = k
    shared = np.flatnonzero(r["op"] != FULL)
    assert np.array_equal(group_of[shared], group_of[r["src"][shared]])
    sc.keep_alpha = (int(shared[0]), m.L - 1)
    mu, var = sc.predict_leaves(Xt, r["ptr"], r["idx"])
    assert np.array_equal(mu, r["mu"]) and np.array_equal(var, r["var"])
    assert sc.passes == 2 and len(sc.groups) >= 3 and sc.ctx.reserved > 3 << 30
    assert np.array_equal(sc.fit()[0], r["m"].leaf_mll) and sc.passes == 3
    for g in sc.keep_alpha:
        assert np.array_equal(sc.alpha(g), r["m"].ctx.gps[g].alpha)
    assert sc.work() == (float(m.L), len(sc.groups)) and sc.timings() == {"fit": float(len(sc.groups))}
    assert set(sc.host_seconds) == {"set_leaves", "set_sharing", "set_test", "fit", "release"}
    before = sc.groups
    g = sc.gradients(STRIDE)
    assert sc.passes == 4 and sc.groups is not before and len(sc.groups) >= 3       # exactly one further pass, groups rebuilt
    assert np.array_equal(g, r["grad"])
    assert np.array_equal(sc.predict_fetch()[0], r["mu"]) and np.array_equal(sc.predict_fetch()[1], r["var"])
    assert np.array_equal(sc.gradients(STRIDE), r["grad"]) and sc.passes == 4        # ... and none for the same question


# ---------------------------------------------------------------------------- 4. Shard on the CPU

def _shards(owner, world, sends):
    """One Shard per rank whose all-gather returns what every rank would send (padding: a value no input holds)."""
    out = []
    for rank in range(world):
        sh = pdist.Shard(owner, rank, world)

        def gather(local, maxlen, rank=rank):
            mine = np.asarray(sends[rank], dtype=np.float64).reshape(-1)
            assert np.array_equal(np.asarray(local, dtype=np.float64).reshape(-1), mine)
            assert maxlen == max(np.asarray(v).size for v in sends)
            return [np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1), np.full(maxlen - np.asarray(v).size, -7.0)])
                    for v in sends]
        sh._all_gather_padded = gather
        out.append(sh)
    return out


def test_shard_gathers_reproduce_the_whole_table():
    owner = np.array([2, 0, 0, 2, 0, 2, 2, 0, 2])                    # rank 1 holds nothing
    world, L = 3, owner.size
    counts = np.array([3, 0, 2, 5, 1, 0, 4, 2, 1])
    ptr = np.concatenate([[0], np.cumsum(counts)])
    rng = np.random.default_rng(5)
    a, b = rng.random(int(ptr[-1])), rng.random(int(ptr[-1]))
    vals, cols = rng.random(L), rng.random((L, 4))
    loc = [np.flatnonzero(owner == r) for r in range(world)]
    flat = [np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in l]).astype(np.int64) if l.size else np.zeros(0, np.int64)
            for l in loc]
    for sh in _shards(owner, world, [vals[l] for l in loc]):
        assert sh.local.dtype == np.int64 and np.array_equal(sh.local, loc[sh.rank])
        assert np.array_equal(sh.gather_leaf_values(vals[sh.local]), vals)
    for sh in _shards(owner, world, [cols[l] for l in loc]):
        assert np.array_equal(sh.gather_leaf_columns(cols[sh.local]), cols)
    for sh in _shards(owner, world, [a[f] for f in flat]):
        assert np.array_equal(sh.gather_ragged(a[flat[sh.rank]], counts), a)
    for sh in _shards(owner, world, [np.stack([a[f], b[f]], axis=1) for f in flat]):
        ga, gb = sh.gather_ragged_pair(a[flat[sh.rank]], b[flat[sh.rank]], counts)
        assert np.array_equal(ga, a) and np.array_equal(gb, b)

    class Exchange:                   # the library's fit exchange: `count` slots of (mll, info) per rank
        def fit_exchange(self, count):
            both = np.full((world, count, 2), -7.0)
            for r in range(world):
                both[r, : loc[r].size] = cols[loc[r], :2]
            return both
    sh = pdist.Shard(owner, 2, world)
    assert np.array_equal(sh.fit_exchange(Exchange()), cols[:, :2])


def test_lpt_owners_are_those_of_the_loops(golden_dir):
    with open(os.path.join(golden_dir, "lpt_owners.json")) as f:
        cases = json.load(f)
    assert [len(c["nobs"]) for c in cases] == [8, 40, 40]
    assert cases[0]["nobs"] == [100, 90, 80, 10, 10, 10, 10, 100] and cases[0]["src"] == [-1] * 7 + [0]
    for c in cases:
        op, src = np.array(c["op"]), np.array(c["src"])
        assert np.count_nonzero(op) > 0 and np.all(op[src[op != 0]] == 0)
        nt = None if c["n_test"] is None else np.array(c["n_test"])
        for rank in range(c["world"]):
            sh = pdist.Shard.lpt(np.array(c["nobs"]), op, src, rank, c["world"], n_test=nt)
            assert sh.owner.dtype == np.int64 and np.array_equal(sh.owner, c["owner"])
            assert np.array_equal(sh.local, np.flatnonzero(np.array(c["owner"]) == rank))
