"""CPU checks of the sharing tables (tests/sharing_tables.py) and their 50-digit fixture (tests/golden/gp_sharing.npz): the
builder's premises, the fused-step expectation against the rule text, and the fixture against the float64 oracle."""
import numpy as np
import pytest

import sharing_tables as st

EPS = np.finfo(np.float64).eps
GEOMETRY_KB = {"g127_300": 0, "g128_129": 1, "g129_130": 1, "g255_400": 1, "g256_257": 2, "g300_385": 2, "g384_640": 3,
               "g128_640": 1, "g640_656": 5, "g768_900": 6, "g1024_1025": 8}


@pytest.fixture(scope="module")
def tables():
    return {name: st.table(name) for name in st.TABLES}


@pytest.fixture(scope="module")
def golden():
    return st.load_golden()


def _owners_at(t, phase, k):
    """Leaves of `phase` that own a diagonal block at step k, written from the rule text alone: a factor owner (not a COPY
    leaf) with more than k blocks, and for a PREFIX leaf k at or past its copied blocks.  A claim that copies no block is FULL."""
    out = []
    for l in range(t.L):
        nb = -(-int(t.n[l]) // 128)
        kb = int(t.plen[l]) // 128 if t.op[l] == st.PREFIX else 0
        ph = 1 if kb > 0 else 0
        if t.op[l] != st.COPY and ph == phase and nb > k >= kb:
            out.append(l)
    return out


def test_lists_ascend_and_prefix_claims_are_strict_prefixes(tables):
    for t in tables.values():
        assert t.obs_ptr[-1] == t.obs_idx.size and t.route_ptr[-1] == t.route_idx.size
        for l in range(t.L):
            assert np.all(np.diff(t.obs[l]) > 0) and 0 <= t.obs[l][0] and t.obs[l][-1] < t.X.shape[0]
            assert np.all(np.diff(t.routes[l]) > 0) if t.routes[l].size > 1 else True
            if t.op[l] == st.FULL:
                assert t.src[l] == -1 and t.plen[l] == 0
                continue
            s = int(t.src[l])
            assert 0 <= s < t.L and s != l and t.op[s] == st.FULL and t.kid[s] == t.kid[l]
            if t.op[l] == st.COPY:
                assert np.array_equal(t.obs[l], t.obs[s])
            else:
                assert t.plen[l] == t.n[s] < t.n[l] and np.array_equal(t.obs[l][:t.n[s]], t.obs[s])
                assert np.all(t.obs[l][t.n[s]:] > t.obs[s][-1])


def test_every_edge_geometry_is_in_the_table_named_with_it(tables):
    where = {"T1": [g for g, kb in GEOMETRY_KB.items() if kb <= 5], "T2": ["g128_129", "g256_257", "g128_640"],
             "T3": ["g129_130", "g300_385", "g384_640"], "T4": ["g640_656", "g768_900", "g1024_1025"],
             "T4d33": ["g640_656", "g768_900", "g1024_1025"], "TD": ["g127_300", "g129_130"]}
    for name, geos in where.items():
        t = tables[name]
        for g in geos:
            l = t.keys.index(g + "/leaf")
            s_rows, n_rows = (int(v) for v in g[1:].split("_"))
            assert t.op[l] == st.PREFIX and t.keys[t.src[l]] == g + "/src" and (t.n[t.src[l]], t.n[l]) == (s_rows, n_rows)
            assert t.kb(l) == GEOMETRY_KB[g]
    assert {st.KINDS[k] for k in tables["T1"].kid} == {0, 3, 8, 10}
    assert tables["T4"].D == 3 and tables["T4d33"].D == 33 and tables["T4"].L == tables["T4d33"].L == 7
    assert max(t.L for t in tables.values()) <= 120 and max(int(t.n.max()) for t in tables.values()) == 1025


def test_fused_expectation_follows_the_32_leaf_rule(tables):
    """include/dsmgp_hip.h, DSMGP_OPT_FUSED_STEPS: a shallow step (K <= 512: k <= 4) runs fused where the step has leaves enough
    -- at least 32 of its phase own a diagonal block there -- or where they outnumber the CUs (no table has that many)."""
    for t in tables.values():
        assert t.L < 200
        for ph in (0, 1):
            for k in range(9):
                nd = len(_owners_at(t, ph, k))
                assert (k in t.fused[ph]) == (k <= 4 and nd >= 32), (t.name, ph, k, nd)
    t1, t2, t3, t4 = (tables[n] for n in ("T1", "T2", "T3", "T4"))
    assert t1.fused == {0: {0, 1, 2, 3, 4}, 1: {1, 2, 3, 4}}
    assert t2.fused == {0: set(), 1: {2, 3, 4}} and len(_owners_at(t2, 0, 0)) == 4 and 0 < len(_owners_at(t2, 1, 1)) < 32
    assert t3.fused == {0: {0, 1, 2, 3, 4}, 1: set()} and len(t3.leaves(st.PREFIX)) == 3
    assert t4.fused == {0: set(), 1: set()} and tables["T4d33"].fused == t4.fused and tables["TD"].fused == t4.fused
    for t in (t1, t2, t3):                 # the table without its phase-1 leaves keeps phase 0 as it is
        r = t.reduced()
        assert r.fused == {0: t.fused[0], 1: set()} and not any(r.kb(l) for l in range(r.L))
        assert sorted(r.keys) == sorted(k for l, k in enumerate(t.keys) if not t.kb(l))


def test_table_premises(tables):
    t1, t2 = tables["T1"], tables["T2"]
    per_source = {}
    for l in t1.leaves(st.PREFIX):
        per_source.setdefault(int(t1.src[l]), set()).add(int(t1.n[l]))
    assert sum(1 for v in per_source.values() if len(v) >= 3) >= 2          # sources with three PREFIX leaves of different lengths
    s = t1.keys.index("g300_385/src")
    lc, lo, lp = (t1.keys.index("g300_385/" + k) for k in ("copy", "copyown", "leaf"))
    assert [t1.op[l] for l in (lc, lo, lp)] == [st.COPY, st.COPY, st.PREFIX] and all(t1.src[l] == s for l in (lc, lo, lp))
    assert t1.mean[lc] == t1.mean[s] and t1.mean[lo] != t1.mean[s]
    assert sorted(t2.n[l] for l in t2.leaves(st.FULL)) == [128, 128, 256, 256]
    for s in t2.leaves(st.FULL):
        mine = [int(t2.n[l]) for l in t2.leaves(st.PREFIX) if t2.src[l] == s]
        assert len(mine) >= 9 and 129 <= min(mine) and max(mine) <= 640
    for t in tables.values():
        counts = [r.size for r in t.routes]
        assert set(counts) <= {0, 1, 16, 17, 129}
        assert all(t.routes[l].size for l in t.leaves(st.COPY))
        bare = [l for l in t.leaves(st.PREFIX) if t.routes[l].size == 0]
        assert all(t.keys[l] == "g384_640/leaf" and t.routes[t.src[l]].size for l in bare)
    for t in (t1, t2):
        assert sum(1 for l in t.leaves(st.PREFIX) if t.routes[l].size == 129) == 2
        assert any(t.routes[t.src[l]].size == 0 and t.routes[l].size for l in t.leaves(st.PREFIX))
    assert any(t1.routes[l].size == 0 and t1.routes[t1.src[l]].size for l in t1.leaves(st.PREFIX))


def test_every_leaf_of_at_most_512_rows_has_a_fixture_entry(tables, golden):
    for t in tables.values():
        if t.D != 3:
            continue
        for l in range(t.L):
            if t.n[l] <= st.MAX_MP_ROWS:
                g = golden[t.keys[l]]
                assert g["alpha"].shape == (t.n[l],) and g["mu"].shape == g["var"].shape == g["kss"].shape == (t.routes[l].size,)
            else:
                assert t.keys[l] not in golden
    assert sorted(golden) == sorted(st.data(3).mp_keys())


def test_fixture_agrees_with_the_float64_oracle(golden):
    """As make_pred_golden.check_moments: 16 cond_2(K_y) eps relative to the target's and the variance's scale."""
    dat = st.data(3)
    worst = 0.0
    for key, g in golden.items():
        s = dat.sets[key]
        kind, hyp = st.KINDS[s["kid"]], st.hyper(s["kid"], 3)
        y = dat.y[s["obs"]]
        o = st.oracle_leaf(kind, hyp, dat.X[s["obs"]], y, s["mean"])
        tol = 16 * g["cond"] * EPS
        e = [abs(o.mll() - g["mll"]) / max(1.0, abs(g["mll"])), np.max(np.abs(o.alpha - g["alpha"])) / np.max(np.abs(g["alpha"]))]
        if s["rows"].size:
            mo, vo = o.prediction(dat.Xt[s["rows"]])
            e += [np.max(np.abs(mo - g["mu"])) / max(1.0, float(np.max(np.abs(y)))),
                  np.max(np.abs(vo - g["var"]) / np.maximum(g["var"], 1.0))]
            assert np.allclose(st.prior_diag(kind, hyp, dat.Xt[s["rows"]]), g["kss"], rtol=12 * EPS, atol=0), key
        assert o.info == 0 and max(e) <= tol, (key, e, tol)
        worst = max(worst, max(e) / tol)
    print(f"\n{len(golden)} sets: worst oracle error / (16 cond eps) = {worst:.3g}")
