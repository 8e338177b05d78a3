"""Leaf tables that drive the shared-Cholesky schedule (COPY / PREFIX leaves) through every phase and step kind, built
deterministically from datagen's counter streams.  Test infrastructure only, like tests/targets_context.py.

Every observation set has a key.  A sharing family is one source set (rows drawn from the low half of the training rows) and
leaf sets = the source's rows followed by a tail of later rows (drawn from the high half), so every leaf list ascends and has
its source's list as a strict prefix.  A set's routed test rows are a function of its key: leaves that use one set in several
tables (or as replicas inside one) share one fixture entry of tests/golden/gp_sharing.npz.

Kernel ids 0..3 are IsoSE, ArdLinear, ArdMatern52 and ArdRQ (kinds 0, 3, 8, 10); a family has one kernel id.

Edge geometries (source rows -> PREFIX leaf rows; TB = 128, kb = source // TB whole blocks are copied):
    127 -> 300   kb = 0: the claim is demoted to FULL            128 -> 129   kb = 1 = the source's nb, a row block with one row
    129 -> 130   kb = 1, the source's ragged block recomputed     255 -> 400   kb = 1 of a two-block source
    256 -> 257   kb = 2, one new row in a block of its own       300 -> 385   kb = 2, the last block holds one row
    384 -> 640   kb = 3, five blocks                             128 -> 640   short source, long continuation
    640 -> 656   kb = 5: the first step past the shallow rule    768 -> 900   kb = 6: blocks copied out of lookahead steps
    1024 -> 1025 kb = 8 = nb - 1

Tables (`table(name)`), with the block steps each phase is expected to run fused (`Table.fused`, asserted here against the rule
of include/dsmgp_hip.h, DSMGP_OPT_FUSED_STEPS, as build_plan applies it: a step k <= 4 of a phase runs fused where at least 32
leaves of the phase own a diagonal block there -- factor owners with nb > k >= kb -- or where there are more such leaves than
CUs, which no table here reaches):
    T1  both phases fused: phase 0 steps 0-4, phase 1 steps 1-4.  Every source of the geometries up to 640 rows twice (the
        replica is a FULL leaf on the same list), 32 FULL fillers of 520..640 rows, four 128-row hubs (one per kernel id)
        with eight PREFIX leaves of 513..640 rows each, sources with three and more PREFIX leaves of different lengths, and a
        source with a COPY leaf of its mean, a COPY leaf with a mean of its own and a PREFIX leaf.
    T2  phase 0 classic (four owners), phase 1 classic at step 1 and fused at steps 2-4: two 128-row and two 256-row sources
        with nine and more PREFIX leaves of 129..640 rows each.
    T3  phase 0 fused (T1's phase-0 leaves), phase 1 classic: three PREFIX leaves (129 -> 130, 300 -> 385, 384 -> 640) whose
        copied blocks come out of fused steps.
    T4  no fused step: 640 -> 656, 768 -> 900, 1024 -> 1025 and a COPY of the 768-row source; D = 3, or D = 33 (`T4d33`),
        where the Gram values go through memory.
    TD  the demoted claim 127 -> 300 next to a PREFIX and a COPY leaf that stay.
Routes: every COPY leaf and every PREFIX leaf but 384 -> 640 (whose source has rows) has routed test rows, 1, 16, 17 or 129 of
them; the sources of 128 -> 129 and 128 -> 640 (129 rows each) have none."""
import importlib.util
import os

import numpy as np

from oracle import gp as ogp
import dense_kernels as dk
from dense_gp import DenseGP

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("_sharing_datagen", os.path.join(_ROOT, "deepstructuredmixtures_amd", "datagen.py"))
_datagen = importlib.util.module_from_spec(_spec)      # the generator alone: importing the package would load the product
_spec.loader.exec_module(_datagen)
uniform, normal = _datagen.uniform, _datagen.normal

TB = 128                      # block size of the factorisation
FUSED_SHALLOW_STEPS = 4       # the rule text: steps k <= 4 ...
FUSED_MIN_LEAVES = 32         # ... with at least 32 participating leaves
MAX_MP_ROWS = 512             # the largest set the 50-digit fixture pays for
KINDS = (0, 3, 8, 10)         # kernel id -> kind
N, N_LOW, NT = 6000, 3000, 200
FULL, COPY, PREFIX = 0, 1, 2
OWN_MEAN_SHIFT = 0.3

# name, source rows, leaf rows, kernel id, routed rows of the source, routed rows of the leaf
GEOMETRIES = [
    ("g127_300", 127, 300, 0, 17, 16),
    ("g128_129", 128, 129, 1, 0, 129),
    ("g129_130", 129, 130, 2, 16, 17),
    ("g255_400", 255, 400, 3, 1, 16),
    ("g256_257", 256, 257, 0, 17, 1),
    ("g300_385", 300, 385, 1, 16, 17),
    ("g384_640", 384, 640, 2, 17, 0),
    ("g128_640", 128, 640, 3, 0, 129),
    ("g640_656", 640, 656, 0, 1, 17),
    ("g768_900", 768, 900, 2, 16, 129),
    ("g1024_1025", 1024, 1025, 3, 1, 16),
]
# further 128- and 256-row sources: the hubs of kernel ids 0 and 2 (ids 1 and 3: the sources of 128 -> 129 and 128 -> 640)
EXTRA_SOURCES = [("h0", 128, 0, 16), ("h2", 128, 2, 1), ("f256", 256, 2, 17)]
HUBS = ["h0", "g128_129", "h2", "g128_640"]                 # 128-row sources, kernel ids 0..3
T2_SOURCES = ["g128_129", "g256_257", "g128_640", "f256"]
BIG = [513, 530, 547, 576, 599, 625, 639, 640]             # rows of the eight long PREFIX leaves of a hub / T2 source
# shorter PREFIX leaves next to the geometry's own: (family, leaf rows, routed rows)
EXTRA_LEAVES = [("g128_129", 200, 16), ("g128_129", 300, 1), ("g256_257", 400, 17), ("g256_257", 600, 16), ("g128_640", 450, 1),
                ("f256", 300, 16)]
N_FILL = 32


def hyper(kid, D):
    """The library hyper-vector (with logNoise) of kernel id `kid` at input width D.  D = 3: IsoSE and ArdLinear as in
    tests/golden/make_pred_golden.py (HYP), ArdMatern52 and ArdRQ as in tests/test_targets_grad_gpu.py (_HYP); wider inputs
    stretch the length-scales by sqrt(D / 3)."""
    s = np.sqrt(D / 3.0)
    if kid == 0:
        return np.array([np.log(0.3 * s), 0.0, np.log(0.1)])
    if kid == 1:
        ls = [0.8, 1.2, 1.7] if D == 3 else s * np.linspace(0.8, 1.7, D)
        return np.concatenate([np.log(ls), [0.0, np.log(0.1)]])
    if kid == 2:
        ls = [0.5, 0.8, 0.6] if D == 3 else s * np.linspace(0.5, 0.8, D)
        return np.concatenate([np.log(ls), [-0.1, np.log(0.2)]])
    ls = [0.5, 0.7, 0.9] if D == 3 else s * np.linspace(0.5, 0.9, D)
    return np.concatenate([np.log(ls), [np.log(0.3), -0.1, np.log(0.2)]])


def oracle_leaf(kind, hyp, X, y, mean):
    """The float64 oracle of one leaf: oracle.gp for IsoSE, tests/dense_gp.py for the kinds oracle/ lacks.
    hyp = the library hyper-vector with logNoise.  All answer info, mll(), prediction(Xt) and L()."""
    if kind == 0:
        return ogp.GaussianProcess(X, y, mean, ogp.make_kernel(0, hyp[:-1]), hyp[-1], exact_dist=True).update_cholesky()
    return DenseGP(kind, hyp, X, y, mean)


def prior_diag(kind, hyp, Xt):
    """k(x*, x*) per row."""
    return dk.prior_diag(kind, hyp[:-1], Xt)


class Data:
    """Training rows, targets, test rows and the keyed observation sets at one input width."""

    def __init__(self, D):
        self.D = D
        self.X = np.asfortranarray(uniform(7100 + D, 0, N * D).reshape((N, D), order="F"))
        self.y = np.sin(3.0 * self.X[:, 0]) * np.cos(2.0 * self.X[:, 1]) + self.X[:, 2] + 0.1 * normal(7200 + D, 0, N)
        self.Xt = np.asfortranarray(uniform(7300 + D, 0, NT * D).reshape((NT, D), order="F"))
        self.sets = {}          # key -> dict(kid, obs, rows, mean, src (key or None))
        self._serial = 0
        for name, s, n, kid, rs, rl in GEOMETRIES:
            self._source(name, s, kid, rs)
            self._leaf(name, "leaf", n, rl)
        for name, s, kid, rs in EXTRA_SOURCES:
            self._source(name, s, kid, rs)
        for fam in sorted(set(HUBS + T2_SOURCES)):
            for j, n in enumerate(BIG):
                if not (fam == "g128_640" and n == 640):             # that one is the geometry's own leaf
                    self._leaf(fam, f"big{j}", n, (1, 16, 17, 16)[j % 4])
        for fam, n, r in EXTRA_LEAVES:
            self._leaf(fam, str(n), n, r)
        # COPY leaves of the 300-row source: with its mean, and with a mean of their own (another entry: another alpha)
        src = self.sets["g300_385/src"]
        self._add("g300_385/copy", src["kid"], src["obs"], 17, src["mean"], "g300_385/src")
        self._add("g300_385/copyown", src["kid"], src["obs"], 16, src["mean"] + OWN_MEAN_SHIFT, "g300_385/src")
        src = self.sets["g768_900/src"]
        self._add("g768_900/copy", src["kid"], src["obs"], 17, src["mean"], "g768_900/src")
        for i in range(N_FILL):                                       # FULL fillers of 520 .. 640 rows
            n = 520 + ((i - 1) * 37) % 121 if i else 640
            obs = np.sort(self._perm(0, N)[:n])
            self._add(f"fill/{i:02d}", i % 4, obs, (0, 1, 16, 0, 17)[i % 5], None, None)

    def _perm(self, lo, hi):
        self._serial += 1
        return lo + np.argsort(uniform(7400 + self.D * 1000 + self._serial, 0, hi - lo), kind="stable")

    def _add(self, key, kid, obs, nrows, mean, src):
        rows = np.sort(self._perm(0, NT)[:nrows]).astype(np.int64)
        obs = np.asarray(obs, dtype=np.int64)
        assert key not in self.sets and np.all(np.diff(obs) > 0)     # ascending lists
        self.sets[key] = dict(kid=kid, obs=obs, rows=rows, mean=float(np.mean(self.y[obs])) if mean is None else mean, src=src)

    def _source(self, name, s, kid, nrows):
        self._add(name + "/src", kid, np.sort(self._perm(0, N_LOW)[:s]), nrows, None, None)

    def _leaf(self, fam, tag, n, nrows):
        src = self.sets[fam + "/src"]
        tail = np.sort(self._perm(N_LOW, N)[:n - src["obs"].size])
        assert 0 < tail.size
        self._add(f"{fam}/{tag}", src["kid"], np.concatenate([src["obs"], tail]), nrows, None, fam + "/src")

    def family_leaves(self, fam):
        return [k for k, s in self.sets.items() if s["src"] == fam + "/src" and s["obs"].size > self.sets[s["src"]]["obs"].size]

    def mp_keys(self):
        """The sets the 50-digit fixture covers: every set of at most MAX_MP_ROWS rows."""
        return [k for k, s in self.sets.items() if s["obs"].size <= MAX_MP_ROWS]


_DATA = {}


def data(D=3):
    if D not in _DATA:
        _DATA[D] = Data(D)
    return _DATA[D]


class Table:
    """One leaf table: `keys[l]` names leaf l's set; op / src / plen are the caller's sharing schedule."""

    def __init__(self, name, dat, entries, fused):
        """entries: (key, op) in leaf order, a source before its COPY / PREFIX leaves; fused: {phase: set of steps}."""
        self.name, self.dat, self.D = name, dat, dat.D
        self.X, self.y, self.Xt = dat.X, dat.y, dat.Xt
        self.keys = [k for k, _ in entries]
        L = self.L = len(entries)
        self.op = np.array([o for _, o in entries], dtype=np.int32)
        self.src = np.full(L, -1, dtype=np.int32)
        self.plen = np.zeros(L, dtype=np.int64)
        first = {}
        for l, k in enumerate(self.keys):
            first.setdefault(k, l)
        for l, (k, o) in enumerate(entries):
            if o != FULL:
                self.src[l] = first[dat.sets[k]["src"]]
                assert self.src[l] < l and self.op[self.src[l]] == FULL
                if o == PREFIX:
                    self.plen[l] = dat.sets[dat.sets[k]["src"]]["obs"].size
        S = [dat.sets[k] for k in self.keys]
        self.obs = [s["obs"] for s in S]
        self.n = np.array([o.size for o in self.obs])
        self.obs_ptr = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.obs_idx = np.concatenate(self.obs)
        self.kid = np.array([s["kid"] for s in S], dtype=np.int32)
        self.mean = np.array([s["mean"] for s in S])
        self.routes = [s["rows"] for s in S]
        self.route_ptr = np.concatenate([[0], np.cumsum([r.size for r in self.routes])]).astype(np.int64)
        self.route_idx = np.concatenate(self.routes)
        self.hyper = {kid: (KINDS[kid], hyper(kid, self.D)) for kid in range(4)}
        self.fused = {ph: set(fused.get(ph, ())) for ph in (0, 1)}
        self._check()

    # -- the premises
    def _check(self):
        for l in range(self.L):
            assert np.all(np.diff(self.obs[l]) > 0), l
            if self.op[l] == COPY:
                assert np.array_equal(self.obs[l], self.obs[self.src[l]]) and self.kid[l] == self.kid[self.src[l]]
            if self.op[l] == PREFIX:
                s = self.obs[self.src[l]]
                assert self.plen[l] == s.size < self.n[l] and np.array_equal(self.obs[l][:s.size], s), l   # a strict prefix
                assert self.kid[l] == self.kid[self.src[l]]
        assert fused_steps(self.n, self.op, self.plen) == self.fused, (self.name, fused_steps(self.n, self.op, self.plen))

    # -- views
    def leaves(self, op):
        return [l for l in range(self.L) if self.op[l] == op]

    def shared(self):
        """The PREFIX and the COPY leaves."""
        return [l for l in range(self.L) if self.op[l] != FULL]

    def kb(self, l):
        return int(self.plen[l]) // TB if self.op[l] == PREFIX else 0

    def kind(self, l):
        return KINDS[self.kid[l]]

    def hyp(self, l):
        return self.hyper[self.kid[l]][1]

    def oracle(self, l):
        o = self.obs[l]
        return oracle_leaf(self.kind(l), self.hyp(l), self.X[o], self.y[o], self.mean[l])

    def reduced(self):
        """The same table without its phase-1 leaves: sources, fillers and COPY leaves only (a demoted claim is FULL)."""
        keep = [(k, COPY if o == COPY else FULL) for l, (k, o) in enumerate(zip(self.keys, self.op))
                if not (o == PREFIX and self.kb(l) > 0)]
        return Table(self.name + "-phase0", self.dat, keep, {0: self.fused[0]})

    def load(self, ctx, sharing=True):
        """set_train, set_leaves, set_hyper and the schedule (or none); the test set is the caller's to register."""
        ctx.set_train(self.X, self.y)
        ctx.set_leaves(self.obs_ptr, self.obs_idx, self.kid, self.mean)
        for kid, (kind, h) in self.hyper.items():
            ctx.set_hyper(kid, kind, h)
        if sharing:
            ctx.set_sharing(self.op, self.src, self.plen)
        else:
            ctx.set_sharing(None, None, None)


def fused_steps(n, op, plen):
    """{phase: set of block steps that run fused} by the rule text: a PREFIX leaf with kb >= 1 is in phase 1 (kb = 0: the
    claim is dropped, the leaf is FULL), a COPY leaf owns no block, and a step k <= 4 of a phase runs fused where at least 32 of
    its leaves have nb > k >= kb."""
    n, op, plen = np.asarray(n), np.asarray(op), np.asarray(plen)
    nb = (n + TB - 1) // TB
    kb = np.where(op == PREFIX, plen // TB, 0)
    phase = np.where((op == PREFIX) & (kb > 0), 1, 0)
    out = {0: set(), 1: set()}
    for ph in (0, 1):
        sel = (phase == ph) & (op != COPY)
        for k in range(int(nb[sel].max()) if sel.any() else 0):
            nd = int(np.count_nonzero(sel & (nb > k) & (k >= kb)))
            if k <= FUSED_SHALLOW_STEPS and nd >= FUSED_MIN_LEAVES:
                out[ph].add(k)
    return out


def _phase0_of_t1(dat):
    small = [g[0] for g in GEOMETRIES if g[1] <= 640]
    srcs = [f + "/src" for f in small] + ["h0/src", "h2/src"]
    ent = [(k, FULL) for k in srcs]
    ent += [(k, FULL) for k in srcs]                                  # each source again: a FULL leaf on the same list
    ent += [(f"fill/{i:02d}", FULL) for i in range(N_FILL)]
    return small, ent


def table(name):
    dat = data(33 if name == "T4d33" else 3)
    if name == "T1":
        small, ent = _phase0_of_t1(dat)
        ent += [(f + "/leaf", PREFIX) for f in small]
        for fam in HUBS:
            ent += [(k, PREFIX) for k in dat.family_leaves(fam) if "/big" in k]
        ent += [(f"{fam}/{n}", PREFIX) for fam, n, _ in EXTRA_LEAVES if fam != "f256"]
        ent += [("g300_385/copy", COPY), ("g300_385/copyown", COPY)]
        t = Table(name, dat, ent, {0: range(5), 1: range(1, 5)})
        for fam in ("g128_129", "g256_257"):                          # sources with three and more PREFIX leaves
            assert len({t.n[l] for l in t.leaves(PREFIX) if t.keys[t.src[l]] == fam + "/src"}) >= 3
        return t
    if name == "T2":
        ent = [(f + "/src", FULL) for f in T2_SOURCES]
        for fam in T2_SOURCES:
            ent += [(k, PREFIX) for k in dat.family_leaves(fam)]
        t = Table(name, dat, ent, {1: range(2, 5)})
        for fam in T2_SOURCES:
            assert sum(1 for l in t.leaves(PREFIX) if t.keys[t.src[l]] == fam + "/src") >= 9
        return t
    if name == "T3":
        _, ent = _phase0_of_t1(dat)
        ent += [(f + "/leaf", PREFIX) for f in ("g129_130", "g300_385", "g384_640")]
        return Table(name, dat, ent, {0: range(5)})
    if name in ("T4", "T4d33"):
        fams = ("g640_656", "g768_900", "g1024_1025")
        ent = [(f + "/src", FULL) for f in fams] + [(f + "/leaf", PREFIX) for f in fams] + [("g768_900/copy", COPY)]
        return Table(name, dat, ent, {})
    if name == "TD":
        ent = [("g127_300/src", FULL), ("g129_130/src", FULL), ("g300_385/src", FULL), ("g127_300/leaf", PREFIX),
               ("g129_130/leaf", PREFIX), ("g300_385/copyown", COPY)]
        return Table(name, dat, ent, {})
    raise KeyError(name)


TABLES = ("T1", "T2", "T3", "T4", "T4d33", "TD")


def load_golden():
    """tests/golden/gp_sharing.npz by set key: mll, alpha, cond, mu, var, kss (at the set's routed rows)."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp_sharing.npz"))
    out = {}
    for name in z.files:
        key, field = name.rsplit("/", 1)
        v = z[name]
        out.setdefault(key, {})[field] = v if v.ndim else v.item()
    return out
