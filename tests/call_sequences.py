"""Call sequences over the entry points of hipabi.Context while the inputs change: the input pools, the alphabet of writers and
readers, a state model of which reader's inputs are current, a deterministic generator of sequences, and the shortest route
that brings a fresh context to the inputs a history has left.  Pure host: NumPy only, neither hipabi nor torch -- the same
sequences drive the dense float64 oracle chain on the CPU (tests/test_call_sequences_host.py) and one long-lived device context
(tests/test_call_sequences_gpu.py).

The property under test: every sum on the device has a fixed order, so what an entry point returns is a function of the
inputs and of a small, named set of path choices (`Model.path_key`): the options, whether the last fit carried a resident test
set (and which), whether K_tn L^-T comes from that fit or from the standalone sweep, a reserved pool, the gradient mask.
Whatever was called before, a reader returns bit for bit what a fresh context returns on `route(model, reader)`, or refuses
with DSMGP_E_STATE where `Model.ready(reader)` says its chain is broken.

    python -m tests.call_sequences --print ID     one sequence with the model's expectation beside every op
    python -m tests.call_sequences --list         ids and lengths
    python -m tests.call_sequences --write        regenerate tests/golden/call_sequences.json (the committed list)
"""
import functools
import importlib.util
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
COMMITTED = os.path.join(_HERE, "golden", "call_sequences.json")


def _datagen():
    """deepstructuredmixtures_amd/datagen.py by path: importing the package would import hipabi."""
    name = "_call_sequences_datagen"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_HERE, "..", "deepstructuredmixtures_amd", "datagen.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


# include/dsmgp_hip.h (tests/test_call_sequences_host.py compares them with hipabi's)
E_ARG, E_STATE = -1, -2
OPT = {"ard": 1, "fused_gram": 2, "fused_steps": 3, "diag_in_update": 4, "fit_graph": 5, "lanes": 6}
OPT_DEFAULT = {"ard": 0, "fused_gram": 1, "fused_steps": 1, "diag_in_update": 1, "fit_graph": 0, "lanes": 0}
PLAN_OPTIONS = ("fused_gram", "fused_steps", "diag_in_update", "lanes")      # a change discards the plan and the test set
FAMILY = {"mixture": 0, "poe": 1, "gpoe": 2, "rbcm": 3}
POOL_BYTES = 1 << 30        # dsmgp_reserve: every arena of the largest pool configuration (table W: 40 x 384^2 doubles, five arenas) fits
TB = 128                    # rows of a tile: what npad and the test tiles are rounded to
TQ = 16                     # columns of the f64 MFMA tile: what Q is rounded to

# ------------------------------------------------------------------------------------------------ the input pools

TRAIN = {"A": (1500, 2, 7101), "B": (1200, 5, 7102)}        # key -> (N, D, seed)


@functools.lru_cache(maxsize=None)
def train(key):
    N, D, seed = TRAIN[key]
    X, y, _ = _datagen().regression_data(N, D, n_test=1, seed=seed)
    return X, y


S_SIZES = (1, 100, 128, 129, 257, 300)


@functools.lru_cache(maxsize=None)
def leaves(key):
    """dict(obs_ptr, obs_idx, kid, shift, op, src, plen): `shift` is added to the leaf's mean of y; op / src / plen are the
    declared sharing schedule (all FULL for W and T).
    S: n = 1, 100, 128, 129, 257, 300, a COPY of the 129-row leaf (a mean of its own, test rows of its own) and a PREFIX leaf
       continuing the 129-row leaf to 300 rows; the 257-row leaf alone has kernel id 1 (the poison step fails it alone).
    W: 40 overlapping leaves of 130 .. 260 rows, kernel ids alternating: >= 32 leaves in the shallow block steps.
    T: one leaf of 300 rows (every other row)."""
    if key == "S":
        obs = [np.arange(0, 1), np.arange(1, 101), np.arange(101, 229), np.arange(300, 429), np.arange(600, 857),
               np.arange(860, 1160), np.arange(300, 429), np.arange(300, 600)]
        assert tuple(o.size for o in obs[:6]) == S_SIZES
        kid = [0, 0, 0, 0, 1, 0, 0, 0]
        op, src, plen = [0, 0, 0, 0, 0, 0, 1, 2], [-1, -1, -1, -1, -1, -1, 3, 3], [0, 0, 0, 0, 0, 0, 0, 129]
        shift = [0.0, 0.0, 0.01, 0.0, -0.02, 0.0, 0.1, 0.03]
    elif key == "W":
        obs = [np.arange((29 * i) % 900, (29 * i) % 900 + 130 + (37 * i) % 131) for i in range(40)]
        kid = [i % 2 for i in range(40)]
        op, src, plen = [0] * 40, [-1] * 40, [0] * 40
        shift = [0.01 * (i % 3) for i in range(40)]
    else:
        obs, kid, op, src, plen, shift = [np.arange(0, 600, 2)], [0], [0], [-1], [0], [0.05]
    ptr = np.concatenate([[0], np.cumsum([o.size for o in obs])]).astype(np.int64)
    return dict(obs_ptr=ptr, obs_idx=np.concatenate(obs).astype(np.int64), kid=np.array(kid, dtype=np.int32),
                shift=np.array(shift), op=np.array(op, dtype=np.int32), src=np.array(src, dtype=np.int32),
                plen=np.array(plen, dtype=np.int64), obs=obs)


def leaf_means(train_key, leaves_key):
    y = train(train_key)[1]
    lv = leaves(leaves_key)
    return np.array([float(np.mean(y[o])) for o in lv["obs"]]) + lv["shift"]


# one hyper-vector class per device kernel class (IsoSE, ArdSE, ArdLinear, ArdSEProduct, IsoMatern52, ArdMatern52, ArdRQ)
KIND = {"isose": 0, "ardse": 1, "ardlin": 3, "ardprod": 4, "isomat52": 6, "ardmat52": 8, "ardrq": 10}
ARD = ("ardse", "ardlin", "ardprod", "ardmat52", "ardrq")
POISON_KID = 1
POISON = (2, (-18.0, 0.0, -30.0))      # IsoLinear, l = exp(-18), noise exp(-60): a rank-D Gram of size 1e15, not positive definite


def hyper(cls, vs, D):
    """(kind, log-scale hyper-vector) of class `cls`, value set "a" or "b": length-scales 0.3 .. 1.5, noise 0.1 / 0.3."""
    if cls == "poison":
        return POISON[0], np.array(POISON[1])
    b = vs == "b"
    ls = (np.linspace(1.5, 0.4, D) if b else np.linspace(0.3, 1.5, D)) if cls in ARD else np.array([0.9 if b else 0.5])
    shape = [np.log(0.7 if b else 1.5)] if cls == "ardrq" else []
    logs = 0.0 if cls == "ardlin" else (np.log(1.3) if b else 0.0)
    return KIND[cls], np.concatenate([np.log(ls), shape, [logs, np.log(0.3 if b else 0.1)]])


TEST_KEYS = ("t0", "t1", "t15", "t40", "t200", "routed")
_T200 = (5, 129, 5, 200, 5, 5, 150, 5)


def test_counts(key, L):
    if key == "t0":
        return [0] * L
    if key == "t200":
        return [_T200[(l + 3) % 8 if L == 1 else l % 8] for l in range(L)]
    c = [int(key[1:])] * L
    if key == "t15" and L > 1:
        c[0] = 0                                        # one leaf without routed rows
    return c


@functools.lru_cache(maxsize=None)
def testset(key, leaves_key, D):
    """(Xt, route_ptr, route_idx) of a host-routed test set: the leaf with the most rows takes every row (no test row is left
    without a leaf), leaf l the rows (5 l + k) mod n_t, ascending."""
    L = leaves(leaves_key)["kid"].size
    counts = test_counts(key, L)
    n_t = max(4, max(counts)) if key == "t0" else max(counts)
    idx = [np.sort((5 * l + np.arange(c)) % n_t) for l, c in enumerate(counts)]
    if key == "t1" and L > 1:       # two rows, so that the scores' standard errors exist; leaf l takes row l mod 2
        n_t, idx = 2, [np.array([l % 2]) for l in range(L)]
    Xt = np.asfortranarray(_datagen().uniform(7200 + TEST_KEYS.index(key), 0, n_t * D).reshape((n_t, D), order="F"))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return Xt, ptr, (np.concatenate(idx) if ptr[-1] else np.zeros(0)).astype(np.int64)


def tree():
    """A small tree over table S for dsmgp_set_tree: a sum root over two split nodes (dimension 0: leaves 1, 2, 3; dimension 1:
    leaves 5, 7), breadth-first as tree._RouteIndex lays it out.  Leaves 0, 4 and 6 get no rows."""
    inf = np.inf
    return dict(kind=np.array([2, 1, 1, 0, 0, 0, 0, 0], dtype=np.int8), first=np.array([1, 3, 6, 8, 8, 8, 8, 8], dtype=np.int64),
                nchild=np.array([2, 3, 2, 0, 0, 0, 0, 0], dtype=np.int64), sdim=np.array([0, 0, 1, 0, 0, 0, 0, 0], dtype=np.int64),
                thr=np.array([[inf] * 3, [0.3, 0.6, 1.0], [0.5, 1.0, inf]] + [[inf] * 3] * 5),
                leaf=np.array([-1, -1, -1, 1, 2, 3, 5, 7], dtype=np.int64))


@functools.lru_cache(maxsize=None)
def routed_testset(D):
    """(Xt, route_ptr, route_idx) of the device-routed test set: the CSR is the host restatement of the walk over `tree()`."""
    n_t = 37
    Xt = np.asfortranarray(_datagen().uniform(7290, 0, n_t * D).reshape((n_t, D), order="F"))
    rows = [[] for _ in range(8)]
    for r in range(n_t):
        rows[(1, 2, 3)[int(np.searchsorted([0.3, 0.6, 1.0], Xt[r, 0]))]].append(r)
        rows[(5, 7)[int(np.searchsorted([0.5, 1.0], Xt[r, 1]))]].append(r)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.int64)
    return Xt, ptr, np.concatenate([np.array(x, dtype=np.int64) for x in rows])


def current_test(m):
    return routed_testset(m.D) if m.test == "routed" else testset(m.test, m.leaves, m.D)


def y_test(Xt):
    return np.sin(3.0 * Xt[:, 0]) + 0.2 * Xt[:, -1]


TARGET_Q = {"q1": 1, "q3": 3, "q16": 16, "q17": 17}


@functools.lru_cache(maxsize=None)
def targets(key, train_key, leaves_key):
    """(Y[N, Q], mean[L, Q], weight[L, Q]): smooth columns of different scale plus noise, the leaf's column means plus a shift,
    non-uniform non-negative weights with zeros (what both gradient calls accept)."""
    Q = TARGET_Q[key]
    X, y = train(train_key)
    N = X.shape[0]
    lv = leaves(leaves_key)
    z = _datagen().normal(7300 + Q, 0, N * Q).reshape((N, Q), order="F")
    Y = np.stack([y if q == 0 else (1.0 + 0.5 * q) * np.sin((1.0 + 0.3 * q) * X[:, q % X.shape[1]] + q) + 0.2 * q
                  for q in range(Q)], axis=1) + 0.1 * z * (np.arange(Q) > 0)
    mean = np.stack([np.mean(Y[o], axis=0) for o in lv["obs"]]) + 0.01 * lv["shift"][:, None]
    L = lv["kid"].size
    w = np.array([[0.0 if (l + 2 * q) % 7 == 3 else 0.5 + 0.25 * ((l + 2 * q) % 5) for q in range(Q)] for l in range(L)])
    return np.asfortranarray(Y), mean, w


def mask(key, L):
    return None if key is None else np.array([l % 2 == 0 for l in range(L)], dtype=np.int32)


def agg_args(family, L):
    """(leaf_coef, leaf_group, n_groups, prior_kernel_id): mixture weights 1 / L (they sum to at most 1 over the leaves of a
    row, so the mixture variance stays positive), PoE 1, gPoE 1 / 2, rBCM two groups by leaf parity and the prior of kernel id 0."""
    if family == "rbcm":
        return None, np.arange(L, dtype=np.int32) % 2, 2, 0
    return np.full(L, {"mixture": 1.0 / L, "poe": 1.0, "gpoe": 0.5}[family]), None, 0, 0


# ------------------------------------------------------------------------------------------------ the alphabet

# Writers (classes): every op that writes state.  A sequence holds concrete instances (op, argument).
WRITERS = ("set_train", "set_leaves", "set_sharing", "set_hyper_values", "set_hyper_kind", "set_test", "set_test_routed",
           "set_joint", "opt_ard", "opt_fused_gram", "opt_fused_steps", "opt_lanes", "opt_diag_in_update", "opt_fit_graph",
           "set_gradient_leaves", "reserve", "release", "fit", "predict_run", "solve_targets", "refused", "poison_then_healthy")

# Readers: "name" or "name.argument".  fit, solve_targets and aggregate_partial are writers whose outputs are read as well.
READERS = ("fit", "download_factor", "predict_fetch", "predict_cov", "predict_gradients.var", "predict_gradients.mean",
           "aggregate.mixture", "aggregate.poe", "aggregate.gpoe", "aggregate.rbcm",
           "aggregate_partial.mixture", "aggregate_partial.poe", "aggregate_partial.gpoe", "aggregate_partial.rbcm",
           "aggregate_finish", "scores", "gradients", "loo", "loo_gradients", "solve_targets", "targets_fetch", "predict_targets",
           "targets_gradients", "loo_targets", "loo_targets_gradients", "routes", "kernel_matrix")

# What a reader needs current, from the words of include/dsmgp_hip.h:
#   fit        "Needs a fit" / "DSMGP_E_STATE ... before fit": dsmgp_download_factor, dsmgp_gradients, dsmgp_loo ("Needs a fit"),
#              dsmgp_loo_gradients ("Needs a fit (DSMGP_E_STATE)"), dsmgp_solve_targets ("Needs a fit on the current leaf table")
#   pred       "Needs dsmgp_predict_run on the current fit (DSMGP_E_STATE otherwise)": dsmgp_predict_cov, dsmgp_predict_gradients;
#              dsmgp_predict_fetch and dsmgp_aggregate* read "the moments the last dsmgp_predict_run left in HBM"
#   targets    "Needs a fit and a dsmgp_solve_targets on the CURRENT fit (DSMGP_E_STATE otherwise)": dsmgp_mll_columns_gradients,
#              dsmgp_loo_columns*, dsmgp_targets_fetch; dsmgp_predict_targets "Needs BOTH dsmgp_solve_targets and dsmgp_predict_run"
#   partial    dsmgp_aggregate_finish: the context's own sums of dsmgp_aggregate_partial
#   done       dsmgp_scores: "the aggregated prediction still in HBM"
#   test       dsmgp_routes: "the CSR of the registered test set"
#   hyper      dsmgp_kernel_matrix: the hyper-vector of the kernel id
NEEDS = {"fit": ("leaves", "hyper"), "download_factor": ("fit",), "predict_fetch": ("pred",), "predict_cov": ("pred",),
         "predict_gradients": ("pred",), "aggregate": ("pred",), "aggregate_partial": ("pred",), "aggregate_finish": ("partial",),
         "scores": ("done",), "gradients": ("fit",), "loo": ("fit",), "loo_gradients": ("fit",), "solve_targets": ("fit",),
         "targets_fetch": ("targets",), "predict_targets": ("targets", "pred"), "targets_gradients": ("targets",),
         "loo_targets": ("targets",), "loo_targets_gradients": ("targets",), "routes": ("test",), "kernel_matrix": ("hyper",)}

# Where the header says in words that a call returns what an EARLIER call left although an input has changed since: none.
# (dsmgp_routes and dsmgp_kernel_matrix keep answering after set_hyper / fit because neither is among their inputs.)
EXCEPTIONS = {}

# Readers that share an arena or a product, from struct dsmgp_ctx (csrc/dsmgp_hip.cpp) and csrc/ctx_state.hpp: every ordered pair inside a
# group must appear back to back in some sequence.
SHARING = {
    "arenaX / P_XINV (L^-T of every factor owner)": ("gradients", "loo", "loo_gradients", "predict_gradients.var",
                                                       "targets_gradients", "loo_targets", "loo_targets_gradients"),
    "P_ALPHA / P_DINV (ensure_alpha, ensure_dinv)": ("download_factor", "gradients", "loo", "loo_gradients",
                                                                "predict_gradients.mean", "solve_targets"),
    "arenaVt / P_VT, arenaCov, arenaB (K_tn L^-T and what is made from it)": ("predict_fetch", "predict_cov",
                                                                                 "predict_gradients.var", "predict_targets"),
    "arenaPV, d_agg_part, d_agg_out / P_PRED, P_PARTIAL, P_TOTAL, P_DONE": ("predict_fetch", "aggregate.mixture", "aggregate.rbcm",
                                                    "aggregate_partial.poe", "aggregate_finish", "scores"),
    "arenaT, arenaA, arenaHc, arenaU / P_Z, P_TG_LISTS": ("solve_targets", "targets_fetch", "predict_targets", "targets_gradients",
                                                             "loo_targets", "loo_targets_gradients"),
    "d_kp (the KParam table)": ("kernel_matrix", "fit", "aggregate.rbcm"),
}

# Sized quantities: the op that sets them and one value on each side of the granule (small, large)
SIZED = {"npad": ("set_leaves", "T", "S"),          # one leaf of 300 rows (384) <-> leaves of 1 .. 300 rows (128 .. 384), offsets move
         "L": ("set_leaves", "S", "W"),             # 8 <-> 40 leaves
         "D": ("set_train", "A", "B"),              # 2 <-> 5 input dimensions
         "Qpad": ("solve_targets", "q3", "q17"),    # 16 <-> 32 padded columns
         "test_rows": ("set_test", "t15", "t200"),  # one test tile <-> a second test tile
         "route_total": ("set_test", "t1", "t40")}
SIZED_FAMILIES = {"npad": ("fit", "download_factor", "gradients", "loo", "loo_gradients", "predict_fetch", "targets_fetch", "loo_targets"),
                  "L": ("fit", "gradients", "loo", "predict_fetch", "aggregate.mixture", "targets_gradients", "loo_targets_gradients"),
                  "D": ("fit", "kernel_matrix", "gradients", "loo_gradients", "predict_gradients.var", "targets_gradients"),
                  "Qpad": ("solve_targets", "targets_fetch", "predict_targets", "targets_gradients", "loo_targets", "loo_targets_gradients"),
                  "test_rows": ("predict_fetch", "predict_cov", "predict_gradients.var", "predict_targets", "aggregate.rbcm", "scores", "routes"),
                  "route_total": ("predict_fetch", "predict_gradients.mean", "predict_targets", "aggregate.poe", "routes")}


def split(reader):
    name, _, arg = reader.partition(".")
    return name, arg


def call_id(op, arg):
    """The reader call an op of a sequence makes ("aggregate.poe", "solve_targets.q17", "loo"), or None for a pure writer."""
    return (op if arg is None else f"{op}.{arg}") if op in NEEDS else None


def reader_id(op, arg):
    """Its entry in READERS: the columns of solve_targets are an input, not another reader."""
    return "solve_targets" if op == "solve_targets" else call_id(op, arg)


# ------------------------------------------------------------------------------------------------ the state model

class Model:
    """What the context holds after a history, as far as results depend on it.  `apply(op, arg)` returns None where the call
    succeeds and the expected error code where it must be refused (nothing changes then); `ready(reader)` says whether the
    reader's chain is unbroken: hyper -> fit -> {gradients, loo, ...}; fit + test set -> predict_run -> aggregate -> scores;
    fit -> solve_targets -> {targets_*, loo_targets_*}; predict_run + solve_targets -> predict_targets."""

    def __init__(self):
        self.train = self.leaves = self.test = self.mask = self.targets = self.fit_test = self.agg = None
        self.sharing = "full"
        self.hyper = {}                 # kernel id -> (class, value set)
        self.opts = dict(OPT_DEFAULT)
        self.joint = True
        self.reserved = self.tree = self.fitted = self.ride = self.predicted = self.targets_valid = False

    @property
    def D(self):
        return TRAIN[self.train][1]

    @property
    def L(self):
        return int(leaves(self.leaves)["kid"].size)

    @property
    def poisoned(self):
        return any(v[0] == "poison" for v in self.hyper.values())

    def _drop_test(self):
        self.test = None
        self.predicted = self.ride = False
        self.agg = None
        if self.reserved:               # the pool is a stack: the targets sit above the test set (free_test)
            self.targets_valid = False

    def _drop_plan(self):
        self.fitted = self.targets_valid = False
        self.fit_test = None
        self._drop_test()

    def has(self, what):
        if what == "leaves":
            return self.leaves is not None
        if what == "hyper":
            return self.leaves is not None and all(int(k) in self.hyper for k in leaves(self.leaves)["kid"])
        if what == "fit":
            return self.fitted
        if what == "test":
            return self.test is not None
        if what == "pred":
            return self.fitted and self.predicted
        if what == "targets":
            return self.fitted and self.targets_valid
        if what == "partial":
            return self.agg is not None
        if what == "done":
            return self.agg is not None and self.agg[1] == "done"
        raise KeyError(what)

    def ready(self, reader):
        return all(self.has(w) for w in NEEDS[split(reader)[0]])

    def apply(self, op, arg=None):
        """Writers and the readers that change state.  Returns the expected error code, or None."""
        if op == "refused":
            if arg == "bad_targets":
                return E_ARG if self.fitted else E_STATE
            return E_ARG                                    # bad_option, bad_sharing, bad_hyper: argument checks only
        if op in NEEDS:
            if not self.ready(op if arg is None else f"{op}.{arg}"):
                return E_STATE
        if op == "set_train":
            self._drop_plan()
            self.train, self.leaves, self.sharing, self.mask, self.tree = arg, None, "full", None, False
            self.hyper = {}     # the library keeps them; a vector of another D is refused, so every sequence sets them again
        elif op == "set_leaves":
            self._drop_plan()
            self.leaves, self.sharing, self.mask, self.tree = arg, "full", None, False
        elif op == "set_sharing":
            self._drop_plan()
            self.sharing = arg
        elif op == "set_hyper":
            self.hyper[int(arg[0])] = (arg[1], arg[2])
            self.fitted = self.predicted = self.ride = False
            self.agg = None
        elif op == "set_option":
            name, value = arg
            if name in PLAN_OPTIONS and self.opts[name] != value:
                self._drop_plan()
            self.opts[name] = value
        elif op == "set_joint":
            self.joint = bool(arg)
        elif op == "set_gradient_leaves":
            self.mask = arg
        elif op == "reserve":
            self._drop_plan()
            self.reserved = bool(arg)
        elif op == "release":
            self._drop_plan()
        elif op == "set_tree":
            self.tree = True
        elif op == "set_test":
            if arg == "routed" and not self.tree:
                return E_STATE
            self.predicted = self.ride = False
            self.agg = None
            if self.reserved:
                self.targets_valid = False
            self.test = arg
        elif op == "fit":
            self.fitted = True
            self.predicted = self.targets_valid = False
            self.agg = None
            self.ride = self.joint and self.test is not None
            self.fit_test = self.test if self.ride else None
        elif op == "predict_run":
            if not (self.fitted and self.test is not None):
                return E_STATE
            self.predicted = True
            self.agg = None
        elif op == "solve_targets":
            self.targets, self.targets_valid = arg, True
        elif op == "aggregate_partial":
            self.agg = (arg, "partial")
        elif op == "aggregate":
            self.agg = (arg, "done")
        elif op == "aggregate_finish":
            self.agg = (self.agg[0], "done")
        return None

    # -- what results depend on
    def input_key(self, reader):
        """The inputs of `reader` (what the dense reference is a function of)."""
        name, arg = split(reader)
        key = [name, arg, self.train, self.leaves, tuple(sorted(self.hyper.items()))]
        need = NEEDS[name]
        if "pred" in need or "partial" in need or "done" in need or "test" in need:
            key.append(self.test)
        if "targets" in need:
            key.append(self.targets)
        if name in ("aggregate_finish", "scores"):
            key.append(self.agg[0])
        if name in ("gradients", "targets_gradients"):
            key.append(self.opts["ard"])
        if name == "gradients":
            key.append(self.mask)
        return tuple(key)

    def path_key(self, reader):
        """The inputs and the path-defining state: what the bits are a function of."""
        name = split(reader)[0]
        need = NEEDS[name]
        path = [self.sharing, tuple(sorted(self.opts.items())), self.reserved]
        if name == "fit":       # the fit about to run: it carries the test set registered now
            return self.input_key(reader) + tuple(path) + (self.test if self.joint else None,)
        path.append(self.fit_test if self.fitted else None)
        if "pred" in need or "partial" in need or "done" in need:
            path.append(self.ride)
        return self.input_key(reader) + tuple(path)


def prerequisites(m, reader, defaults=None):
    """The fewest ops that make `reader` ready on a context in state `m` (a copy is advanced; `m` is not touched)."""
    import copy
    d = dict(test="t15", targets="q3", family="poe")
    d.update(defaults or {})
    m = copy.deepcopy(m)
    ops = []

    def do(op, arg=None):
        ops.append([op, arg])
        assert m.apply(op, arg) is None, (op, arg)

    name, arg = split(reader)
    need = NEEDS[name]
    chain = {"pred", "targets", "partial", "done", "fit"} & set(need)
    if chain and not m.fitted:
        do("fit")
    if {"pred", "partial", "done"} & set(need) and not m.predicted:
        if m.test is None:
            do("set_test", d["test"])
        do("predict_run")
    if "test" in need and m.test is None:
        do("set_test", d["test"])
    if "targets" in need and not m.targets_valid:
        do("solve_targets", m.targets or d["targets"])
    if "partial" in need and m.agg is None:
        do("aggregate_partial", d["family"])
    if "done" in need and not m.has("done"):
        do("aggregate", m.agg[0] if m.agg else d["family"])
    return ops


def route(m, reader):
    """The shortest call list that brings a fresh context to the inputs and the path-defining state of `m`, up to (not
    including) `reader`: set_train, set_leaves, set_sharing, the options that differ from their defaults, reserve if reserved,
    set_hyper, the test set BEFORE the fit if and only if the last fit carried one (the set it carried, which a later
    set_test may have replaced: the factor's split-K order belongs to the lists that fit ran), fit if the history's fit is
    current, and then only the reader's own prerequisites."""
    name, arg = split(reader)
    ops = [["set_train", m.train]]
    if m.leaves is None:
        return ops
    ops.append(["set_leaves", m.leaves])
    if m.sharing != "full":
        ops.append(["set_sharing", m.sharing])
    ops += [["set_option", [k, v]] for k, v in sorted(m.opts.items()) if v != OPT_DEFAULT[k]]
    if m.reserved:
        ops.append(["reserve", 1])
    ops += [["set_hyper", [k, v[0], v[1]]] for k, v in sorted(m.hyper.items())]
    fresh = Model()
    for op, a in ops:
        assert fresh.apply(op, a) is None
    tail = []

    def do(op, a=None):
        tail.append([op, a])
        assert fresh.apply(op, a) is None, (op, a)

    need = NEEDS[name]
    if name == "fit":       # the reader is the fit itself: its test set is the one registered now
        if m.test is not None and m.joint:
            if m.test == "routed":
                do("set_tree")
            do("set_test", m.test)
        return ops + tail
    if m.fitted:
        if m.fit_test is not None:
            if m.fit_test == "routed":
                do("set_tree")
            do("set_test", m.fit_test)
        do("fit")
    if {"pred", "partial", "done", "test"} & set(need) and m.test is not None:
        if not (fresh.test == m.test and fresh.ride == m.ride):
            if m.test == "routed" and not fresh.tree:
                do("set_tree")
            do("set_test", m.test)
        if {"pred", "partial", "done"} & set(need) and m.predicted:
            do("predict_run")
    if ("targets" in need) and m.targets_valid:
        do("solve_targets", m.targets)
    if "partial" in need and m.agg is not None:
        do("aggregate_partial", m.agg[0])
    if "done" in need and m.has("done"):
        do("aggregate", m.agg[0])
    if name == "gradients" and m.mask is not None:
        do("set_gradient_leaves", m.mask)
    return ops + tail


# ------------------------------------------------------------------------------------------------ running ops on a context

def run_op(ctx, m, op, arg):
    """One writer on `ctx` (hipabi.Context or the oracle chain: the same methods); `m` is the model BEFORE the op.  Returns what
    the op reads back (fit, solve_targets, aggregate_partial), else None."""
    if op == "set_train":
        ctx.set_train(*train(arg))
    elif op == "set_leaves":
        lv = leaves(arg)
        ctx.set_leaves(lv["obs_ptr"], lv["obs_idx"], lv["kid"], leaf_means(m.train, arg))
    elif op == "set_sharing":
        lv = leaves(m.leaves)
        if arg == "declared":
            ctx.set_sharing(lv["op"], lv["src"], lv["plen"])
        else:
            ctx.set_sharing(None, None, None)
    elif op == "set_hyper":
        kind, vec = hyper(arg[1], arg[2], m.D)
        ctx.set_hyper(int(arg[0]), kind, vec)
    elif op == "set_option":
        ctx.set_option(OPT[arg[0]], int(arg[1]))
    elif op == "set_joint":
        ctx.set_joint(bool(arg))
    elif op == "set_gradient_leaves":
        ctx.set_gradient_leaves(mask(arg, m.L))
    elif op == "reserve":
        ctx.reserve(POOL_BYTES if arg else 0)
    elif op == "release":
        ctx.release()
    elif op == "set_tree":
        t = tree()
        ctx.set_tree(t["kind"], t["first"], t["nchild"], t["sdim"], t["thr"], t["leaf"])
    elif op == "set_test":
        if arg == "routed":
            ctx.set_test_routed(routed_testset(m.D)[0])
        else:
            ctx.set_test(*testset(arg, m.leaves, m.D))
    elif op == "predict_run":
        ctx.predict_run()
    elif op == "refused":
        if arg == "bad_option":
            ctx.set_option(OPT["lanes"], 9)
        elif arg == "bad_hyper":
            ctx.set_hyper(0, 99, [0.0, 0.0, 0.0])
        elif arg == "bad_sharing":
            L = m.L
            ctx.set_sharing(np.ones(L, dtype=np.int32), np.arange(L, dtype=np.int32), np.zeros(L, dtype=np.int64))
        else:
            Y = targets("q1", m.train, m.leaves)[0].copy()
            Y[3, 0] = np.nan
            ctx.solve_targets(Y)
    else:
        return read(ctx, m, op if arg is None else f"{op}.{arg}")
    return None


def read(ctx, m, reader):
    """One reader on `ctx`; `m` is the model before the call.  Returns a tuple of float64 / int64 arrays."""
    name, arg = split(reader)
    L = m.L
    stride = m.D + 3
    if name == "fit":
        mll, info = ctx.fit()[:2]
        return mll, np.asarray(info, dtype=np.int64)
    if name == "download_factor":
        out = []
        for l in sorted({0, L - 1}):
            out += list(ctx.download_factor(l, int(leaves(m.leaves)["obs"][l].size)))
        return tuple(out)
    if name == "predict_fetch":
        return tuple(ctx.predict_fetch())
    if name == "predict_cov":
        ptr = current_test(m)[1] if m.test else np.array([0, 1])       # (no test set: the call is refused)
        l = int(np.argmax(np.diff(ptr)))
        return (ctx.predict_cov(l, int(ptr[l + 1] - ptr[l]), with_noise=True),)
    if name == "predict_gradients":
        dmu, dvar = ctx.predict_gradients(want_var=arg == "var")
        return (dmu, dvar) if arg == "var" else (dmu,)
    if name in ("aggregate", "aggregate_partial"):
        coef, group, G, prior = agg_args(arg, L)
        if name == "aggregate_partial":
            return (ctx.aggregate_partial(FAMILY[arg], coef, group, G),)
        return tuple(ctx.aggregate(FAMILY[arg], coef, group, G, plain=False, prior_kernel_id=prior))
    if name == "aggregate_finish":
        return tuple(ctx.aggregate_finish(None, plain=False, prior_kernel_id=0))
    if name == "scores":
        sc = ctx.scores(y_test(current_test(m)[0]) if m.test else np.zeros(getattr(ctx, "n_t", 0)))
        return (np.array([sc[k] for k in ("mse", "sse", "mae", "sae", "nlpd")]),)
    if name == "gradients":
        return (ctx.gradients(stride),)
    if name == "loo":
        return tuple(ctx.loo())
    if name == "loo_gradients":
        return tuple(ctx.loo_gradients(stride))
    if name == "solve_targets":
        Y, mean, _ = targets(arg, m.train, m.leaves)
        return (ctx.solve_targets(Y, mean)[0],)
    if name == "targets_fetch":
        return (ctx.targets_fetch(L - 1),)
    if name == "predict_targets":
        return (ctx.predict_targets(),)
    if name == "targets_gradients":
        return (ctx.targets_gradients(stride, targets(m.targets, m.train, m.leaves)[2] if m.targets_valid else None),)
    if name == "loo_targets":
        return tuple(ctx.loo_targets())
    if name == "loo_targets_gradients":
        return tuple(ctx.loo_targets_gradients(stride, targets(m.targets, m.train, m.leaves)[2] if m.targets_valid else None))
    if name == "routes":
        return tuple(np.asarray(a, dtype=np.int64) for a in ctx.routes())
    if name == "kernel_matrix":
        X = train(m.train)[0]
        return tuple(ctx.kernel_matrix(k, np.asfortranarray(X[:130]), np.asfortranarray(X[130:263])) for k in sorted(m.hyper))
    raise KeyError(reader)


# ------------------------------------------------------------------------------------------------ the generator

class _Seq:
    """A sequence under construction: ops go through a model so that every emitted prerequisite is the minimal one."""

    def __init__(self, sid):
        self.id, self.ops, self.m = sid, [], Model()

    def do(self, op, arg=None):
        self.ops.append([op, arg])
        return self.m.apply(op, arg)

    def base(self, tr="A", lv="S", sharing="declared", h0=("isose", "a"), h1=("ardmat52", "a")):
        self.do("set_train", tr)
        self.do("set_leaves", lv)
        if sharing != "full":
            self.do("set_sharing", sharing)
        self.hypers(h0, h1)

    def hypers(self, h0, h1):
        self.do("set_hyper", [0, h0[0], h0[1]])
        self.do("set_hyper", [1, h1[0], h1[1]])

    def reach(self, reader, **defaults):
        """The reader's minimal prerequisites, then the reader."""
        for op, arg in prerequisites(self.m, reader, defaults):
            self.do(op, arg)
        name, arg = split(reader)
        if name == "solve_targets":
            arg = defaults.get("targets") or self.m.targets or "q3"
        self.do(name, arg or None)

    def full(self, test="t15", tg="q3"):
        """Everything current: fit, predict_run, targets, an aggregate."""
        self.do("fit")
        self.do("set_test", test)
        self.do("predict_run")
        self.do("solve_targets", tg)
        self.do("aggregate", "rbcm")


_HYPER_CYCLE = [("isose", "a"), ("ardse", "a"), ("ardlin", "a"), ("ardprod", "a"), ("isomat52", "a"), ("ardmat52", "a"),
                ("ardrq", "a"), ("isose", "b"), ("ardse", "b"), ("ardlin", "b"), ("ardprod", "b"), ("isomat52", "b"),
                ("ardmat52", "b"), ("ardrq", "b")]


# what the header promises NaN rows for under a failed leaf (the aggregates mix leaves; a failed leaf's factor is not defined)
POISON_READERS = ("fit", "predict_fetch", "predict_gradients.var", "gradients", "loo", "loo_gradients", "solve_targets", "targets_fetch",
                  "predict_targets", "targets_gradients", "loo_targets", "loo_targets_gradients", "routes", "kernel_matrix")
NEEDS_ROWS = ("aggregate", "aggregate_partial", "aggregate_finish", "scores", "predict_cov")     # no 0 / 0, no 0 x 0 matrix


def _writer_instances(s, w, i, r="fit"):
    """The i-th instance of writer class `w` on the sequence's current state, as a list of ops (the setters that a writer
    needs to leave a usable context ride along: new training data come with their leaf table and hyper-vectors)."""
    m = s.m
    if w == "set_train":
        tr = "B" if m.train == "A" else "A"
        return [["set_train", tr], ["set_leaves", "S"], ["set_sharing", "declared"], ["set_hyper", [0, "isose", "a"]],
                ["set_hyper", [1, "ardmat52", "a"]]]
    if w == "set_leaves":
        lv = ("T", "S")[i % 2] if m.leaves != "T" else "S"
        return [["set_leaves", lv]] + ([["set_sharing", "declared"]] if lv == "S" else [])
    if w == "set_sharing":
        return [["set_sharing", "full" if m.sharing == "declared" else "declared"]]
    if w == "set_hyper_values":
        cls, vs = m.hyper[0]
        return [["set_hyper", [0, cls, "b" if vs == "a" else "a"]]]
    if w == "set_hyper_kind":
        cls = _HYPER_CYCLE[(i + 1) % 7][0]
        if cls == m.hyper[0][0]:
            cls = _HYPER_CYCLE[(i + 2) % 7][0]
        return [["set_hyper", [0, cls, "a"]]]
    if w == "set_test":
        keys = ("t1", "t40", "t15", "t200") + (() if split(r)[0] in NEEDS_ROWS else ("t0",))
        k = keys[i % len(keys)]
        return [["set_test", keys[(i + 1) % len(keys)] if k == m.test else k]]
    if w == "set_test_routed":
        return ([] if m.tree else [["set_tree", None]]) + [["set_test", "routed"]]
    if w == "set_joint":
        return [["set_joint", 0 if m.joint else 1]]
    if w.startswith("opt_"):
        name = w[4:]
        if name == "lanes":
            return [["set_option", [name, (1, 2, 0)[i % 3] if m.opts[name] != (1, 2, 0)[i % 3] else (2, 0, 1)[i % 3]]]]
        return [["set_option", [name, 0 if m.opts[name] else 1]]]
    if w == "set_gradient_leaves":
        return [["set_gradient_leaves", None if m.mask else "m1"]]
    if w == "reserve":
        return [["reserve", 0 if m.reserved else 1]]
    if w == "release":
        return [["release", None]]
    if w == "fit":
        return [["fit", None]]
    if w == "predict_run":
        return [["predict_run", None]] if m.fitted and m.test else prerequisites(m, "predict_fetch")
    if w == "solve_targets":
        keys = ("q1", "q17", "q3", "q16")
        return ([] if m.fitted else [["fit", None]]) + [["solve_targets", keys[i % 4] if keys[i % 4] != m.targets else keys[(i + 1) % 4]]]
    if w == "refused":
        return [["refused", ("bad_option", "bad_hyper", "bad_sharing", "bad_targets")[i % 4]]]
    raise KeyError(w)


def generate():
    """The list of sequences: dict(id, ops).  Deterministic: no clock, no hash(), no random draws."""
    out = []

    # (1) every writer before every reader: w, the reader's minimal prerequisites, the reader.  Two halves per writer.
    for w in WRITERS:
        if w == "poison_then_healthy":
            continue
        for half in range(2):
            s = _Seq(f"writer-{w}-{half}")
            s.base()
            s.full()
            rs = READERS[half::2]
            for i, r in enumerate(rs):
                for op, arg in _writer_instances(s, w, 2 * i + half, r):
                    s.do(op, arg)
                if s.m.test == "t0" and split(r)[0] in NEEDS_ROWS:
                    s.do("set_test", "t1")
                s.reach(r)
            out.append(s)

    # (2) every broken chain once: the writer, then every reader whose chain it breaks (refused), then a healthy one
    for w in WRITERS:
        if w in ("poison_then_healthy", "refused"):
            continue
        s = _Seq(f"broken-{w}")
        s.base()
        s.full()
        for op, arg in _writer_instances(s, w, 0):
            s.do(op, arg)
        broken = [r for r in READERS if not s.m.ready(r) and r not in ("fit",)]
        for r in broken:
            name, arg = split(r)
            if name == "solve_targets":
                arg = "q3"
            s.do(name, arg or None)
        for r in ("loo", "predict_fetch", "scores", "targets_fetch"):
            s.reach(r)
        out.append(s)
    # the staleness this work started from: partial sums and aggregated moments of an earlier fit
    s = _Seq("broken-aggregate-after-refit")
    s.base()
    s.do("fit")
    s.do("set_test", "t40")
    s.do("predict_run")
    s.do("aggregate_partial", "rbcm")
    s.do("set_hyper", [0, "isose", "b"])
    s.do("aggregate_finish")
    s.do("scores")
    s.do("fit")
    s.do("aggregate_finish")
    s.do("scores")
    s.do("predict_run")
    s.do("aggregate_finish")
    s.reach("aggregate_finish", family="rbcm")
    s.reach("scores")
    s.do("fit")                     # a refit alone (the same hyper-parameters) drops them as well
    s.do("scores")
    s.reach("scores")
    out.append(s)

    # (3) ordered pairs of readers that share an arena or a flag: a refit, r1 by its prerequisites, r2 by its own
    for gi, (group, rs) in enumerate(SHARING.items()):
        pairs = [(a, b) for a in rs for b in rs if a != b]
        for part in range(0, len(pairs), 10):
            s = _Seq(f"pairs-{gi}-{part // 10}")
            s.base(h0=_HYPER_CYCLE[gi][:1] + ("a",), h1=("ardse", "b"))
            s.do("set_option", ["ard", 1])
            for a, b in pairs[part:part + 10]:
                s.do("fit")
                s.reach(a, test="t40", family="rbcm")
                s.reach(b, test="t40", family="rbcm")
            out.append(s)

    # (4) sized quantities: grow then shrink, and shrink then grow, before each reader family that depends on them
    for q, (op, small, large) in SIZED.items():
        for order, vals in (("grow-shrink", (small, large, small)), ("shrink-grow", (large, small, large))):
            s = _Seq(f"sized-{q}-{order}")
            s.base(lv="S" if q != "npad" else vals[0], sharing="declared" if q != "npad" or vals[0] == "S" else "full")
            for v in vals:
                if op == "set_train":
                    for o, a in [["set_train", v], ["set_leaves", "S"], ["set_sharing", "declared"], ["set_hyper", [0, "ardprod", "a"]],
                                 ["set_hyper", [1, "ardrq", "a"]]]:
                        s.do(o, a)
                elif op == "set_leaves":
                    s.do("set_leaves", v)
                    if v == "S":
                        s.do("set_sharing", "declared")
                elif op == "set_test":
                    s.do("set_test", v)
                for r in SIZED_FAMILIES[q]:
                    s.reach(r, **({"targets": v} if op == "solve_targets" else {}))
            out.append(s)

    # (5) table W: >= 32 leaves, the block steps run fused; every hyper class once on the two kernel ids, jointly and standalone,
    # one lane and two, under a pool
    s = _Seq("table-W-classes")
    s.base(lv="W", sharing="full", h0=("isose", "a"), h1=("ardse", "a"))
    for i in range(0, 14, 2):
        s.hypers(_HYPER_CYCLE[i], _HYPER_CYCLE[i + 1])
        if i % 4 == 0:
            s.do("set_test", ("t15", "t200", "t1", "t40")[(i // 4) % 4])
        s.do("fit")
        for r in ("predict_fetch", "gradients", "aggregate.mixture", "scores") + (("loo_gradients",) if i == 0 else ()):
            s.reach(r)
    out.append(s)
    s = _Seq("table-W-paths")
    s.base(lv="W", sharing="full", h0=("ardprod", "b"), h1=("isomat52", "a"))
    for o, a in (("set_option", ["lanes", 1]), ("reserve", 1), ("set_option", ["fused_steps", 0]), ("set_option", ["lanes", 2]),
                 ("set_option", ["fit_graph", 1]), ("set_joint", 0), ("reserve", 0), ("set_option", ["fused_steps", 1])):
        s.do(o, a)
        s.do("set_test", "t40")
        s.do("fit")
        for r in ("predict_fetch", "predict_gradients.var", "loo", "solve_targets", "predict_targets", "loo_targets", "aggregate.rbcm"):
            s.reach(r, targets="q3")
    out.append(s)

    # (6) the pool's stack: test sets replaced under a reserved pool between the calls that carve arenas above them
    s = _Seq("pool-stack")
    s.base()
    s.do("reserve", 1)
    for i, t in enumerate(("t15", "t200", "t1", "routed", "t40")):
        s.do("fit")
        s.do("solve_targets", ("q17", "q3")[i % 2])
        s.reach("loo_targets_gradients")
        s.reach("gradients")
        if t == "routed":
            s.do("set_tree")
        s.do("set_test", t)
        for r in ("targets_fetch", "predict_targets", "predict_cov", "predict_gradients.var", "loo_gradients", "loo_targets", "routes"):
            ready = s.m.ready(r)
            s.do(split(r)[0], split(r)[1] or None)      # refused where the targets went with the pool's stack
            if not ready:
                s.reach(r)
    out.append(s)

    # (7) the poison hyper-vector, then a healthy one: NaN rows land in every arena of the failed leaf, then every reader once
    # right after the healthy vector
    for half in range(2):
        s = _Seq(f"writer-poison_then_healthy-{half}")
        s.base()
        s.full(test="t40")
        for i, r in enumerate(READERS[half::2]):
            s.do("set_hyper", [POISON_KID, "poison", "a"])
            for p in (POISON_READERS if i == 0 else (r if r in POISON_READERS else "fit",)):
                s.reach(p, test="t40")
            s.do("set_hyper", [POISON_KID, "ardmat52", "ab"[i % 2]])
            s.reach(r, test="t40")
        out.append(s)

    ids = [s.id for s in out]
    assert len(set(ids)) == len(ids)
    return [dict(id=s.id, ops=s.ops) for s in out]


# ------------------------------------------------------------------------------------------------ coverage of a sequence list

COMPLETION = ("set_leaves", "set_sharing", "set_hyper", "set_tree")     # the setters that ride along with new data / a new table


def writer_class(before, op, arg):
    """The class in WRITERS of one op of a sequence (None: a pure reader, or set_tree)."""
    if op == "set_hyper":
        old = before.hyper.get(int(arg[0]))
        if old is not None and old[0] == "poison":
            return "poison_then_healthy"
        if arg[1] == "poison":
            return None
        return "set_hyper_values" if old is not None and old[0] == arg[1] else "set_hyper_kind"
    if op == "set_test":
        return "set_test_routed" if arg == "routed" else "set_test"
    if op == "set_option":
        return "opt_" + arg[0]
    return op if op in WRITERS else None


def _walk(seq):
    """[(op, arg, model before, expected code)]"""
    import copy
    m, out = Model(), []
    for op, arg in seq["ops"]:
        before = copy.deepcopy(m)
        out.append((op, arg, before, m.apply(op, arg)))
    return out


def _reached(steps, j, after):
    """The readers r such that steps[j:] is exactly r's minimal prerequisites on the state `after`, then r."""
    found = set()
    for k in range(j, min(j + 6, len(steps))):
        op, arg, _, code = steps[k]
        if op not in NEEDS or code is not None:
            continue
        try:
            pre = [o for o, _ in prerequisites(after, call_id(op, arg))]
        except AssertionError:      # not reachable from here (no leaf table yet)
            continue
        if k - j == len(pre) and [s[0] for s in steps[j:k]] == pre and all(s[3] is None for s in steps[j:k]):
            found.add(reader_id(op, arg))
    return found


def coverage(seqs):
    """dict(writer_reader={(w, r)}, pairs={(r1, r2)}, broken={(w, r)}, sized={(quantity, order, r)}) of a sequence list."""
    import copy
    wr, pairs, broken, sized = set(), set(), set(), set()
    for seq in seqs:
        steps = _walk(seq)
        n = len(steps)
        for i, (op, arg, before, code) in enumerate(steps):
            if op == "refused":
                wr |= {("refused", r) for r in _reached(steps, i + 1, before)}
            if code is not None:
                if code == E_STATE and op in NEEDS:
                    p = i - 1
                    while p >= 0 and steps[p][3] is not None:
                        p -= 1
                    while p > 0 and steps[p][0] in COMPLETION and steps[p - 1][0] in COMPLETION + ("set_train", "set_leaves"):
                        p -= 1
                    if p >= 0:
                        w = writer_class(steps[p][2], steps[p][0], steps[p][1])
                        if w:
                            broken.add((w, reader_id(op, arg)))
                continue
            after = copy.deepcopy(before)
            after.apply(op, arg)
            w = writer_class(before, op, arg)
            if w:
                j, a = i + 1, after
                if w in ("set_train", "set_leaves"):
                    while j < n and steps[j][0] in COMPLETION and steps[j][3] is None:
                        j += 1
                    a = steps[j][2] if j < n else after
                wr |= {(w, r) for r in _reached(steps, j, a)}
            if op in NEEDS:
                pairs |= {(reader_id(op, arg), r) for r in _reached(steps, i + 1, after)}
        for q, (setter, small, large) in SIZED.items():
            hist = []                                   # [value, readers answered while it held]
            for op, arg, before, code in steps:
                if code is None and op == setter and (setter != "set_test" or arg in (small, large)):
                    hist.append([arg, set()])
                if code is None and op in NEEDS and hist:
                    hist[-1][1].add(reader_id(op, arg))
            for (v0, _), (v1, r1), (v2, r2) in zip(hist, hist[1:], hist[2:]):
                order = {(small, large, small): "grow-shrink", (large, small, large): "shrink-grow"}.get((v0, v1, v2))
                if order:
                    sized |= {(q, order, r) for r in r1 & r2}
    return dict(writer_reader=wr, pairs=pairs, broken=broken, sized=sized)


def expected_broken():
    """{(w, r)}: for every writer class, the readers whose chain one instance breaks on a context where everything is current."""
    out = set()
    for w in WRITERS:
        if w in ("refused", "poison_then_healthy"):
            continue
        s = _Seq("x")
        s.base()
        s.full()
        for op, arg in _writer_instances(s, w, 0):
            s.do(op, arg)
        out |= {(w, r) for r in READERS if r != "fit" and not s.m.ready(r)}
    return out


def committed():
    with open(COMMITTED) as f:
        return json.load(f)


def annotate(seq):
    """[(index, op, arg, expectation)] with the model's verdict beside every op: "ok", "E_ARG", "E_STATE"."""
    m = Model()
    rows = []
    for i, (op, arg) in enumerate(seq["ops"]):
        code = m.apply(op, arg)
        rows.append((i, op, arg, {None: "ok", E_ARG: "E_ARG", E_STATE: "E_STATE"}[code]))
    return rows


def main(argv):
    seqs = committed() if os.path.exists(COMMITTED) and "--write" not in argv else generate()
    if "--write" in argv:
        with open(COMMITTED, "w") as f:
            f.write("[\n" + ",\n".join(json.dumps(s, separators=(",", ":")) for s in seqs) + "\n]\n")
        print(f"wrote {len(seqs)} sequences, {sum(len(s['ops']) for s in seqs)} ops")
    elif "--print" in argv:
        sid = argv[argv.index("--print") + 1]
        for i, op, arg, exp in annotate(next(s for s in seqs if s["id"] == sid)):
            print(f"{i:4d}  {op:22s} {json.dumps(arg):28s} {exp}")
    else:
        for s in seqs:
            print(f"{s['id']:40s} {len(s['ops']):4d} ops")


if __name__ == "__main__":
    main(sys.argv[1:])
