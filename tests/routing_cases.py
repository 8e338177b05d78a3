"""Trees, test-row sets and an independent reference for the routing of test rows (dsmgp_set_tree / dsmgp_set_test_routed on
the device, dsmgp_tree_route on the host), in plain NumPy.

The device walk and the host routine share one source (csrc/route_walk.hpp), so neither can serve as the other's reference.
`route_reference` is the literal recursion over the flat tree arrays, written here: a sum node forwards its rows to every
child in order, a split node forwards a row to the child np.searchsorted(thr[:nc], v, side="left"), and an index at or beyond
nc, or a NaN coordinate, means the row lies outside.

The cases are built to cross the edges of the device chain (csrc/kernels.hpp):
  scan_counts_kernel    chunks of 1024 counts with a running carry -- over the rows (n_t > 1024) and over the leaves (L > 1024)
  route_rank_kernel     chunks of 256 bitmap words = 8192 rows with a running carry
  route_fill_kernel /   bit arithmetic inside one 32-row word: a full word, a word that holds only bit 31 or only bit 0,
  route_walk_kernel     n_t a multiple of 32
  route_walk_row        a fixed stack of ROUTE_STACK = 96 pending nodes
`assert_case_reaches_its_edge` states, from the reference CSR alone, that a case crosses the edges it is named for."""
import functools

import numpy as np

ROUTE_STACK = 96              # csrc/route_walk.hpp
SCAN_CHUNK = 1024             # scan_counts_kernel
RANK_CHUNK_ROWS = 256 * 32    # route_rank_kernel: 256 words of 32 rows
N_T = (1, 31, 32, 33, 1023, 1024, 1025, 2048, 8191, 8192, 8193, 8224, 16385)


class Tree:
    """Flat tree arrays in the layout dsmgp_set_tree takes; `n_leaves` = size of the leaf table the regions index."""

    def __init__(self, name, kind, first_child, n_child, split_dim, thr, leaf_id, n_leaves, D):
        self.name = name
        self.kind = np.asarray(kind, dtype=np.int8)
        self.first_child = np.asarray(first_child, dtype=np.int64)
        self.n_child = np.asarray(n_child, dtype=np.int64)
        self.split_dim = np.asarray(split_dim, dtype=np.int64)
        self.thr = np.ascontiguousarray(thr, dtype=np.float64)
        self.leaf_id = np.asarray(leaf_id, dtype=np.int64)
        self.n_leaves = int(n_leaves)
        self.D = int(D)

    def arrays(self):
        """(kind, first_child, n_child, split_dim, thr, leaf_id): the arguments of Context.set_tree, in order."""
        return self.kind, self.first_child, self.n_child, self.split_dim, self.thr, self.leaf_id

    @property
    def reach(self):
        """An upper bound of the leaves one row can reach (every region): the capacity hipabi.tree_route asks for."""
        return int(np.sum(self.kind == 0))


def flatten(name, spec, n_leaves, D):
    """Tree from a nested spec -- ("leaf", id) | ("sum", [children]) | ("split", dim, [thresholds], [children]) -- with the
    children of every node consecutive and behind their parent (breadth first)."""
    nodes = [spec]
    first, i = [], 0
    while i < len(nodes):
        ch = [] if nodes[i][0] == "leaf" else nodes[i][-1]
        first.append(len(nodes) if ch else 0)
        nodes.extend(ch)
        i += 1
    n = len(nodes)
    ld = max([1] + [len(s[2]) for s in nodes if s[0] == "split"])
    kind, nch, sdim, leaf = np.zeros(n, np.int8), np.zeros(n, np.int64), np.zeros(n, np.int64), np.full(n, -1, np.int64)
    thr = np.zeros((n, ld))
    for i, s in enumerate(nodes):
        if s[0] == "leaf":
            leaf[i] = s[1]
        elif s[0] == "sum":
            kind[i], nch[i] = 2, len(s[1])
        else:
            assert len(s[2]) == len(s[3])
            kind[i], nch[i], sdim[i] = 1, len(s[3]), s[1]
            thr[i, :len(s[2])] = s[2]
    return Tree(name, kind, first, nch, sdim, thr, leaf, n_leaves, D)


# ------------------------------------------------------------------------------------------------------------ the reference

class RowEntries:
    """Per test row its (leaf, entry) pairs in ascending entry order, as pred_tolerance.row_entries gives them, made row by row
    on demand from the arrays of the whole set (a list of lists of 10^6 tuples is slow to build and rarely walked)."""

    def __init__(self, route_ptr, route_idx, n_t):
        self.row_ent = np.argsort(route_idx, kind="stable")                       # entries by row, ascending entry within a row
        self.ent_leaf = np.repeat(np.arange(len(route_ptr) - 1), np.diff(route_ptr))
        self.row_ptr = np.concatenate([[0], np.cumsum(np.bincount(route_idx, minlength=n_t))]).astype(np.int64)

    def __len__(self):
        return len(self.row_ptr) - 1

    def __getitem__(self, r):
        e = self.row_ent[self.row_ptr[r]:self.row_ptr[r + 1]]
        return [(int(l), int(i)) for l, i in zip(self.ent_leaf[e], e)]

    def __iter__(self):
        return (self[r] for r in range(len(self)))

    def counts(self):
        return np.diff(self.row_ptr)


def route_reference(tree, Xt):
    """(route_ptr, route_idx, entries): per leaf the ascending test rows that reach it, and per row its (leaf, entry) pairs.
    ValueError("outside") where a row reaches a split node and lies beyond its last threshold (NaN: beyond every threshold)."""
    Xt = np.asarray(Xt, dtype=np.float64)
    n_t = Xt.shape[0]
    per_leaf = [[] for _ in range(tree.n_leaves)]

    def forward(node, rows):
        k = int(tree.kind[node])
        c0, nc = int(tree.first_child[node]), int(tree.n_child[node])
        if k == 0:
            if tree.leaf_id[node] >= 0:
                per_leaf[int(tree.leaf_id[node])].append(rows)
        elif k == 2:
            for j in range(nc):
                forward(c0 + j, rows)
        else:
            v = Xt[rows, int(tree.split_dim[node])]
            child = np.searchsorted(tree.thr[node, :nc], v, side="left")
            if np.any(np.isnan(v)) or np.any(child >= nc):
                raise ValueError("test point outside the region of a split node")
            for j in np.unique(child):
                forward(c0 + int(j), rows[child == j])

    forward(0, np.arange(n_t, dtype=np.int64))
    lists = [np.sort(np.concatenate(p), kind="stable") if p else np.zeros(0, np.int64) for p in per_leaf]
    route_ptr = np.concatenate([[0], np.cumsum([a.size for a in lists])]).astype(np.int64)
    route_idx = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
    return route_ptr, route_idx, RowEntries(route_ptr, route_idx, n_t)


# ------------------------------------------------------------------------------------------------------------------ trees

A_CHILDREN = 400
# ascending, exactly representable, 0.0 among them (child 200), the last +inf
A_THR = np.concatenate([(np.arange(A_CHILDREN - 1) - 200) * 0.25, [np.inf]])


@functools.lru_cache(maxsize=None)
def tree_a(shard=False):
    """Wide: a sum root over 3 split nodes on dimensions 0, 1, 2 with 400 regions each: L = 1200 (past one scan chunk),
    thr_ld = 400, D = 3.  Leaves are numbered depth-first: child k of split s is leaf 400 s + k.  shard: every second region
    carries -1 (held elsewhere); the leaf table keeps its 1200 slots, so the odd leaves -- 1023 among them -- stay empty."""
    splits = [("split", s, list(A_THR), [("leaf", -1 if shard and k % 2 else A_CHILDREN * s + k) for k in range(A_CHILDREN)])
              for s in range(3)]
    return flatten("A-shard" if shard else "A", ("sum", splits), 3 * A_CHILDREN, 3)


@functools.lru_cache(maxsize=None)
def tree_b(extra=0):
    """Stack: a sum root over (a sum node of 95 + extra regions, one region).  The root leaves 1 node pending while the inner
    node pushes its 95 + extra: route_stack_need = 96 + extra, and the walk really holds that many.  Both variants index one
    leaf table of 97 slots (B leaves the last one empty), so that a context can be offered B+ after B."""
    n = ROUTE_STACK - 1 + extra
    inner = ("sum", [("leaf", k) for k in range(n)])
    return flatten("B" + "+" * extra, ("sum", [inner, ("leaf", n)]), ROUTE_STACK + 1, 1)


@functools.lru_cache(maxsize=None)
def tree_c(which):
    """Well-formed for the host list builder, not representable by the device path (one bit per (leaf, row), a row's entries in
    visit order): 'order' meets leaves 1, 2, 0 along the depth-first walk; 'twice' names leaf 0 in two regions."""
    ids = {"order": (1, 2, 0), "twice": (0, 1, 0)}[which]
    return flatten("C-" + which, ("sum", [("leaf", i) for i in ids]), 3, 1)


# --------------------------------------------------------------------------------------------------------------- row sets

def _coord(child, on):
    """A coordinate that tree A's split sends to `child`: ON its threshold (the low side takes it) or 0.125 below it."""
    child = np.asarray(child)
    on = np.broadcast_to(on, child.shape)
    below = np.where(child == A_CHILDREN - 1, A_THR[A_CHILDREN - 2] + 0.125, A_THR[child] - 0.125)
    return np.where(on, A_THR[child], below)


_MUL, _OFF = (7, 11, 13), (0, 200, 300)          # child of row r under split d: (7 r) % 400, (11 r + 200) % 400, (13 r + 300) % 400


def rows_spread(n_t, finite=False):
    """Coordinates spread over all children; every third row lies exactly on its thresholds; rows r % 16 = 3, 5, 7, 9, 11 carry
    -inf, +inf, -0.0 against the threshold 0.0, the smallest denormal and its negative.  finite: -+1e3 in place of every -+inf
    (the same children; for the cases whose moments are compared)."""
    r = np.arange(n_t)
    X = np.stack([_coord((_MUL[d] * r + _OFF[d]) % A_CHILDREN, r % 3 == 0) for d in range(3)], axis=1)
    big = 1e3 if finite else np.inf
    for m, d, v in ((3, 0, -big), (5, 1, big), (7, 2, -0.0), (9, 0, 5e-324), (11, 1, -5e-324)):
        X[r % 16 == m, d] = v
    return np.clip(X, -big, big)             # (finite: a row ON the last threshold, +inf, as well)


ONE_CHILD = (10, 20, 300)


def rows_one_child(n_t):
    """Every row to the same child of each split node: that leaf's bitmap words are all ones, every other leaf is empty."""
    return np.tile(_coord(np.array(ONE_CHILD), False), (n_t, 1))


EDGE_BIT31, EDGE_BIT0, EDGE_CHUNK, EDGE_BOTH = 4, 6, 8, 398      # children of splits 0, 0, 1, 2


def rows_edges(n_t):
    """Sparse leaves whose rows sit on the word and chunk edges: under split 0, child 4 takes the rows r % 32 == 31 and child 6
    the rows r % 32 == 0; under split 1, child 8 takes r % 8192 in {0, 8191}; under split 2, child 398 takes r % 32 in {0, 31}.
    Every other row goes to some other child."""
    r = np.arange(n_t)
    c = np.stack([(_MUL[d] * r + _OFF[d]) % A_CHILDREN for d in range(3)], axis=1)
    for d, reserved in ((0, (EDGE_BIT31, EDGE_BIT0)), (1, (EDGE_CHUNK,)), (2, (EDGE_BOTH,))):
        c[np.isin(c[:, d], reserved), d] += 1
    c[r % 32 == 31, 0] = EDGE_BIT31
    c[r % 32 == 0, 0] = EDGE_BIT0
    c[np.isin(r % RANK_CHUNK_ROWS, (0, RANK_CHUNK_ROWS - 1)), 1] = EDGE_CHUNK
    c[np.isin(r % 32, (0, 31)), 2] = EDGE_BOTH
    return _coord(c, (r % 3 == 0)[:, None])


ZERO_ROWS = (1022, 1023, 1024, 1025, 8190, 8191, 8192, 8193)


def rows_zeros(n_t):
    """For the shard variant: every row goes to even (held) children, except ZERO_ROWS, which go to odd ones in all three
    dimensions and so reach no held leaf -- row counts of zero on both sides of the scan's chunk edges."""
    r = np.arange(n_t)
    c = np.stack([2 * ((_MUL[d] * r + _OFF[d] // 2) % (A_CHILDREN // 2)) for d in range(3)], axis=1)
    c[np.isin(r, ZERO_ROWS)] += 1
    return _coord(c, (r % 3 == 0)[:, None])


def rows_all(n_t):
    """Tree B has no split node: every row reaches every leaf, whatever its coordinate."""
    return np.linspace(-1.0, 1.0, n_t).reshape(n_t, 1)


# ------------------------------------------------------------------------------------------------------------------ cases

class Case:
    def __init__(self, tree, rows, n_t, Xt, edges):
        self.tree, self.rows, self.n_t, self.Xt, self.edges = tree, rows, n_t, Xt, tuple(edges)
        self.id = f"{tree.name}-{rows}-{n_t}"


_ROW_SETS = {"spread": rows_spread, "one_child": rows_one_child, "edges": rows_edges, "zeros": rows_zeros, "all": rows_all}
EDGES = ("leaf_carry", "row_carry_1024", "row_carry_8192", "full_word", "bit31", "bit0", "stack96", "zero_rows")


def _edges_named(tree, rows, n_t):
    """The edges a case is built to cross, from its construction (see the row-set docstrings)."""
    e = []
    if tree.n_leaves > SCAN_CHUNK:
        e.append("leaf_carry")               # every row set reaches leaves below 400 (split 0) and from 1024 on (split 2, child >= 224)
    if n_t > SCAN_CHUNK and not (rows == "zeros" and n_t <= max(ZERO_ROWS[:4]) + 1):
        e.append("row_carry_1024")           # (zeros: rows 1024 and 1025 carry nothing; the first row past them is 1026)
    if n_t > RANK_CHUNK_ROWS and not (rows == "zeros" and n_t <= max(ZERO_ROWS) + 1):
        e.append("row_carry_8192")
    if rows in ("one_child", "all") and n_t >= 32:
        e.append("full_word")
    if rows == "edges":
        e.append("bit0")
        if n_t >= 32:
            e.append("bit31")
    if tree.name == "B":
        e.append("stack96")
    if rows == "zeros" and n_t > 1024:
        e.append("zero_rows")
    return e


@functools.lru_cache(maxsize=None)
def case(tree_name, rows, n_t):
    tree = {"A": tree_a, "A-shard": lambda: tree_a(True), "B": tree_b}[tree_name]()
    return Case(tree, rows, n_t, _ROW_SETS[rows](n_t), _edges_named(tree, rows, n_t))


ROW_SETS_OF = {"A": ("spread", "one_child", "edges"), "A-shard": ("spread", "one_child", "edges", "zeros"), "B": ("all",)}
CASE_KEYS = [(t, rows, n_t) for t, sets in ROW_SETS_OF.items() for rows in sets for n_t in N_T]


@functools.lru_cache(maxsize=None)
def reference(tree_name, rows, n_t):
    """route_reference of a case, computed once and shared (callers must not write into it)."""
    c = case(tree_name, rows, n_t)
    ptr, idx, ent = route_reference(c.tree, c.Xt)
    ptr.setflags(write=False)
    idx.setflags(write=False)
    return ptr, idx, ent


def _words(rows, n_t):
    """The 32-row bitmap words of one leaf's row list."""
    w = np.zeros((n_t + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(w, rows >> 5, np.uint32(1) << (rows & 31).astype(np.uint32))
    return w


def assert_case_reaches_its_edge(case, csr):
    """From the reference CSR alone: the case crosses every edge in case.edges.  A case that does not is wrong, not skippable."""
    ptr, idx, ent = csr
    n_t, L = case.n_t, len(ptr) - 1
    cnt = np.diff(ptr)
    leaves = [idx[ptr[l]:ptr[l + 1]] for l in np.flatnonzero(cnt)]
    assert set(case.edges) <= set(EDGES)
    for e in case.edges:
        if e == "leaf_carry":          # the per-leaf scan's carry: counts on both sides of leaf 1024
            ok = L > SCAN_CHUNK and np.any(cnt[:SCAN_CHUNK] > 0) and np.any(cnt[SCAN_CHUNK:] > 0)
        elif e == "row_carry_1024":    # the per-row scan's carry: entries on both sides of row 1024
            rc = ent.counts()
            ok = n_t > SCAN_CHUNK and np.any(rc[:SCAN_CHUNK] > 0) and np.any(rc[SCAN_CHUNK:] > 0)
        elif e == "row_carry_8192":    # the rank kernel's carry: one leaf with rows on both sides of row 8192
            ok = any(a[0] < RANK_CHUNK_ROWS <= a[-1] for a in leaves)
        elif e == "full_word":
            ok = any(np.any(_words(a, n_t) == 0xFFFFFFFF) for a in leaves)
        elif e == "bit31":
            ok = any(np.any(_words(a, n_t) == 0x80000000) for a in leaves)
        elif e == "bit0":
            ok = any(np.any(_words(a, n_t) == 1) for a in leaves)
        elif e == "stack96":           # a row that reaches 96 leaves below one sum node
            ok = np.any(ent.counts() == ROUTE_STACK)
        elif e == "zero_rows":         # rows without entries on both sides of the row scan's first chunk edge, neighbours with
            rc = ent.counts()
            ok = rc[1023] == 0 and rc[1024] == 0 and rc[1021] > 0 and (n_t <= 1026 or rc[1026] > 0)
        assert ok, (case.id, e)
