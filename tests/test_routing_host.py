"""CPU suite: the routing cases of tests/routing_cases.py cross the edges they are named for, and the library's host routine
dsmgp_tree_route equals the independent NumPy recursion `route_reference` on every one of them, entry by entry.  This proves
the reference (two separate statements of the walk agree) and validates the cases that tests/test_routing_gpu.py runs through
the device chain."""
import numpy as np
import pytest

from deepstructuredmixtures_amd import hipabi
from pred_tolerance import row_entries
import routing_cases as rc

HOST_KEYS = [k for k in rc.CASE_KEYS if k[0] != "A-shard"]       # the host routine refuses a region without a leaf (-1)


def _host(tree, Xt):
    return hipabi.tree_route(*tree.arrays(), tree.n_leaves, Xt, tree.reach)


@pytest.mark.parametrize("key", rc.CASE_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_every_case_reaches_the_edge_it_is_named_for(key):
    c = rc.case(*key)
    assert c.Xt.shape == (c.n_t, c.tree.D)
    rc.assert_case_reaches_its_edge(c, rc.reference(*key))


def test_every_edge_is_reached_by_some_case_of_every_tree_that_can():
    """The edge names are derived per case; here the other direction: no edge is left without a case."""
    by_tree = {t: set() for t in rc.ROW_SETS_OF}
    for key in rc.CASE_KEYS:
        by_tree[key[0]] |= set(rc.case(*key).edges)
    assert by_tree["A"] == {"leaf_carry", "row_carry_1024", "row_carry_8192", "full_word", "bit31", "bit0"}
    assert by_tree["A-shard"] == by_tree["A"] | {"zero_rows"}
    assert by_tree["B"] == {"row_carry_1024", "row_carry_8192", "full_word", "stack96"}
    assert set().union(*by_tree.values()) == set(rc.EDGES)
    # n_t a multiple of 32 (the last word is full), one short of it and one past it, around both carries
    assert {32, 1024, 8192, 8224} <= set(rc.N_T) and {31, 33, 1023, 1025, 8191, 8193} <= set(rc.N_T)
    # the one_child set: one leaf per split node holds every row, every other leaf is empty
    ptr, idx, _ = rc.reference("A", "one_child", 8224)
    full = [400 * s + k for s, k in enumerate(rc.ONE_CHILD)]
    assert np.array_equal(np.flatnonzero(np.diff(ptr)), full) and np.array_equal(idx, np.tile(np.arange(8224), 3))
    # the shard keeps leaf 1023 (odd) empty next to held leaves: a zero at the leaf scan's chunk edge
    ptr, _, _ = rc.reference("A-shard", "zeros", 16385)
    cnt = np.diff(ptr)
    assert cnt[1023] == 0 and np.all(cnt[1::2] == 0) and cnt[1022] > 0 and cnt[1024] > 0


def test_lazy_row_entries_are_what_pred_tolerance_row_entries_gives():
    for key in (("A", "spread", 1025), ("A-shard", "zeros", 1025), ("B", "all", 33)):
        ptr, idx, ent = rc.reference(*key)
        assert list(ent) == row_entries(ptr, idx, key[2]) and len(ent) == key[2]
    ptr, idx, ent = rc.route_reference(rc.tree_c("twice"), np.zeros((2, 1)))
    assert list(ent) == row_entries(ptr, idx, 2) == [[(0, 0), (0, 1), (1, 4)], [(0, 2), (0, 3), (1, 5)]]


def test_reference_on_a_tree_small_enough_to_route_by_hand():
    """split on dimension 1 at (0.0, 2.0, +inf) over (leaf 0, sum(leaf 1, leaf 2), leaf 3)."""
    t = rc.flatten("hand", ("split", 1, [0.0, 2.0, np.inf], [("leaf", 0), ("sum", [("leaf", 1), ("leaf", 2)]), ("leaf", 3)]), 4, 2)
    assert t.kind.tolist() == [1, 0, 2, 0, 0, 0] and t.first_child.tolist() == [1, 0, 4, 0, 0, 0]
    assert t.n_child.tolist() == [3, 0, 2, 0, 0, 0] and t.leaf_id.tolist() == [-1, 0, -1, 3, 1, 2]
    Xt = np.array([[9.0, 0.0], [9.0, -0.0], [9.0, 5e-324], [9.0, 2.0], [9.0, 2.5], [9.0, -np.inf], [9.0, np.inf]])
    ptr, idx, ent = rc.route_reference(t, Xt)
    assert ptr.tolist() == [0, 3, 5, 7, 9] and idx.tolist() == [0, 1, 5, 2, 3, 2, 3, 4, 6]
    assert ent[2] == [(1, 3), (2, 5)] and ent[6] == [(3, 8)]
    hp, hi = _host(t, Xt)
    assert np.array_equal(hp, ptr) and np.array_equal(hi, idx)


@pytest.mark.parametrize("key", HOST_KEYS, ids=lambda k: "-".join(map(str, k)))
def test_host_routine_equals_the_reference_entry_by_entry(key):
    c = rc.case(*key)
    ptr, idx, _ = rc.reference(*key)
    for Xt in (np.ascontiguousarray(c.Xt), np.asfortranarray(c.Xt)):
        hp, hi = _host(c.tree, Xt)
        assert np.array_equal(hp, ptr) and np.array_equal(hi, idx)


def test_a_nan_row_is_outside_for_both():
    for row, d in ((0, 0), (1024, 1), (2047, 2)):
        Xt = rc.rows_spread(2048).copy()
        Xt[row, d] = np.nan
        with pytest.raises(ValueError, match="outside"):
            rc.route_reference(rc.tree_a(), Xt)
        with pytest.raises(ValueError, match="outside"):              # hipabi.tree_route words DSMGP_E_DOMAIN (-6) so, and only it
            _host(rc.tree_a(), Xt)


def test_plus_inf_beyond_a_finite_last_threshold_is_outside_for_both():
    t = rc.flatten("finite", ("split", 0, [0.0, 1.0], [("leaf", 0), ("leaf", 1)]), 2, 1)
    ok = np.array([[-np.inf], [0.0], [1.0]])
    ptr, idx, _ = rc.route_reference(t, ok)
    hp, hi = _host(t, ok)
    assert ptr.tolist() == [0, 2, 3] and np.array_equal(hp, ptr) and np.array_equal(hi, idx)
    for v in (np.inf, np.nextafter(1.0, 2.0)):
        with pytest.raises(ValueError, match="outside"):
            rc.route_reference(t, np.array([[0.5], [v]]))
        with pytest.raises(ValueError, match="outside"):
            _host(t, np.array([[0.5], [v]]))


def test_host_routes_the_tree_one_past_the_device_stack():
    t = rc.tree_b(1)
    Xt = rc.rows_all(33)
    ptr, idx, ent = rc.route_reference(t, Xt)
    assert np.all(ent.counts() == rc.ROUTE_STACK + 1)
    hp, hi = _host(t, Xt)
    assert np.array_equal(hp, ptr) and np.array_equal(hi, idx)


def test_what_the_host_routine_does_with_the_trees_the_device_cannot_represent():
    """Recorded facts that the device-side refusal (dsmgp_set_tree) is stated against: dsmgp_tree_route is a list builder for any
    tree.  Leaves met out of order still give a CSR by ascending leaf; a leaf named twice lists the row twice, so that
    route_ptr[L] counts 3 entries per row where a bitmap of one bit per (leaf, row) can hold 2."""
    Xt = rc.rows_all(5)
    order, twice = rc.tree_c("order"), rc.tree_c("twice")
    hp, hi = _host(order, Xt)
    assert hp.tolist() == [0, 5, 10, 15] and np.array_equal(hi, np.tile(np.arange(5), 3))
    rp, ri, _ = rc.route_reference(order, Xt)
    assert np.array_equal(hp, rp) and np.array_equal(hi, ri)
    hp, hi = _host(twice, Xt)
    assert hp.tolist() == [0, 10, 15, 15] and np.array_equal(hi[:10], np.repeat(np.arange(5), 2))
    rp, ri, _ = rc.route_reference(twice, Xt)
    assert np.array_equal(hp, rp) and np.array_equal(hi, ri)
