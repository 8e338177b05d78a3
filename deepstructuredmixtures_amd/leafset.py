"""A subset of the leaves as a leaf table of its own: the one place where the table is sliced and answers are put back.

A sub-context of `hipabi.MultiContext`, a group of `hipabi.StreamingContext` and a rank of `dist.Shard` each see some of the
leaves, numbered from 0 in ascending global order.  Per-leaf arrays are indexed by `loc`; per-entry arrays (the rows of a
leaf, the test rows routed to it) are CSR segments that follow one another in its table.  No loop over leaves: 18k at depth 4."""
import numpy as np

SHARE_FULL = 0      # tree.SHARE_FULL, DSMGP_SHARE_FULL


def csr_ptr(counts):
    """Row pointer of a CSR table with `counts[i]` entries in row i."""
    return np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(counts, dtype=np.int64)])


def share_roots(op, src, L):
    """Per leaf, the leaf whose factor it rides on (itself where it is factorised in full), one level of chaining resolved.
    Leaves with the same root travel together: a COPY / PREFIX leaf needs its source in the same table."""
    root = np.arange(L, dtype=np.int64)
    if op is not None:
        rides = (np.asarray(op) != SHARE_FULL) & (np.asarray(src) >= 0)
        root[rides] = np.asarray(src)[rides]
        root = root[root]
    return root


class LeafSubset:
    """Sorted global leaf ids `loc` out of `L` leaves."""

    def __init__(self, loc, L):
        self.loc = np.asarray(loc, dtype=np.int64)
        self.L = int(L)

    def _entries(self, ptr):
        """(lptr, gidx): the subset's own row pointer and, per entry of it, the entry's place in the whole table."""
        ptr = np.asarray(ptr, dtype=np.int64)
        lptr = csr_ptr(ptr[self.loc + 1] - ptr[self.loc])
        return lptr, np.repeat(ptr[self.loc] - lptr[:-1], np.diff(lptr)) + np.arange(lptr[-1])

    def take_csr(self, ptr, idx):
        """(lptr, lidx) of the subset's rows; the inputs themselves where the subset is every leaf in order."""
        if self.loc.size == self.L and np.array_equal(self.loc, np.arange(self.L)):
            return ptr, idx
        lptr, gidx = self._entries(ptr)
        return lptr, np.asarray(idx)[gidx]

    def take_sharing(self, op, src, plen):
        """The schedule in local leaf numbers (int32, int32, int64); a leaf whose source is not in the subset becomes FULL."""
        if op is None:
            return None, None, None
        op, src, plen = (np.asarray(a)[self.loc] for a in (op, src, plen))
        lsrc = np.where(src >= 0, self.global_to_local()[src], -1)
        keep = (op != SHARE_FULL) & (lsrc >= 0)
        return (np.where(keep, op, SHARE_FULL).astype(np.int32), np.where(keep, lsrc, -1).astype(np.int32),
                np.where(keep, plen, 0).astype(np.int64))

    def put_entries(self, out, ptr, local):
        """out[entries of the subset's leaves] = local (first axis): the inverse of `take_csr` on `ptr`."""
        out[self._entries(ptr)[1]] = local

    def put_leaves(self, out, local):
        out[self.loc] = local

    def global_to_local(self):
        """Per global leaf id its number in the subset, -1: not in it."""
        g2l = np.full(self.L, -1, dtype=np.int64)
        g2l[self.loc] = np.arange(self.loc.size)
        return g2l
