"""glistcompare L1 .. LN --pairwise in numpy: the contract gt4hip_pairwise_multi and gt4hip_table_pairwise are tested against.

With c_i(w) the count of word w in list i, 0 where it is absent (a stored record with count 0 is the same as absence):
    shared[i][j]    = the number of words w with c_i(w) > 0 and c_j(w) > 0
    min_total[i][j] = the sum over all words of min(c_i(w), c_j(w))
both n x n, uint64, symmetric; the diagonal holds a list's words with a count other than 0 and the sum of its counts."""
import numpy as np


def count_table(lists):
    """(distinct keys of all lists ascending, counts[row][list], 0 where a list does not hold the key)"""
    n = len(lists)
    keys = np.unique(np.concatenate([np.asarray(l["key"], dtype=np.uint64) for l in lists])) if n else np.zeros(0, dtype=np.uint64)
    counts = np.zeros((len(keys), n), dtype=np.uint64)
    for j, l in enumerate(lists):
        counts[np.searchsorted(keys, l["key"]), j] = l["count"]
    return keys, counts


def pairwise_of_table(counts):
    """(shared, min_total) of a table of counts[row][list]"""
    counts = np.asarray(counts, dtype=np.uint64)
    n = counts.shape[1]
    held = (counts != 0).astype(np.int64)
    shared = (held.T @ held).astype(np.uint64)
    min_total = np.zeros((n, n), dtype=np.uint64)
    for i in range(n):
        min_total[i] = np.minimum(counts[:, i:i + 1], counts).sum(axis=0, dtype=np.uint64)
    return shared, min_total


def pairwise(lists):
    """(shared, min_total) of lists of records with strictly ascending keys"""
    return pairwise_of_table(count_table(lists)[1])


def union_size(shared, i, j):
    return int(shared[i][i]) + int(shared[j][j]) - int(shared[i][j])


def jaccard(shared, i, j):
    u = union_size(shared, i, j)
    return int(shared[i][j]) / u if u else 0.0


def transcript(names, shared, min_total):
    """what `glistcompare names... --pairwise` prints"""
    out = ["#I\tJ\tLIST_I\tLIST_J\tSHARED\tMIN_TOTAL\tUNION\tJACCARD\n"]
    for i in range(len(names)):
        for j in range(i, len(names)):
            out.append("%d\t%d\t%s\t%s\t%d\t%d\t%d\t%.6f\n" % (i, j, names[i], names[j], int(shared[i][j]), int(min_total[i][j]), union_size(shared, i, j),
                                                             jaccard(shared, i, j)))
    return "".join(out)
