"""glistcompare -u --min_lists M --max_lists X in numpy: the contract gt4hip_select_multi is tested against.

For a word w, p(w) is the number of lists that hold it with a count other than 0.  The result is the subsequence of the
union of the lists (the oracle's union_multi: same rule, cutoff and override) whose words have M <= p <= X.  A record with
count 0 does not make its list a holder."""
import numpy as np

import oracle_lib as O
from genometester4_amd.listio import RECORD_DTYPE


def presence(lists):
    """(words held by at least one list with a count other than 0, ascending; in how many lists each)"""
    held = [np.asarray(l["key"], dtype=np.uint64)[np.asarray(l["count"]) != 0] for l in lists]
    if not held or not sum(len(h) for h in held):
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.int64)
    return np.unique(np.concatenate(held), return_counts=True)


def select(lists, min_lists, max_lists, cutoff=1, rule=0, count_override=1):
    """(rc, n_words, total_count, records) as oracle_lib.union_multi returns them"""
    n = len(lists)
    if not (1 <= min_lists <= max_lists <= n):
        raise ValueError("1 <= min_lists <= max_lists <= %d is needed" % n)
    rc, _, _, union = O.union_multi(lists, cutoff, rule, count_override)
    if rc:
        return rc, None, None, None
    words, p = presence(lists)
    chosen = words[(p >= min_lists) & (p <= max_lists)]
    out = np.ascontiguousarray(union[np.isin(union["key"], chosen)], dtype=RECORD_DTYPE)
    return 0, len(out), int(out["count"].astype(np.uint64).sum()), out
