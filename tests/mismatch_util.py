"""Seeded inputs of the -mm (difference up to N mismatches) tests: every list is rebuilt from its seed, so the
golden file (tests/golden/mm_cases.json) holds only argv, transcripts and hashes."""
import numpy as np

from genometester4_amd.listio import make_records


def revcomp(words, k):
    """get_reverse_complement (reference src/sequence.c:65-79) of every word of a uint64 array"""
    x = ~np.asarray(words, dtype=np.uint64)
    out = np.zeros_like(x)
    for _ in range(k):
        out = (out << np.uint64(2)) | (x & np.uint64(3))
        x = x >> np.uint64(2)
    return out


def canonical(words, k):
    w = np.asarray(words, dtype=np.uint64)
    return np.minimum(w, revcomp(w, k))


def key_limit(k):
    return (1 << (2 * k)) - 1  # largest key


def _random_keys(rng, n, k):
    hi = key_limit(k)
    if n >= hi + 1:
        return np.arange(hi + 1, dtype=np.uint64)
    keys = np.unique(rng.integers(0, hi, size=n, dtype=np.uint64, endpoint=True))
    while len(keys) < n:
        keys = np.unique(np.concatenate([keys, rng.integers(0, hi, size=n - len(keys), dtype=np.uint64, endpoint=True)]))
    return keys[:n] if len(keys) > n else keys


def _counts(rng, n, max_count):
    return rng.integers(1, max_count, size=n, dtype=np.uint32, endpoint=True)


def dense_pair(seed, k, p_a=0.4, p_b=0.4, max_count=4):
    """small k: every key of the 4^k space in A with probability p_a, in B with p_b (neighbours do hit)"""
    rng = np.random.default_rng(seed)
    space = np.arange(1 << (2 * k), dtype=np.uint64)
    ka = space[rng.random(len(space)) < p_a]
    kb = space[rng.random(len(space)) < p_b]
    return make_records(ka, _counts(rng, len(ka), max_count)), make_records(kb, _counts(rng, len(kb), max_count))


def _mutate(rng, words, k, n_sub):
    """every word with n_sub distinct positions substituted (XOR 1..3 at bits 2i)"""
    w = words.copy()
    for j in range(len(w)):
        pos = rng.choice(k, size=n_sub, replace=False)
        for p in pos:
            w[j] ^= np.uint64(int(rng.integers(1, 4)) << (2 * int(p)))
    return w


def planted_pair(seed, k, n_a, shared=0.3, planted=0.3, max_count=4, n_sub_max=3):
    """A: random canonical words.  B: a share of A's words, 1..n_sub_max-mismatch variants of another share of them
    (canonical, and for one in four the other strand: a key a canonical lookup never finds), and random words."""
    rng = np.random.default_rng(seed)
    ka = np.unique(canonical(_random_keys(rng, n_a, k), k))
    sel = rng.random(len(ka))
    parts = [ka[sel < shared]]
    src = ka[(sel >= shared) & (sel < shared + planted)]
    if len(src):
        n_sub = rng.integers(1, n_sub_max + 1, size=len(src))
        var = np.concatenate([_mutate(rng, src[n_sub == s], k, int(s)) for s in range(1, n_sub_max + 1)])
        can = canonical(var, k)
        other = revcomp(can, k)
        flip = rng.random(len(can)) < 0.25
        parts.append(np.where(flip, other, can))
    parts.append(canonical(_random_keys(rng, max(1, n_a // 4), k), k))
    kb = np.unique(np.concatenate(parts))
    return make_records(ka, _counts(rng, len(ka), max_count)), make_records(kb, _counts(rng, len(kb), max_count))


def shared_half_pair(seed, n, k=25, max_count=8):
    """two random lists of n records sharing n / 2 keys (the -mm performance workload)"""
    rng = np.random.default_rng(seed)
    keys = _random_keys(rng, n + n // 2, k)
    rng.shuffle(keys)
    common, only_a, only_b = keys[: n // 2], keys[n // 2: n], keys[n:]
    ka = np.sort(np.concatenate([common, only_a]))
    kb = np.sort(np.concatenate([common, only_b[: n - n // 2]]))
    return make_records(ka, _counts(rng, len(ka), max_count)), make_records(kb, _counts(rng, len(kb), max_count))
