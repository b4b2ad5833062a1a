"""The device blocks a call takes for itself (TempBlocks and TempTable of gt4hip_host.h) all go back to the context's
pool, on the error returns that come after the blocks exist as on success: a round of calls is run once, which leaves
the pool warm, the free device memory is read, the round is repeated twenty times, and the free memory must not have
fallen.  Every repeat must also give what the first round gave (results, or error code and message): these are no
correctness tests, the units have their own.

Sizes: the smallest that reach the code after its blocks exist.  Three lists of about 300 records make a ragged count
table (any two non-empty lists do: one launch of the tile kernel) of one segment.  5,000 words are one tile of the
radix sort and of the fold; k = 16 and k = 32 sort in 4 and 8 passes and end in place, k = 11 in 3 passes and is copied
back from the scratch block."""
import numpy as np
import pytest

import subset_model as SM
from genometester4_amd import capi
from genometester4_amd.listio import make_records

pytestmark = pytest.mark.gpu

ROUNDS = 20
N_WORDS = 5000


@pytest.fixture()
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def no_leak(ctx, one_round):
    first = one_round()
    free0 = ctx.device_memory()[0]  # (the pool holds what the first round left)
    for _ in range(ROUNDS):
        assert one_round() == first
    assert ctx.device_memory()[0] >= free0
    return first


def refused(call):
    with pytest.raises(capi.Gt4HipError) as e:
        call()
    return e.value.code, str(e.value)


def three_lists(ctx, k=25, n=300):
    rng = np.random.default_rng(k)
    keys = np.unique(rng.integers(0, 1 << (2 * k - 4), size=2 * n, dtype=np.uint64))  # (words of k - 1 bases too)
    lists = []
    for _ in range(3):
        mine = np.sort(rng.choice(keys, size=n, replace=False))
        lists.append(make_records(mine, rng.integers(1, 9, size=n, dtype=np.uint32)))
    return [ctx.upload(x, k) for x in lists]


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def back(t):
    return t.cpu().numpy().view(np.uint64).tobytes()


def test_select_into_a_list_too_small(ctx):
    """EINVAL after table_select holds its five workspace blocks (and select_multi the table)"""
    dev = three_lists(ctx)
    small = ctx.alloc(1, 25)
    table = ctx.device_table(dev)
    assert table.n_keys > 1

    def one_round():
        return refused(lambda: ctx.select_multi(dev, 1, 3, out=small)), refused(lambda: ctx.table_select(table, 1, 3, out=small))

    for code, text in no_leak(ctx, one_round):
        assert code == capi.EINVAL and "capacity" in text


def test_multi_of_two_word_lengths(ctx):
    dev = three_lists(ctx)
    other = ctx.upload(dev[1].download(), 24)
    mixed = [dev[0], other, dev[2]]

    def one_round():
        return refused(lambda: ctx.pairwise_multi(mixed)), refused(lambda: ctx.select_multi(mixed, 1, 3))

    for code, text in no_leak(ctx, one_round):
        assert code == capi.EWORDLEN and "word lengths differ" in text


@pytest.mark.parametrize("k", [11, 16, 32])
def test_sorts_in_place(ctx, k):
    rng = np.random.default_rng(k)
    words = rng.integers(0, 1 << (2 * k - 1), size=N_WORDS, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    w0, v0 = on_device(words), on_device(np.arange(N_WORDS))
    w, v = w0.clone(), v0.clone()

    def one_round():
        w.copy_(w0)
        ctx.sort_words(w.data_ptr(), N_WORDS, k)
        sorted_words = back(w)
        w.copy_(w0)
        v.copy_(v0)
        ctx.sort_pairs(w.data_ptr(), v.data_ptr(), N_WORDS, k)
        return sorted_words, back(w), back(v)

    sorted_words, pair_words, _ = no_leak(ctx, one_round)
    assert sorted_words == pair_words == np.sort(words).tobytes()


def test_words_to_list_and_index(ctx):
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 1 << 32, size=500, dtype=np.uint64)
    words = keys[rng.integers(0, 500, size=N_WORDS)]
    counts = np.unique(words, return_counts=True)[1]
    assert 0 < (counts >= 10).sum() < len(counts) and counts.max() < 1000  # min_locations 10 keeps some k-mers, 1000 none
    w0, v0 = on_device(words), on_device(np.arange(N_WORDS))
    w, v = w0.clone(), v0.clone()

    def one_round():
        w.copy_(w0)
        lst = ctx.device_words_to_list(w.data_ptr(), N_WORDS, 16)
        got = [lst.download().tobytes()]
        lst.free()
        for lo in (10, 1000):
            w.copy_(w0)
            v.copy_(v0)
            kmers, n_locations, locs = ctx.pairs_to_index(w.data_ptr(), v.data_ptr(), N_WORDS, 16, lo)
            got.append((kmers.tobytes(), n_locations, locs.tobytes()))
        return got

    lst, some, none = no_leak(ctx, one_round)
    assert len(lst) == 12 * len(counts) and len(some[0]) == 16 * (counts >= 10).sum() and len(none[0]) == 0


def test_table_download_cuts_and_subset(ctx):
    dev = three_lists(ctx)
    table = ctx.device_table(dev)
    assert table.ragged

    def one_round():
        keys, counts = table.download()
        got = [keys.tobytes(), counts.tobytes(), ctx.shard_cuts(dev, 4)]  # 900 samples, 4 shards
        for method in (SM.RAND, SM.RAND_UNIQUE, SM.RAND_WEIGHTED_UNIQUE):
            n_words, total, out = ctx.subset(dev[0], method, 100, SM.state48(5))
            got.append((n_words, total, out.download().tobytes()))
            out.free()
        return got

    got = no_leak(ctx, one_round)
    assert len(got[0]) == 8 * table.n_keys and got[2][0] == 0 and got[2] == sorted(got[2])
