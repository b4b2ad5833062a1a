"""The kernels of gt4hip_seqprofile.hip run with fewer workgroups than blocks of work, by the method of
tests/test_grid_cap_gpu.py: seven blocks of work for the kernel under test, once as six full blocks and one item and once as
seven full ones; the call uncapped, then under "grid_cap" = 1, 2, 3 on a context with "poison"; the two outputs byte for
byte, the output against the CPU model, and counter "grid_capped" still in the first run and up by the striding launches of
the call in the second.

  gt4hip_seqprofile.hip  k_seq_zero           gt4hip_grid  blocks of "mm_threads" words: three per sequence and the flag
                         k_seq_profile<true>  gt4hip_grid  tiles of "profile_tile" words                 test_profile_words[mm0]
                         k_seq_profile<false> gt4hip_grid  the same tiles, behind k_query<false> on the same words  [mm1]
"""
import numpy as np
import pytest

import seqprofile_model as SP
from genometester4_amd import capi
from genometester4_amd.listio import make_records
from test_grid_cap_gpu import BLOCKS, CAP, FULL, blocks, capped, once, size
from test_gqseq_gpu import dev, raw_of, some_words, the_list

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    c.set_option("poison", 1)
    yield c
    c.set_option("grid_cap", 0)
    c.close()


def runs_for(n_words, n_seqs, seed):
    """n_seqs run lengths that add up to n_words: a third of the sequences empty, one long run, the rest a few words each"""
    rng = np.random.default_rng(seed)
    runs = rng.integers(1, 9, size=n_seqs)
    runs[rng.random(n_seqs) < 0.33] = 0
    runs[n_seqs // 2] = 0
    runs[n_seqs // 2] = n_words - int(runs.sum())
    assert runs[n_seqs // 2] > 0 and int(runs.sum()) == n_words
    return runs


@CAP
@FULL
@pytest.mark.parametrize("mm", [0, 1], ids=["mm0", "mm1"])
def test_profile_words(ctx, cap, full, mm):
    """k_seq_zero over seven blocks of sums, k_seq_profile<mm == 0> over seven tiles of words; with mm the values come from
    k_query<false>, whose blocks of variants are far more than the cap as well: three launches that stride"""
    W, T = ctx.get_counter("mm_threads"), ctx.get_counter("profile_tile")
    k = 9 if mm else 25
    n = size(T, full)
    n_seqs = (size(W, full) - 1) // 3  # 3 n_seqs + 1 words to zero: six blocks and one word, or seven blocks
    assert blocks(n, T) == BLOCKS and blocks(3 * n_seqs + 1, W) == BLOCKS and (3 * n_seqs + 1 == size(W, full))
    keys, counts = the_list(k, 40_000 if mm else 3000, 3 if mm else 1)
    words = some_words(keys, k, n, 20 + n, 0.5)
    runs = runs_for(n, n_seqs, n)
    ords = np.repeat(np.arange(n_seqs, dtype=np.uint64) + np.uint64(3), runs)
    dw, dr = dev(words), dev(raw_of(ords))
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    got = capped(ctx, cap, 3 if mm else 2, lambda: ctx.query_profile_words(ix, dw.data_ptr(), dr.data_ptr(), n, 3, n_seqs, mm))
    ix.free()
    want = once(("gqseq", full, mm), lambda: SP.profile_words(keys, counts, words, ords.astype(np.int64), n_seqs, k, mm, 0, 1, 0xFFFFFFFF, 3))
    assert want[:, 1].sum() > n // 4 and (want[:, 0] == 0).sum() > n_seqs // 4
    assert np.array_equal(np.stack([got["n_words"], got["n_hits"], got["sum"]], axis=1), want)
