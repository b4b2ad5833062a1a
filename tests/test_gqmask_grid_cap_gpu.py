"""The kernels of gt4hip_mask.hip run with fewer workgroups than blocks of work, by the method of tests/test_grid_cap_gpu.py:
seven tiles of codes and seven tiles of text for the kernels under test, once as six full tiles and one item and once as
seven full ones; the call uncapped, then under "grid_cap" = 1, 2, 3 on a context with "poison"; the two outputs byte for
byte, the output against the CPU model, and counter "grid_capped" still in the first run and up by the striding launches of
the call in the second.

  gt4hip_mask.hip  k_mask_ends<true>   gt4hip_grid  tiles of "maker_code_tile" codes                         test_mask_text[mm0]
                   k_mask_ends<false>  gt4hip_grid  the same tiles, behind k_query<false> on the piece's words          [mm1]
                   k_mask_apply        gt4hip_grid  tiles of "maker_text_tile" bytes (hard with mm0, soft with mm1)

The text goes in as two pieces, the name line and a sequence without a line break: every byte of the second piece is a
code, so its tiles of codes are its tiles of text."""
import numpy as np
import pytest

import mask_model as MM
import reader_texts as RT
from genometester4_amd import capi
from genometester4_amd.listio import make_records
from test_grid_cap_gpu import BLOCKS, CAP, FULL, blocks, capped, once, size

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    c.set_option("poison", 1)
    yield c
    c.set_option("grid_cap", 0)
    c.close()


@CAP
@FULL
@pytest.mark.parametrize("mm", [0, 1], ids=["mm0", "mm1"])
def test_mask_text(ctx, cap, full, mm):
    """the reader's four striding kernels, k_mask_ends and k_mask_apply over seven tiles; with mm the values come from
    k_query<false>, whose blocks of variants are far more than the cap as well"""
    T = ctx.get_counter("maker_code_tile")
    assert T == ctx.get_counter("maker_text_tile")
    k, soft = (9, True) if mm else (25, False)
    n = size(T, full)
    assert blocks(n, T) == BLOCKS
    head = b">s\n"
    text = head + RT.bases(n)

    def expectation():
        words = np.array(MM.read_bases(text, k)[0], dtype=np.uint64)
        rng = np.random.default_rng(n + mm)
        keys = np.unique(words[rng.random(len(words)) < (0.02 if mm else 0.3)])
        counts = rng.integers(1, 9, size=len(keys), dtype=np.uint32)
        return keys, counts, MM.mask_text(keys, counts, text, k, mm, 0, 2, 7, soft)
    keys, counts, m = once(("gqmask", full, mm), expectation)
    assert 0 < m.counts[1] < m.counts[0] and 0 < m.counts[2] < n
    ix = ctx.upload(make_records(keys, counts), k).query_index()
    got = capped(ctx, cap, 7 if mm else 6, lambda: ctx.query_mask_text(ix, [head, text[len(head):]], mm, 0, 2, 7, soft), uncut=not mm)
    ix.free()
    masked, recs = got
    assert masked == m.text
    assert recs[0] == {"n_words": 0, "n_hits": 0, "n_covered": 0, "back": 0}
    assert recs[1] == {"n_words": m.counts[0], "n_hits": m.counts[1], "n_covered": m.counts[2], "back": 0}
