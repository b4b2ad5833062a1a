/*
 * gt4hip_pair.hip -- operations on two lists: gt4hip_compare, and the pair-merge driver every other operation is built
 * from (gt4hip_run_pair: workspace sizing, partition, the merge kernel on its single-pass or two-pass path, read-back,
 * the rerun on the two-pass path; gt4hip_pair_with_outputs: the same with output lists made on demand).  Host code only,
 * no kernel: the launches are gt4hip_kernels.hip's.  `make prof` compiles this file again for the [phases] line.
 */
#include "gt4hip_host.h"

#include <stdio.h>
#include <string.h>

using namespace gt4;

size_t gt4hip_lookback_desc_bytes (uint64_t tiles)
{
  const uint64_t rows = (tiles + 63) / 64;
  return (((size_t) rows * 64 * 16 + (size_t) (rows + 1) * 32 + (size_t) rows * 32) + 255) & ~(size_t) 255; /* agg, carry, rowsum */
}

/* descriptor workspace of a pair merge: the single pass's, or u64[4] per tile on the two-pass path, in the same buffer */
static size_t desc_bytes_for (uint64_t tiles)
{
  const size_t two = ((size_t) tiles * 32 + 255) & ~(size_t) 255;
  return std::max (gt4hip_lookback_desc_bytes (tiles), two);
}

/* What the partition launch of a pair call zeroes for its merge launch (PartZero): the control block, and with `desc` (the
 * single-pass path) the chained scan's words of the streams in `ops` alone, not of all four. */
static PartZero pair_zero (gt4hip_context *ctx, uint64_t tiles, uint32_t ops, bool desc)
{
  static_assert (sizeof (PairControl) % 16 == 0, "the control block is zeroed in 16-byte chunks");
  PartZero z;
  memset (&z, 0, sizeof z);
  z.ctl = ctx->ctl;
  z.ctl_chunks = (uint32_t) (sizeof (PairControl) / 16);
  if (desc) {
    z.ops = ops;
    z.desc = ctx->desc;
    z.rows = (tiles + 63) / 64;
  }
  return z;
}

int gt4hip_run_pair (gt4hip_context *ctx, const uint32_t *A, uint64_t nA, const uint32_t *B, uint64_t nB, const PairParams &p_in,
                     bool count_only, uint32_t *const dst[4], PairRun *run, bool force_two_pass)
{
  if (p_in.ops == 8u) {
    /* the second complement alone is the first complement of the swapped pair
     * (include_in_complement (f2, f1, 0), glistcompare.c:862, :896): same specialised kernel */
    PairParams q = p_in;
    q.ops = 4u;
    q.rule[2] = p_in.rule[3];
    q.subtract = 0;
    uint32_t *const d2[4] = { NULL, NULL, dst ? dst[3] : NULL, NULL };
    const int rc = gt4hip_run_pair (ctx, B, nB, A, nA, q, count_only, d2, run, force_two_pass);
    run->n_words[3] = run->n_words[2];
    run->total_count[3] = run->total_count[2];
    run->n_words[2] = run->total_count[2] = 0;
    return rc;
  }
  if (p_in.ops == 2u && nA > nB && p_in.rule[1] != 2u && p_in.rule[1] != RULE_MINZ) {
    /* an intersection searches with the records of its first list: let that be the shorter one.
     * Keep test and every rule but SUBTRACT / the N-way running MIN are symmetric in (f1, f2);
     * FIRST and SECOND trade places. */
    PairParams q = p_in;
    if (q.rule[1] == 5u) q.rule[1] = 6u;
    else if (q.rule[1] == 6u) q.rule[1] = 5u;
    return gt4hip_run_pair (ctx, B, nB, A, nA, q, count_only, dst, run, force_two_pass);
  }
  PairParams p = p_in;
  p.spin_limit = ctx->spin_limit;
  p.a_rows_off = ctx->a_rows < 0 ? 1u : 0u;
  memset (run, 0, sizeof *run);
  const uint64_t total = nA + nB;
  if (!total || !p.ops) return GT4HIP_OK;
  const bool two_pass = (ctx->two_pass || force_two_pass) && !count_only;
  /* count-only calls: 512-thread workgroups; everything that materialises records: 1024 */
  const int geom = ctx->force_geom ? (ctx->force_geom > 0 ? 1 : 0) : (count_only ? 0 : 1);
  /* the kernels of this call: the first launch (the only one unless two_pass), and pass 2 of the two-pass path */
  const PairVariant v1 = pair_variant (geom, (count_only || two_pass) ? MODE_COUNT : MODE_LOOKBACK, p);
  const PairVariant v2 = pair_variant (geom, MODE_OFFSETS, p);
  const uint64_t tile_records = merge_tile_records (v1);
  const uint64_t tiles = (total + tile_records - 1) / tile_records;
  if (tiles >= 0xffffffffull) return gt4hip_fail (ctx, GT4HIP_EINVAL, "lists too long: %llu merge tiles", (unsigned long long) tiles);
  run->tiles = tiles;
  /* the scanner as a group of wavefronts pays off where one wavefront cannot keep up (more than ~2e4
   * rows of 64 tiles per launch: the small geometry on billions of records); below that the single
   * wavefront's shorter path to the carry is worth more (option "scan_group": -1 never, 1 always) */
  /* tiles by ticket (dynamic dealing) for the record-writing single-pass kernels of the large
   * geometry: their ~40 tiles per microsecond are well below the ~88 returning atomics per microsecond
   * one counter sustains (the count-only geometry's 200+ are not: 8.7 -> 23.8 ms), and arrival order
   * spares the fast workers the wait for the slow ones in the chained scan (measured at 2 x 2e9:
   * intersection 12.75 -> 12.55 ms, union 21.7 -> 21.45, union + intersection 27.05 -> 26.25; the first
   * complement alone is 2 % SLOWER and stays round-robin).  Option "dynamic": 1 always, -1 never. */
  p.dynamic = ctx->dynamic > 0 ? 1u : (ctx->dynamic < 0 ? 0u : ((geom == 1 && !count_only && p.ops != 4u && p.ops != 8u) ? 1u : 0u));
  p.scan_group = ctx->scan_group > 0 ? 1u : (ctx->scan_group < 0 ? 0u : (tiles > (20000ull << 6) ? 1u : 0u));
  int rc;
  if ((rc = gt4hip_grow (ctx, (void **) &ctx->part, &ctx->part_bytes, (size_t) (tiles + 1) * 16 + (size_t) (tiles / 64 + 3) * 8))) return rc; /* tile ranges + coarse co-ranks */
  const bool need_desc = !count_only;
  if (need_desc && (rc = gt4hip_grow (ctx, (void **) &ctx->desc, &ctx->desc_bytes, desc_bytes_for (tiles)))) return rc;
  if (two_pass) {
    const size_t nb = (size_t) ((tiles + 2047) / 2048) * 32;
    if ((rc = gt4hip_grow (ctx, (void **) &ctx->block_sums, &ctx->block_sums_bytes, nb))) return rc;
  }
  int grid = ctx->n_cus * merge_blocks_per_cu (v1);
  if (ctx->grid_override > 0) grid = (int) ctx->grid_override;
  if (v1.mode == MODE_LOOKBACK && grid < 2) grid = 2; /* the first workgroup to arrive is the scanner: option "grid" = 1 would leave it without a worker */
  if ((uint64_t) grid > tiles + 1) grid = (int) tiles + 1; /* workers + the scanner workgroup */
  int grid2 = ctx->n_cus * merge_blocks_per_cu (v2); /* (pass 2: no workgroup waits for another) */
  if (ctx->grid_override > 0) grid2 = (int) ctx->grid_override;
  if ((uint64_t) grid2 > tiles) grid2 = (int) tiles;

  PairOutputs outs;
  for (int s = 0; s < 4; s++) outs.rec[s] = (count_only || !dst) ? NULL : dst[s];

  hipStream_t st = ctx->stream;
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], st));
  /* (no fill launches: the partition launch zeroes the control block and the descriptor words this call reads) */
  HIPCHK (ctx, launch_partition (st, A, nA, B, nB, tiles, tile_records, ctx->part, ctx->part_guided >= 0, pair_zero (ctx, tiles, p.ops, need_desc && !two_pass)));
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], st));
  if (count_only) {
    HIPCHK (ctx, launch_pair_merge (st, v1, grid, A, nA, B, nB, ctx->part, tiles, p, outs, NULL, ctx->ctl));
  } else if (two_pass) {
    HIPCHK (ctx, launch_pair_merge (st, v1, grid, A, nA, B, nB, ctx->part, tiles, p, outs, ctx->desc, ctx->ctl));
    HIPCHK (ctx, launch_scan_tiles (st, ctx->desc, tiles, ctx->block_sums));
    HIPCHK (ctx, hipMemsetAsync (ctx->ctl, 0, sizeof (PairControl), st));
    HIPCHK (ctx, launch_pair_merge (st, v2, grid2, A, nA, B, nB, ctx->part, tiles, p, outs, ctx->desc, ctx->ctl));
  } else {
    HIPCHK (ctx, launch_pair_merge (st, v1, grid, A, nA, B, nB, ctx->part, tiles, p, outs, ctx->desc, ctx->ctl));
  }
  HIPCHK (ctx, hipEventRecord (ctx->ev[2], st));
  HIPCHK (ctx, hipMemcpyAsync (ctx->ctl_host, ctx->ctl, sizeof (PairControl), hipMemcpyDeviceToHost, st));
  HIPCHK (ctx, hipEventRecord (ctx->ev[3], st));
  HIPCHK (ctx, hipStreamSynchronize (st));
  float ms = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[1], ctx->ev[2]) == hipSuccess) run->merge_ms = ms;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[3]) == hipSuccess) run->device_ms = ms;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->partition_ms = ms;
PROF (
  {
    static const char *names[8] = { "p0 wait+lds", "B0", "ring+fetch issue", "p1 rank", "B1", "p2 scan/publish", "B2+out+B3+scatter", "housekeeping" };
    unsigned long long tot = 0;
    for (int i = 0; i < 8; i++) tot += ctx->ctl_host->phase_cycles[i];
    fprintf (stderr, "[phases] tiles %llu merge %.3f ms:", (unsigned long long) tiles, run->merge_ms);
    for (int i = 0; i < 8; i++) fprintf (stderr, " %s %.1f%%", names[i], tot ? 100.0 * ctx->ctl_host->phase_cycles[i] / tot : 0.0);
    fprintf (stderr, " | avg cycles/tile %.0f\n", tiles ? (double) tot / tiles : 0.0);
    const unsigned long long *rs = ctx->ctl_host->resolve_stats;
    if (rs[0]) fprintf (stderr, "[resolve] sampled %llu avg spins %.2f first-look agg-not-ready %.1f%% carry-not-ready %.1f%% | [scanner] rows %llu polling rounds %llu rows complete at batch load %llu\n", rs[0], (double) rs[1] / rs[0], 100.0 * rs[3] / rs[0], 100.0 * rs[4] / rs[0], rs[7], rs[5], rs[6]);
  }
)
  if (ctx->ctl_host->error) {
    const unsigned flags = ctx->ctl_host->error;
    if (!two_pass && !count_only && !(flags & 2u)) {
      /* a bounded wait of the single-pass path gave up (a worker was not resident, or the device
       * is shared): the count + scan + write path has no inter-workgroup dependency -- rerun there */
      ctx->single_pass_fallbacks++;
      return gt4hip_run_pair (ctx, A, nA, B, nB, p, count_only, dst, run, true);
    }
    return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "merge kernel reported error flags 0x%x", flags);
  }
  for (int s = 0; s < 4; s++) {
    run->n_words[s] = ctx->ctl_host->n_words[s];
    run->total_count[s] = ctx->ctl_host->total_count[s];
  }
  return GT4HIP_OK;
}

extern "C" int gt4hip_pair_partition (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, uint64_t tile_records, uint64_t *host_part)
{
  if (!ctx || !a || !b || !host_part || !tile_records) return GT4HIP_EINVAL;
  if (a->word_length != b->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ (%u != %u)", b->word_length, a->word_length);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  const uint64_t tiles = (a->n_words + b->n_words + tile_records - 1) / tile_records;
  if (tiles >= 0xffffffffull) return gt4hip_fail (ctx, GT4HIP_EINVAL, "lists too long: %llu merge tiles", (unsigned long long) tiles);
  int rc;
  if ((rc = gt4hip_grow (ctx, (void **) &ctx->part, &ctx->part_bytes, (size_t) (tiles + 1) * 16 + (size_t) (tiles / 64 + 3) * 8))) return rc;
  PartZero none;
  memset (&none, 0, sizeof none);
  HIPCHK (ctx, launch_partition (ctx->stream, (const uint32_t *) a->dev, a->n_words, (const uint32_t *) b->dev, b->n_words, tiles, tile_records, ctx->part,
                                 ctx->part_guided >= 0, none));
  return gt4hip_read_back (ctx, host_part, ctx->part, (size_t) (tiles + 1) * 16, "gt4hip_pair_partition: reading the tile ranges back failed");
}

static uint64_t worst_case (int s, uint64_t nA, uint64_t nB)
{
  switch (s) {
    case 0: return nA + nB;
    case 1: return nA < nB ? nA : nB;
    case 2: return nA;
    default: return nB;
  }
}

int gt4hip_pair_with_outputs (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, const PairParams &p, bool count_only,
                              gt4hip_list *out[4], PairRun *run)
{
  TempLists made;
  gt4hip_list *use[4] = { NULL, NULL, NULL, NULL };
  uint32_t *dst[4] = { NULL, NULL, NULL, NULL };
  int rc;
  for (int s = 0; s < 4 && !count_only; s++) {
    if (!((p.ops >> s) & 1u)) continue;
    if ((rc = gt4hip_output_list (ctx, s, out[s], worst_case (s, a->n_words, b->n_words), a->word_length, made, &use[s]))) return rc;
    dst[s] = (uint32_t *) use[s]->dev;
  }
  if ((rc = gt4hip_run_pair (ctx, (const uint32_t *) a->dev, a->n_words, (const uint32_t *) b->dev, b->n_words, p, count_only, dst, run))) return rc;
  made.release ();
  for (int s = 0; s < 4; s++)
    if (use[s]) {
      out[s] = use[s];
      out[s]->n_words = run->n_words[s];
      out[s]->word_length = a->word_length;
    }
  return GT4HIP_OK;
}

extern "C" int gt4hip_compare (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b,
                                const gt4hip_compare_params *prm, gt4hip_compare_result *res)
{
  if (!ctx || !a || !b || !prm || !res) return GT4HIP_EINVAL;
  if (prm->ops & ~15u) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare: unknown op bits 0x%x", prm->ops);
  if (prm->rule < 0 || prm->rule > 7) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare: unknown rule %d", prm->rule);
  if (a->word_length != b->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ (%u != %u)", b->word_length, a->word_length);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  PairParams p;
  memset (&p, 0, sizeof p);
  p.ops = prm->ops;
  /* DEFAULT resolves per output: ADD for union (:463), MIN for intersection (:472), SUBTRACT for
   * both complements (:486) */
  const uint32_t r = (uint32_t) prm->rule;
  p.rule[0] = r ? r : GT4HIP_RULE_ADD;
  p.rule[1] = r ? r : GT4HIP_RULE_MIN;
  p.rule[2] = r ? r : GT4HIP_RULE_SUBTRACT;
  p.rule[3] = r ? r : GT4HIP_RULE_SUBTRACT;
  p.cutoff = prm->cutoff;
  p.subtract = prm->subtract ? 1u : 0u;
  p.count_override = prm->count_override;
  p.filter = FILTER_REFERENCE;
  PairRun run;
  gt4hip_list *out[4];
  for (int s = 0; s < 4; s++) out[s] = ((prm->ops >> s) & 1u) && !prm->count_only ? res->out[s] : NULL;
  int rc = gt4hip_pair_with_outputs (ctx, a, b, p, prm->count_only != 0, out, &run);
  if (rc) return rc;
  for (int s = 0; s < 4; s++) {
    res->n_words[s] = run.n_words[s];
    res->total_count[s] = run.total_count[s];
    res->out[s] = out[s];
  }
  res->merge_kernel_ms = run.merge_ms;
  res->device_ms = run.device_ms;
  res->merge_tiles = run.tiles;
  return GT4HIP_OK;
}
