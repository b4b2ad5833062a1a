/* gt4hip_nway_host.h -- N-way: the launch of the tile kernel by mode, and the host side of one call as a list of stages
 * (nway_run: key probe, sample levels, per level the partition with its retries and the launch, read-back, the ragged
 * table's index).  No kernel.  Included by gt4hip_nway_body.h inside namespace gt4::<anon>::km8 / km32; no include guard. */
constexpr int NWAY_NT = GT4_NWAY_NT;
constexpr int NWAY_NBF = GT4_NWAY_NBF;
/* positions per thread: the modes that keep no ordered copy of the tile (GT4_NWAY_LEAD) have LDS for one more */
#define GT4_NWAY_RPT_LEAD GT4_NWAY_RPT
constexpr int nway_rpt (int mode) { return nway_lead (mode) ? GT4_NWAY_RPT_LEAD : GT4_NWAY_RPT; }
constexpr int nway_cap (int mode) { return NWAY_NT * nway_rpt (mode); }
constexpr int NWAY_CAP_MIN = NWAY_NT * (GT4_NWAY_RPT_LEAD < GT4_NWAY_RPT ? GT4_NWAY_RPT_LEAD : GT4_NWAY_RPT);

/* f (std::integral_constant<int, MODE> ()) for the run-time `mode`: the one place that names the five instances */
template <typename F>
auto nway_with_mode (int mode, F f)
{
  if (mode == NWAY_DUPS) return f (std::integral_constant<int, NWAY_DUPS> ());
  if (mode == NWAY_COUNT) return f (std::integral_constant<int, NWAY_COUNT> ());
  if (mode == NWAY_TABLE) return f (std::integral_constant<int, NWAY_TABLE> ());
  if (mode == NWAY_PROBE) return f (std::integral_constant<int, NWAY_PROBE> ());
  return f (std::integral_constant<int, NWAY_UNION> ());
}

hipError_t launch_nway_mode (hipStream_t s, int mode, int grid, const NwayParams &p, const u64 *part, u32 *out, u64 *desc, PairControl *ctl)
{
  return nway_with_mode (mode, [&] (auto m) {
    constexpr int MODE = decltype (m)::value;
    hipLaunchKernelGGL ((k_nway_merge<NWAY_NT, nway_rpt (MODE), NWAY_NBF, MODE>), dim3 (grid), dim3 (NWAY_NT), 0, s, p, part, out, desc, ctl);
    return hipGetLastError ();
  });
}

int nway_blocks_per_cu (int mode)
{
  static int cache[5] = { 0, 0, 0, 0, 0 };
  if (!cache[mode]) {
    int n = 0;
    const hipError_t e = nway_with_mode (mode, [&] (auto m) {
      constexpr int MODE = decltype (m)::value;
      return hipOccupancyMaxActiveBlocksPerMultiprocessor (&n, k_nway_merge<NWAY_NT, nway_rpt (MODE), NWAY_NBF, MODE>, NWAY_NT, 0);
    });
    if (e != hipSuccess || n < 1) n = 1;
    const int by_regs = nway_waves_per_simd (NWAY_NT) * 4 / (NWAY_NT / 64);
    if (by_regs >= 1 && n > by_regs) n = by_regs;
    cache[mode] = n;
  }
  return cache[mode];
}

/* ------------------------------------------------------------------ host orchestration */

namespace host_part {

struct Level {
  NwayParams p;            /* lists of this level (level 0: the caller's; above: sample lists) */
  u64 total;
};

/* One call: its arguments and what the stages hand on.  A stage returns GT4HIP_OK, an error, or NWAY_TREE. */
struct NwayCall {
  gt4hip_context *ctx;
  const gt4hip_list *const *lists;
  u32 k, rule, cutoff, ovr, filter;
  bool count_only;
  gt4hip_list *out;
  gt4hip_count_table *table; /* NULL: a union; else the count table (probe: its rows are the records of lists[0]) */
  const uint32_t *cols;
  bool probe;
  bool may_decline;          /* option "kway" = 1 (the default) lets a union decline clustered keys */
  u64 one_tile;              /* records that fit one tile whatever they are */
  std::vector<Level> levels;
  TempLists samples;         /* the sample lists of the levels above 0 */
  TempLists merged;          /* the merged sample records of the level above the one in the making: one list or none
                              * (the last member: they go back to the pool first, then the sample lists) */
  const gt4hip_list *above () const { return merged.lists.empty () ? NULL : merged.lists[0]; }
};
constexpr int NWAY_TREE = -1; /* not an error: nothing was produced, *used = 0, the caller takes the pairwise tree */

/* samples per tile: a tile between two boundary keys G samples apart holds at most G + k - 1 samples
 * (ties at the boundaries), each list at most (its samples + 1) * S - 1 records, every run rounded up
 * to whole wavefronts.  `sure`: the G for which no tile can overflow; the first try takes the expected
 * tile (G * S records) plus GT4_NWAY_MARGIN (five) standard deviations of the lists' offsets against their sample grids; tiles beyond the
 * capacity are cut in two (k_nway_emit). */
void nway_samples_per_tile (u32 k, int positions, u32 *first_try, u32 *sure)
{
  const double cap = (double) positions - 0.5 * NWAY_HS * k; /* half a slot of padding per run, on average */
  const double margin = GT4_NWAY_MARGIN * NWAY_SAMPLE * sqrt ((double) k / 6.0);
  long g1 = (long) ((cap - margin) / NWAY_SAMPLE);
  long g0 = ((long) positions - (long) NWAY_HS * k) / NWAY_SAMPLE - (2L * k - 1);
  if (g0 < 1) g0 = 1;
  if (g1 < g0) g1 = g0;
  *first_try = (u32) g1;
  *sure = (u32) g0;
}

/* Clustered keys?  Windows of the longest list, probed in front of everything else and read at once (read with the first
 * partition read-back, a call that declines had sampled, merged samples and partitioned for nothing -- 1.3 ms of a
 * 53 ms tree on the clustered bench lists). */
int nway_key_probe (NwayCall &c)
{
  gt4hip_context *const ctx = c.ctx;
  if (!c.may_decline) return GT4HIP_OK;
  uint32_t longest = 0;
  for (uint32_t i = 1; i < c.k; i++)
    if (c.lists[i]->n_words > c.lists[longest]->n_words) longest = i;
  const u64 nl = c.lists[longest]->n_words;
  if (nl < 16ull * NWAY_PROBE_KEYS) return GT4HIP_OK;
  const u32 windows = (u32) (nl / (4 * NWAY_PROBE_KEYS) < NWAY_PROBE_WINDOWS ? nl / (4 * NWAY_PROBE_KEYS) : NWAY_PROBE_WINDOWS);
  const hipError_t e = hipMemsetAsync ((char *) ctx->scratch + 32, 0, 8, ctx->stream);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "N-way key probe failed: %s", hipGetErrorString (e));
  hipLaunchKernelGGL (k_nway_probe, dim3 (windows), dim3 (256), 0, ctx->stream, (const u32 *) c.lists[longest]->dev, nl, windows, (u32) nway_buckets (NWAY_NBF * nway_cap (NWAY_UNION)), (u32 *) ctx->scratch + 8);
  const int rc = gt4hip_read_back (ctx, ctx->scratch_host + 4, (char *) ctx->scratch + 32, 8, "N-way key probe failed");
  if (rc) return rc;
  if (5ull * (u32) ctx->scratch_host[4] <= windows) return GT4HIP_OK;
  ctx->kway_declined++;
  return NWAY_TREE;
}

/* sample levels (every NWAY_SAMPLE-th key of every list of the level below) until one fits a single tile */
int nway_sample_levels (NwayCall &c)
{
  while (c.levels.back ().total > c.one_tile) {
    const Level &lo = c.levels.back ();
    Level up;
    memset (&up, 0, sizeof up);
    up.p.k = c.k;
    for (uint32_t i = 0; i < c.k; i++) {
      const u64 m = lo.p.n[i] / NWAY_SAMPLE;
      gt4hip_list *s = NULL;
      const int rc = gt4hip_list_new (c.ctx, m ? m : 1, c.lists[0]->word_length, &s);
      if (rc) return rc;
      up.p.list[i] = (const u32 *) c.samples.adopt (s)->dev;
      up.p.n[i] = m;
      up.total += m;
    }
    if (up.total) {
      u64 g = (up.total + 255) / 256;
      if (g > 16384) g = 16384;
      hipLaunchKernelGGL (k_nway_sample, dim3 ((unsigned) g), dim3 (256), 0, c.ctx->stream, lo.p, up.p);
    }
    c.levels.push_back (up);
  }
  return GT4HIP_OK;
}

/* The control block -> ctx->ctl_host, and what it says: GT4HIP_OK, an internal error, or NWAY_TREE where a bounded wait
 * gave up (a shared device): the tree redoes the call. */
int nway_read_outcome (gt4hip_context *ctx, const char *what)
{
  const int rc = gt4hip_read_back (ctx, ctx->ctl_host, ctx->ctl, sizeof (PairControl), what);
  if (rc || !ctx->ctl_host->error) return rc;
  const unsigned flags = ctx->ctl_host->error;
  if (flags & 2u) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "N-way merge kernel reported error flags 0x%x", flags);
  ctx->single_pass_fallbacks++;
  return NWAY_TREE;
}

/* the launches that cut `lv` into `tiles` tiles at every G-th of the merged samples -> ctx->kway_part */
int nway_cut_level (NwayCall &c, const Level &lv, u32 G, u64 tiles, u32 n_buckets)
{
  gt4hip_context *const ctx = c.ctx;
  hipStream_t st = ctx->stream;
  const gt4hip_list *const merged = c.above ();
  const u64 m_total = merged ? merged->n_words : 0;
  int rc;
  if ((rc = gt4hip_grow (ctx, (void **) &ctx->kway_part, &ctx->kway_part_bytes, (size_t) (tiles + 1) * NWAY_PSTRIDE * 8))) return rc;
  if (merged && ctx->kway_vt != 97 && G <= NWAY_G_MAX) {
    /* from the merged samples' list numbers (option "kway_vt" = 97 keeps the searches over whole brackets: tests) */
    const u64 n_br = (tiles + 1 + NWAY_BRACKET - 1) / NWAY_BRACKET;
    if ((rc = gt4hip_grow (ctx, (void **) &ctx->kway_cnt, &ctx->kway_cnt_bytes, (size_t) n_br * NWAY_MAX * 4))) return rc;
    hipLaunchKernelGGL (k_nway_sample_counts, dim3 ((unsigned) ((n_br + 3) / 4)), dim3 (256), 0, st, (const u32 *) merged->dev, m_total, G, n_br, (u32 *) ctx->kway_cnt);
    hipLaunchKernelGGL (k_nway_bracket_bases, dim3 (1), dim3 (NWAY_MAX > 8 ? 1024 : 64 * NWAY_MAX), 0, st, (u32 *) ctx->kway_cnt, n_br);
    hipLaunchKernelGGL (k_nway_partition_rows, dim3 ((unsigned) n_br), dim3 (64), 0, st, lv.p, (const u32 *) merged->dev, m_total, G, n_buckets,
                        (const u32 *) ctx->kway_cnt, (u64 *) ctx->kway_part);
  } else {
    const u64 threads = (tiles + 1) * NWAY_PSTRIDE;
    for (int pass = 0; pass < 2; pass++)
      hipLaunchKernelGGL (k_nway_partition, dim3 ((unsigned) ((threads + 255) / 256)), dim3 (256), 0, st, lv.p, merged ? (const u32 *) merged->dev : NULL,
                          m_total, G, n_buckets, (u64 *) ctx->kway_part, pass);
  }
  return GT4HIP_OK;
}

/* Level l -> tiles that fit the capacity of `mode`: cut at every G-th merged sample, tiles that do not fit cut in two;
 * where that does not do, again with fewer samples per tile, down to the number that cannot overflow.  *part_final:
 * the table the tile kernel reads (the partition's, or the one with the split tiles), *tiles_out its tiles. */
int nway_partition_level (NwayCall &c, int l, int mode, const u64 **part_final, u64 *tiles_out)
{
  gt4hip_context *const ctx = c.ctx;
  hipStream_t st = ctx->stream;
  Level &lv = c.levels[l];
  const bool top = !c.above ();
  const u64 m_total = top ? 0 : c.above ()->n_words;
  const int cap = nway_cap (mode); /* positions of a tile */
  const u32 n_buckets = (u32) nway_buckets (NWAY_NBF * cap);
  u32 G, g_sure;
  nway_samples_per_tile (c.k, cap, &G, &g_sure);
  if (ctx->kway_g > 0) G = (u32) ctx->kway_g;
  int rc;
  for (;;) {
    u64 tiles = m_total ? m_total / G + 2 : 1;
    if (tiles >= 0xfffffff0ull) return gt4hip_fail (ctx, GT4HIP_EINVAL, "lists too long: %llu tiles", (unsigned long long) tiles);
    lv.p.num_tiles = (u32) tiles;
    if ((rc = nway_cut_level (c, lv, G, tiles, n_buckets))) return rc;
    /* tiles that do not fit are cut in two (k_nway_need / _scan / _emit): flags = { more than two pieces,
     * clustered tiles, tiles cut, tiles of the final table } */
    const u64 n_blocks = (tiles + 1 + NWAY_SPLIT_BLOCK - 1) / NWAY_SPLIT_BLOCK;
    if ((rc = gt4hip_grow (ctx, (void **) &ctx->kway_need, &ctx->kway_need_bytes, (size_t) (tiles + 1 + n_blocks + 4) * 4))) return rc;
    u32 *const need = (u32 *) ctx->kway_need, *const block_sums = need + tiles + 1;
    *part_final = (const u64 *) ctx->kway_part;
    *tiles_out = tiles;
    if (tiles == 1 && top && lv.total <= c.one_tile) {
      /* the top level: one tile that fits by construction -- nothing to cut, nothing to read back */
      if (l == 0) ctx->kway_splits = 0;
      return GT4HIP_OK;
    }
    hipMemsetAsync (ctx->scratch, 0, 32, st);
    hipLaunchKernelGGL (k_nway_need, dim3 ((unsigned) n_blocks), dim3 (NWAY_SPLIT_BLOCK), 0, st, (const u64 *) ctx->kway_part, (u32) tiles, (u32) (cap / NWAY_HS), need, block_sums,
                        (u32 *) ctx->scratch);
    hipLaunchKernelGGL (k_nway_need_scan, dim3 (1), dim3 (1024), 0, st, block_sums, (u32) n_blocks, (u32 *) ctx->scratch + 3);
    if ((rc = gt4hip_read_back (ctx, ctx->scratch_host, ctx->scratch, 40, "N-way partition failed"))) return rc;
    const u32 *const fl = (const u32 *) ctx->scratch_host;
    bool overflow = fl[0] != 0;
    u32 splits = 0;
    if (!overflow && fl[2]) {
      const u64 tiles2 = fl[3];
      if ((rc = gt4hip_grow (ctx, (void **) &ctx->kway_part2, &ctx->kway_part2_bytes, (size_t) (tiles2 + 1) * NWAY_PSTRIDE * 8))) return rc;
      hipLaunchKernelGGL (k_nway_emit, dim3 ((unsigned) n_blocks), dim3 (NWAY_SPLIT_BLOCK), 0, st, lv.p, (const u64 *) ctx->kway_part, (u32) tiles, need, block_sums,
                          n_buckets, (u32) (cap / NWAY_HS), (u64 *) ctx->kway_part2, (u32 *) ctx->scratch);
      if ((rc = gt4hip_read_back (ctx, ctx->scratch_host + 4, ctx->scratch, 4, "N-way partition failed"))) return rc;
      overflow = (u32) ctx->scratch_host[4] != 0;
      if (!overflow) {
        splits = fl[2];
        *part_final = (const u64 *) ctx->kway_part2;
        *tiles_out = tiles = tiles2;
        lv.p.num_tiles = (u32) tiles;
      }
    }
    if (!overflow) {
      if (l == 0) ctx->kway_splits = splits;
      if (l > 0 || !c.may_decline || tiles < 64 || 5ull * fl[1] <= tiles) return GT4HIP_OK;
      /* the probe of the longest list did not see it, the tiles' own samples do: clustered keys */
      ctx->kway_declined++;
      return NWAY_TREE;
    }
    /* a tile would overflow LDS: fewer samples per tile, down to the number that cannot overflow */
    ctx->kway_overflows++;
    /* The cuts come from the merged samples of the level above, whose launch is not read back on its own.  If a bounded
     * wait gave up there (a shared device) the samples are incomplete and the partition built on them is garbage: that
     * is not a capacity problem -- the tree redoes the call, as a give-up in the last launch does. */
    if (!top && (rc = nway_read_outcome (ctx, "N-way partition failed"))) return rc;
    if (G <= g_sure) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "N-way partition: a tile exceeds the capacity at %u samples per tile", G);
    const u32 g2 = G - (G + 7) / 8;
    G = g2 > g_sure ? g2 : g_sure;
  }
}

/* Level 0 of a count table: the table exists before the launch, which writes keys and counts directly. */
int nway_table_outputs (NwayCall &c, Level &lv, u64 tiles)
{
  gt4hip_context *const ctx = c.ctx;
  gt4hip_count_table *const table = c.table;
  int rc;
  if (c.probe) { /* rows = the records of list 0 */
    if ((rc = gt4hip_table_alloc (ctx, table, c.lists[0]->n_words, table->n_lists))) return rc;
    table->n_keys = c.lists[0]->n_words;
    /* (up to ROW_COLS_MAX columns every row leaves the kernel whole, zeros included: no memset -- round 5) */
    if (table->n_lists > (uint32_t) NwayShared<NWAY_NT, nway_rpt (NWAY_PROBE), NWAY_NBF, NWAY_PROBE>::ROW_COLS_MAX)
      hipMemsetAsync (table->device_counts, 0, (size_t) table->n_keys * table->n_lists * 4, ctx->stream);
  } else {
    /* ONE launch (round 4): every tile writes its rows where its records start -- a tile has at most as many distinct
     * keys as records, so the table is allocated for the records and stays RAGGED (unused rows behind every tile's;
     * gt4hip_table_download and gt4hip_table_compact know, see gt4hip_count_table).  Round 3 counted every tile's
     * distinct keys in a launch of their own first: the records were read twice. */
    if ((rc = gt4hip_grow (ctx, (void **) &ctx->desc, &ctx->desc_bytes, (size_t) tiles * 4 + 32 + (size_t) ((tiles + 1 + 1023) / 1024) * 8))) return rc; /* the tiles' totals, then their sums per block of 1024 */
    if ((rc = gt4hip_table_alloc (ctx, table, lv.total, table->n_lists))) return rc;
    lv.p.tile_totals = (u32 *) ctx->desc;
  }
  lv.p.table_keys = (u64 *) table->device_keys;
  lv.p.table_counts = (u32 *) table->device_counts;
  lv.p.table_cols = table->n_lists;
  for (uint32_t i = 0; i < c.k; i++) lv.p.table_col[i] = c.cols[i];
  return GT4HIP_OK;
}

/* One launch of the tile kernel over level l (above level 0: the merged samples -> dst; nothing is read back there: the
 * error word, if any, stays set through the later launches and is seen with the last one). */
int nway_launch_level (NwayCall &c, int l, int mode, u64 tiles, const u64 *part_final, u32 *dst)
{
  gt4hip_context *const ctx = c.ctx;
  hipStream_t st = ctx->stream;
  NwayParams &p = c.levels[l].p;
  p.rule = c.rule;
  p.cutoff = c.cutoff;
  p.count_override = c.ovr;
  p.filter = c.filter;
  p.spin_limit = ctx->spin_limit;
  p.force_fallback = ctx->kway_vt == 99 ? 1u : (ctx->kway_vt == 98 ? 2u : 0u); /* option "kway_vt" = 99 / 98: every tile takes the search path / the pivot-run buckets (tests) */
  p.scan_group = ctx->scan_group > 0 ? 1u : (ctx->scan_group < 0 ? 0u : (tiles > (48000ull << 6) ? 1u : 0u));
  p.dynamic = ctx->dynamic > 0 ? 1u : (ctx->dynamic < 0 ? 0u : (mode == NWAY_UNION ? 1u : 0u));
  int grid = ctx->n_cus * nway_blocks_per_cu (mode);
  if (ctx->grid_override > 0) grid = (int) ctx->grid_override;
  if (mode == NWAY_UNION) {
    const int rc = gt4hip_grow (ctx, (void **) &ctx->desc, &ctx->desc_bytes, gt4hip_lookback_desc_bytes (tiles));
    if (rc) return rc;
    hipMemsetAsync (ctx->desc, 0, gt4hip_lookback_desc_bytes (tiles), st);
    if (grid < 2) grid = 2; /* the first workgroup to arrive is the scanner: option "grid" = 1 would leave it without a worker */
    if ((u64) grid > tiles + 1) grid = (int) tiles + 1;
  } else if ((u64) grid > tiles) {
    grid = (int) tiles;
  }
  hipMemsetAsync (ctx->ctl, 0, offsetof (PairControl, error), st); /* (totals, ticket; the error word stays) */
  hipMemsetAsync (&ctx->ctl->role, 0, sizeof (PairControl) - offsetof (PairControl, role), st);
  if (l == 0) hipEventRecord (ctx->ev[1], st);
  hipError_t e = launch_nway_mode (st, mode, grid, p, part_final, dst, (u64 *) ctx->desc, ctx->ctl);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "N-way merge launch failed: %s", hipGetErrorString (e));
  if (l == 0) hipEventRecord (ctx->ev[2], st);
  e = l == 0 ? hipEventRecord (ctx->ev[3], st) : hipSuccess;
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "hipEventRecord failed: %s", hipGetErrorString (e));
  return GT4HIP_OK;
}

/* the ragged table's index: rows before every tile (compact) and where the tile's rows lie (padded) */
int nway_ragged_index (NwayCall &c, u64 tiles, const u64 *part_final)
{
  gt4hip_context *const ctx = c.ctx;
  hipStream_t st = ctx->stream;
  const int rc = gt4hip_table_set_ragged (ctx, c.table, tiles);
  if (rc) return rc;
  const u64 nb = (tiles + 1 + 1023) / 1024;
  u64 *const bsum = (u64 *) ((char *) ctx->desc + (((size_t) tiles * 4 + 15) & ~(size_t) 15)); /* (behind the tiles' totals) */
  hipLaunchKernelGGL (k_nway_base_sums, dim3 ((unsigned) nb), dim3 (1024), 0, st, (const u32 *) ctx->desc, tiles, bsum);
  hipLaunchKernelGGL (k_nway_base_scan, dim3 (1), dim3 (1024), 0, st, bsum, nb);
  hipLaunchKernelGGL (k_nway_tile_bases, dim3 ((unsigned) nb), dim3 (1024), 0, st, (const u32 *) ctx->desc, tiles, (const u64 *) bsum, (u64 *) gt4hip_table_compact_bases (c.table));
  hipLaunchKernelGGL (k_nway_padded_bases, dim3 ((unsigned) ((tiles + 256) / 256)), dim3 (256), 0, st, part_final, tiles, c.k, (u64 *) gt4hip_table_padded_bases (c.table));
  const hipError_t e = hipStreamSynchronize (st);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "count table index failed: %s", hipGetErrorString (e));
  return GT4HIP_OK;
}

PROF (void nway_print_phases (const gt4hip_context *ctx, u64 tiles) {
  static const char *names[24] = { "p0: zeroing", "B1", "scan1", "B2", "scan2", "B3", "group", "B4", "rank", "fold", "service", "B5", "writeout+fill", "order", "B6", "stage+publish", "sv:-", "sv:table", "sv:ticket+row", "sv:try writeout | header", "p0: wait for records", "p0: buckets+atomics", "p0: fetch issue", "back edge" };
  unsigned long long tot = 0;
  for (int i = 0; i < 24; i++) tot += ctx->ctl_host->phase_cycles[i];
  fprintf (stderr, "[nway phases] tiles %llu:", (unsigned long long) tiles);
  for (int i = 0; i < 24; i++) fprintf (stderr, " %s %.1f%%", names[i], tot ? 100.0 * ctx->ctl_host->phase_cycles[i] / tot : 0.0);
  fprintf (stderr, " | avg cycles/tile %.0f\n", tiles ? (double) tot / tiles : 0.0);
})

/* the call's times (events 0 .. 3: whole call, the last launch) and tiles, for the result and the counters */
void nway_record_timings (gt4hip_context *ctx, u64 tiles, double *device_ms)
{
  float ms = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[3]) == hipSuccess) *device_ms = ms;
  if (hipEventElapsedTime (&ms, ctx->ev[1], ctx->ev[2]) == hipSuccess) ctx->nway_kernel_ms = ms;
  ctx->nway_tiles = tiles;
}

/* The stages in order.  Host read-backs (round 5: nine per call of three levels -> four; each is a drained stream plus
 * 20 - 30 us, 0.3 ms of a 4.7 ms call on an eighth of the bench's lists, i.e. of one GPU's shard at 8 GPUs): a top level of
 * one tile reads nothing back, the sample levels' control blocks are not read back. */
int nway_stages (NwayCall &c, uint64_t *n_words, uint64_t *total_count, double *device_ms)
{
  gt4hip_context *const ctx = c.ctx;
  hipStream_t st = ctx->stream;
  const hipError_t e0 = hipEventRecord (ctx->ev[0], st);
  if (e0 != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "hipEventRecord failed: %s", hipGetErrorString (e0));
  hipMemsetAsync (ctx->ctl, 0, sizeof (PairControl), st);
  ctx->nway_sample_tiles = 0;
  int rc;
  if ((rc = nway_key_probe (c))) return rc;
  if ((rc = nway_sample_levels (c))) return rc;
  /* top-down: the merged samples of level l+1 cut level l into tiles */
  for (int l = (int) c.levels.size () - 1; l >= 0; l--) {
    Level &lv = c.levels[l];
    const int mode = l > 0 ? NWAY_DUPS : (c.table ? (c.probe ? NWAY_PROBE : NWAY_TABLE) : (c.count_only ? NWAY_COUNT : NWAY_UNION));
    const u64 *part_final = NULL;
    u64 tiles = 1;
    if ((rc = nway_partition_level (c, l, mode, &part_final, &tiles))) return rc;
    if (l > 0 && tiles > ctx->nway_sample_tiles) ctx->nway_sample_tiles = tiles;
    c.merged.clear ();
    u32 *dst = (l > 0 || c.count_only) ? NULL : (u32 *) c.out->dev;
    if (l > 0) {
      gt4hip_list *m = NULL;
      if ((rc = gt4hip_list_new (ctx, lv.total ? lv.total : 1, c.lists[0]->word_length, &m))) return rc;
      c.merged.adopt (m)->n_words = lv.total;
      dst = (u32 *) m->dev;
    } else if (c.table && (rc = nway_table_outputs (c, lv, tiles))) {
      return rc;
    }
    if ((rc = nway_launch_level (c, l, mode, tiles, part_final, dst))) return rc;
    if (l > 0) continue;
    /* the last launch reads its control block back: a refused tile or a wait that gave up must not go unseen */
    if ((rc = nway_read_outcome (ctx, "N-way merge failed"))) return rc;
    PROF (nway_print_phases (ctx, tiles);)
    *n_words = ctx->ctl_host->n_words[0];
    *total_count = ctx->ctl_host->total_count[0];
    if (c.table && !c.probe) {
      c.table->n_keys = *n_words;
      if ((rc = nway_ragged_index (c, tiles, part_final))) return rc;
    }
    nway_record_timings (ctx, tiles, device_ms);
  }
  return GT4HIP_OK;
}

}  // namespace host_part
using namespace host_part;

int nway_run (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t k, uint32_t rule, uint32_t cutoff, uint32_t ovr, uint32_t filter, bool count_only,
              gt4hip_list *out, uint64_t *n_words, uint64_t *total_count, double *device_ms, int *used, gt4hip_count_table *table, const uint32_t *cols, bool probe)
{
  *used = 0;
  if (k < 2 || k > NWAY_MAX) return GT4HIP_OK;
  NwayCall c = { ctx, lists, k, rule, cutoff, ovr, filter, count_only, out, table, cols, probe };
  c.may_decline = ctx->kway_enabled == 1 && !table && ctx->kway_vt == 0;
  c.one_tile = (u64) NWAY_CAP_MIN - (u64) NWAY_HS * k;
  Level l0;
  memset (&l0, 0, sizeof l0);
  l0.p.k = k;
  for (uint32_t i = 0; i < k; i++) {
    l0.p.list[i] = (const u32 *) lists[i]->dev;
    l0.p.n[i] = lists[i]->n_words;
    l0.total += lists[i]->n_words;
  }
  c.levels.push_back (l0);
  const int rc = nway_stages (c, n_words, total_count, device_ms);
  *used = rc == GT4HIP_OK;
  return rc == NWAY_TREE ? GT4HIP_OK : rc;
}
