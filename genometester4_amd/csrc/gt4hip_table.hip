/*
 * gt4hip_table.hip -- per-key count tables (gt4_union / gt4_is_union of include/gt4_set_operations.h, glistquery):
 * blocks and tables from the block pool, the ragged table one launch of the N-way tile kernel leaves (its index,
 * gt4hip_table_compact, gt4hip_table_download), gt4hip_union_table and gt4hip_probe_table* by that launch or, where
 * it does not apply, by a pair merge per column.
 * One kernel lives here: k_table_gather (rows of a ragged table, gathered).
 */
#include "gt4hip_host.h"

#include <string.h>
#include <chrono>
#include <new>

using namespace gt4;

/* Device memory that comes from the context's block pool and goes back to it (big hipMalloc / hipFree
 * pairs per call stall for a second every few calls on this driver): a list object owns the block. */
int gt4hip_block_alloc (gt4hip_context *ctx, size_t bytes, void **dev, void **owner)
{
  gt4hip_list *l = NULL;
  const int rc = gt4hip_list_new (ctx, bytes / GT4HIP_RECORD_BYTES + 1, 1, &l);
  if (rc) return rc;
  *dev = l->dev;
  *owner = l;
  return GT4HIP_OK;
}

void gt4hip_block_free (void *owner)
{
  if (owner) gt4hip_list_free ((gt4hip_list *) owner);
}

int gt4hip_table_alloc (gt4hip_context *ctx, gt4hip_count_table *table, uint64_t n, uint32_t n_lists)
{
  int rc = gt4hip_block_alloc (ctx, (size_t) n * 8, &table->device_keys, &table->owner[0]);
  if (!rc) rc = gt4hip_block_alloc (ctx, (size_t) n * n_lists * 4, &table->device_counts, &table->owner[1]);
  if (rc) {
    gt4hip_table_free (table);
    return gt4hip_fail (ctx, GT4HIP_ENOMEM, "count table allocation failed (%llu keys x %u lists)", (unsigned long long) n, n_lists);
  }
  return GT4HIP_OK;
}

/* ---- ragged tables (see gt4hip_count_table in include/gt4hip.h) */
namespace {
struct TableRagged {
  uint64_t tiles;
  unsigned long long *compact, *padded; /* device, tiles + 1 entries each, one block */
  void *owner;
};

/* rows [first, first + count) of a ragged table, gathered: one thread per row finds its tile (the last one whose
 * compact base is not beyond the row) and copies the row from where the tile's rows lie */
__global__ void k_table_gather (const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, uint32_t n_lists,
                                const unsigned long long *__restrict__ compact, const unsigned long long *__restrict__ padded, uint64_t tiles,
                                uint64_t first, uint64_t count, unsigned long long *__restrict__ out_keys, uint32_t *__restrict__ out_counts)
{
  const uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t r = first + i;
  uint64_t lo = 0, hi = tiles; /* compact[lo] <= r < compact[hi] (compact[tiles] = n_keys) */
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (compact[mid] <= r) lo = mid;
    else hi = mid;
  }
  const uint64_t src = padded[lo] + (r - compact[lo]);
  if (out_keys) out_keys[i] = keys[src];
  if (out_counts)
    for (uint32_t j = 0; j < n_lists; j++) out_counts[i * n_lists + j] = counts[src * n_lists + j];
}
}  // namespace

int gt4hip_table_set_ragged (gt4hip_context *ctx, gt4hip_count_table *table, uint64_t tiles)
{
  TableRagged *r = new (std::nothrow) TableRagged ();
  if (!r) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  void *dev = NULL;
  if (gt4hip_block_alloc (ctx, (size_t) (tiles + 1) * 16, &dev, &r->owner)) {
    delete r;
    return gt4hip_fail (ctx, GT4HIP_ENOMEM, "count table index of %llu tiles", (unsigned long long) tiles);
  }
  r->tiles = tiles;
  r->compact = (unsigned long long *) dev;
  r->padded = r->compact + tiles + 1;
  table->ragged = r;
  return GT4HIP_OK;
}

void *gt4hip_table_compact_bases (gt4hip_count_table *table) { return table && table->ragged ? ((TableRagged *) table->ragged)->compact : NULL; }
void *gt4hip_table_padded_bases (gt4hip_count_table *table) { return table && table->ragged ? ((TableRagged *) table->ragged)->padded : NULL; }
uint64_t gt4hip_table_ragged_tiles (const gt4hip_count_table *table) { return table && table->ragged ? ((const TableRagged *) table->ragged)->tiles : 0; }

static hipError_t table_gather (gt4hip_context *ctx, const gt4hip_count_table *t, uint64_t first, uint64_t count, void *out_keys, void *out_counts)
{
  const TableRagged *r = (const TableRagged *) t->ragged;
  hipLaunchKernelGGL (k_table_gather, dim3 ((unsigned) ((count + 255) / 256)), dim3 (256), 0, ctx->stream, (const unsigned long long *) t->device_keys,
                      (const uint32_t *) t->device_counts, t->n_lists, r->compact, r->padded, r->tiles, first, count, (unsigned long long *) out_keys, (uint32_t *) out_counts);
  return hipGetLastError ();
}

extern "C" int gt4hip_table_compact (gt4hip_context *ctx, gt4hip_count_table *t)
{
  if (!ctx || !t) return GT4HIP_EINVAL;
  if (!t->ragged) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_count_table c;
  memset (&c, 0, sizeof c);
  c.n_keys = t->n_keys;
  c.n_lists = t->n_lists;
  if (t->n_keys) {
    const int rc = gt4hip_table_alloc (ctx, &c, t->n_keys, t->n_lists);
    if (rc) return rc;
    /* (at most 2^31 blocks of 256 rows per launch) */
    for (uint64_t first = 0; first < t->n_keys; first += 1ull << 32) {
      const uint64_t cnt = t->n_keys - first < (1ull << 32) ? t->n_keys - first : (1ull << 32);
      const hipError_t e = table_gather (ctx, t, first, cnt, (char *) c.device_keys + first * 8, (char *) c.device_counts + first * t->n_lists * 4);
      if (e != hipSuccess) {
        gt4hip_table_free (&c);
        return gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_table_compact: %s", hipGetErrorString (e));
      }
    }
    HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  }
  gt4hip_table_free (t);
  *t = c;
  return GT4HIP_OK;
}

/* A column of the table is itself a MERGE: with K the table's key list (every key of list j is in
 * K), union (K, L_j) under rule SECOND, every key kept, is K's keys with L_j's count or 0 -- a list
 * aligned with K, whose count column is copied into the table.  One streaming pass over K and L_j
 * per list instead of a binary search over L_j per key. */
static int table_column_by_union (gt4hip_context *ctx, const gt4hip_list *keys, const gt4hip_list *lj, gt4hip_list *tmp, gt4hip_count_table *t,
                                  uint32_t column)
{
  PairParams p = gt4hip_nway_params (GT4HIP_OP_UNION, GT4HIP_RULE_SECOND, 0, 0, FILTER_RAW);
  uint32_t *dst[4] = { (uint32_t *) tmp->dev, NULL, NULL, NULL };
  PairRun run;
  int rc = gt4hip_run_pair (ctx, (const uint32_t *) keys->dev, keys->n_words, (const uint32_t *) lj->dev, lj->n_words, p, false, dst, &run);
  if (rc) return rc;
  if (run.n_words[0] != keys->n_words) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "count table: a list holds keys outside the key list");
  HIPCHK (ctx, launch_extract_column (ctx->stream, ctx->grid_limit, (const uint32_t *) tmp->dev, keys->n_words, (uint32_t *) t->device_counts, t->n_lists, column));
  return GT4HIP_OK;
}

/* The lists one launch of the tile kernel builds a table from: the non-empty ones (the first `keep` lists even when
 * empty) -> work[], their columns -> cols[], *k of them.  false: more than `width` of them, or a word length other than
 * lists[0]'s -- the launch does not apply. */
static bool table_gather_lists (const gt4hip_list *const lists[], uint32_t n_lists, uint32_t keep, uint32_t width, const gt4hip_list *work[32],
                                uint32_t cols[32], uint32_t *k)
{
  *k = 0;
  for (uint32_t j = 0; j < n_lists; j++) {
    if (j >= keep && !lists[j]->n_words) continue;
    if (*k == width || lists[j]->word_length != lists[0]->word_length) return false;
    work[*k] = lists[j];
    cols[(*k)++] = j;
  }
  return true;
}

extern "C" int gt4hip_union_table (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, gt4hip_count_table *table)
{
  if (!ctx || !lists || !n_lists || !table) return GT4HIP_EINVAL;
  const auto t_begin = std::chrono::steady_clock::now ();
  struct Stamp { /* wall time of the whole call (several launches and read-backs), for bench.py --workload table */
    gt4hip_context *c;
    std::chrono::steady_clock::time_point t0;
    ~Stamp () { c->table_ms = std::chrono::duration<double, std::milli> (std::chrono::steady_clock::now () - t0).count (); }
  } stamp = { ctx, t_begin };
  memset (table, 0, sizeof *table);
  table->n_lists = n_lists;
  for (uint32_t j = 0; j < n_lists; j++)
    if (!lists[j]) return GT4HIP_EINVAL;
  /* up to 32 non-empty lists (eight with option "kway_max" = 8): ONE launch of the N-way tile kernel writes keys and counts
   * directly, every tile's rows where its records start (a ragged table: one row slot per input RECORD, up to n_lists
   * times the distinct keys) */
  const uint32_t table_width = ctx->kway_max == 8 ? 8u : 32u;
  if (ctx->kway_enabled) {
    const gt4hip_list *work[32];
    uint32_t cols[32], k;
    if (table_gather_lists (lists, n_lists, 0, table_width, work, cols, &k) && k >= 2) {
      HIPCHK (ctx, hipSetDevice (ctx->device));
      int used = 0;
      const int rc = gt4hip_nway_table (ctx, work, k, cols, table, 0, 0, &used);
      /* the ragged table did not fit: the path below needs one row per DISTINCT key only */
      if (rc && rc != GT4HIP_ENOMEM) return rc;
      if (rc == GT4HIP_ENOMEM) {
        used = 0;
        ctx->err[0] = 0;
      }
      if (used) {
        ctx->kway_calls++;
        return GT4HIP_OK;
      }
      memset (table, 0, sizeof *table);
      table->n_lists = n_lists;
    }
  }
  /* otherwise: all distinct keys ascending = N-way union with nothing filtered out (count >= 0), then a merge per column */
  gt4hip_multi_result u;
  memset (&u, 0, sizeof u);
  int rc = gt4hip_union_multi (ctx, lists, n_lists, 0, GT4HIP_RULE_MAX, 0, 0, &u);
  if (rc) return rc;
  const uint64_t n = u.n_words;
  table->n_keys = n;
  if (!n) {
    gt4hip_list_free (u.out);
    return GT4HIP_OK;
  }
  uint64_t longest = 0;
  for (uint32_t j = 0; j < n_lists; j++)
    if (lists[j]->n_words > longest) longest = lists[j]->n_words;
  gt4hip_list *tmp = NULL;
  rc = gt4hip_table_alloc (ctx, table, n, n_lists);
  if (!rc) rc = gt4hip_list_new (ctx, n + longest, lists[0]->word_length, &tmp);
  if (!rc) {
    hipError_t e = launch_extract_keys (ctx->stream, ctx->grid_limit, (const uint32_t *) u.out->dev, n, (unsigned long long *) table->device_keys);
    if (e != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "count table kernels failed: %s", hipGetErrorString (e));
  }
  for (uint32_t j = 0; j < n_lists && !rc; j++) rc = table_column_by_union (ctx, u.out, lists[j], tmp, table, j);
  if (!rc && hipStreamSynchronize (ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "count table kernels failed");
  if (tmp) gt4hip_list_free (tmp);
  gt4hip_list_free (u.out);
  if (rc) gt4hip_table_free (table);
  return rc;
}

int gt4hip_union_table_checked (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, gt4hip_count_table *table)
{
  for (uint32_t j = 0; j < n_lists; j++) {
    if (!lists[j]) return GT4HIP_EINVAL;
    if (lists[j]->word_length != lists[0]->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ");
  }
  return gt4hip_union_table (ctx, lists, n_lists, table);
}

/* keys = the keys of lists[0]; column j = the count of each of them in list j (0 when absent), or,
 * with `presence`, 1 when list j holds the key and 0 when it does not (a count may be 0 itself).
 * Two merges per list: lists[0] n L_j keeping L_j's count, then aligned with lists[0] as above. */
extern "C" int gt4hip_probe_table_ex (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, int presence, gt4hip_count_table *table)
{
  if (!ctx || !lists || !n_lists || !table || !lists[0]) return GT4HIP_EINVAL;
  for (uint32_t j = 0; j < n_lists; j++)
    if (!lists[j]) return GT4HIP_EINVAL;
  memset (table, 0, sizeof *table);
  table->n_lists = n_lists;
  const gt4hip_list *base = lists[0];
  const uint64_t n = base->n_words;
  table->n_keys = n;
  if (!n) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  /* up to 32 non-empty lists (the base first; eight with option "kway_max" = 8): one launch of the N-way tile kernel */
  if (ctx->kway_enabled) {
    const uint32_t table_width = ctx->kway_max == 8 ? 8u : 32u;
    const gt4hip_list *work[32];
    uint32_t cols[32], k;
    if (table_gather_lists (lists, n_lists, 1 /* the base, lists[0], even when empty */, table_width, work, cols, &k) && k >= 2) {
      int used = 0;
      const int rc = gt4hip_nway_table (ctx, work, k, cols, table, 1, presence, &used);
      if (rc) return rc;
      if (used) {
        ctx->kway_calls++;
        return GT4HIP_OK;
      }
      memset (table, 0, sizeof *table);
      table->n_lists = n_lists;
      table->n_keys = n;
    }
  }
  gt4hip_list *tmp = NULL, *inter = NULL;
  int rc = gt4hip_table_alloc (ctx, table, n, n_lists);
  if (!rc) rc = gt4hip_list_new (ctx, 2 * n, base->word_length, &tmp);
  if (!rc) rc = gt4hip_list_new (ctx, n, base->word_length, &inter);
  if (!rc) {
    hipError_t e = launch_extract_keys (ctx->stream, ctx->grid_limit, (const uint32_t *) base->dev, n, (unsigned long long *) table->device_keys);
    if (e != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "count table kernels failed: %s", hipGetErrorString (e));
  }
  for (uint32_t j = 0; j < n_lists && !rc; j++) {
    PairParams p = gt4hip_nway_params (GT4HIP_OP_INTRSEC, presence ? GT4HIP_RULE_NUMBER : GT4HIP_RULE_SECOND, 0, 1, FILTER_RAW);
    uint32_t *dst[4] = { NULL, (uint32_t *) inter->dev, NULL, NULL };
    PairRun run;
    rc = gt4hip_run_pair (ctx, (const uint32_t *) base->dev, n, (const uint32_t *) lists[j]->dev, lists[j]->n_words, p, false, dst, &run);
    if (rc) break;
    inter->n_words = run.n_words[1];
    rc = table_column_by_union (ctx, base, inter, tmp, table, j);
  }
  if (!rc && hipStreamSynchronize (ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "count table kernels failed");
  if (tmp) gt4hip_list_free (tmp);
  if (inter) gt4hip_list_free (inter);
  if (rc) gt4hip_table_free (table);
  return rc;
}

extern "C" int gt4hip_probe_table (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, gt4hip_count_table *table)
{
  return gt4hip_probe_table_ex (ctx, lists, n_lists, 0, table);
}

extern "C" int gt4hip_table_download (gt4hip_context *ctx, const gt4hip_count_table *t, uint64_t first, uint64_t count,
                                       uint64_t *host_keys, uint32_t *host_counts)
{
  if (!ctx || !t || first > t->n_keys || count > t->n_keys - first) return GT4HIP_EINVAL;
  if (!count) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (t->ragged) {
    /* gathered into a staging block on the device, then copied */
    TempBlocks blk;
    char *tmp = NULL;
    const size_t kb = (size_t) count * 8, cb = (size_t) count * t->n_lists * 4;
    if (blk.get (ctx, kb + cb, (void **) &tmp)) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_table_download: %zu bytes of staging", kb + cb);
    hipError_t e = table_gather (ctx, t, first, count, host_keys ? tmp : NULL, host_counts ? tmp + kb : NULL);
    if (e == hipSuccess && host_keys) e = hipMemcpyAsync (host_keys, tmp, kb, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && host_counts) e = hipMemcpyAsync (host_counts, tmp + kb, cb, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize (ctx->stream);
    if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_table_download: %s", hipGetErrorString (e));
    return GT4HIP_OK;
  }
  if (host_keys) HIPCHK (ctx, hipMemcpyAsync (host_keys, (const char *) t->device_keys + first * 8, (size_t) count * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (host_counts)
    HIPCHK (ctx, hipMemcpyAsync (host_counts, (const char *) t->device_counts + first * t->n_lists * 4, (size_t) count * t->n_lists * 4,
                                 hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

extern "C" void gt4hip_table_free (gt4hip_count_table *t)
{
  if (!t) return;
  if (t->owner[0]) gt4hip_block_free (t->owner[0]);
  else if (t->device_keys) hipFree (t->device_keys);
  if (t->owner[1]) gt4hip_block_free (t->owner[1]);
  else if (t->device_counts) hipFree (t->device_counts);
  if (t->ragged) {
    TableRagged *r = (TableRagged *) t->ragged;
    if (r->owner) gt4hip_block_free (r->owner);
    delete r;
  }
  t->ragged = NULL;
  t->device_keys = t->device_counts = NULL;
  t->owner[0] = t->owner[1] = NULL;
  t->n_keys = 0;
}
