/* gt4hip_gmer.hip -- gmer_counter on the device, gfx950, wave64: how often the reads contain every k-mer of a database
 * (reference src/gmer_counter.c:751-815, src/database.c:94-282).
 *
 * The reference keeps the database's words in a trie and looks every word of the reads up in it; a hit carries
 * (node + 1) << kmer_bits | kmer, which leads to a 16- or 32-bit counter.  Here the database is what the lookups of
 * gt4hip_query.hip already probe: the canonical words sorted into 12-byte list records -- the k-mer's index stands where a
 * list keeps its count -- under the bucket index of gt4hip_index.h, and one 64-bit counter per k-mer.
 *
 *   k_gmer_prepare  word i -> min (word, reverse complement), value i; words at or above 4^k are flagged
 *   (gt4hip_sort_pairs: stable, so equal words keep the order of their indices)
 *   k_gmer_pack     sorted (word, index) -> record; two equal neighbours: the smallest such place (atomicMin)
 *   k_index_build   (gt4hip_index.h)
 *   k_gmer_count    the hot kernel: a grid-stride loop over the reads' words, one find () each; a hit is one no-return
 *                   64-bit atomic on its counter.  Nearly every probe misses (3e7 k-mers against 1e11 words), so the
 *                   loop is the index's two dependent loads and a short bisection.  A wavefront whose hits ALL fall on
 *                   one k-mer -- 64 consecutive words of a poly-A read -- adds their number with one atomic instead of
 *                   serialising 64 on one address (one ballot and one readlane in wavefronts that have a hit; measured
 *                   both ways, profiles/gmer/README.md); GT4HIP_GMER_PLAIN_ATOMICS leaves every hit its own.  The hits and the
 *                   n_kmer_gc term are summed per lane over the whole loop and reduced once: one atomic each per
 *                   wavefront and launch.
 *
 * gt4hip_gmer_count_text is gt4hip_text_to_words on a piece and k_gmer_count on the context's word buffer: the words never
 * reach the host.  The --stats counts of the text are k_mk_text_counts below, launched by the reader (gt4hip_maker.hip) on the
 * arrays it has just filled, with the reader's own classification (gt4hip_maker_tile.h). */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"
#include "gt4hip_maker_tile.h"

#include <string.h>

namespace gt4 {
namespace {

__global__ __launch_bounds__ (MM_THREADS) void k_gmer_prepare (u64 *__restrict__ words, u64 *__restrict__ values, u64 n, u32 k, u32 *bad)
{
  bool wrong = false;
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) {
    const u64 w = words[i];
    wrong |= k < 32 && (w >> (2 * k)) != 0;
    words[i] = canonical (w, k, 1);
    values[i] = i;
  }
  if (__builtin_amdgcn_ballot_w64 (wrong) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr (bad, 1u);
}

/* *dup = the smallest i with words[i - 1] == words[i] (preset to ~0) */
__global__ __launch_bounds__ (MM_THREADS) void k_gmer_pack (const u64 *__restrict__ words, const u64 *__restrict__ values, u64 n, u32 *__restrict__ rec,
                                                            unsigned long long *dup)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) {
    const u64 w = words[i];
    if (i && words[i - 1] == w) atomicMin (dup, (unsigned long long) i);
    rec[3 * i] = (u32) w;
    rec[3 * i + 1] = (u32) (w >> 32);
    rec[3 * i + 2] = (u32) values[i];
  }
}

/* counters[index of w] += 1 for every word w found; totals[0] += hits, totals[1] += sum over the hits of (w ^ w >> 1) & 1 */
template <bool COMBINE>
__global__ __launch_bounds__ (MM_THREADS) void k_gmer_count (const u64 *__restrict__ words, u64 n, Index ix, unsigned long long *counters,
                                                             unsigned long long *totals)
{
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 gtid = (u64) blockIdx.x * MM_THREADS + threadIdx.x;
  const u64 stride = (u64) gridDim.x * MM_THREADS;
  u64 hits = 0, gc = 0;
  for (u64 g0 = gtid - lane; g0 < n; g0 += stride) { /* wavefront-uniform */
    const u64 i = g0 + lane;
    u64 j = ~0ull, w = 0;
    if (i < n) {
      w = words[i];
      j = find (ix, w);
    }
    const bool hit = j != ~0ull;
    u32 idx = 0;
    if (hit) {
      idx = ix.rec[3 * j + 2];
      hits++;
      gc += (w ^ (w >> 1)) & 1;
    }
    if (COMBINE) {
      const u64 m = __builtin_amdgcn_ballot_w64 (hit);
      if (m) {
        const int first = __builtin_ctzll (m);
        const u32 idx0 = (u32) __builtin_amdgcn_readlane ((int) idx, first);
        if (__builtin_amdgcn_ballot_w64 (hit && idx != idx0) == 0) {
          if (lane == first) atomicAdd (&counters[idx0], (unsigned long long) __popcll (m));
        } else if (hit) {
          atomicAdd (&counters[idx], 1ull);
        }
      }
    } else if (hit) {
      atomicAdd (&counters[idx], 1ull);
    }
  }
  hits = wave_sum (hits);
  gc = wave_sum (gc);
  if (lane == 0) {
    if (hits) atomicAdd (&totals[0], (unsigned long long) hits);
    if (gc) atomicAdd (&totals[1], (unsigned long long) gc);
  }
}

/* gmer_counter --stats (gt4hip_text_to_words_counted), launched by the reader behind its k_mk_codes: out[0] += 'N' / 'n' among the bytes in front of the
 * NUL -- FastQ: but those of '+' lines (lines so far mod 4 == 2), which the reference's reader takes without its
 * read_character callback (src/fasta.c:200-216) --, out[1] += codes 0..3, out[2] += codes 1 and 2 (C, G).  A thread takes
 * 16 bytes of text and the 16 codes of the same number: there are no more codes than bytes.  `codes` as in k_mk_codes. */
template <bool FASTQ>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_text_counts (const unsigned char *__restrict__ text, u64 n, u64 n_tiles, const u32 *tile_state,
                                                                 const unsigned char *__restrict__ codes, const MakerInfo *info, unsigned long long *out)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE], s_has[MK_THREADS / WAVE], s_tail[MK_THREADS / WAVE];
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n, n_codes = info->n_codes;
  u32 c_n = 0, c_nucl = 0, c_gc = 0;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (t * MK_TILE >= n_eff) break; /* (uniform, as in k_mk_codes) */
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[4];
    if (FASTQ) {
      const TileHead h = tile_head (text, n_eff, off, tile_state + t, s_sum, s_has, s_tail);
      u32 phase = h.phase;
#pragma unroll
      for (int j = 0; j < MK_PER; j++) {
        const u32 c = MK_BYTE (h.w, j); /* 0 at n_eff and behind */
        c_n += phase != 2u && (c | 0x20u) == 'n';
        if (c == '\n') phase = (phase + 1u) & 3u;
      }
      __syncthreads ();
    } else {
      load16 (text, n_eff, off, w);
#pragma unroll
      for (int j = 0; j < MK_PER; j++) c_n += (MK_BYTE (w, j) | 0x20u) == 'n';
    }
    if (off < n_codes) {
      load16 (codes, n_codes, off, w);
#pragma unroll
      for (int j = 0; j < MK_PER; j++) {
        const u32 c = off + j < n_codes ? MK_BYTE (w, j) : 4u;
        c_nucl += c < 4u;
        c_gc += c == 1u || c == 2u;
      }
    }
  }
  c_n = dpp_wave_sum_u32 (c_n), c_nucl = dpp_wave_sum_u32 (c_nucl), c_gc = dpp_wave_sum_u32 (c_gc);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (c_n) atomicAdd (&out[0], (unsigned long long) c_n);
    if (c_nucl) atomicAdd (&out[1], (unsigned long long) c_nucl);
    if (c_gc) atomicAdd (&out[2], (unsigned long long) c_gc);
  }
}

}  // namespace
}  // namespace gt4

using namespace gt4;

void gt4hip_launch_text_counts (hipStream_t stream, int grid, bool fastq, const unsigned char *d_text, size_t n_bytes, uint64_t tiles, const uint32_t *tile_state,
                                const unsigned char *codes, const void *info, unsigned long long *out)
{
  if (fastq) hipLaunchKernelGGL (k_mk_text_counts<true>, dim3 (grid), dim3 (MK_THREADS), 0, stream, d_text, (u64) n_bytes, (u64) tiles, tile_state, codes, (const MakerInfo *) info, out);
  else hipLaunchKernelGGL (k_mk_text_counts<false>, dim3 (grid), dim3 (MK_THREADS), 0, stream, d_text, (u64) n_bytes, (u64) tiles, tile_state, codes, (const MakerInfo *) info, out);
}

struct gt4hip_gmer_db {
  gt4hip_context *ctx;
  gt4hip_list *list;     /* n records: canonical word, index of the k-mer */
  Index ix;
  void *off_owner;
  unsigned long long *counters;
  void *counters_owner;
  u64 n;
  u32 k;
  double last_ms;
};

extern "C" void gt4hip_gmer_db_free (gt4hip_gmer_db *db)
{
  if (!db) return;
  gt4hip_block_free (db->off_owner);
  gt4hip_block_free (db->counters_owner);
  gt4hip_list_free (db->list);
  delete db;
}

extern "C" uint64_t gt4hip_gmer_db_n_kmers (const gt4hip_gmer_db *db) { return db ? db->n : 0; }
extern "C" double gt4hip_gmer_db_last_ms (const gt4hip_gmer_db *db) { return db ? db->last_ms : 0.0; }

extern "C" int gt4hip_gmer_db_create (gt4hip_context *ctx, const uint64_t *host_words, uint64_t n, uint32_t word_length, gt4hip_gmer_db **out)
{
  if (!ctx || !out || (n && !host_words)) return GT4HIP_EINVAL;
  *out = NULL;
  const u32 k = word_length;
  if (k < 1 || k > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_db_create: word length %u", k);
  if (n >= (1ull << 32)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_db_create: %llu k-mers: a record holds the index in 32 bits", (unsigned long long) n);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_gmer_db *db = new (std::nothrow) gt4hip_gmer_db ();
  if (!db) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  db->ctx = ctx;
  db->n = n;
  db->k = k;
  db->last_ms = 0;
  TempBlocks blk;
  u64 *d_words = NULL, *d_values = NULL;
  u32 *bad = (u32 *) ctx->scratch;           /* word 0 */
  unsigned long long *dup = ctx->scratch + 1; /* word 1 */
  int rc = gt4hip_list_new (ctx, n, k, &db->list);
  if (!rc) rc = gt4hip_block_alloc (ctx, n ? n * 8 : 16, (void **) &db->counters, &db->counters_owner);
  if (!rc) rc = blk.get (ctx, n * 8, (void **) &d_words);
  if (!rc) rc = blk.get (ctx, n * 8, (void **) &d_values);
  if (!rc && hipMemsetAsync (db->counters, 0, n ? n * 8 : 16, ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: hipMemsetAsync failed");
  if (!rc && n) {
    rc = gt4hip_io_upload (ctx, host_words, d_words, n * 8);
    if (!rc && hipMemsetAsync (ctx->scratch, 0, 8, ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: hipMemsetAsync failed");
    if (!rc) {
      hipLaunchKernelGGL (k_gmer_prepare, dim3 (gt4hip_grid (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, d_words, d_values, n, k, bad);
      if (hipGetLastError () != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: canonicalising the words failed");
    }
    if (!rc) rc = gt4hip_read_scratch (ctx, 1);
    if (!rc && (u32) ctx->scratch_host[0]) rc = gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_db_create: a word does not fit %u bases", k);
    if (!rc) rc = gt4hip_sort_pairs (ctx, d_words, d_values, n, k);
    if (!rc && hipMemsetAsync (dup, 0xff, 8, ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: hipMemsetAsync failed");
    if (!rc) {
      hipLaunchKernelGGL (k_gmer_pack, dim3 (gt4hip_grid (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, (const u64 *) d_words, (const u64 *) d_values, n,
                          (u32 *) db->list->dev, dup);
      if (hipGetLastError () != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: packing the words failed");
    }
    if (!rc) rc = gt4hip_read_scratch (ctx, 2);
    if (!rc && ctx->scratch_host[1] != ~0ull) {
      const u64 at = ctx->scratch_host[1];
      u64 pair[2] = { 0, 0 };
      rc = gt4hip_read_back (ctx, pair, d_values + at - 1, 16, "gt4hip_gmer_db_create: reading the duplicate back failed");
      if (!rc) rc = gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_db_create: k-mers %llu and %llu are the same canonical word", (unsigned long long) pair[0], (unsigned long long) pair[1]);
    }
  }
  if (!rc) {
    size_index (db->list, &db->ix);
    void *off = NULL;
    rc = gt4hip_block_alloc (ctx, (db->ix.nb + 1) * 8, &off, &db->off_owner);
    if (!rc) rc = fill_index (ctx, &db->ix, off);
    if (!rc && hipStreamSynchronize (ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_gmer_db_create: building the index failed");
  }
  if (rc) {
    gt4hip_gmer_db_free (db);
    return rc;
  }
  *out = db;
  return GT4HIP_OK;
}

namespace {

/* k_gmer_count on n device words; totals[0..1] of the launch -> tot */
int count_device_words (gt4hip_context *ctx, gt4hip_gmer_db *db, const u64 *d_words, u64 n, unsigned flags, u64 tot[2])
{
  tot[0] = tot[1] = 0;
  db->last_ms = 0;
  if (!n) return GT4HIP_OK;
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 16, ctx->stream));
  const int grid = gt4hip_grid (ctx, n, MM_THREADS);
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], ctx->stream));
  if (flags & GT4HIP_GMER_PLAIN_ATOMICS) hipLaunchKernelGGL (k_gmer_count<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, d_words, n, db->ix, db->counters, ctx->scratch);
  else hipLaunchKernelGGL (k_gmer_count<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, d_words, n, db->ix, db->counters, ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], ctx->stream));
  const int rc = gt4hip_read_scratch (ctx, 2);
  if (rc) return rc;
  float ms = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) db->last_ms = ms;
  tot[0] = ctx->scratch_host[0];
  tot[1] = ctx->scratch_host[1];
  return GT4HIP_OK;
}

}  // namespace

extern "C" int gt4hip_gmer_count_words (gt4hip_context *ctx, gt4hip_gmer_db *db, const uint64_t *words, uint64_t n, unsigned flags, uint64_t *n_hits,
                                        uint64_t *kmer_gc)
{
  if (!ctx || !db || db->ctx != ctx || (n && !words) || (flags & ~(unsigned) (GT4HIP_GMER_ON_DEVICE | GT4HIP_GMER_PLAIN_ATOMICS))) return GT4HIP_EINVAL;
  if (n_hits) *n_hits = 0;
  if (kmer_gc) *kmer_gc = 0;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!n) return GT4HIP_OK;
  TempBlocks blk;
  const u64 *d_words = (const u64 *) words;
  if (!(flags & GT4HIP_GMER_ON_DEVICE)) {
    u64 *d = NULL;
    int rc = blk.get (ctx, n * 8, (void **) &d);
    if (!rc) rc = gt4hip_io_upload (ctx, words, d, n * 8);
    if (rc) return rc;
    d_words = d;
  } else if ((size_t) words & 7) {
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_count_words: device words must be 8-byte aligned");
  }
  u64 tot[2];
  const int rc = count_device_words (ctx, db, d_words, n, flags, tot);
  if (rc) return rc;
  if (n_hits) *n_hits = tot[0];
  if (kmer_gc) *kmer_gc = tot[1];
  return GT4HIP_OK;
}

extern "C" int gt4hip_gmer_count_text (gt4hip_context *ctx, gt4hip_gmer_db *db, const void *text, size_t n_bytes, unsigned flags, const gt4hip_maker_carry *in,
                                       gt4hip_maker_carry *out, gt4hip_gmer_stats *stats, uint64_t *error_offset)
{
  if (!ctx || !db || db->ctx != ctx || (flags & ~(unsigned) (GT4HIP_GMER_ON_DEVICE | GT4HIP_GMER_PLAIN_ATOMICS))) return GT4HIP_EINVAL;
  if (stats) memset (stats, 0, sizeof *stats);
  uint64_t *d_words = NULL, n_words = 0, counts[3] = { 0, 0, 0 };
  int rc = gt4hip_text_to_words_counted (ctx, text, n_bytes, db->k, flags & GT4HIP_GMER_ON_DEVICE ? GT4HIP_MAKER_TEXT_ON_DEVICE : 0, in, out, &d_words, &n_words,
                                         error_offset, stats ? counts : NULL);
  if (rc) return rc;
  u64 tot[2];
  rc = count_device_words (ctx, db, (const u64 *) d_words, n_words, flags, tot);
  gt4hip_words_free (ctx, d_words);
  if (rc) return rc;
  if (stats) {
    stats->n_n = counts[0], stats->n_nucl = counts[1], stats->n_gc = counts[2];
    stats->n_words = n_words, stats->n_hits = tot[0], stats->n_kmer_gc = tot[1] * db->k;
  }
  return GT4HIP_OK;
}

extern "C" int gt4hip_gmer_counts_download (gt4hip_context *ctx, const gt4hip_gmer_db *db, uint64_t first, uint64_t n, uint64_t *host_counts)
{
  if (!ctx || !db || db->ctx != ctx || (n && !host_counts)) return GT4HIP_EINVAL;
  if (first > db->n || n > db->n - first) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_gmer_counts_download: [%llu, +%llu) of %llu counters", (unsigned long long) first, (unsigned long long) n, (unsigned long long) db->n);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!n) return GT4HIP_OK;
  return gt4hip_read_back (ctx, host_counts, db->counters + first, (size_t) n * 8, "gt4hip_gmer_counts_download failed");
}

extern "C" int gt4hip_gmer_counts_reset (gt4hip_context *ctx, gt4hip_gmer_db *db)
{
  if (!ctx || !db || db->ctx != ctx) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  HIPCHK (ctx, hipMemsetAsync (db->counters, 0, db->n ? db->n * 8 : 16, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}
