/*
 * gt4hip_select.hip -- glistcompare -u --min_lists M --max_lists X: the records of an N-way union whose word lies in M to X
 * of the N lists.  gt4hip_table_select reads a per-key count table as gt4hip_union_table leaves it, ragged or
 * contiguous, and writes the selected list; gt4hip_select_multi builds the table and hands it over.
 *
 * The table is walked in SEGMENTS of consecutive rows (gt4hip_table_walk.h: SelTable, segment_of, shared with gt4hip_pairwise.hip): the rows of one tile of the N-way tile kernel in a ragged table (they
 * lie together where the tile's records start, so no row is searched for), GT4HIP_SELECT_SEGMENT rows in a contiguous one.
 * Three kernels live here:
 *   k_select_decide<G, MAXR, VEC>  one group of G lanes per row, consecutive lanes on consecutive dwords of the row (VEC 1:
 *                             G = min (64, next power of two >= n_lists)) or, where a row is a multiple of four counts, on
 *                             consecutive 16-byte pieces (VEC 4: a quarter of the lanes), a loop over the columns beyond the
 *                             group, four rows of a group in flight; a DPP reduction inside the group gives p (columns that are not 0) and the folded count
 *                             (the union's arithmetic: a 32-bit sum that wraps, or the maximum; rule NUMBER: the override);
 *                             keep = M <= p <= X and count >= cutoff.  Writes the folded count and the decision per row, and
 *                             per segment the kept rows and the 64-bit sum of their counts (one wavefront reduction each, no
 *                             atomic: nothing has to be zeroed)
 *   k_select_scan             one workgroup: where every segment's records start in the output, and the two totals
 *   k_select_emit             a thread per row, GT4HIP_SELECT_TILE rows at a time: the kept rows ranked in order (ballots),
 *                             packed into 12-byte records in LDS and written as 16-byte stores (write_out_tile)
 * --count_only stops behind the scan.  No word of the workspace is read before the same call has written it.
 */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_table_walk.h"

#include <string.h>

namespace gt4 {
namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / WAVE;
constexpr u32 SEL_TILE = GT4HIP_SELECT_TILE;
constexpr int SEL_RPT = (int) (SEL_TILE / SEL_THREADS); /* rows per thread and tile of the emit kernel */
constexpr int SEL_UNR = 4;                              /* rows a lane group has in flight */
static_assert (SEL_TILE % SEL_THREADS == 0, "whole rounds of one row per thread");

struct SelRule {
  u32 min_lists, max_lists, cutoff;
  u32 number, count_override; /* rule NUMBER: every kept record carries the override */
};

/* sum / maximum over the G lanes of a group, in every lane of it: DPP inside a row of 16 lanes (quad permutes, then the two
 * mirrors: after the quads hold their sums, lane i and lane 7 - i lie in different quads, lane i and lane 15 - i in different
 * halves), the LDS crossbar for the steps across rows.  Every lane of the wavefront must be active. */
template <int G, bool MAXR>
__device__ __forceinline__ u32 group_fold (u32 v)
{
  auto op = [] (u32 a, u32 b) { return MAXR ? (a > b ? a : b) : a + b; };
  if (G >= 2) v = op (v, (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0xB1, 0xf, 0xf, false));  /* quad_perm [1,0,3,2] */
  if (G >= 4) v = op (v, (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0x4E, 0xf, 0xf, false));  /* quad_perm [2,3,0,1] */
  if (G >= 8) v = op (v, (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0x141, 0xf, 0xf, false)); /* row_half_mirror */
  if (G >= 16) v = op (v, (u32) __builtin_amdgcn_update_dpp (0, (int) v, 0x140, 0xf, 0xf, false)); /* row_mirror */
  if (G >= 32) v = op (v, (u32) __shfl_xor ((int) v, 16, WAVE));
  if (G >= 64) v = op (v, (u32) __shfl_xor ((int) v, 32, WAVE));
  return v;
}

template <int G, bool MAXR, int VEC>
__global__ __launch_bounds__ (SEL_THREADS) void k_select_decide (SelTable t, SelRule q, u32 *__restrict__ row_cnt, unsigned char *__restrict__ row_keep,
                                                                 u32 *__restrict__ seg_cnt, u64 *__restrict__ seg_sum)
{
  static_assert (VEC == 1 || VEC == 4, "a dword or 16 bytes per lane");
  constexpr u32 NG = SEL_THREADS / G; /* groups, = rows a workgroup reads per step and row in flight */
  typedef u32 vec_t __attribute__ ((ext_vector_type (VEC)));
  __shared__ u32 w_kept[SEL_WAVES];
  __shared__ u64 w_sum[SEL_WAVES];
  const u32 tid = threadIdx.x, grp = tid / G, j = tid % G;
  const u32 cols = t.n_lists / VEC; /* (VEC 4: the host launches it for rows of a multiple of four counts only) */
  for (u64 s = blockIdx.x; s < t.segments; s += gridDim.x) {
    u64 row_base, src_base;
    u32 rows;
    segment_of (t, s, row_base, src_base, rows);
    u32 kept = 0;
    u64 sum = 0;
    for (u32 base = 0; base < rows; base += NG * SEL_UNR) { /* (the bound is the workgroup's: every lane reaches the DPP steps) */
      const vec_t *rowp[SEL_UNR];
      bool valid[SEL_UNR];
      u32 p[SEL_UNR], f[SEL_UNR];
#pragma unroll
      for (int u = 0; u < SEL_UNR; u++) {
        const u32 i = base + (u32) u * NG + grp;
        valid[u] = i < rows;
        rowp[u] = reinterpret_cast<const vec_t *> (t.counts + (src_base + (valid[u] ? i : 0u)) * t.n_lists);
        p[u] = f[u] = 0;
      }
      for (u32 c0 = 0; c0 < cols; c0 += G) {
        const u32 c = c0 + j;
        vec_t v[SEL_UNR];
#pragma unroll
        for (int u = 0; u < SEL_UNR; u++) v[u] = valid[u] && c < cols ? __builtin_nontemporal_load (rowp[u] + c) : (vec_t) 0u;
#pragma unroll
        for (int u = 0; u < SEL_UNR; u++)
#pragma unroll
          for (int e = 0; e < VEC; e++) {
            const u32 w = v[u][e];
            p[u] += w != 0u;
            f[u] = MAXR ? (f[u] > w ? f[u] : w) : f[u] + w;
          }
      }
#pragma unroll
      for (int u = 0; u < SEL_UNR; u++) {
        const u32 pp = group_fold<G, false> (p[u]);
        u32 ff = group_fold<G, MAXR> (f[u]);
        if (q.number) ff = q.count_override;
        const bool keep = valid[u] && pp >= q.min_lists && pp <= q.max_lists && ff >= q.cutoff;
        if (j == 0 && valid[u]) {
          const u64 row = row_base + base + (u32) u * NG + grp;
          if (row_cnt) {
            row_cnt[row] = ff;
            row_keep[row] = keep ? 1 : 0;
          }
          kept += keep;
          sum += keep ? ff : 0u;
        }
      }
    }
    kept = dpp_wave_sum_u32 (kept);
    sum = wave_sum (sum);
    if ((tid & (WAVE - 1)) == 0) {
      w_kept[tid / WAVE] = kept;
      w_sum[tid / WAVE] = sum;
    }
    __syncthreads ();
    if (tid == 0) {
      u32 k = 0;
      u64 m = 0;
      for (int w = 0; w < SEL_WAVES; w++) {
        k += w_kept[w];
        m += w_sum[w];
      }
      seg_cnt[s] = k;
      seg_sum[s] = m;
    }
    __syncthreads ();
  }
}

/* exclusive scan of the segments' kept rows; totals[0] = all of them, totals[1] = the sum of their counts */
/* (workgroup_scan of gt4hip_device.h, open-coded with the sum of seg_sum in its loop: as a call with the sum in a loop of its own
 * behind it the select kernels measured 0.04 ms slower, profiles/HISTORY.md) */
__global__ __launch_bounds__ (1024) void k_select_scan (const u32 *__restrict__ seg_cnt, const u64 *__restrict__ seg_sum, u64 segments, u64 *__restrict__ seg_off,
                                                        u64 *__restrict__ totals)
{
  __shared__ u64 wsum[1024 / WAVE];
  __shared__ u64 carry;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads ();
  u64 counts = 0;
  for (u64 base = 0; base < segments; base += 1024) {
    const u64 i = base + threadIdx.x;
    const u64 v = i < segments ? seg_cnt[i] : 0;
    counts += i < segments ? seg_sum[i] : 0;
    const u64 incl = wave_inclusive_scan (v, lane);
    if (lane == WAVE - 1) wsum[wv] = incl;
    __syncthreads ();
    u64 before = carry;
    for (int w = 0; w < wv; w++) before += wsum[w];
    if (i < segments) seg_off[i] = before + incl - v;
    __syncthreads ();
    if (threadIdx.x == 1023) carry = before + incl;
    __syncthreads ();
  }
  counts = wave_sum (counts);
  if (lane == 0) wsum[wv] = counts;
  __syncthreads ();
  if (threadIdx.x == 0) {
    u64 c = 0;
    for (int w = 0; w < 1024 / WAVE; w++) c += wsum[w];
    totals[0] = carry;
    totals[1] = c;
  }
}

__global__ __launch_bounds__ (SEL_THREADS) void k_select_emit (SelTable t, const u32 *__restrict__ row_cnt, const unsigned char *__restrict__ row_keep,
                                                               const u32 *__restrict__ seg_cnt, const u64 *__restrict__ seg_off, u32 *__restrict__ out)
{
  __shared__ __attribute__ ((aligned (16))) u32 stage[3 * SEL_TILE + 4];
  __shared__ u32 wtot[SEL_RPT][SEL_WAVES];
  const u32 tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  for (u64 s = blockIdx.x; s < t.segments; s += gridDim.x) {
    if (!seg_cnt[s]) continue; /* (the workgroup's: nothing of this segment is kept) */
    u64 row_base, src_base;
    u32 rows;
    segment_of (t, s, row_base, src_base, rows);
    u64 off = seg_off[s];
    for (u32 sub = 0; sub < rows; sub += SEL_TILE) {
      bool k[SEL_RPT];
      u32 rank[SEL_RPT];
#pragma unroll
      for (int r = 0; r < SEL_RPT; r++) {
        const u32 i = sub + (u32) r * SEL_THREADS + tid;
        k[r] = i < rows && row_keep[row_base + (i < rows ? i : 0u)] != 0;
      }
#pragma unroll
      for (int r = 0; r < SEL_RPT; r++) {
        const u64 b = __builtin_amdgcn_ballot_w64 (k[r]);
        rank[r] = (u32) __popcll (b & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[r][wv] = (u32) __popcll (b);
      }
      __syncthreads ();
      u32 run = 0, pos[SEL_RPT] = {};
#pragma unroll
      for (int r = 0; r < SEL_RPT; r++)
#pragma unroll
        for (int w = 0; w < SEL_WAVES; w++) { /* (rounds in order, the wavefronts of a round in order: the rows' order) */
          if ((u32) w == wv) pos[r] = run + rank[r];
          run += wtot[r][w];
        }
      const u32 tot = uniform32 (run);
#pragma unroll
      for (int r = 0; r < SEL_RPT; r++) {
        if (!k[r]) continue;
        const u32 i = sub + (u32) r * SEL_THREADS + tid;
        const u64 key = t.keys[src_base + i];
        stage[3 * pos[r]] = (u32) key;
        stage[3 * pos[r] + 1] = (u32) (key >> 32);
        stage[3 * pos[r] + 2] = row_cnt[row_base + i];
      }
      __syncthreads ();
      write_out_tile<SEL_THREADS> (out, off, tot, stage, (int) tid);
      off += tot;
      __syncthreads (); /* the staging area and the wavefronts' totals are free again */
    }
  }
}

}  // namespace
}  // namespace gt4

using namespace gt4;

namespace {

template <int G, int VEC>
void launch_decide (bool maxr, dim3 grid, hipStream_t st, const SelTable &t, const SelRule &q, u32 *row_cnt, unsigned char *row_keep, u32 *seg_cnt, u64 *seg_sum)
{
  if (maxr) hipLaunchKernelGGL ((k_select_decide<G, true, VEC>), grid, dim3 (SEL_THREADS), 0, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else hipLaunchKernelGGL ((k_select_decide<G, false, VEC>), grid, dim3 (SEL_THREADS), 0, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
}

/* lanes per row: the next power of two that holds the row's loads (dwords, or 16-byte pieces), at least 2, at most a wavefront */
template <int VEC>
void launch_decide_width (bool maxr, dim3 grid, hipStream_t st, const SelTable &t, const SelRule &q, u32 *row_cnt, unsigned char *row_keep, u32 *seg_cnt, u64 *seg_sum)
{
  const u32 cols = t.n_lists / VEC;
  if (cols <= 2) launch_decide<2, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else if (cols <= 4) launch_decide<4, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else if (cols <= 8) launch_decide<8, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else if (cols <= 16) launch_decide<16, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else if (cols <= 32) launch_decide<32, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else launch_decide<64, VEC> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
}

int empty_selection (gt4hip_context *ctx, uint32_t word_length, bool count_only, gt4hip_multi_result *res)
{
  res->n_words = res->total_count = 0;
  if (count_only) {
    res->out = NULL;
    return GT4HIP_OK;
  }
  if (res->out) {
    res->out->n_words = 0;
    return GT4HIP_OK;
  }
  return gt4hip_list_new (ctx, 0, word_length, &res->out);
}

/* the rule of a union (src/glistcompare.c:518-523), resolved; GT4HIP_ERULE with the union's wording otherwise */
int union_rule (gt4hip_context *ctx, const char *who, int32_t *rule)
{
  if (*rule == GT4HIP_RULE_DEFAULT) *rule = GT4HIP_RULE_ADD;
  else if (*rule != GT4HIP_RULE_ADD && *rule != GT4HIP_RULE_MAX && *rule != GT4HIP_RULE_NUMBER)
    return gt4hip_fail (ctx, GT4HIP_ERULE, "%s: Invalid rule %u (only ADD, MAX and NUMBER allowed)", who, (unsigned) *rule);
  return GT4HIP_OK;
}

int check_bounds (gt4hip_context *ctx, const char *who, uint32_t min_lists, uint32_t max_lists, uint32_t n_lists)
{
  if (min_lists < 1 || max_lists < min_lists || max_lists > n_lists)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: min_lists %u, max_lists %u: 1 <= min_lists <= max_lists <= %u lists is needed", who, min_lists, max_lists, n_lists);
  return GT4HIP_OK;
}

int table_select (gt4hip_context *ctx, const gt4hip_count_table *table, uint32_t word_length, uint32_t min_lists, uint32_t max_lists, uint32_t cutoff,
                  int32_t rule, uint32_t ovr, bool count_only, gt4hip_multi_result *res)
{
  res->device_ms = 0;
  res->records_read = table->n_keys;
  res->records_written = 0;
  if (!table->n_keys) return empty_selection (ctx, word_length, count_only, res);
  if (!table->device_keys || !table->device_counts) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_table_select: a table of %llu keys without its arrays", (unsigned long long) table->n_keys);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  hipStream_t st = ctx->stream;
  const SelTable t = table_walk (table);
  if (!t.segments) return empty_selection (ctx, word_length, count_only, res);
  const SelRule q = { min_lists, max_lists, cutoff, rule == GT4HIP_RULE_NUMBER ? 1u : 0u, ovr };

  TempBlocks blk;
  u32 *row_cnt = NULL, *seg_cnt = NULL;
  unsigned char *row_keep = NULL;
  u64 *seg_sum = NULL, *seg_off = NULL;
  int rc = GT4HIP_OK;
  if (!count_only) {
    rc = blk.get (ctx, (size_t) t.n_keys * 4, (void **) &row_cnt);
    if (!rc) rc = blk.get (ctx, (size_t) t.n_keys, (void **) &row_keep);
  }
  if (!rc) rc = blk.get (ctx, (size_t) t.segments * 4, (void **) &seg_cnt);
  if (!rc) rc = blk.get (ctx, (size_t) t.segments * 8, (void **) &seg_sum);
  if (!rc) rc = blk.get (ctx, (size_t) t.segments * 8, (void **) &seg_off);
  if (rc) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_table_select: the workspace of %llu rows in %llu segments", (unsigned long long) t.n_keys, (unsigned long long) t.segments);

  const dim3 grid ((unsigned) gt4hip_grid (ctx, t.segments));
  const bool maxr = rule == GT4HIP_RULE_MAX;
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], st));
  /* rows of a multiple of four counts in arrays that are 16-byte aligned (the library's own are): 16 bytes per lane */
  const bool wide = ctx->select_vec >= 0 && t.n_lists % 4 == 0 && ((uintptr_t) t.counts & 15) == 0;
  ctx->select_wide = wide;
  if (wide) launch_decide_width<4> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  else launch_decide_width<1> (maxr, grid, st, t, q, row_cnt, row_keep, seg_cnt, seg_sum);
  HIPCHK (ctx, hipGetLastError ());
  hipLaunchKernelGGL (k_select_scan, dim3 (1), dim3 (1024), 0, st, seg_cnt, seg_sum, t.segments, seg_off, (u64 *) ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], st));
  if ((rc = gt4hip_read_scratch (ctx, 2))) return rc;
  const uint64_t n_words = ctx->scratch_host[0], total_count = ctx->scratch_host[1];
  float ms = 0;
  HIPCHK (ctx, hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]));
  res->device_ms = ms;
  if (n_words > t.n_keys) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "gt4hip_table_select: %llu of %llu rows kept", (unsigned long long) n_words, (unsigned long long) t.n_keys);
  res->n_words = n_words;
  res->total_count = total_count;
  if (count_only) {
    res->out = NULL;
    return GT4HIP_OK;
  }
  TempLists made;
  gt4hip_list *o = NULL;
  if ((rc = gt4hip_output_list (ctx, -1, res->out, n_words, word_length, made, &o))) return rc;
  if (n_words) {
    HIPCHK (ctx, hipEventRecord (ctx->ev[2], st));
    gt4hip_grid_again (ctx, t.segments, (int) grid.x);
    hipLaunchKernelGGL (k_select_emit, grid, dim3 (SEL_THREADS), 0, st, t, (const u32 *) row_cnt, (const unsigned char *) row_keep, (const u32 *) seg_cnt,
                        (const u64 *) seg_off, (u32 *) o->dev);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, hipEventRecord (ctx->ev[3], st));
    HIPCHK (ctx, hipStreamSynchronize (st));
    HIPCHK (ctx, hipEventElapsedTime (&ms, ctx->ev[2], ctx->ev[3]));
    res->device_ms += ms;
  }
  made.release ();
  o->n_words = n_words;
  res->out = o;
  res->records_written = n_words;
  return GT4HIP_OK;
}

}  // namespace

extern "C" int gt4hip_table_select (gt4hip_context *ctx, const gt4hip_count_table *table, uint32_t min_lists, uint32_t max_lists, uint32_t cutoff,
                                     int32_t rule, uint32_t ovr, int32_t count_only, gt4hip_multi_result *res)
{
  if (!ctx || !table || !res) return GT4HIP_EINVAL;
  int rc = union_rule (ctx, "table_select", &rule);
  if (!rc) rc = check_bounds (ctx, "gt4hip_table_select", min_lists, max_lists, table->n_lists);
  if (rc) return rc;
  /* (the table does not know its word length: a list made here says 32, the widest) */
  return table_select (ctx, table, res->out ? res->out->word_length : 32u, min_lists, max_lists, cutoff, rule, ovr, count_only != 0, res);
}

extern "C" int gt4hip_select_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, uint32_t min_lists, uint32_t max_lists,
                                     uint32_t cutoff, int32_t rule, uint32_t ovr, int32_t count_only, gt4hip_multi_result *res)
{
  if (!ctx || !lists || !n_lists || !res) return GT4HIP_EINVAL;
  int rc = union_rule (ctx, "select_multi", &rule);
  if (!rc) rc = check_bounds (ctx, "gt4hip_select_multi", min_lists, max_lists, n_lists);
  if (rc) return rc;
  TempTable t;
  if ((rc = gt4hip_union_table_checked (ctx, lists, n_lists, &t.table))) return rc;
  return table_select (ctx, &t.table, lists[0]->word_length, min_lists, max_lists, cutoff, rule, ovr, count_only != 0, res);
}
