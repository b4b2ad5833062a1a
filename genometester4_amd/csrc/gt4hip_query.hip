/* gt4hip_query.hip -- glistquery on the device, gfx950, wave64: batched lookups of words "up to N mismatches" in a
 * resident list (gt4_word_dict_lookup_mm as search_one_word drives it, reference src/word-dict.c:74-106,
 * src/glistquery.c:543-568) and the whole-list statistics behind --median, --distribution and --gc
 * (src/glistquery.c:831-932).
 *
 * The lookup is gt4hip_mismatch.hip's level kernel with another reduction.  The reference enumerates, per query, the
 * word itself and every word that differs from it in 1..N bases at positions >= pm_3, canonicalises each one and binary
 * searches the whole list for it, summing the counts found.  Here:
 *
 *   - the list's bucket index (gt4hip_index.h) is built once per list and kept (gt4hip_query_index);
 *   - the variants of a query are ranked: rank 0 is the word itself, then the C(k', 1) * 3 variants with one
 *     substitution, the C(k', 2) * 9 with two, ... (k' = k - pm_3; inside a level the order of variant_mask);
 *   - one kernel runs over the flattened (query, rank) space with a grid-stride loop, consecutive lanes on
 *     consecutive ranks.  A lane that finds its variant loads the record's count; the counts are summed inside the
 *     wavefront, segmented at query boundaries, and the head lane of a segment issues ONE u32 atomic for it.  The
 *     shuffles of the segmented sum run only in wavefronts that have a hit at all (rare at k >= 20);
 *   - u32 sums wrap as the reference's unsigned int does;
 *   - N == 0 is one probe per query: no atomics, found = present (a stored count of 0 is still found).
 *
 * --all (gt4hip_query_lookup_all) returns the hits themselves in (query, rank) order: tiles of the flattened space
 * count their hits, one scan turns the counts into offsets, and a second pass over the same tiles repeats the probes
 * and writes every hit to its place.  Nothing of the size of the variant space is ever stored.
 *
 * The statistics are one streaming pass each over the 12-byte records: four records per thread as three 16-byte
 * loads where the list is 16-byte aligned, a wavefront reduction, one atomic per wavefront.
 */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"

#include <string.h>

#define GT4HIP_QUERY_MAX_MM 32

namespace gt4 {
namespace {

struct Query {
  const u64 *words;
  u64 n;         /* queries */
  u64 n_var;     /* V: ranks per query */
  u64 total;     /* n * V */
  u64 stride_w;  /* the grid's stride as (queries, ranks) */
  u64 stride_r;
  Index ix;
  u32 k, kp;     /* word length; positions that may change, k - pm_3 */
  u32 shift;     /* 2 * pm_3 */
  u32 n_mm;
  u32 canonize;
  u64 base[GT4HIP_QUERY_MAX_MM + 2]; /* base[c]: first rank with c substitutions; base[n_mm + 1] = V */
  u64 pow3[GT4HIP_QUERY_MAX_MM + 1];
};

__device__ __forceinline__ u64 canonical (u64 w, u32 k, u32 canonize)
{
  if (!canonize) return w;
  const u64 rc = revcomp (w, k);
  return rc < w ? rc : w;
}

/* variant `r` of query word `wq` (already canonical), as it is looked up */
template <bool WIDE>
__device__ __forceinline__ u64 query_variant (const Query &Q, u64 wq, u64 r)
{
  u32 c = Q.n_mm;
  while (r < Q.base[c]) c--;
  const u64 mask = variant_mask<WIDE> (r - Q.base[c], Q.pow3[c], Q.kp, c) << Q.shift;
  return canonical (wq ^ mask, Q.k, Q.canonize);
}

/* n_mm == 0: one probe per query */
__global__ __launch_bounds__ (MM_THREADS) void k_query_exact (const u64 *words, u64 n, Index ix, u32 k, u32 canonize, u32 *values, unsigned char *found)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) {
    const u64 j = find (ix, canonical (words[i], k, canonize));
    values[i] = j != ~0ull ? ix.rec[3 * j + 2] : 0u;
    found[i] = j != ~0ull;
  }
}

/* values[q] += the counts of the variants of q found in the list (values zeroed before the launch) */
template <bool WIDE>
__global__ __launch_bounds__ (MM_THREADS) void k_query (Query Q, u32 *values)
{
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 gtid = (u64) blockIdx.x * MM_THREADS + threadIdx.x;
  const u64 stride = (u64) gridDim.x * MM_THREADS;
  u64 w = gtid / Q.n_var, r = gtid - (gtid / Q.n_var) * Q.n_var;
  for (u64 g0 = gtid - lane; g0 < Q.total; g0 += stride) { /* wavefront-uniform */
    const bool valid = g0 + lane < Q.total;
    u32 val = 0;
    bool hit = false;
    if (valid) {
      const u64 cv = query_variant<WIDE> (Q, canonical (Q.words[w], Q.k, Q.canonize), r);
      const u64 j = find (Q.ix, cv);
      if (j != ~0ull) {
        val = Q.ix.rec[3 * j + 2];
        hit = val != 0; /* a stored count of 0 adds nothing */
      }
    }
    if (__builtin_amdgcn_ballot_w64 (hit)) {
      /* segments of lanes on the same query: lanes run consecutive ranks, so queries ascend across the wavefront */
      const u64 wprev = shfl_up_u64 (w, 1);
      const bool head = valid && (lane == 0 || wprev != w);
      const u64 S = __builtin_amdgcn_ballot_w64 (head) | ~__builtin_amdgcn_ballot_w64 (valid);
      const u64 after = lane == WAVE - 1 ? 0 : S & (~0ull << (lane + 1));
      const int end = after ? __builtin_ctzll (after) - 1 : WAVE - 1; /* last lane of this lane's segment */
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        const u32 o = __shfl_down (val, d, WAVE);
        if (lane + d <= end) val += o;
      }
      if (head && val) atomicAdd (&values[w], val);
    }
    r += Q.stride_r;
    w += Q.stride_w;
    if (r >= Q.n_var) {
      r -= Q.n_var;
      w++;
    }
  }
}

__global__ __launch_bounds__ (MM_THREADS) void k_query_found (const u32 *values, u64 n, unsigned char *found)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) found[i] = values[i] != 0;
}

/* --all.  Tile t covers items [t * MM_TILE, (t + 1) * MM_TILE) of the flattened space, as in the compaction of
 * gt4hip_mismatch.hip.  FILL == false: tile_cnt[t] = hits of the tile.  FILL == true: the hits to hits[tile_off[t]...]
 * in item order (the probes are repeated: the variant space itself is never stored). */
template <bool FILL>
__global__ __launch_bounds__ (MM_THREADS) void k_query_all (Query Q, u64 n_tiles, u32 *tile_cnt, const u64 *tile_off, gt4hip_query_hit *hits)
{
  __shared__ u32 part[MM_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    u64 pos = FILL ? tile_off[t] : 0;
    u32 mine = 0;
    for (int rd = 0; rd < MM_ROUNDS; rd++) {
      const u64 g = t * MM_TILE + (u64) rd * MM_THREADS + threadIdx.x;
      u64 q = 0, r = 0, cv = 0, j = ~0ull;
      if (g < Q.total) {
        q = g / Q.n_var;
        r = g - q * Q.n_var;
        cv = query_variant<true> (Q, canonical (Q.words[q], Q.k, Q.canonize), r);
        j = find (Q.ix, cv);
      }
      const bool hit = j != ~0ull;
      if (!FILL) {
        mine += hit;
      } else {
        const u64 m = __builtin_amdgcn_ballot_w64 (hit);
        if (lane == 0) part[wv] = (u32) __popcll (m);
        __syncthreads ();
        u32 before = 0, round = 0;
        for (int x = 0; x < MM_THREADS / WAVE; x++) {
          before += x < wv ? part[x] : 0;
          round += part[x];
        }
        if (hit) {
          gt4hip_query_hit h;
          h.query = q;
          h.rank = r;
          h.word = cv;
          h.count = Q.ix.rec[3 * j + 2];
          h.reserved = 0;
          hits[pos + before + (u32) __popcll (m & ((1ull << lane) - 1))] = h;
        }
        pos += round;
        __syncthreads ();
      }
    }
    if (!FILL) {
      mine = dpp_wave_sum_u32 (mine);
      if (lane == 0) part[wv] = mine;
      __syncthreads ();
      if (threadIdx.x == 0) {
        u32 s = 0;
        for (int x = 0; x < MM_THREADS / WAVE; x++) s += part[x];
        tile_cnt[t] = s;
      }
      __syncthreads ();
    }
  }
}

/* ------------------------------------------------------------------ statistics: one pass over the records */

/* f (key, count) for every record, each once: four records per thread as three 16-byte loads where the list allows it */
template <class F>
__device__ __forceinline__ void for_each_record (const u32 *__restrict__ rec, u64 n, F f)
{
  const u64 tid = (u64) blockIdx.x * MM_THREADS + threadIdx.x, step = (u64) gridDim.x * MM_THREADS;
  const u64 groups = ((size_t) rec & 15) == 0 ? n / 4 : 0;
  const u32x4 *v = (const u32x4 *) rec;
  for (u64 g = tid; g < groups; g += step) {
    const u32x4 a = v[3 * g], b = v[3 * g + 1], c = v[3 * g + 2];
    f ((u64) a.x | ((u64) a.y << 32), a.z);
    f ((u64) a.w | ((u64) b.x << 32), b.y);
    f ((u64) b.z | ((u64) b.w << 32), c.x);
    f ((u64) c.y | ((u64) c.z << 32), c.w);
  }
  for (u64 i = groups * 4 + tid; i < n; i += step) f (load_key (rec, i), rec[3 * i + 2]);
}

/* out[0] = smallest count, out[1] = largest (preset to ~0 and 0) */
__global__ __launch_bounds__ (MM_THREADS) void k_count_stats (const u32 *rec, u64 n, u32 *out)
{
  u32 lo = ~0u, hi = 0;
  for_each_record (rec, n, [&] (u64, u32 c) {
    lo = c < lo ? c : lo;
    hi = c > hi ? c : hi;
  });
#pragma unroll
  for (int m = WAVE / 2; m > 0; m >>= 1) {
    const u32 a = __shfl_xor (lo, m, WAVE), b = __shfl_xor (hi, m, WAVE);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    atomicMin (&out[0], lo);
    atomicMax (&out[1], hi);
  }
}

/* out[0] += records with count < med, out[1] += records with count > med */
__global__ __launch_bounds__ (MM_THREADS) void k_count_split (const u32 *rec, u64 n, u32 med, unsigned long long *out)
{
  u64 below = 0, above = 0;
  for_each_record (rec, n, [&] (u64, u32 c) {
    below += c < med;
    above += c > med;
  });
  below = wave_sum (below);
  above = wave_sum (above);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (below) atomicAdd (&out[0], below);
    if (above) atomicAdd (&out[1], above);
  }
}

constexpr u32 HIST_LDS_BINS = 4096;

/* hist[c - 1] += 1 for every record with 1 <= count c <= max.  LDS: up to HIST_LDS_BINS bins per workgroup (u32: a
 * workgroup sees fewer than 2^32 records), flushed with one u64 atomic per used bin; above that global atomics. */
template <bool LDS>
__global__ __launch_bounds__ (MM_THREADS) void k_count_histogram (const u32 *rec, u64 n, u32 max, unsigned long long *hist)
{
  __shared__ u32 bins[LDS ? HIST_LDS_BINS : 1];
  if (LDS) {
    for (u32 i = threadIdx.x; i < max; i += MM_THREADS) bins[i] = 0;
    __syncthreads ();
  }
  for_each_record (rec, n, [&] (u64, u32 c) {
    if (c == 0 || c > max) return;
    if (LDS) atomicAdd (&bins[c - 1], 1u);
    else atomicAdd (&hist[c - 1], 1ull);
  });
  if (LDS) {
    __syncthreads ();
    for (u32 i = threadIdx.x; i < max; i += MM_THREADS)
      if (bins[i]) atomicAdd (&hist[i], (unsigned long long) bins[i]);
  }
}

/* *out += count * (G and C bases of the word): a base is G or C when its two bits differ (A 00, C 01, G 10, T 11) */
__global__ __launch_bounds__ (MM_THREADS) void k_gc (const u32 *rec, u64 n, u64 mask, unsigned long long *out)
{
  u64 acc = 0;
  for_each_record (rec, n, [&] (u64 w, u32 c) { acc += (u64) c * (u32) __popcll ((w ^ (w >> 1)) & 0x5555555555555555ull & mask); });
  acc = wave_sum (acc);
  if ((threadIdx.x & (WAVE - 1)) == 0 && acc) atomicAdd (out, acc);
}

}  // namespace
}  // namespace gt4

using namespace gt4;

/* ------------------------------------------------------------------ host side */

struct gt4hip_query_index {
  gt4hip_context *ctx;
  const gt4hip_list *list;
  Index ix;
  void *owner;
  double last_ms;
};

namespace {

/* V and the per-level tables; false when V does not fit 64 bits */
bool variant_space (u32 k, u32 n_mm, u32 pm_3, u64 *base, u64 *pow3, u64 *n_var)
{
  const u32 kp = k - pm_3;
  unsigned __int128 v = 0, p = 1;
  for (u32 c = 0; c <= n_mm; c++) {
    base[c] = (u64) v;
    pow3[c] = (u64) p;
    v += (unsigned __int128) BINOM_HOST.v[kp][c] * p;
    if (v >> 64) return false;
    p *= 3;
  }
  base[n_mm + 1] = (u64) v;
  *n_var = (u64) v;
  return true;
}

int check_params (gt4hip_context *ctx, const char *who, const gt4hip_query_index *qi, const gt4hip_query_params *prm)
{
  const u32 k = qi->list->word_length;
  if (k < 1 || k > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: word length %u", who, k);
  if (prm->n_mm > GT4HIP_QUERY_MAX_MM || prm->pm_3 > 32 || (prm->n_mm && prm->n_mm + prm->pm_3 > k))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: %u mismatches and %u protected bases do not fit a word of %u", who, prm->n_mm, prm->pm_3, k);
  return GT4HIP_OK;
}

int fill_query (gt4hip_context *ctx, const char *who, const gt4hip_query_index *qi, const gt4hip_query_params *prm, const u64 *dev_words, u64 n, Query *Q)
{
  memset (Q, 0, sizeof *Q);
  const u32 k = qi->list->word_length;
  Q->words = dev_words;
  Q->n = n;
  Q->ix = qi->ix;
  Q->k = k;
  Q->n_mm = prm->n_mm;
  Q->kp = prm->n_mm ? k - prm->pm_3 : k;
  Q->shift = prm->n_mm ? 2 * prm->pm_3 : 0;
  Q->canonize = prm->canonize != 0;
  if (!variant_space (k, prm->n_mm, prm->n_mm ? prm->pm_3 : 0, Q->base, Q->pow3, &Q->n_var))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: a word of %u has more than 2^64 variants with %u mismatches", who, k, prm->n_mm);
  if (n > ~0ull / Q->n_var)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: %llu queries of %llu variants each do not fit 64 bits: split the batch", who, (unsigned long long) n,
                        (unsigned long long) Q->n_var);
  Q->total = n * Q->n_var;
  return GT4HIP_OK;
}

struct Timer {
  hipEvent_t e0 = NULL, e1 = NULL;
  ~Timer ()
  {
    if (e0) hipEventDestroy (e0);
    if (e1) hipEventDestroy (e1);
  }
};

}  // namespace

extern "C" int gt4hip_query_index_create (gt4hip_context *ctx, const gt4hip_list *list, gt4hip_query_index **out)
{
  if (!ctx || !list || !out) return GT4HIP_EINVAL;
  *out = NULL;
  if (list->word_length < 1 || list->word_length > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_query_index_create: word length %u", list->word_length);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_query_index *qi = new gt4hip_query_index ();
  qi->ctx = ctx;
  qi->list = list;
  qi->last_ms = 0;
  size_index (list, &qi->ix);
  void *off = NULL;
  int rc = gt4hip_block_alloc (ctx, (qi->ix.nb + 1) * 8, &off, &qi->owner);
  if (!rc) rc = fill_index (ctx, &qi->ix, off);
  if (!rc && hipStreamSynchronize (ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_query_index_create: building the index failed");
  if (rc) {
    gt4hip_query_index_free (qi);
    return rc;
  }
  *out = qi;
  return GT4HIP_OK;
}

extern "C" void gt4hip_query_index_free (gt4hip_query_index *qi)
{
  if (!qi) return;
  gt4hip_block_free (qi->owner);
  delete qi;
}

extern "C" double gt4hip_query_index_last_ms (const gt4hip_query_index *qi) { return qi ? qi->last_ms : 0.0; }

extern "C" int gt4hip_query_variants (uint32_t word_length, const gt4hip_query_params *prm, uint64_t *n_variants)
{
  u64 base[GT4HIP_QUERY_MAX_MM + 2], pow3[GT4HIP_QUERY_MAX_MM + 1];
  if (!prm || !n_variants || word_length < 1 || word_length > 32 || prm->n_mm > GT4HIP_QUERY_MAX_MM) return GT4HIP_EINVAL;
  if (prm->n_mm && prm->n_mm + prm->pm_3 > word_length) return GT4HIP_EINVAL;
  unsigned long long v = 0;
  if (!variant_space (word_length, prm->n_mm, prm->n_mm ? prm->pm_3 : 0, base, pow3, &v)) return GT4HIP_EINVAL;
  *n_variants = v;
  return GT4HIP_OK;
}

/* the host's copy of the device's unranking (query_variant, variant_mask) */
extern "C" int gt4hip_query_variant_mask (uint32_t word_length, const gt4hip_query_params *prm, uint64_t rank, uint64_t *mask)
{
  u64 base[GT4HIP_QUERY_MAX_MM + 2], pow3[GT4HIP_QUERY_MAX_MM + 1];
  unsigned long long v = 0;
  if (!prm || !mask || word_length < 1 || word_length > 32 || prm->n_mm > GT4HIP_QUERY_MAX_MM) return GT4HIP_EINVAL;
  if (prm->n_mm && prm->n_mm + prm->pm_3 > word_length) return GT4HIP_EINVAL;
  const u32 pm_3 = prm->n_mm ? prm->pm_3 : 0;
  if (!variant_space (word_length, prm->n_mm, pm_3, base, pow3, &v) || rank >= v) return GT4HIP_EINVAL;
  u32 c = prm->n_mm;
  while (rank < base[c]) c--;
  u64 comb = (rank - base[c]) / pow3[c], sub = (rank - base[c]) % pow3[c], m = 0;
  u32 x = word_length - pm_3;
  for (u32 j = c; j >= 1; j--) {
    x--;
    while (BINOM_HOST.v[x][j] > comb) x--;
    comb -= BINOM_HOST.v[x][j];
    m |= (u64) (sub % 3u + 1u) << (2u * x);
    sub /= 3u;
  }
  *mask = m << (2 * pm_3);
  return GT4HIP_OK;
}

extern "C" int gt4hip_query_lookup (gt4hip_context *ctx, gt4hip_query_index *qi, const uint64_t *words, uint64_t n, const gt4hip_query_params *prm,
                                    uint32_t *values, uint8_t *found)
{
  if (!ctx || !qi || !prm || (n && (!words || !values || !found))) return GT4HIP_EINVAL;
  int rc = check_params (ctx, "gt4hip_query_lookup", qi, prm);
  if (rc) return rc;
  qi->last_ms = 0;
  ctx->query_wide = 0;
  if (!n) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  Blocks blk;
  u64 *d_words = NULL;
  u32 *d_values = NULL;
  unsigned char *d_found = NULL;
  if ((rc = blk.get (ctx, n * 8, (void **) &d_words)) || (rc = blk.get (ctx, n * 4, (void **) &d_values)) || (rc = blk.get (ctx, n, (void **) &d_found))) return rc;
  Query Q;
  if ((rc = fill_query (ctx, "gt4hip_query_lookup", qi, prm, d_words, n, &Q))) return rc;
  Timer tm;
  HIPCHK (ctx, hipEventCreate (&tm.e0));
  HIPCHK (ctx, hipEventCreate (&tm.e1));
  HIPCHK (ctx, hipMemcpyAsync (d_words, words, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK (ctx, hipEventRecord (tm.e0, ctx->stream));
  if (!prm->n_mm) {
    hipLaunchKernelGGL (k_query_exact, dim3 (grid_for (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, d_words, n, Q.ix, Q.k, Q.canonize, d_values,
                        d_found);
  } else {
    HIPCHK (ctx, hipMemsetAsync (d_values, 0, n * 4, ctx->stream));
    const int grid = grid_for (ctx, Q.total, MM_THREADS);
    const u64 stride = (u64) grid * MM_THREADS;
    Q.stride_w = stride / Q.n_var;
    Q.stride_r = stride % Q.n_var;
    ctx->query_wide = !(Q.n_var + stride < 0xffffffffull);
    if (!ctx->query_wide) hipLaunchKernelGGL (k_query<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, d_values);
    else hipLaunchKernelGGL (k_query<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, d_values);
    HIPCHK (ctx, hipGetLastError ());
    hipLaunchKernelGGL (k_query_found, dim3 (grid_for (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, d_values, n, d_found);
  }
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (tm.e1, ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (values, d_values, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (found, d_found, n, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  float ms = 0;
  if (hipEventElapsedTime (&ms, tm.e0, tm.e1) == hipSuccess) qi->last_ms = ms;
  return GT4HIP_OK;
}

extern "C" int gt4hip_query_lookup_all (gt4hip_context *ctx, gt4hip_query_index *qi, const uint64_t *words, uint64_t n, const gt4hip_query_params *prm,
                                        gt4hip_query_hit *hits, uint64_t capacity, uint64_t *n_hits)
{
  if (!ctx || !qi || !prm || !n_hits || (n && !words) || (capacity && !hits)) return GT4HIP_EINVAL;
  int rc = check_params (ctx, "gt4hip_query_lookup_all", qi, prm);
  if (rc) return rc;
  *n_hits = 0;
  qi->last_ms = 0;
  if (!n) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  Blocks blk;
  u64 *d_words = NULL;
  if ((rc = blk.get (ctx, n * 8, (void **) &d_words))) return rc;
  Query Q;
  if ((rc = fill_query (ctx, "gt4hip_query_lookup_all", qi, prm, d_words, n, &Q))) return rc;
  const u64 tiles = Q.total / MM_TILE + (Q.total % MM_TILE != 0);
  if (tiles > (1ull << 31))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_query_lookup_all: %llu queries of %llu variants each are too many for one call: split the batch",
                        (unsigned long long) n, (unsigned long long) Q.n_var);
  u32 *tile_cnt = NULL;
  u64 *tile_off = NULL;
  if ((rc = blk.get (ctx, tiles * 4, (void **) &tile_cnt)) || (rc = blk.get (ctx, tiles * 8, (void **) &tile_off))) return rc;
  Timer tm;
  HIPCHK (ctx, hipEventCreate (&tm.e0));
  HIPCHK (ctx, hipEventCreate (&tm.e1));
  HIPCHK (ctx, hipMemcpyAsync (d_words, words, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK (ctx, hipEventRecord (tm.e0, ctx->stream));
  const int grid = grid_for (ctx, tiles, 1);
  hipLaunchKernelGGL (k_query_all<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, tiles, tile_cnt, (const u64 *) NULL, (gt4hip_query_hit *) NULL);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, ctx->stream, tile_cnt, tiles, tile_off, ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  const u64 total_hits = ctx->scratch_host[0];
  *n_hits = total_hits;
  if (total_hits && total_hits <= capacity) {
    gt4hip_query_hit *d_hits = NULL;
    if ((rc = blk.get (ctx, total_hits * sizeof (gt4hip_query_hit), (void **) &d_hits))) return rc;
    hipLaunchKernelGGL (k_query_all<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, tiles, tile_cnt, tile_off, d_hits);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, hipEventRecord (tm.e1, ctx->stream));
    HIPCHK (ctx, hipMemcpyAsync (hits, d_hits, total_hits * sizeof (gt4hip_query_hit), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    HIPCHK (ctx, hipEventRecord (tm.e1, ctx->stream));
  }
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  float ms = 0;
  if (hipEventElapsedTime (&ms, tm.e0, tm.e1) == hipSuccess) qi->last_ms = ms;
  return GT4HIP_OK;
}

/* ------------------------------------------------------------------ statistics */

extern "C" int gt4hip_list_count_stats (gt4hip_context *ctx, const gt4hip_list *list, uint32_t *min, uint32_t *max)
{
  if (!ctx || !list || !min || !max) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  u32 *out = (u32 *) ctx->scratch;
  u32 *host = (u32 *) ctx->scratch_host;
  host[0] = ~0u;
  host[1] = 0;
  if (list->n_words) {
    HIPCHK (ctx, hipMemcpyAsync (out, host, 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL (k_count_stats, dim3 (grid_for (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev,
                        list->n_words, out);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, hipMemcpyAsync (host, out, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  }
  *min = host[0];
  *max = host[1];
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_count_split (gt4hip_context *ctx, const gt4hip_list *list, uint32_t med, uint64_t *below, uint64_t *above)
{
  if (!ctx || !list || !below || !above) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  *below = *above = 0;
  if (!list->n_words) return GT4HIP_OK;
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 16, ctx->stream));
  hipLaunchKernelGGL (k_count_split, dim3 (grid_for (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev,
                      list->n_words, med, ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  *below = ctx->scratch_host[0];
  *above = ctx->scratch_host[1];
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_count_histogram (gt4hip_context *ctx, const gt4hip_list *list, uint32_t max, uint64_t *hist)
{
  if (!ctx || !list || (max && !hist)) return GT4HIP_EINVAL;
  if (!max) return GT4HIP_OK;
  memset (hist, 0, (size_t) max * 8);
  if (!list->n_words) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  Blocks blk;
  unsigned long long *d = NULL;
  int rc = blk.get (ctx, (size_t) max * 8, (void **) &d);
  if (rc) return rc;
  HIPCHK (ctx, hipMemsetAsync (d, 0, (size_t) max * 8, ctx->stream));
  const int grid = grid_for (ctx, list->n_words, MM_THREADS * 4);
  if (max <= HIST_LDS_BINS)
    hipLaunchKernelGGL (k_count_histogram<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev, list->n_words, max, d);
  else hipLaunchKernelGGL (k_count_histogram<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev, list->n_words, max, d);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (hist, d, (size_t) max * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_gc (gt4hip_context *ctx, const gt4hip_list *list, uint64_t *weighted_gc_bases)
{
  if (!ctx || !list || !weighted_gc_bases) return GT4HIP_EINVAL;
  *weighted_gc_bases = 0;
  const u32 k = list->word_length;
  if (k < 1 || k > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_list_gc: word length %u", k);
  if (!list->n_words) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  const u64 mask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1;
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 8, ctx->stream));
  hipLaunchKernelGGL (k_gc, dim3 (grid_for (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev, list->n_words,
                      mask, ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  *weighted_gc_bases = ctx->scratch_host[0];
  return GT4HIP_OK;
}
