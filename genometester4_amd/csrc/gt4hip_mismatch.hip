/* gt4hip_mismatch.hip -- glistcompare -mm N: the difference "up to N mismatches" (compare_wordmaps_mm,
 * reference src/glistcompare.c:958-1168), gfx950, wave64.
 *
 * The reference builds the difference table(s) in one merge, then runs levels c = 1..N: every word still in
 * the table enumerates its variants with exactly c substituted bases, canonicalises each one
 * (min (v, revcomp (v))) and looks it up in the other list by binary search; the word survives the level
 * while the number of variants PRESENT there stays below the cutoff.  Every lookup is independent, so here:
 *
 *   - a bucket index over each input list: offsets[p] = first record whose key has top-b-bit prefix >= p
 *     (one streaming pass over the 12-byte records).  A lookup reads offsets[p], offsets[p + 1] and binary
 *     searches a window of ~8 records (one or two 128-B lines) instead of ~log2 n levels of the whole list;
 *   - the pre-pass probes every record of a in b's index (and of b in a's for diff2) and applies the merge's
 *     rules per record, then compacts the kept records stably into the table (no pair-merge kernel involved);
 *   - a level runs over the flattened (word, variant rank) space with a grid-stride loop: consecutive lanes
 *     take consecutive ranks, so a wavefront mostly works on one word; hits are reduced with ballots,
 *     segmented at word boundaries, one u32 atomic per (word, wavefront segment).  A word already decided
 *     (count >= cutoff without subtract, a variant in b and not in a with subtract) skips its probes;
 *   - between levels the survivors are compacted in table order (tile counts, one scan, stable scatter),
 *     so level c + 1, ~k times the work of level c, only runs on words still alive.
 */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"

#include <string.h>

namespace gt4 {
namespace {


/* The merge of compare_wordmaps_mm (:1005-1052) per record of x (side 0: x = list 1, the other = list 2, table
 * diff1; side 1: x = list 2, the other = list 1, table diff2): keep[i] and the table count val[i]. */
__global__ __launch_bounds__ (MM_THREADS) void k_prepass (const u32 *x, u64 nx, Index other, u32 side, u32 cutoff, u32 subtract,
                                                          u32 *keep, u32 *val)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < nx; i += (u64) gridDim.x * MM_THREADS) {
    const u64 key = load_key (x, i);
    const u32 f = x[3 * i + 2];
    const u64 j = find (other, key);
    u32 k = 0, v = 0;
    if (j != ~0ull) {
      const u32 fo = other.rec[3 * j + 2];
      const u32 f1 = side ? fo : f;
      u32 f2 = side ? f : fo;
      const bool g1 = f1 >= cutoff, g2 = f2 >= cutoff; /* before the subtraction */
      if (subtract && f1 <= f2) f2 -= f1;
      if (side == 0) {
        k = g1 && !g2;
        v = f1 - f2;
      } else {
        k = g2 && !g1;
        v = f2 - f1;
      }
    } else {
      k = side ? f >= cutoff : (f >= cutoff && !subtract); /* -du never adds keys that only list 1 has */
      v = f;
    }
    keep[i] = k;
    val[i] = v;
  }
}

/* (k_tile_count and k_tile_scan: gt4hip_index.h) */

/* Kept items to their place: source keys from packed records (SRC_REC) or a key array, counts from `cnt`;
 * destination packed records (DST_REC; null: count only) or key + count arrays.  *sum += counts kept. */
template <bool SRC_REC, bool DST_REC>
__global__ __launch_bounds__ (MM_THREADS) void k_scatter (const u32 *keep, u64 n, u64 n_tiles, const u64 *tile_off, const void *src_keys,
                                                          const u32 *cnt, void *dst_keys, u32 *dst_cnt, unsigned long long *sum)
{
  __shared__ u32 part[MM_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  u64 my_sum = 0;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    u64 pos = tile_off[t];
    for (int r = 0; r < MM_ROUNDS; r++) {
      const u64 i = t * MM_TILE + (u64) r * MM_THREADS + threadIdx.x;
      const bool k = i < n && keep[i];
      /* (round_place of gt4hip_index.h, open-coded: with this kernel and k_tile_count on the helpers the -mm pre-pass
       * measured 1.5 % slower than with this text, profiles/HISTORY.md) */
      const u64 m = __builtin_amdgcn_ballot_w64 (k);
      if (lane == 0) part[wv] = (u32) __popcll (m);
      __syncthreads ();
      u32 before = 0, round = 0;
      for (int w = 0; w < MM_THREADS / WAVE; w++) {
        before += w < wv ? part[w] : 0;
        round += part[w];
      }
      if (k) {
        const u64 o = pos + before + (u32) __popcll (m & ((1ull << lane) - 1));
        const u64 key = SRC_REC ? load_key ((const u32 *) src_keys, i) : ((const u64 *) src_keys)[i];
        const u32 c = cnt[i];
        my_sum += c;
        if (DST_REC) {
          if (dst_keys) {
            u32 *d = (u32 *) dst_keys + 3 * o;
            d[0] = (u32) key;
            d[1] = (u32) (key >> 32);
            d[2] = c;
          }
        } else {
          ((u64 *) dst_keys)[o] = key;
          dst_cnt[o] = c;
        }
      }
      pos += round;
      __syncthreads ();
    }
  }
  if (sum) {
    my_sum = wave_sum (my_sum);
    if (lane == 0 && my_sum) atomicAdd (sum, (unsigned long long) my_sum);
  }
}

/* ------------------------------------------------------------------ one level */

struct Level {
  const u64 *words;
  u64 n_words;
  u64 n_var;     /* C(k, c) * 3^c variants per word */
  u64 pow3;      /* 3^c */
  u64 total;     /* n_words * n_var */
  u64 stride_w;  /* the grid's stride as (words, ranks) */
  u64 stride_r;
  Index m;       /* looked up: list 2 for diff1, list 1 for diff2 */
  Index q;       /* subtract: list 1 for diff1, nothing for diff2 (the reference's missing dictionary) */
  u32 k, c;
  u32 subtract;
  u32 cutoff;
  u32 early;     /* decided words may skip their probes (exact unless a u32 count could wrap) */
  u32 *cnt;      /* per word: variants counted (present in m; with subtract: in q and not in m) */
  u32 *drop;     /* per word, subtract: a variant is in m and not in q */
};


template <bool WIDE>
__global__ __launch_bounds__ (MM_THREADS) void k_level (Level L, unsigned long long *probes)
{
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 gtid = (u64) blockIdx.x * MM_THREADS + threadIdx.x;
  const u64 stride = (u64) gridDim.x * MM_THREADS;
  u64 w = gtid / L.n_var, r = gtid - (gtid / L.n_var) * L.n_var;
  u32 my_probes = 0;
  for (u64 g0 = gtid - lane; g0 < L.total; g0 += stride) { /* wavefront-uniform */
    const bool valid = g0 + lane < L.total;
    bool hit = false, kill = false;
    if (valid) {
      const bool skip = L.early && (L.subtract ? L.drop[w] != 0 : L.cnt[w] >= L.cutoff);
      if (!skip) {
        const u64 v = L.words[w] ^ variant_mask<WIDE> (r, L.pow3, L.k, L.c);
        const u64 cv = canonical (v, L.k, 1);
        const bool pm = find (L.m, cv) != ~0ull;
        my_probes++;
        if (L.subtract) {
          const bool pq = L.q.n && find (L.q, cv) != ~0ull;
          my_probes += L.q.n != 0;
          hit = pq && !pm;  /* present_m - present_q = -1 */
          kill = pm && !pq; /* present_m > present_q: the word is dropped (search_query, :1121) */
        } else {
          hit = pm;
        }
      }
    }
    /* segments of lanes on the same word: lanes run consecutive ranks, so words are ascending across the wavefront */
    const u64 wprev = shfl_up_u64 (w, 1);
    const bool head = valid && (lane == 0 || wprev != w);
    const u64 H = __builtin_amdgcn_ballot_w64 (hit), K = __builtin_amdgcn_ballot_w64 (kill);
    const u64 S = __builtin_amdgcn_ballot_w64 (head) | ~__builtin_amdgcn_ballot_w64 (valid);
    if (head) {
      const u64 after = lane == WAVE - 1 ? 0 : S & (~0ull << (lane + 1));
      const u64 seg = (after ? (after & (0ull - after)) - 1 : ~0ull) & (~0ull << lane);
      const u32 nh = (u32) __popcll (H & seg);
      if (nh) atomicAdd (&L.cnt[w], nh);
      if (K & seg) L.drop[w] = 1;
    }
    r += L.stride_r;
    w += L.stride_w;
    if (r >= L.n_var) {
      r -= L.n_var;
      w++;
    }
  }
  const u64 s = wave_sum ((u64) my_probes);
  if (lane == 0 && s) atomicAdd (probes, (unsigned long long) s);
}

/* keep[w] = the word survives the level: s < cutoff (unsigned), s = ~0 for a dropped word, else the count
 * (with subtract the sum of -1 terms, mod 2^32) */
__global__ __launch_bounds__ (MM_THREADS) void k_decide (const u32 *cnt, const u32 *drop, u64 n, u32 subtract, u32 cutoff, u32 *keep)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) {
    const u32 s = subtract ? (drop[i] ? ~0u : 0u - cnt[i]) : cnt[i];
    keep[i] = s < cutoff;
  }
}

}  // namespace
}  // namespace gt4

using namespace gt4;

/* ------------------------------------------------------------------ host side */

namespace {


/* Stable compaction of the n items with keep[i] != 0; returns the count in *kept (synchronises).  Scratch:
 * tile_cnt (u32) and tile_off (u64) with room for n / MM_TILE + 1 tiles. */
template <bool SRC_REC, bool DST_REC>
int compact (gt4hip_context *ctx, const u32 *keep, u64 n, u32 *tile_cnt, u64 *tile_off, const void *src_keys, const u32 *cnt, void *dst_keys,
             u32 *dst_cnt, u64 *kept, u64 *sum)
{
  *kept = 0;
  if (sum) *sum = 0;
  if (!n) return GT4HIP_OK;
  const u64 tiles = (n + MM_TILE - 1) / MM_TILE;
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 16, ctx->stream));
  const int grid = gt4hip_grid (ctx, tiles, 1);
  hipLaunchKernelGGL (k_tile_count, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, keep, n, tiles, tile_cnt);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, ctx->stream, tile_cnt, tiles, tile_off, ctx->scratch);
  gt4hip_grid_again (ctx, tiles, grid);
  hipLaunchKernelGGL ((k_scatter<SRC_REC, DST_REC>), dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, keep, n, tiles, tile_off, src_keys, cnt, dst_keys,
                      dst_cnt, sum ? ctx->scratch + 1 : (unsigned long long *) NULL);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, 16, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  *kept = ctx->scratch_host[0];
  if (sum) *sum = ctx->scratch_host[1];
  return GT4HIP_OK;
}

/* One table (diff1 or diff2) through the pre-pass and its levels. */
struct Side {
  int slot;             /* 2: diff1, 3: diff2 */
  const gt4hip_list *x; /* the list the table comes from */
  Index other;          /* pre-pass: exact keys of x in the other list */
  Index m, q;           /* levels */
  u64 *keys[2];         /* table, ping-pong */
  u32 *cnt[2];
  int cur;
  u64 n;                /* words in the table */
  u32 *keep, *val, *scnt, *drop, *tile_cnt;
  u64 *tile_off;
  bool done;            /* final records written */
};

int side_alloc (gt4hip_context *ctx, TempBlocks &blk, Side &s)
{
  const u64 n = s.x->n_words, tiles = n / MM_TILE + 2;
  int rc = GT4HIP_OK;
  if (!rc) rc = blk.get (ctx, n * 4, (void **) &s.keep);
  if (!rc) rc = blk.get (ctx, n * 4, (void **) &s.val);
  if (!rc) rc = blk.get (ctx, n * 4, (void **) &s.scnt);
  if (!rc) rc = blk.get (ctx, n * 4, (void **) &s.drop);
  if (!rc) rc = blk.get (ctx, tiles * 4, (void **) &s.tile_cnt);
  if (!rc) rc = blk.get (ctx, tiles * 8, (void **) &s.tile_off);
  for (int i = 0; i < 2 && !rc; i++) {
    rc = blk.get (ctx, n * 8, (void **) &s.keys[i]);
    if (!rc) rc = blk.get (ctx, n * 4, (void **) &s.cnt[i]);
  }
  return rc;
}

/* The level's work, (words, ranks), or 0 when it does not fit 64 bits */
u64 level_work (u64 n_words, u32 k, u32 c, u64 *n_var, u64 *pow3)
{
  u64 p = 1;
  for (u32 i = 0; i < c; i++) p *= 3;
  *pow3 = p;
  *n_var = BINOM_HOST.v[k][c] * p;
  if (*n_var && n_words > ~0ull / *n_var) return 0;
  return n_words * *n_var;
}

int run_level (gt4hip_context *ctx, Side &s, u32 k, u32 c, u32 cutoff, u32 subtract, uint64_t *probes)
{
  HIPCHK (ctx, hipMemsetAsync (s.scnt, 0, s.n * 4, ctx->stream));
  HIPCHK (ctx, hipMemsetAsync (s.drop, 0, s.n * 4, ctx->stream));
  if (c <= k) {
    Level L;
    memset (&L, 0, sizeof L);
    L.words = s.keys[s.cur];
    L.n_words = s.n;
    L.total = level_work (s.n, k, c, &L.n_var, &L.pow3);
    if (!L.total) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare_mismatch: level %u of %llu words has more than 2^64 variants", c,
                                      (unsigned long long) s.n);
    L.m = s.m;
    L.q = s.q;
    L.k = k;
    L.c = c;
    L.subtract = subtract;
    L.cutoff = cutoff;
    L.early = subtract || L.n_var <= 0xffffffffull;
    L.cnt = s.scnt;
    L.drop = s.drop;
    const int grid = gt4hip_grid (ctx, L.total, MM_THREADS);
    const u64 stride = (u64) grid * MM_THREADS;
    L.stride_w = stride / L.n_var;
    L.stride_r = stride % L.n_var;
    HIPCHK (ctx, hipMemsetAsync (ctx->scratch + 2, 0, 8, ctx->stream));
    const bool wide = !(L.n_var + stride < 0xffffffffull);
    ctx->mm_wide_levels += wide;
    ctx->mm_unskipped_levels += !L.early;
    if (!wide) hipLaunchKernelGGL (k_level<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, L, ctx->scratch + 2);
    else hipLaunchKernelGGL (k_level<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, L, ctx->scratch + 2);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host + 2, ctx->scratch + 2, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
    *probes += ctx->scratch_host[2];
  }
  /* above k there are no variants: s = 0 */
  hipLaunchKernelGGL (k_decide, dim3 (gt4hip_grid (ctx, s.n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, s.scnt, s.drop, s.n, subtract, cutoff, s.keep);
  HIPCHK (ctx, hipGetLastError ());
  return GT4HIP_OK;
}

}  // namespace

/* a HIP call of gt4hip_compare_mismatch: on failure, release what the call made and report */
#define MMCHK(call)                                                                                                   \
  do {                                                                                                                \
    const hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) return fail (gt4hip_fail (ctx, GT4HIP_EHIP, "%s failed: %s", #call, hipGetErrorString (e_))); \
  } while (0)

extern "C" int gt4hip_compare_mismatch (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, const gt4hip_mismatch_params *prm,
                                        gt4hip_compare_result *res)
{
  if (!ctx || !a || !b || !prm || !res) return GT4HIP_EINVAL;
  if (!prm->ops || (prm->ops & ~(uint32_t) (GT4HIP_OP_DIFF1 | GT4HIP_OP_DIFF2)))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare_mismatch: op bits 0x%x (only DIFF1 and DIFF2)", prm->ops);
  if (!prm->n_mismatch) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare_mismatch: n_mismatch must be at least 1");
  if (a->word_length != b->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ (%u != %u)", b->word_length, a->word_length);
  const u32 k = a->word_length;
  if (k < 1 || k > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_compare_mismatch: word length %u", k);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  const bool count_only = prm->count_only != 0;
  const u32 cutoff = prm->cutoff, subtract = prm->subtract ? 1u : 0u, nmm = prm->n_mismatch;

  /* the caller's output lists must hold the worst case, as in gt4hip_compare */
  for (int slot = 2; slot < 4; slot++) {
    if (!((prm->ops >> slot) & 1u) || count_only || !res->out[slot]) continue;
    const u64 need = slot == 2 ? a->n_words : b->n_words;
    if (res->out[slot]->capacity < need)
      return gt4hip_fail (ctx, GT4HIP_EINVAL, "output %d: capacity %llu < worst case %llu", slot, (unsigned long long) res->out[slot]->capacity,
                          (unsigned long long) need);
  }

  gt4hip_mismatch_stats st;
  memset (&st, 0, sizeof st);
  ctx->mm_wide_levels = ctx->mm_unskipped_levels = 0;
  TempBlocks blk;
  hipEvent_t e0 = NULL, e1 = NULL, e2 = NULL;
  gt4hip_list *made[4] = { NULL, NULL, NULL, NULL };
  u64 out_n[4] = { 0, 0, 0, 0 }, out_sum[4] = { 0, 0, 0, 0 };
  int rc = GT4HIP_OK;
  auto fail = [&] (int code) {
    for (int s = 0; s < 4; s++)
      if (made[s]) gt4hip_list_free (made[s]);
    if (e0) hipEventDestroy (e0);
    if (e1) hipEventDestroy (e1);
    if (e2) hipEventDestroy (e2);
    return code;
  };
  if (hipEventCreate (&e0) != hipSuccess || hipEventCreate (&e1) != hipSuccess || hipEventCreate (&e2) != hipSuccess)
    return fail (gt4hip_fail (ctx, GT4HIP_EHIP, "hipEventCreate failed"));

  Index ia, ib, none;
  memset (&none, 0, sizeof none);
  if ((rc = build_index (ctx, blk, a, &ia)) || (rc = build_index (ctx, blk, b, &ib))) return fail (rc);

  Side sides[2];
  int n_sides = 0;
  if (prm->ops & GT4HIP_OP_DIFF1) {
    Side &s = sides[n_sides++];
    memset (&s, 0, sizeof s);
    s.slot = 2;
    s.x = a;
    s.other = ib;
    s.m = ib;
    s.q = subtract ? ia : none;
  }
  if (prm->ops & GT4HIP_OP_DIFF2) {
    Side &s = sides[n_sides++];
    memset (&s, 0, sizeof s);
    s.slot = 3;
    s.x = b;
    s.other = ia;
    s.m = ia;
    s.q = none; /* the reference passes no second dictionary for diff2 (:1071): its lookups give 0 */
  }
  for (int i = 0; i < n_sides; i++)
    if ((rc = side_alloc (ctx, blk, sides[i]))) return fail (rc);

  /* ---- pre-pass */
  MMCHK (hipEventRecord (e0, ctx->stream));
  for (int i = 0; i < n_sides; i++) {
    Side &s = sides[i];
    const u64 nx = s.x->n_words;
    if (nx) {
      hipLaunchKernelGGL (k_prepass, dim3 (gt4hip_grid (ctx, nx, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) s.x->dev, nx, s.other,
                          (u32) (s.slot == 3), cutoff, subtract, s.keep, s.val);
      if (hipGetLastError () != hipSuccess) return fail (gt4hip_fail (ctx, GT4HIP_EHIP, "k_prepass launch failed"));
    }
    if ((rc = compact<true, false> (ctx, s.keep, nx, s.tile_cnt, s.tile_off, s.x->dev, s.val, s.keys[0], s.cnt[0], &s.n, NULL))) return fail (rc);
    s.cur = 0;
    st.prepass_words[s.slot - 2] = s.n;
    st.probes += nx;
  }
  MMCHK (hipEventRecord (e1, ctx->stream));
  MMCHK (hipEventSynchronize (e1));
  float ms = 0;
  if (hipEventElapsedTime (&ms, e0, e1) == hipSuccess) st.prepass_ms = ms;

  /* ---- levels c = 1..N; above k every level is the same (s = 0), so the last one stands for them all */
  const u32 last = nmm <= k ? nmm : k + 1;
  for (u32 c = 1; c <= last; c++) {
    const bool final_level = c == last;
    const u32 li = c - 1;
    MMCHK (hipEventRecord (e1, ctx->stream));
    for (int i = 0; i < n_sides; i++) {
      Side &s = sides[i];
      if (s.done) continue;
      if (li < GT4HIP_MM_MAX_LEVELS) st.level_words[li] += s.n;
      uint64_t probes = 0;
      if (s.n && (rc = run_level (ctx, s, k, c, cutoff, subtract, &probes))) return fail (rc);
      if (li < GT4HIP_MM_MAX_LEVELS) st.level_probes[li] += probes;
      st.probes += probes;
      if (!final_level) {
        u64 kept = 0;
        if ((rc = compact<false, false> (ctx, s.keep, s.n, s.tile_cnt, s.tile_off, s.keys[s.cur], s.cnt[s.cur], s.keys[s.cur ^ 1], s.cnt[s.cur ^ 1], &kept,
                                         NULL)))
          return fail (rc);
        s.cur ^= 1;
        s.n = kept;
        continue;
      }
      /* the output: survivors of the last level as packed records, in table order */
      u64 n_out = 0;
      if ((rc = compact<false, true> (ctx, s.keep, s.n, s.tile_cnt, s.tile_off, s.keys[s.cur], s.cnt[s.cur], NULL, NULL, &n_out, &out_sum[s.slot])))
        return fail (rc);
      out_n[s.slot] = n_out;
      if (!count_only) {
        gt4hip_list *o = res->out[s.slot];
        if (!o) {
          if ((rc = gt4hip_list_new (ctx, n_out, k, &made[s.slot]))) return fail (rc);
          o = made[s.slot];
        }
        if (n_out) {
          u64 again = 0;
          if ((rc = compact<false, true> (ctx, s.keep, s.n, s.tile_cnt, s.tile_off, s.keys[s.cur], s.cnt[s.cur], o->dev, NULL, &again, NULL)))
            return fail (rc);
        }
        o->n_words = n_out;
        o->word_length = k;
      }
      s.done = true;
    }
    MMCHK (hipEventRecord (e2, ctx->stream));
    MMCHK (hipEventSynchronize (e2));
    if (li < GT4HIP_MM_MAX_LEVELS && hipEventElapsedTime (&ms, e1, e2) == hipSuccess) st.level_ms[li] = ms;
  }
  st.n_levels = nmm < GT4HIP_MM_MAX_LEVELS ? nmm : GT4HIP_MM_MAX_LEVELS;
  if (hipEventElapsedTime (&ms, e0, e2) == hipSuccess) res->device_ms = ms;

  for (int slot = 0; slot < 4; slot++) {
    const bool on = (prm->ops >> slot) & 1u;
    res->n_words[slot] = on ? out_n[slot] : 0;
    res->total_count[slot] = on ? out_sum[slot] : 0;
    if (!on || count_only) res->out[slot] = NULL;
    else if (made[slot]) res->out[slot] = made[slot];
  }
  res->merge_kernel_ms = st.prepass_ms;
  res->merge_tiles = 0;
  ctx->mm_stats = st;
  hipEventDestroy (e0);
  hipEventDestroy (e1);
  hipEventDestroy (e2);
  return GT4HIP_OK;
}

extern "C" int gt4hip_mismatch_stats_get (gt4hip_context *ctx, gt4hip_mismatch_stats *stats)
{
  if (!ctx || !stats) return GT4HIP_EINVAL;
  *stats = ctx->mm_stats;
  return GT4HIP_OK;
}
