/* gt4hip_index.h -- what the mismatch difference (gt4hip_mismatch.hip) and the query entry points (gt4hip_query.hip)
 * share: the bucket index over a packed list and its lookup, the reverse complement and the canonical form of a word, the
 * enumeration of substitution variants by rank, the steps of the stable compaction over tiles (a tile's total, the scan
 * of the totals, a kept item's place in its round) with the count and scan kernels, and the host code that
 * sizes and builds an index.  Include after gt4hip_device.h and gt4hip_host.h; everything here has internal linkage, every file that
 * includes it gets its own copy. */
#ifndef GT4HIP_INDEX_H
#define GT4HIP_INDEX_H

namespace gt4 {
namespace {

constexpr int MM_THREADS = 256;
constexpr int MM_ROUNDS = 8;                        /* compaction: items per thread and tile */
constexpr u64 MM_TILE = (u64) MM_THREADS * MM_ROUNDS; /* items per compaction tile */
static_assert (MM_THREADS == GT4HIP_MM_THREADS && MM_ROUNDS == GT4HIP_MM_ROUNDS, "counters \"mm_threads\" and \"mm_tile\" (gt4hip_host.h)");
constexpr u32 MM_MAX_INDEX_BITS = 22;               /* 32 MiB of offsets at most: well inside the Infinity Cache */

/* C(n, r) for n, r <= 32 */
struct Binomials {
  u64 v[33][33];
  constexpr Binomials () : v ()
  {
    for (int n = 0; n <= 32; n++) {
      v[n][0] = 1;
      for (int r = 1; r <= n; r++) v[n][r] = v[n - 1][r - 1] + (r <= n - 1 ? v[n - 1][r] : 0);
    }
  }
};
constexpr Binomials BINOM_HOST;
__constant__ Binomials c_binom = Binomials ();

/* A list and its bucket index.  n == 0 (an empty list, or no list at all) holds nothing. */
struct Index {
  const u32 *rec;
  u64 n;
  const u64 *off; /* nb + 1 entries */
  u64 nb;         /* buckets, 2^b */
  u32 shift;      /* prefix = key >> shift, clamped to nb - 1 */
};

__device__ __forceinline__ u64 bucket_of (u64 key, u32 shift, u64 nb)
{
  const u64 p = key >> shift;
  return p < nb ? p : nb - 1;
}

/* record index of `key` in the list, or ~0 */
__device__ __forceinline__ u64 find (const Index &ix, u64 key)
{
  if (ix.n == 0) return ~0ull;
  const u64 p = bucket_of (key, ix.shift, ix.nb);
  u64 lo = ix.off[p], hi = ix.off[p + 1];
  if (hi > ix.n) hi = ix.n; /* keys out of order leave the index meaningless, never out of bounds */
  while (lo < hi) {
    const u64 mid = (lo + hi) >> 1;
    const u64 k = load_key (ix.rec, mid);
    if (k < key) lo = mid + 1;
    else if (k > key) hi = mid;
    else return mid;
  }
  return ~0ull;
}

/* get_reverse_complement (reference src/sequence.c:65-79) by bit reversal: complement, swap the two bits of
 * every base so that the reversal keeps them in order, reverse, drop the 64 - 2k bits that came from above the word */
__device__ __forceinline__ u64 revcomp (u64 w, u32 k)
{
  u64 x = ~w;
  x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
  return __builtin_bitreverse64 (x) >> (64u - 2u * k);
}

/* the word as a list holds it: the smaller of itself and its reverse complement (canonize == 0: itself) */
__device__ __forceinline__ u64 canonical (u64 w, u32 k, u32 canonize)
{
  if (!canonize) return w;
  const u64 rc = revcomp (w, k);
  return rc < w ? rc : w;
}

/* offsets[s] for s in (prefix (i - 1), prefix (i)] is i; the slots after the last record's prefix are n */
__global__ __launch_bounds__ (MM_THREADS) void k_index_build (const u32 *rec, u64 n, u32 shift, u64 nb, u64 *off)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i <= n; i += (u64) gridDim.x * MM_THREADS) {
    const u64 first = i ? bucket_of (load_key (rec, i - 1), shift, nb) + 1 : 0;
    const u64 last = i < n ? bucket_of (load_key (rec, i), shift, nb) : nb;
    for (u64 s = first; s <= last; s++) off[s] = i;
  }
}

/* ------------------------------------------------------------------ stable compaction */

/* Tile t covers items [t * MM_TILE, (t + 1) * MM_TILE); round r of it items t * MM_TILE + r * MM_THREADS + thread.  A
 * count pass adds up what every tile keeps (tile_total), one scan turns the counts into offsets (k_tile_scan), a fill pass
 * gives every kept item of a round its place behind the tile's offset (round_place).  All three are a workgroup's: every
 * thread of it calls them, the same number of times. */
constexpr int MM_WAVES = MM_THREADS / WAVE;

__device__ __forceinline__ u32 wave_total (u32 v) { return dpp_wave_sum_u32 (v); }
__device__ __forceinline__ u64 wave_total (u64 v) { return wave_sum (v); }

/* A tile's total in two steps with a barrier between them: every wavefront posts its sum to its entry of `part` (MM_WAVES
 * entries of LDS), then one thread adds the entries. */
template <class T>
__device__ __forceinline__ void wave_post (T mine, T *part)
{
  mine = wave_total (mine);
  if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = mine;
}
template <class T>
__device__ __forceinline__ T posted (const T *part)
{
  T s = 0;
  for (int w = 0; w < MM_WAVES; w++) s += part[w];
  return s;
}

/* *out = the sum of every thread's `mine`, stored by thread 0; part is free again on return.  Two barriers a call, and no
 * more for a second quantity with a row of its own. */
template <class T>
__device__ __forceinline__ void tile_total (T mine, T *part, T *out)
{
  wave_post (mine, part);
  __syncthreads ();
  if (threadIdx.x == 0) *out = posted (part);
  __syncthreads ();
}
template <class T, class U>
__device__ __forceinline__ void tile_total (T mine, T *part, T *out, U mine2, U *part2, U *out2)
{
  wave_post (mine, part);
  wave_post (mine2, part2);
  __syncthreads ();
  if (threadIdx.x == 0) {
    *out = posted (part);
    *out2 = posted (part2);
  }
  __syncthreads ();
}

/* what the wavefronts before this thread's posted to `part`, and in *round what all of them did */
template <class T>
__device__ __forceinline__ T waves_before (const T *part, T *round)
{
  const int wv = threadIdx.x / WAVE;
  T before = 0, all = 0;
  for (int w = 0; w < MM_WAVES; w++) {
    before += w < wv ? part[w] : 0;
    all += part[w];
  }
  *round = all;
  return before;
}

/* One round of a fill pass: this thread's place among the round's kept items, in thread order, and their number in
 * *round.  part: MM_WAVES entries of LDS.  One barrier inside; part is read after it, so the caller ends the round with a
 * barrier of its own before the next round writes it again. */
__device__ __forceinline__ u32 round_place (bool keep, u32 *part, u32 *round)
{
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 m = __builtin_amdgcn_ballot_w64 (keep);
  if (lane == 0) part[threadIdx.x / WAVE] = (u32) __popcll (m);
  __syncthreads ();
  return waves_before (part, round) + (u32) __popcll (m & ((1ull << lane) - 1));
}

/* A quantity per item beside it (the sum of `v` over the threads before this one), in a row of LDS of its own and inside
 * the same two barriers: wave_offset BEFORE round_place gives the part of the sum that lies in this wavefront and posts the
 * wavefront's total, waves_before (part, &round) AFTER round_place adds the wavefronts before it. */
__device__ __forceinline__ u64 wave_offset (u64 v, u64 *part)
{
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 incl = wave_inclusive_scan (v, lane);
  if (lane == WAVE - 1) part[threadIdx.x / WAVE] = incl;
  return incl - v;
}

[[maybe_unused]] __global__ __launch_bounds__ (MM_THREADS) void k_tile_count (const u32 *keep, u64 n, u64 n_tiles, u32 *tile_cnt)
{
  __shared__ u32 part[MM_WAVES];
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    u32 c = 0;
    for (int r = 0; r < MM_ROUNDS; r++) {
      const u64 i = t * MM_TILE + (u64) r * MM_THREADS + threadIdx.x;
      c += i < n && keep[i];
    }
    /* (tile_total, open-coded: with this kernel and k_scatter on the helpers the -mm pre-pass measured 1.5 % slower
     * than with this text, profiles/HISTORY.md) */
    c = dpp_wave_sum_u32 (c);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = c;
    __syncthreads ();
    if (threadIdx.x == 0) {
      u32 s = 0;
      for (int w = 0; w < MM_WAVES; w++) s += part[w];
      tile_cnt[t] = s;
    }
    __syncthreads ();
  }
}

/* exclusive scan of the tile counts, widened to 64 bits, total in *total (k_tile_scan64 of gt4hip_query.hip: 64-bit counts) */
[[maybe_unused]] __global__ __launch_bounds__ (1024) void k_tile_scan (const u32 *tile_cnt, u64 n_tiles, u64 *tile_off, unsigned long long *total)
{
  workgroup_scan<1> ({tile_cnt}, {tile_off}, n_tiles, total);
}

/* Variant `r` of the c-substitution variants of a k-base word: r = combination * 3^c + substitutions, the
 * combination (positions p_c > .. > p_1) unranked in the combinatorial number system, the substitutions as base-3
 * digits (XOR masks 1, 2, 3 at bits 2p, gt4_word_table_generate_mismatches, src/word-table.c:361). */
template <bool WIDE>
__device__ __forceinline__ u64 variant_mask (u64 r, u64 pow3, u32 k, u32 c)
{
  u64 comb, sub;
  if (WIDE) {
    comb = r / pow3;
    sub = r - comb * pow3;
  } else {
    const u32 q = (u32) r / (u32) pow3;
    comb = q;
    sub = (u32) r - q * (u32) pow3;
  }
  u64 mask = 0;
  u32 x = k;
  for (u32 j = c; j >= 1; j--) {
    x--;
    while (c_binom.v[x][j] > comb) x--;
    comb -= c_binom.v[x][j];
    const u32 d = (u32) (sub % 3u) + 1u;
    sub /= 3u;
    mask |= (u64) d << (2u * x);
  }
  return mask;
}

}  // namespace
}  // namespace gt4

namespace {

using namespace gt4;

/* the geometry of a list's index: 2^b buckets, b = log2 (n) - 3 (windows of ~8 records), at most MM_MAX_INDEX_BITS */
void size_index (const gt4hip_list *l, Index *ix)
{
  const u32 k = l->word_length;
  u32 b = 0;
  for (u64 n = l->n_words; n > 1; n >>= 1) b++; /* floor (log2 n) */
  b = b > 3 ? b - 3 : 1;
  if (b > MM_MAX_INDEX_BITS) b = MM_MAX_INDEX_BITS;
  if (b > 2 * k) b = 2 * k;
  ix->rec = (const u32 *) l->dev;
  ix->n = l->n_words;
  ix->nb = 1ull << b;
  ix->shift = 2 * k - b;
  ix->off = NULL;
}

/* fills `off` (nb + 1 entries of device memory) and makes it the index's table */
int fill_index (gt4hip_context *ctx, Index *ix, void *off)
{
  ix->off = (const u64 *) off;
  hipLaunchKernelGGL (k_index_build, dim3 (gt4hip_grid (ctx, ix->n + 1, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, ix->rec, ix->n, ix->shift, ix->nb,
                      (u64 *) off);
  HIPCHK (ctx, hipGetLastError ());
  return GT4HIP_OK;
}

[[maybe_unused]] int build_index (gt4hip_context *ctx, TempBlocks &blk, const gt4hip_list *l, Index *ix)
{
  size_index (l, ix);
  void *off = NULL;
  const int rc = blk.get (ctx, (ix->nb + 1) * 8, &off);
  if (rc) return rc;
  return fill_index (ctx, ix, off);
}

}  // namespace

#endif
