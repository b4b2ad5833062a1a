/*
 * gt4hip_subset.hip -- glistcompare --subset: the reference's selection sampling (subset (), src/glistcompare.c:719-787)
 * as a parallel fixed-point iteration.
 *
 * The reference walks the ITEMS of a list once (records for rand_unique and rand_weighted_unique, occurrences for rand)
 * and selects item i iff out_i > 0 and drand48 () <= ratio_i (out_i), out_i = SIZE - s_i, s_i = items selected before i.
 *   draws      v_i = X_(i+1) / 2^48 of the 48-bit LCG: every thread jumps to its first item through a table of the 48
 *              affine maps of 2^k steps, then steps;
 *   decisions  a tile of SUBSET_TILE items solves itself in LDS for a given carry-in (s at its first item): every thread
 *              walks its SUBSET_V consecutive items serially from its own carry-in, the carry-ins of the threads are
 *              iterated until a round changes none of them (thread 0's is the tile's, so at least one more thread is
 *              final after every round: at most SUBSET_THREADS + 1 rounds; rand_weighted_unique stages what its ratio
 *              reads per item in LDS for all of them).  Only the tiles' carry-ins are kept between
 *              the passes: a pass solves every tile from its carry-in, the tile sums are scanned (reduce-then-scan over
 *              separate launches), and the passes end when a scan gives back the carry-ins it was computed from.  Tile
 *              0's carry-in is 0, so after pass p the carry-ins of tiles 0..p are final: at most tiles + 1 passes;
 *   output     the last pass runs again with the final carry-ins and writes: the unique methods put record i where its
 *              s_i says; rand adds the selected occurrences of every record up, and a second scan over the records
 *              with a non-zero sum places them.
 * No workgroup waits for another one anywhere here.  The comparison evaluates the reference's C expressions in IEEE
 * double: no reciprocal, no contraction (the file is compiled without -ffast-math, and contraction is switched off).
 */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"

#include <string.h>

#pragma STDC FP_CONTRACT OFF

namespace gt4 {
namespace {

constexpr int SUBSET_THREADS = 256;
constexpr int SUBSET_V = 16; /* consecutive items of a thread */
static_assert ((u64) SUBSET_THREADS * SUBSET_V == GT4HIP_SUBSET_TILE, "the counter \"subset_tile\" names the tile of the kernels");
/* rand_weighted_unique: `in` and the count of a tile's items are staged in LDS, read once and in order, for all rounds.
 * Item j of thread t lies at j * STAGE_ROW + t: the walk (one j, consecutive t) and the fill (consecutive items: j runs
 * fastest, rows 4 apart) both spread over the banks. */
constexpr int STAGE_ROW = SUBSET_THREADS + 4;
constexpr int SCAN_THREADS = 256;
constexpr int SCAN_V = GT4HIP_SUBSET_SCAN_V;
constexpr u64 SCAN_TILE = (u64) SCAN_THREADS * SCAN_V;
static_assert (SCAN_TILE == 256u * GT4HIP_SUBSET_SCAN_V, "counter \"subset_scan_tile\" (gt4hip_api.hip)");

constexpr u64 LCG_A = 0x5DEECE66Dull, LCG_C = 0xBull, LCG_MASK = (1ull << 48) - 1;

/* x -> a[k] x + c[k] (mod 2^48) is 2^k steps of drand48's generator: affine maps compose */
struct LcgJump {
  u64 a[48], c[48];
  constexpr LcgJump () : a (), c ()
  {
    u64 A = LCG_A, C = LCG_C;
    for (int k = 0; k < 48; k++) {
      a[k] = A;
      c[k] = C;
      C = (A * C + C) & LCG_MASK;
      A = (A * A) & LCG_MASK;
    }
  }
};
constexpr LcgJump JUMP_HOST;
__constant__ LcgJump c_jump = LcgJump ();

/* the state `steps` steps behind x (the period is 2^48: only the low 48 bits of `steps` count) */
__host__ __device__ __forceinline__ u64 lcg_jump (const LcgJump &J, u64 x, u64 steps)
{
  for (int k = 0; k < 48; k++)
    if ((steps >> k) & 1u) x = (J.a[k] * x + J.c[k]) & LCG_MASK;
  return x;
}

/* ------------------------------------------------------------------ exclusive prefix sums, reduce-then-scan */

enum { SCAN_REC_COUNT, SCAN_U64, SCAN_U32_NONZERO };

/* element i of the scan's input: the count of record i / a 64-bit word / 1 where a 32-bit word is not 0 */
template <int MODE>
__device__ __forceinline__ u64 scan_load (const void *in, u64 i)
{
  if (MODE == SCAN_REC_COUNT) return ((const u32 *) in)[3 * i + 2];
  if (MODE == SCAN_U64) return ((const u64 *) in)[i];
  return ((const u32 *) in)[i] != 0;
}

/* sum over the block's threads; every thread of the block calls it, the result is the same in all of them */
__device__ __forceinline__ u64 block_sum_u64 (u64 v, u64 *s_wave, int tid)
{
  v = wave_sum (v);
  __syncthreads (); /* s_wave may still be read from the call before */
  if ((tid & (WAVE - 1)) == 0) s_wave[tid / WAVE] = v;
  __syncthreads ();
  u64 t = 0;
  for (int w = 0; w < SCAN_THREADS / WAVE; w++) t += s_wave[w];
  return t;
}

/* sums[b] = sum of the elements of scan tile b */
template <int MODE>
__global__ __launch_bounds__ (SCAN_THREADS) void k_subset_scan_reduce (const void *in, u64 n, u64 n_tiles, u64 *sums)
{
  __shared__ u64 s_wave[SCAN_THREADS / WAVE];
  const int tid = threadIdx.x;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 first = t * SCAN_TILE + (u64) tid * SCAN_V;
    u64 v = 0;
    for (int j = 0; j < SCAN_V; j++)
      if (first + j < n) v += scan_load<MODE> (in, first + j);
    v = block_sum_u64 (v, s_wave, tid);
    if (tid == 0) sums[t] = v;
  }
}

/* out[i] = offsets[tile of i] + sum of the tile's elements before i, i < n; out[n] = the sum of all n.  offsets: the
 * exclusive prefix sums of k_subset_scan_reduce's sums, or NULL where one tile holds everything.  n >= 1. */
template <int MODE>
__global__ __launch_bounds__ (SCAN_THREADS) void k_subset_scan_apply (const void *in, u64 n, u64 n_tiles, const u64 *offsets, u64 *out)
{
  __shared__ u64 s_wave[SCAN_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 first = t * SCAN_TILE + (u64) tid * SCAN_V;
    u64 v[SCAN_V], mine = 0;
    for (int j = 0; j < SCAN_V; j++) {
      v[j] = first + j < n ? scan_load<MODE> (in, first + j) : 0;
      mine += v[j];
    }
    const u64 inc = wave_inclusive_scan (mine, lane);
    __syncthreads (); /* s_wave: the tile before */
    if (lane == WAVE - 1) s_wave[wave] = inc;
    __syncthreads ();
    u64 run = (offsets ? offsets[t] : 0) + inc - mine;
    for (int w = 0; w < wave; w++) run += s_wave[w];
    for (int j = 0; j < SCAN_V; j++) {
      if (first + j < n) out[first + j] = run;
      run += v[j];
      if (first + j == n - 1) out[n] = run;
    }
  }
}

/* ------------------------------------------------------------------ the decisions */

struct SubsetJob {
  const u32 *rec;    /* the list, n records */
  u64 n;
  const u64 *prefix; /* exclusive prefix sums of the counts, n + 1 entries; NULL for rand_unique, which reads none */
  u64 items;         /* records (the unique methods) or occurrences (rand) */
  u64 total_in;      /* the reference's `in` at item 0: num_words (rand_unique) or sum_counts */
  u64 size;          /* SIZE */
  u64 x0;            /* X0 */
  u64 tiles;
};

struct SubsetEmit {
  u32 *out_rec;      /* the unique methods: the output records */
  u64 out_capacity;
  u32 *selected;     /* rand: selected occurrences per record, zeroed */
  u64 *total_count;  /* the unique methods: sum of the selected records' counts, zeroed */
};

enum { EMIT_NONE, EMIT_RECORDS, EMIT_OCCURRENCES };

/* The reference's loop over items [b, e) from s selected before b and the generator's state x in front of b's draw.
 * WEIGHTED: rand_weighted_unique, val <= (double) count * out / in with in = sum_counts - counts before; else
 * val <= (double) out / in with in = total_in - item (rand_unique: records left; rand: occurrences left).
 * st_in, st_count (WEIGHTED): the thread's column of the tile's stage.  Returns the number selected. */
template <bool WEIGHTED, int EMIT>
__device__ __forceinline__ u32 subset_walk (const SubsetJob &J, const SubsetEmit &E, u64 b, u64 e, u64 x, u64 s, u64 *count_sum, const u64 *st_in,
                                            const u32 *st_count)
{
  u32 cnt = 0;
  /* rand: the record that owns item b is the last one whose prefix is <= b; records of count 0 own nothing */
  u64 r = 0, r_end = 0;
  u32 r_sel = 0;
  if (EMIT == EMIT_OCCURRENCES && b < e) {
    u64 lo = 0, hi = J.n; /* first j in [1, n] with prefix[j] > b: prefix[0] = 0 <= b < items = prefix[n] */
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (J.prefix[mid + 1] > b) hi = mid;
      else lo = mid + 1;
    }
    r = lo < J.n ? lo : J.n - 1;
    r_end = J.prefix[r + 1];
  }
  for (u64 i = b; i < e; i++) {
    x = (LCG_A * x + LCG_C) & LCG_MASK;
    if (EMIT == EMIT_OCCURRENCES) {
      while (i >= r_end && r + 1 < J.n) {
        if (r_sel) atomicAdd (&E.selected[r], r_sel);
        r_sel = 0;
        r += 1;
        r_end = J.prefix[r + 1];
      }
    }
    const u64 have = s + cnt;
    if (have >= J.size) continue; /* out == 0: the reference has stopped */
    const double val = (double) x * 0x1p-48;
    const double out = (double) (J.size - have);
    double ratio;
    u32 c = 0;
    if (WEIGHTED) {
      c = st_count[(i - b) * STAGE_ROW];
      const u64 in = st_in[(i - b) * STAGE_ROW];
      ratio = ((double) c * out) / (double) in;
    } else {
      const u64 in = J.total_in - i;
      ratio = out / (double) in;
    }
    if (!(val <= ratio)) continue;
    if (EMIT == EMIT_RECORDS && have < E.out_capacity) {
      const u32 *src = J.rec + 3 * i;
      u32 *dst = E.out_rec + 3 * have;
      if (!WEIGHTED) c = src[2];
      dst[0] = src[0];
      dst[1] = src[1];
      dst[2] = c;
      *count_sum += c;
    }
    if (EMIT == EMIT_OCCURRENCES) r_sel += 1;
    cnt += 1;
  }
  if (EMIT == EMIT_OCCURRENCES && r_sel) atomicAdd (&E.selected[r], r_sel);
  return cnt;
}

/* One pass: every tile solved from its carry-in; tile_sum[t] = items selected in tile t.  error[0] is set where a tile's
 * rounds pass their proven bound.  EMIT: the carry-ins are final, and the tile writes what it selected. */
template <bool WEIGHTED, int EMIT>
__global__ __launch_bounds__ (SUBSET_THREADS) void k_subset_pass (SubsetJob J, const u64 *carry, u64 *tile_sum, SubsetEmit E, u64 *error)
{
  __shared__ u32 s_wave[SUBSET_THREADS / WAVE];
  __shared__ u64 s_sum[SCAN_THREADS / WAVE];
  __shared__ u64 s_in[WEIGHTED ? SUBSET_V * STAGE_ROW : 1];
  __shared__ u32 s_count[WEIGHTED ? SUBSET_V * STAGE_ROW : 1];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  for (u64 tile = blockIdx.x; tile < J.tiles; tile += gridDim.x) {
    if (WEIGHTED) {
      __syncthreads (); /* the tile before has done its last walk */
      for (int r = 0; r < SUBSET_V; r++) {
        const u32 l = (u32) r * SUBSET_THREADS + tid;
        const u64 item = tile * GT4HIP_SUBSET_TILE + l;
        if (item < J.items) {
          const u32 at = (l % SUBSET_V) * STAGE_ROW + l / SUBSET_V;
          s_in[at] = J.total_in - J.prefix[item];
          s_count[at] = J.rec[3 * item + 2];
        }
      }
      __syncthreads ();
    }
    const u64 first = tile * GT4HIP_SUBSET_TILE + (u64) tid * SUBSET_V;
    const u64 b = first < J.items ? first : J.items, e = first + SUBSET_V < J.items ? first + SUBSET_V : J.items;
    const u64 s_tile = carry[tile];
    const u64 x = lcg_jump (c_jump, J.x0, b);
    u32 off = 0, total = 0; /* selected in the tile before this thread's items, as the round before saw it */
    for (int round = 0;; round++) {
      const u32 cnt = subset_walk<WEIGHTED, EMIT_NONE> (J, E, b, e, x, s_tile + off, NULL, s_in + tid, s_count + tid);
      const u32 inc = dpp_inclusive_scan_u32 (cnt);
      if (lane == WAVE - 1) s_wave[wave] = inc;
      __syncthreads ();
      u32 before = inc - cnt;
      total = 0;
      for (int w = 0; w < SUBSET_THREADS / WAVE; w++) {
        const u32 t = s_wave[w];
        if (w < wave) before += t;
        total += t;
      }
      const int changed = before != off;
      off = before;
      if (!__syncthreads_or (changed)) break; /* (also: s_wave is free again) */
      if (round > SUBSET_THREADS + 1) {
        if (tid == 0) error[0] = 1;
        break;
      }
    }
    if (tid == 0) tile_sum[tile] = total;
    if (EMIT != EMIT_NONE) {
      u64 count_sum = 0;
      subset_walk<WEIGHTED, EMIT> (J, E, b, e, x, s_tile + off, &count_sum, s_in + tid, s_count + tid);
      if (EMIT == EMIT_RECORDS) {
        count_sum = block_sum_u64 (count_sum, s_sum, tid);
        if (tid == 0 && count_sum) atomicAdd (E.total_count, count_sum);
      }
    }
  }
}

/* the carry-ins the first pass starts from: what a walk that selects in proportion would have reached.  Any start leads
 * to the same fixed point; tile 0's is 0, which is final. */
__global__ void k_subset_guess (SubsetJob J, int weighted, u64 *carry)
{
  for (u64 t = (u64) blockIdx.x * blockDim.x + threadIdx.x; t < J.tiles; t += (u64) gridDim.x * blockDim.x) {
    const u64 before = weighted ? J.prefix[t * GT4HIP_SUBSET_TILE] : t * GT4HIP_SUBSET_TILE;
    u64 g = J.total_in ? (u64) ((unsigned __int128) J.size * before / J.total_in) : 0;
    carry[t] = g < J.size ? g : J.size;
  }
}

/* word[0] += 1 per block that holds a tile whose carry-in the scan changed; word[1] = the items selected in all tiles */
__global__ __launch_bounds__ (SCAN_THREADS) void k_subset_changed (const u64 *cur, const u64 *nxt, u64 tiles, u64 *word)
{
  int diff = 0;
  for (u64 t = (u64) blockIdx.x * blockDim.x + threadIdx.x; t < tiles; t += (u64) gridDim.x * blockDim.x) diff |= cur[t] != nxt[t];
  if (__syncthreads_or (diff) && threadIdx.x == 0) atomicAdd (&word[0], 1ull);
  if (blockIdx.x == 0 && threadIdx.x == 0) word[1] = nxt[tiles];
}

/* rand: record i with selected[i] != 0 goes to out[pos[i]] with that count */
__global__ void k_subset_compact (const u32 *rec, const u32 *selected, const u64 *pos, u64 n, u32 *out_rec, u64 out_capacity)
{
  for (u64 i = (u64) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64) gridDim.x * blockDim.x) {
    const u32 c = selected[i];
    const u64 p = pos[i];
    if (!c || p >= out_capacity) continue;
    out_rec[3 * p] = rec[3 * i];
    out_rec[3 * p + 1] = rec[3 * i + 1];
    out_rec[3 * p + 2] = c;
  }
}

/* ------------------------------------------------------------------ host */

struct Timer {
  hipEvent_t e0 = NULL, e1 = NULL;
  ~Timer ()
  {
    if (e0) hipEventDestroy (e0);
    if (e1) hipEventDestroy (e1);
  }
};

/* one level of a scan: the sums of its tiles and their prefix sums, sized once for every pass */
struct ScanLevel {
  u64 n, n_tiles;
  u64 *sums, *offsets; /* n_tiles and n_tiles + 1 entries; NULL where n_tiles == 1 */
};

/* the levels of a scan over n >= 1 elements: level 0 is the input itself, level l + 1 the tile sums of level l */
int scan_plan (gt4hip_context *ctx, u64 n, TempBlocks &blk, std::vector<ScanLevel> &levels)
{
  levels.clear ();
  for (;;) {
    ScanLevel L = { n, (n + SCAN_TILE - 1) / SCAN_TILE, NULL, NULL };
    if (L.n_tiles > 1) {
      int rc;
      if ((rc = blk.get (ctx, L.n_tiles * 8, (void **) &L.sums)) || (rc = blk.get (ctx, (L.n_tiles + 1) * 8, (void **) &L.offsets))) return rc;
    }
    levels.push_back (L);
    if (L.n_tiles <= 1) return GT4HIP_OK;
    n = L.n_tiles;
  }
}

template <int MODE>
void scan_level (gt4hip_context *ctx, const ScanLevel &L, const void *in, u64 *out, bool reduce)
{
  const int grid = gt4hip_grid (ctx, L.n_tiles);
  if (reduce) hipLaunchKernelGGL (k_subset_scan_reduce<MODE>, dim3 (grid), dim3 (SCAN_THREADS), 0, ctx->stream, in, L.n, L.n_tiles, L.sums);
  else hipLaunchKernelGGL (k_subset_scan_apply<MODE>, dim3 (grid), dim3 (SCAN_THREADS), 0, ctx->stream, in, L.n, L.n_tiles, (const u64 *) L.offsets, out);
}

/* out[0 .. n] = the exclusive prefix sums of the n elements of `in` and their total: the tile sums of every level, bottom
 * up, then the prefix sums top down */
template <int MODE>
hipError_t scan_run (gt4hip_context *ctx, const std::vector<ScanLevel> &levels, const void *in, u64 *out)
{
  const size_t top = levels.size () - 1;
  for (size_t l = 0; l < top; l++) {
    if (l == 0) scan_level<MODE> (ctx, levels[0], in, NULL, true);
    else scan_level<SCAN_U64> (ctx, levels[l], levels[l - 1].sums, NULL, true);
  }
  for (size_t l = top; l > 0; l--) scan_level<SCAN_U64> (ctx, levels[l], levels[l - 1].sums, levels[l - 1].offsets, false);
  scan_level<MODE> (ctx, levels[0], in, out, false);
  return hipGetLastError ();
}

const char *const METHOD_NAMES[3] = { "rand", "rand_unique", "rand_weighted_unique" };

template <int EMIT>
void launch_pass (gt4hip_context *ctx, bool weighted, const SubsetJob &J, const u64 *carry, u64 *tile_sum, const SubsetEmit &E, u64 *error)
{
  const int grid = gt4hip_grid (ctx, J.tiles);
  if (weighted && EMIT != EMIT_OCCURRENCES) hipLaunchKernelGGL ((k_subset_pass<true, EMIT == EMIT_OCCURRENCES ? EMIT_NONE : EMIT>), dim3 (grid), dim3 (SUBSET_THREADS), 0, ctx->stream, J, carry, tile_sum, E, error);
  else hipLaunchKernelGGL ((k_subset_pass<false, EMIT>), dim3 (grid), dim3 (SUBSET_THREADS), 0, ctx->stream, J, carry, tile_sum, E, error);
}

int empty_result (gt4hip_context *ctx, uint32_t word_length, gt4hip_list **out, uint64_t *n_words, uint64_t *total_count)
{
  const int rc = gt4hip_list_new (ctx, 0, word_length, out);
  if (rc) return rc;
  *n_words = *total_count = 0;
  return GT4HIP_OK;
}

}  // namespace
}  // namespace gt4

using namespace gt4;

extern "C" uint64_t gt4hip_subset_state_at (uint64_t state48, uint64_t position)
{
  return lcg_jump (JUMP_HOST, state48 & LCG_MASK, position);
}

extern "C" int gt4hip_list_subset (gt4hip_context *ctx, const gt4hip_list *list, const gt4hip_subset_params *prm, gt4hip_list **out,
                                   uint64_t *n_words, uint64_t *total_count)
{
  if (!ctx || !list || !prm || !out || !n_words || !total_count) return GT4HIP_EINVAL;
  *out = NULL;
  if (prm->method > GT4HIP_SUBSET_RAND_WEIGHTED_UNIQUE) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_list_subset: unknown method %u", prm->method);
  ctx->subset_passes = 0;
  ctx->subset_ms = 0;
  const char *const name = METHOD_NAMES[prm->method];
  const bool weighted = prm->method == GT4HIP_SUBSET_RAND_WEIGHTED_UNIQUE, occurrences = prm->method == GT4HIP_SUBSET_RAND;
  if (!list->n_words || !prm->size) return empty_result (ctx, list->word_length, out, n_words, total_count);
  HIPCHK (ctx, hipSetDevice (ctx->device));

  TempBlocks blk;
  Timer tm;
  std::vector<ScanLevel> levels;
  int rc;
  HIPCHK (ctx, hipEventCreate (&tm.e0));
  HIPCHK (ctx, hipEventCreate (&tm.e1));
  HIPCHK (ctx, hipEventRecord (tm.e0, ctx->stream));

  SubsetJob J;
  memset (&J, 0, sizeof J);
  J.rec = (const u32 *) list->dev;
  J.n = list->n_words;
  J.size = prm->size;
  J.x0 = prm->state48 & LCG_MASK;
  J.items = J.total_in = J.n;
  /* the prefix sums of the counts, once: `in` of rand_weighted_unique, the item -> record map of rand */
  if (prm->method != GT4HIP_SUBSET_RAND_UNIQUE) {
    u64 *prefix = NULL;
    if ((rc = blk.get (ctx, (J.n + 1) * 8, (void **) &prefix)) || (rc = scan_plan (ctx, J.n, blk, levels))) return rc;
    HIPCHK (ctx, scan_run<SCAN_REC_COUNT> (ctx, levels, J.rec, prefix));
    if ((rc = gt4hip_read_back (ctx, ctx->scratch_host, prefix + J.n, 8, "gt4hip_list_subset: reading the sum of the counts back failed"))) return rc;
    J.prefix = prefix;
    J.total_in = ctx->scratch_host[0];
    if (occurrences) J.items = J.total_in;
  }
  if (!J.items)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_list_subset: %s %llu: the list holds no occurrence to select from (every count is 0)", name,
                        (unsigned long long) J.size);
  J.tiles = (J.items + GT4HIP_SUBSET_TILE - 1) / GT4HIP_SUBSET_TILE;

  /* what is kept between the passes: one carry-in per tile (twice: the one a pass read and the one its scan gives) */
  u64 *carry[2] = { NULL, NULL }, *tile_sum = NULL;
  if ((rc = blk.get (ctx, (J.tiles + 1) * 8, (void **) &carry[0])) || (rc = blk.get (ctx, (J.tiles + 1) * 8, (void **) &carry[1])) ||
      (rc = blk.get (ctx, J.tiles * 8, (void **) &tile_sum)) || (rc = scan_plan (ctx, J.tiles, blk, levels)))
    return rc;
  SubsetEmit E;
  memset (&E, 0, sizeof E);
  u64 *const word = ctx->scratch; /* [0] carry-ins changed, [1] items selected, [2] a tile passed its bound, [3] total_count */

  hipLaunchKernelGGL (k_subset_guess, dim3 (gt4hip_grid (ctx, (J.tiles + 255) / 256)), dim3 (256), 0, ctx->stream, J, weighted ? 1 : 0, carry[0]);
  HIPCHK (ctx, hipGetLastError ());
  u64 selected = 0;
  for (u64 pass = 1;; pass++) {
    /* after pass p the carry-ins of tiles 0 .. p are final: pass tiles + 1 cannot change any */
    if (pass > J.tiles + 1)
      return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "gt4hip_list_subset: %s %llu: the carry-ins of %llu tiles still changed in pass %llu", name,
                          (unsigned long long) J.size, (unsigned long long) J.tiles, (unsigned long long) (pass - 1));
    HIPCHK (ctx, hipMemsetAsync (word, 0, 32, ctx->stream));
    launch_pass<EMIT_NONE> (ctx, weighted, J, carry[0], tile_sum, E, word + 2);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, scan_run<SCAN_U64> (ctx, levels, tile_sum, carry[1]));
    hipLaunchKernelGGL (k_subset_changed, dim3 (gt4hip_grid (ctx, (J.tiles + SCAN_THREADS - 1) / SCAN_THREADS)), dim3 (SCAN_THREADS), 0, ctx->stream,
                        (const u64 *) carry[0], (const u64 *) carry[1], J.tiles, word);
    HIPCHK (ctx, hipGetLastError ());
    if ((rc = gt4hip_read_scratch (ctx, 3))) return rc;
    ctx->subset_passes = pass;
    if (ctx->scratch_host[2]) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "gt4hip_list_subset: a tile's rounds passed their bound in pass %llu", (unsigned long long) pass);
    std::swap (carry[0], carry[1]);
    if (!ctx->scratch_host[0]) {
      selected = ctx->scratch_host[1];
      break;
    }
  }
  /* the walk fell short behind the last item: the reference does not terminate there, or writes the last record twice */
  if (selected < J.size)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_list_subset: %s %llu: only %llu of %llu could be selected from the %llu %s of the list",
                        name, (unsigned long long) J.size, (unsigned long long) selected, (unsigned long long) J.size, (unsigned long long) J.items,
                        occurrences ? "occurrences" : "records");
  if (selected > J.size) return gt4hip_fail (ctx, GT4HIP_EINTERNAL, "gt4hip_list_subset: %llu selected of %llu", (unsigned long long) selected, (unsigned long long) J.size);

  /* the last pass again, writing */
  TempLists made;
  gt4hip_list *res = NULL;
  HIPCHK (ctx, hipMemsetAsync (word, 0, 32, ctx->stream));
  if (!occurrences) {
    if ((rc = gt4hip_list_new (ctx, selected, list->word_length, &res))) return rc;
    made.adopt (res);
    E.out_rec = (u32 *) res->dev;
    E.out_capacity = selected;
    E.total_count = word + 3;
    launch_pass<EMIT_RECORDS> (ctx, weighted, J, carry[0], tile_sum, E, word + 2);
    HIPCHK (ctx, hipGetLastError ());
    if ((rc = gt4hip_read_scratch (ctx, 4))) return rc;
    *n_words = selected;
    *total_count = ctx->scratch_host[3];
  } else {
    u32 *sel = NULL;
    u64 *pos = NULL;
    if ((rc = blk.get (ctx, J.n * 4, (void **) &sel)) || (rc = blk.get (ctx, (J.n + 1) * 8, (void **) &pos)) || (rc = scan_plan (ctx, J.n, blk, levels))) return rc;
    HIPCHK (ctx, hipMemsetAsync (sel, 0, J.n * 4, ctx->stream));
    E.selected = sel;
    launch_pass<EMIT_OCCURRENCES> (ctx, false, J, carry[0], tile_sum, E, word + 2);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, scan_run<SCAN_U32_NONZERO> (ctx, levels, sel, pos));
    if ((rc = gt4hip_read_back (ctx, ctx->scratch_host, pos + J.n, 8, "gt4hip_list_subset: reading the number of records back failed"))) return rc;
    const u64 kept = ctx->scratch_host[0];
    if ((rc = gt4hip_list_new (ctx, kept, list->word_length, &res))) return rc;
    made.adopt (res);
    hipLaunchKernelGGL (k_subset_compact, dim3 (gt4hip_grid (ctx, (J.n + 255) / 256)), dim3 (256), 0, ctx->stream, J.rec, (const u32 *) sel, (const u64 *) pos, J.n,
                        (u32 *) res->dev, kept);
    HIPCHK (ctx, hipGetLastError ());
    *n_words = kept;
    *total_count = selected;
  }
  HIPCHK (ctx, hipEventRecord (tm.e1, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  float ms = 0;
  if (hipEventElapsedTime (&ms, tm.e0, tm.e1) == hipSuccess) ctx->subset_ms = ms;
  made.release ();
  *out = res;
  return GT4HIP_OK;
}
