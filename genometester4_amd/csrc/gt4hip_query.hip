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
 * and writes every hit to its place (k_query_hits<FILL, LOC>, on the compaction steps of gt4hip_index.h).  Nothing of
 * the size of the variant space is ever stored.
 *
 * --locations (gt4hip_location_index, gt4hip_query_lookup_locations) returns the hits with every place they occur in a
 * resident GT4I index: the same kernel with LOC set also counts the hits' locations (64-bit), a second scan turns those
 * into offsets, the fill pass leaves per hit where its locations start in the output and in the index, and one segmented
 * gather, dealt by output element, copies and decodes them (k_gather_locations).  Both entry points are one host body in
 * stages (lookup_hits).
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

/* The arrays of a hit pass over `n_tiles` tiles.  The count pass writes tile_cnt (and tile_loc); the scans make tile_off
 * (and tile_loc_off) of them; the fill pass reads those and writes the rest.  The second group is --locations' only. */
struct HitPass {
  u64 n_tiles;
  u32 *tile_cnt;          /* hits of a tile */
  const u64 *tile_off;
  gt4hip_query_hit *hits;
  const u64 *first;       /* per record of the list: its first location in the index */
  u64 *tile_loc;          /* locations of a tile's hits */
  const u64 *tile_loc_off;
  u64 *seg_off, *seg_src; /* per hit: its first location's place in the output, and in the index */
};

/* --all and --locations.  Tile t covers items [t * MM_TILE, (t + 1) * MM_TILE) of the flattened space, as in the
 * compaction of gt4hip_mismatch.hip.  FILL == false: tile_cnt[t] = hits of the tile.  FILL == true: the hits to
 * hits[tile_off[t]...] in item order (the probes are repeated: the variant space itself is never stored).  LOC: the
 * locations of every hit are counted beside it, a record's count being their number: tile_loc[t] = those of the tile's
 * hits, and for hit h the place of its first location in the output (seg_off[h], from tile_loc_off[t] on) and in the index
 * (seg_src[h]). */
template <bool FILL, bool LOC>
__global__ __launch_bounds__ (MM_THREADS) void k_query_hits (Query Q, HitPass P)
{
  __shared__ u32 part[MM_WAVES];
  __shared__ u64 lpart[LOC ? MM_WAVES : 1];
  for (u64 t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
    u64 pos = FILL ? P.tile_off[t] : 0, lpos = FILL && LOC ? P.tile_loc_off[t] : 0;
    u32 mine = 0;
    u64 lmine = 0;
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
      u32 cnt = 0;
      if constexpr (LOC) cnt = hit ? Q.ix.rec[3 * j + 2] : 0u;
      if constexpr (!FILL) {
        mine += hit;
        lmine += cnt;
      } else {
        u32 round;
        u64 loff = 0, lround = 0;
        if constexpr (LOC) loff = wave_offset (cnt, lpart);
        const u64 h = pos + round_place (hit, part, &round);
        if constexpr (LOC) loff += lpos + waves_before (lpart, &lround);
        if (hit) {
          gt4hip_query_hit o;
          o.query = q;
          o.rank = r;
          o.word = cv;
          o.count = LOC ? cnt : Q.ix.rec[3 * j + 2];
          o.reserved = 0;
          P.hits[h] = o;
        }
        if constexpr (LOC) {
          if (hit) {
            P.seg_off[h] = loff;
            P.seg_src[h] = P.first[j];
          }
        }
        pos += round;
        lpos += lround;
        __syncthreads ();
      }
    }
    if constexpr (!FILL) {
      if constexpr (LOC) tile_total (mine, part, &P.tile_cnt[t], lmine, lpart, &P.tile_loc[t]);
      else tile_total (mine, part, &P.tile_cnt[t]);
    }
  }
}

/* ------------------------------------------------------------------ --locations: the hits with where they occur */

/* One pass over the k-mer section of a GT4I index, entries [i0, i0 + n) of n_all (the piece holds entry i0 + n too
 * unless that is the end): the packed record (count = distance to the next first location, in 32 bits as
 * imap_get_count, src/index-map.c:129-139), the first location on its own, and the check that makes every later read
 * of the location array safe: first locations never descend and never pass num_locations. */
__global__ __launch_bounds__ (MM_THREADS) void k_index_split (const u64 *__restrict__ kmers, u64 i0, u64 n, u64 n_all, u64 num_locations, u32 *__restrict__ rec,
                                                              u64 *__restrict__ first, u32 *bad)
{
  bool wrong = false;
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) {
    const u64 word = kmers[2 * i], loc = kmers[2 * i + 1];
    const u64 next = i0 + i + 1 < n_all ? kmers[2 * i + 3] : num_locations;
    wrong |= loc > next || next > num_locations;
    rec[3 * (i0 + i)] = (u32) word;
    rec[3 * (i0 + i) + 1] = (u32) (word >> 32);
    rec[3 * (i0 + i) + 2] = (u32) (next - loc);
    first[i0 + i] = loc;
  }
  if (__builtin_amdgcn_ballot_w64 (wrong) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr (bad, 1u);
}

/* k_tile_scan of 64-bit counts: the locations of a tile's hits do not fit 32 bits */
__global__ __launch_bounds__ (1024) void k_tile_scan64 (const u64 *tile_cnt, u64 n_tiles, u64 *tile_off, unsigned long long *total)
{
  workgroup_scan<1> ({tile_cnt}, {tile_off}, n_tiles, total);
}

/* how a packed location comes apart (index_map_get_location, src/index-map.c:197-208) */
struct LocationBits {
  u32 file_shift, seq_shift; /* n_subseq_bits + n_pos_bits + 1 (0 with file_mask 0 where that is 64), n_pos_bits + 1 */
  u64 file_mask, seq_mask, pos_mask;
};

constexpr int GATHER_ROUNDS = 8;
constexpr u32 GATHER_TILE = MM_THREADS * GATHER_ROUNDS; /* output locations per tile */
static_assert (GATHER_ROUNDS == GT4HIP_GATHER_ROUNDS, "counter \"gather_tile\" (gt4hip_host.h)");
constexpr u32 GATHER_LDS_SEGS = GATHER_TILE + 1;        /* segments of a tile kept in LDS: every tile without zero-length ones fits */

/* The first index i of the ascending a[0..n) with a[i] > o (n when there is none), by a whole wavefront: every step
 * probes 64 evenly spaced entries of what is left and keeps the stretch between the last probe <= o and the first > o. */
__device__ __forceinline__ u64 wave_upper_bound (const u64 *__restrict__ a, u64 n, u64 o, int lane)
{
  u64 lo = 0, hi = n; /* the answer lies in [lo, hi] */
  while (lo < hi) {
    const u64 step = (hi - lo) / WAVE + 1;
    const u64 i = lo + (u64) lane * step;
    const int c = __popcll (__builtin_amdgcn_ballot_w64 (i < hi && a[i] <= o)); /* a prefix of the lanes */
    if (c == 0) {
      hi = lo;
    } else {
      const u64 up = lo + (u64) c * step;
      lo += (u64) (c - 1) * step + 1;
      hi = up < hi ? up : hi;
    }
  }
  return lo;
}

/* The segmented gather.  Segment h (one hit) is seg_off[h + 1] - seg_off[h] packed locations from locs[seg_src[h]] on,
 * and goes to out[seg_off[h]...]; seg_off ascends, seg_off[n_segs] = n_out, equal neighbours are empty segments.  The
 * work is dealt by OUTPUT element: a workgroup takes GATHER_TILE consecutive outputs and finds the segments that cover
 * them with two searches of seg_off (the last segment that starts at or before the tile's first and its last output:
 * empty segments sort in front of the one that holds an output and are never chosen); a search is a wavefront's, 64
 * probes a step, so 10^7 segments take four dependent loads where a binary search takes 24.  A tile inside one segment (a
 * k-mer with 10^5 locations) copies straight; otherwise the tile's segment starts go to LDS, relative to the tile, and
 * every output finds its own by a search there (a run of more than GATHER_LDS_SEGS segments, which only empty ones can
 * make, is searched in global memory).  Consecutive lanes read consecutive 8-byte words of a segment and write
 * consecutive 16-byte records. */
__global__ __launch_bounds__ (MM_THREADS) void k_gather_locations (const u64 *__restrict__ seg_off, const u64 *__restrict__ seg_src, u64 n_segs, u64 n_out,
                                                                   const u64 *__restrict__ locs, LocationBits B, gt4hip_location *__restrict__ out)
{
  __shared__ u32 rel[GATHER_LDS_SEGS];
  __shared__ u64 delta[GATHER_LDS_SEGS];
  __shared__ u64 bound[2];
  const u64 n_tiles = (n_out + GATHER_TILE - 1) / GATHER_TILE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 o0 = t * GATHER_TILE;
    const u64 o1 = o0 + GATHER_TILE < n_out ? o0 + GATHER_TILE : n_out; /* one past the tile's last output */
    /* first index with seg_off > o0 (wavefront 0) and with seg_off > o1 - 1 (wavefront 1), side by side */
    if (threadIdx.x < 2 * WAVE) {
      const u64 b = wave_upper_bound (seg_off, n_segs, threadIdx.x < WAVE ? o0 : o1 - 1, threadIdx.x & (WAVE - 1));
      if ((threadIdx.x & (WAVE - 1)) == 0) bound[threadIdx.x / WAVE] = b;
    }
    __syncthreads ();
    const u64 hA = bound[0] - 1, hB = bound[1] - 1; /* seg_off[0] = 0 <= o0: both bounds are >= 1 */
    const u64 m = hB - hA + 1;
    const bool one = m == 1, lds = m <= GATHER_LDS_SEGS;
    const u64 d_one = seg_src[hA] - seg_off[hA];
    if (!one && lds) {
      for (u32 x = threadIdx.x; x < (u32) m; x += MM_THREADS) {
        const u64 so = seg_off[hA + x];
        rel[x] = so > o0 ? (u32) (so - o0) : 0u;
        delta[x] = seg_src[hA + x] - so;
      }
    }
    __syncthreads ();
#pragma unroll
    for (int rd = 0; rd < GATHER_ROUNDS; rd++) {
      const u32 e = (u32) rd * MM_THREADS + threadIdx.x;
      const u64 o = o0 + e;
      if (o < o1) {
        u64 d = d_one;
        if (!one && lds) {
          u32 lo = 0, hi = (u32) m; /* first x with rel[x] > e */
          while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (rel[mid] <= e) lo = mid + 1;
            else hi = mid;
          }
          d = delta[lo - 1];
        } else if (!one) {
          u64 lo = hA, hi = hB + 1;
          while (lo < hi) {
            const u64 mid = (lo + hi) >> 1;
            if (seg_off[mid] <= o) lo = mid + 1;
            else hi = mid;
          }
          d = seg_src[lo - 1] - seg_off[lo - 1];
        }
        const u64 code = locs[d + o];
        const u64 pos_dir = (((code >> 1) & B.pos_mask) << 1) | (code & 1);
        u32x4 r; /* a gt4hip_location, in one 16-byte store */
        r.x = (u32) pos_dir;
        r.y = (u32) (pos_dir >> 32);
        r.z = (u32) ((code >> B.file_shift) & B.file_mask);
        r.w = (u32) ((code >> B.seq_shift) & B.seq_mask);
        ((u32x4 *) out)[o] = r;
      }
    }
    __syncthreads ();
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
static_assert (HIST_LDS_BINS == GT4HIP_HIST_LDS_BINS, "counter \"hist_lds_bins\" (gt4hip_host.h)");

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
  double gather_ms; /* the gather kernel of the last gt4hip_query_lookup_locations */
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
  qi->last_ms = qi->gather_ms = 0;
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

int gt4hip_query_check_params (gt4hip_context *ctx, const char *who, const gt4hip_query_index *qi, const gt4hip_query_params *prm) { return check_params (ctx, who, qi, prm); }
const gt4hip_list *gt4hip_query_index_list (const gt4hip_query_index *qi) { return qi->list; }
const uint64_t *gt4hip_query_index_offsets (const gt4hip_query_index *qi) { return (const uint64_t *) qi->ix.off; }
void gt4hip_query_index_set_ms (gt4hip_query_index *qi, double ms) { qi->last_ms = ms; }

int gt4hip_query_lookup_device (gt4hip_context *ctx, const char *who, gt4hip_query_index *qi, const gt4hip_query_params *prm, const uint64_t *d_words, uint64_t n,
                                uint32_t *d_values, unsigned char *d_found)
{
  Query Q;
  int rc;
  if ((rc = fill_query (ctx, who, qi, prm, (const u64 *) d_words, n, &Q))) return rc;
  ctx->query_wide = 0;
  if (!prm->n_mm) {
    hipLaunchKernelGGL (k_query_exact, dim3 (gt4hip_grid (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, Q.words, (u64) n, Q.ix, Q.k, Q.canonize, d_values,
                        d_found);
  } else {
    HIPCHK (ctx, hipMemsetAsync (d_values, 0, n * 4, ctx->stream));
    const int grid = gt4hip_grid (ctx, Q.total, MM_THREADS);
    const u64 stride = (u64) grid * MM_THREADS;
    Q.stride_w = stride / Q.n_var;
    Q.stride_r = stride % Q.n_var;
    ctx->query_wide = !(Q.n_var + stride < 0xffffffffull);
    if (!ctx->query_wide) hipLaunchKernelGGL (k_query<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, d_values);
    else hipLaunchKernelGGL (k_query<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, Q, d_values);
    HIPCHK (ctx, hipGetLastError ());
    if (d_found) hipLaunchKernelGGL (k_query_found, dim3 (gt4hip_grid (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) d_values, (u64) n, d_found);
  }
  HIPCHK (ctx, hipGetLastError ());
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
  TempBlocks blk;
  u64 *d_words = NULL;
  u32 *d_values = NULL;
  unsigned char *d_found = NULL;
  if ((rc = blk.get (ctx, n * 8, (void **) &d_words)) || (rc = blk.get (ctx, n * 4, (void **) &d_values)) || (rc = blk.get (ctx, n, (void **) &d_found))) return rc;
  Query Q; /* (a batch that cannot be ranked is refused before anything is enqueued) */
  if ((rc = fill_query (ctx, "gt4hip_query_lookup", qi, prm, d_words, n, &Q))) return rc;
  Timer tm;
  HIPCHK (ctx, hipEventCreate (&tm.e0));
  HIPCHK (ctx, hipEventCreate (&tm.e1));
  HIPCHK (ctx, hipMemcpyAsync (d_words, words, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK (ctx, hipEventRecord (tm.e0, ctx->stream));
  if ((rc = gt4hip_query_lookup_device (ctx, "gt4hip_query_lookup", qi, prm, (const uint64_t *) d_words, n, d_values, d_found))) return rc;
  HIPCHK (ctx, hipEventRecord (tm.e1, ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (values, d_values, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (found, d_found, n, hipMemcpyDeviceToHost, ctx->stream));
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
    hipLaunchKernelGGL (k_count_stats, dim3 (gt4hip_grid (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev,
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
  hipLaunchKernelGGL (k_count_split, dim3 (gt4hip_grid (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev,
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
  TempBlocks blk;
  unsigned long long *d = NULL;
  int rc = blk.get (ctx, (size_t) max * 8, (void **) &d);
  if (rc) return rc;
  HIPCHK (ctx, hipMemsetAsync (d, 0, (size_t) max * 8, ctx->stream));
  const int grid = gt4hip_grid (ctx, list->n_words, MM_THREADS * 4);
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
  hipLaunchKernelGGL (k_gc, dim3 (gt4hip_grid (ctx, list->n_words, MM_THREADS * 4)), dim3 (MM_THREADS), 0, ctx->stream, (const u32 *) list->dev, list->n_words,
                      mask, ctx->scratch);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  *weighted_gc_bases = ctx->scratch_host[0];
  return GT4HIP_OK;
}

/* ------------------------------------------------------------------ --locations */

struct gt4hip_location_index {
  gt4hip_context *ctx;
  gt4hip_list *list;     /* the k-mer section as packed records */
  u64 *first;            /* n_words first locations */
  u64 *locs;             /* n_locations packed locations */
  void *first_owner, *locs_owner;
  u64 n_locations;
  LocationBits bits;
};

static_assert (sizeof (gt4hip_location) == 16, "a location is one 16-byte store");

extern "C" void gt4hip_location_index_free (gt4hip_location_index *li)
{
  if (!li) return;
  gt4hip_block_free (li->first_owner);
  gt4hip_block_free (li->locs_owner);
  gt4hip_list_free (li->list);
  delete li;
}

extern "C" const gt4hip_list *gt4hip_location_index_list (const gt4hip_location_index *li) { return li ? li->list : NULL; }
extern "C" uint64_t gt4hip_location_index_n_locations (const gt4hip_location_index *li) { return li ? li->n_locations : 0; }

extern "C" int gt4hip_location_index_create (gt4hip_context *ctx, const void *host_kmers, uint64_t n_words, const void *host_locations, uint64_t num_locations,
                                             uint32_t word_length, uint32_t n_file_bits, uint32_t n_subseq_bits, uint32_t n_pos_bits, gt4hip_location_index **out)
{
  if (!ctx || !out || (n_words && !host_kmers) || (num_locations && !host_locations)) return GT4HIP_EINVAL;
  *out = NULL;
  if (word_length < 1 || word_length > 32) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_location_index_create: word length %u", word_length);
  if (n_file_bits > 64 || n_subseq_bits > 64 || n_pos_bits > 64 || n_file_bits + n_subseq_bits + n_pos_bits + 1 > 64)
    return gt4hip_fail (ctx, GT4HIP_EFORMAT, "gt4hip_location_index_create: a location of %u + %u + %u + 1 bits does not fit 64", n_file_bits, n_subseq_bits, n_pos_bits);
  if (n_words > (1ull << 59) || num_locations > (1ull << 60)) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_location_index_create: %llu k-mers, %llu locations", (unsigned long long) n_words, (unsigned long long) num_locations);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_location_index *li = new (std::nothrow) gt4hip_location_index ();
  if (!li) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  li->ctx = ctx;
  li->n_locations = num_locations;
  const auto mask = [] (u32 bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1; };
  const u32 fs = n_subseq_bits + n_pos_bits + 1;
  li->bits.file_shift = fs < 64 ? fs : 0;
  li->bits.file_mask = fs < 64 ? mask (n_file_bits) : 0;
  li->bits.seq_shift = n_pos_bits + 1 < 64 ? n_pos_bits + 1 : 0;
  li->bits.seq_mask = n_pos_bits + 1 < 64 ? mask (n_subseq_bits) : 0;
  li->bits.pos_mask = mask (n_pos_bits);
  /* the k-mer section goes through a device buffer of PIECE entries (and the one behind them: the end of the last count) */
  const u64 PIECE = 1ull << 22;
  TempBlocks blk;
  u64 *tmp = NULL;
  u32 *bad = (u32 *) ctx->scratch;
  int rc = gt4hip_list_new (ctx, n_words, word_length, &li->list);
  if (!rc) rc = gt4hip_block_alloc (ctx, n_words ? n_words * 8 : 16, (void **) &li->first, &li->first_owner);
  if (!rc) rc = gt4hip_block_alloc (ctx, num_locations ? num_locations * 8 : 16, (void **) &li->locs, &li->locs_owner);
  if (!rc) rc = blk.get (ctx, ((n_words < PIECE ? n_words : PIECE) + 1) * 16, (void **) &tmp);
  if (!rc && hipMemsetAsync (bad, 0, 4, ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_location_index_create: hipMemsetAsync failed");
  for (u64 i0 = 0; !rc && i0 < n_words; i0 += PIECE) {
    const u64 n = n_words - i0 < PIECE ? n_words - i0 : PIECE, with_next = i0 + n < n_words ? n + 1 : n;
    rc = gt4hip_io_upload (ctx, (const char *) host_kmers + i0 * 16, tmp, with_next * 16);
    if (rc) break;
    hipLaunchKernelGGL (k_index_split, dim3 (gt4hip_grid (ctx, n, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, (const u64 *) tmp, i0, n, n_words, num_locations,
                        (u32 *) li->list->dev, li->first, bad);
    if (hipGetLastError () != hipSuccess || hipStreamSynchronize (ctx->stream) != hipSuccess) rc = gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_location_index_create: decoding the k-mer section failed");
  }
  if (!rc) rc = gt4hip_read_back (ctx, ctx->scratch_host, bad, 4, "gt4hip_location_index_create: reading the check back failed");
  if (!rc && *(const u32 *) ctx->scratch_host)
    rc = gt4hip_fail (ctx, GT4HIP_EFORMAT, "gt4hip_location_index_create: the first locations of the k-mers descend or pass the %llu locations of the index",
                      (unsigned long long) num_locations);
  if (!rc && num_locations) rc = gt4hip_io_upload (ctx, host_locations, li->locs, num_locations * 8);
  if (rc) {
    gt4hip_location_index_free (li);
    return rc;
  }
  *out = li;
  return GT4HIP_OK;
}

/* ------------------------------------------------------------------ --all and --locations: one call in stages */

namespace {

/* A call of gt4hip_query_lookup_all (li == NULL) or gt4hip_query_lookup_locations, `who` in its messages. */
struct HitCall {
  gt4hip_context *ctx;
  const char *who;
  gt4hip_query_index *qi;
  const gt4hip_location_index *li;
  TempBlocks blk;
  Timer tm, tg; /* tm: the call's kernels (last_ms); tg.e0: where the gather starts (gather_ms) */
  Query Q;
  HitPass P;
  int grid;
  u64 total_hits, total_locs;
};

template <bool FILL>
void launch_hits (const HitCall &c)
{
  if (c.li) hipLaunchKernelGGL ((k_query_hits<FILL, true>), dim3 (c.grid), dim3 (MM_THREADS), 0, c.ctx->stream, c.Q, c.P);
  else hipLaunchKernelGGL ((k_query_hits<FILL, false>), dim3 (c.grid), dim3 (MM_THREADS), 0, c.ctx->stream, c.Q, c.P);
}

/* the query words on the device, the Query, the tiles and their arrays; the clock starts behind the upload */
int hits_prepare (HitCall &c, const uint64_t *words, u64 n, const gt4hip_query_params *prm)
{
  gt4hip_context *ctx = c.ctx;
  int rc;
  u64 *d_words = NULL;
  if ((rc = c.blk.get (ctx, n * 8, (void **) &d_words))) return rc;
  if ((rc = fill_query (ctx, c.who, c.qi, prm, d_words, n, &c.Q))) return rc;
  const u64 tiles = c.Q.total / MM_TILE + (c.Q.total % MM_TILE != 0);
  if (tiles > (1ull << 31))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: %llu queries of %llu variants each are too many for one call: split the batch", c.who, (unsigned long long) n,
                        (unsigned long long) c.Q.n_var);
  c.P.n_tiles = tiles;
  c.grid = gt4hip_grid (ctx, tiles, 1);
  if ((rc = c.blk.get (ctx, tiles * 4, (void **) &c.P.tile_cnt))) return rc;
  if (c.li && (rc = c.blk.get (ctx, tiles * 8, (void **) &c.P.tile_loc))) return rc;
  if ((rc = c.blk.get (ctx, tiles * 8, (void **) &c.P.tile_off))) return rc;
  if (c.li) {
    if ((rc = c.blk.get (ctx, tiles * 8, (void **) &c.P.tile_loc_off))) return rc;
    c.P.first = c.li->first;
  }
  HIPCHK (ctx, hipEventCreate (&c.tm.e0));
  HIPCHK (ctx, hipEventCreate (&c.tm.e1));
  if (c.li) HIPCHK (ctx, hipEventCreate (&c.tg.e0));
  HIPCHK (ctx, hipMemcpyAsync (d_words, words, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK (ctx, hipEventRecord (c.tm.e0, ctx->stream));
  return GT4HIP_OK;
}

/* the count pass, the scan of the hits (and of their locations), the totals back on the host */
int hits_count (HitCall &c)
{
  gt4hip_context *ctx = c.ctx;
  launch_hits<false> (c);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, ctx->stream, (const u32 *) c.P.tile_cnt, c.P.n_tiles, (u64 *) c.P.tile_off, ctx->scratch);
  if (c.li)
    hipLaunchKernelGGL (k_tile_scan64, dim3 (1), dim3 (1024), 0, ctx->stream, (const u64 *) c.P.tile_loc, c.P.n_tiles, (u64 *) c.P.tile_loc_off, ctx->scratch + 1);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, ctx->scratch, c.li ? 16 : 8, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  c.total_hits = ctx->scratch_host[0];
  c.total_locs = c.li ? ctx->scratch_host[1] : 0;
  return GT4HIP_OK;
}

/* the fill pass, the gather of the locations where there is an index, the clock stopped, the copies to the caller started */
int hits_fill (HitCall &c, gt4hip_query_hit *hits, gt4hip_location *locations)
{
  gt4hip_context *ctx = c.ctx;
  const u64 total_hits = c.total_hits, total_locs = c.total_locs;
  int rc;
  if (total_locs > (1ull << 59)) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "%s: %llu locations", c.who, (unsigned long long) total_locs);
  gt4hip_location *d_locs = NULL;
  if ((rc = c.blk.get (ctx, total_hits * sizeof (gt4hip_query_hit), (void **) &c.P.hits))) return rc;
  if (c.li && ((rc = c.blk.get (ctx, total_hits * 8, (void **) &c.P.seg_off)) || (rc = c.blk.get (ctx, total_hits * 8, (void **) &c.P.seg_src)) ||
               (rc = c.blk.get (ctx, total_locs * sizeof (gt4hip_location), (void **) &d_locs))))
    return rc;
  gt4hip_grid_again (ctx, c.P.n_tiles, c.grid);
  launch_hits<true> (c);
  HIPCHK (ctx, hipGetLastError ());
  if (c.li) {
    HIPCHK (ctx, hipEventRecord (c.tg.e0, ctx->stream));
    if (total_locs) {
      const u64 g_tiles = (total_locs + GATHER_TILE - 1) / GATHER_TILE;
      hipLaunchKernelGGL (k_gather_locations, dim3 (gt4hip_grid (ctx, g_tiles, 1)), dim3 (MM_THREADS), 0, ctx->stream, (const u64 *) c.P.seg_off, (const u64 *) c.P.seg_src,
                          total_hits, total_locs, (const u64 *) c.li->locs, c.li->bits, d_locs);
      HIPCHK (ctx, hipGetLastError ());
    }
  }
  HIPCHK (ctx, hipEventRecord (c.tm.e1, ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (hits, c.P.hits, total_hits * sizeof (gt4hip_query_hit), hipMemcpyDeviceToHost, ctx->stream));
  if (!c.li) return GT4HIP_OK;
  if (total_locs * sizeof (gt4hip_location) < ((size_t) 32 << 20)) {
    HIPCHK (ctx, hipMemcpyAsync (locations, d_locs, total_locs * sizeof (gt4hip_location), hipMemcpyDeviceToHost, ctx->stream));
  } else { /* in pieces through the staging threads, as large lists are */
    HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
    if ((rc = gt4hip_io_download (ctx, d_locs, locations, total_locs * sizeof (gt4hip_location)))) return rc;
  }
  return GT4HIP_OK;
}

/* The hits of n > 0 words, and with `li` their locations; the caller has checked its arguments.  *n_hits and *n_locations are
 * always the totals; the arrays are filled only where both capacities suffice. */
int lookup_hits (gt4hip_context *ctx, const char *who, gt4hip_query_index *qi, const gt4hip_location_index *li, const uint64_t *words, u64 n,
                 const gt4hip_query_params *prm, gt4hip_query_hit *hits, u64 hit_capacity, uint64_t *n_hits, gt4hip_location *locations, u64 loc_capacity,
                 uint64_t *n_locations)
{
  HIPCHK (ctx, hipSetDevice (ctx->device));
  HitCall c = { ctx, who, qi, li };
  int rc;
  if ((rc = hits_prepare (c, words, n, prm)) || (rc = hits_count (c))) return rc;
  *n_hits = c.total_hits;
  if (li) *n_locations = c.total_locs;
  if (c.total_hits && c.total_hits <= hit_capacity && c.total_locs <= loc_capacity) {
    if ((rc = hits_fill (c, hits, locations))) return rc;
  } else {
    if (li) HIPCHK (ctx, hipEventRecord (c.tg.e0, ctx->stream));
    HIPCHK (ctx, hipEventRecord (c.tm.e1, ctx->stream));
  }
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  float ms = 0;
  if (hipEventElapsedTime (&ms, c.tm.e0, c.tm.e1) == hipSuccess) qi->last_ms = ms;
  if (li && hipEventElapsedTime (&ms, c.tg.e0, c.tm.e1) == hipSuccess) qi->gather_ms = ms;
  return GT4HIP_OK;
}

}  // namespace

extern "C" int gt4hip_query_lookup_all (gt4hip_context *ctx, gt4hip_query_index *qi, const uint64_t *words, uint64_t n, const gt4hip_query_params *prm,
                                        gt4hip_query_hit *hits, uint64_t capacity, uint64_t *n_hits)
{
  if (!ctx || !qi || !prm || !n_hits || (n && !words) || (capacity && !hits)) return GT4HIP_EINVAL;
  const int rc = check_params (ctx, "gt4hip_query_lookup_all", qi, prm);
  if (rc) return rc;
  *n_hits = 0;
  qi->last_ms = 0;
  if (!n) return GT4HIP_OK;
  return lookup_hits (ctx, "gt4hip_query_lookup_all", qi, NULL, words, n, prm, hits, capacity, n_hits, NULL, 0, NULL);
}

extern "C" int gt4hip_query_lookup_locations (gt4hip_context *ctx, gt4hip_query_index *qi, const gt4hip_location_index *li, const uint64_t *words, uint64_t n,
                                              const gt4hip_query_params *prm, gt4hip_query_hit *hits, uint64_t hit_capacity, uint64_t *n_hits,
                                              gt4hip_location *locations, uint64_t loc_capacity, uint64_t *n_locations)
{
  if (!ctx || !qi || !li || !prm || !n_hits || !n_locations || (n && !words) || (hit_capacity && !hits) || (loc_capacity && !locations)) return GT4HIP_EINVAL;
  if (qi->list != li->list) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_query_lookup_locations: the query index was not made of this location index's list");
  const int rc = check_params (ctx, "gt4hip_query_lookup_locations", qi, prm);
  if (rc) return rc;
  *n_hits = *n_locations = 0;
  qi->last_ms = qi->gather_ms = 0;
  if (!n) return GT4HIP_OK;
  return lookup_hits (ctx, "gt4hip_query_lookup_locations", qi, li, words, n, prm, hits, hit_capacity, n_hits, locations, loc_capacity, n_locations);
}

extern "C" double gt4hip_query_index_gather_ms (const gt4hip_query_index *qi) { return qi ? qi->gather_ms : 0.0; }
