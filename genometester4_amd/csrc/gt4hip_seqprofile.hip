/* gt4hip_seqprofile.hip -- glistquery --per_sequence on the device, gfx950, wave64: every word of a text looked up in a
 * resident list and the results added up per sequence of the text (not in the reference; what its `glistquery -s` prints
 * for one sequence at a time, counted).
 *
 * The reader (gt4hip_text_to_locations, gt4hip_maker.hip) leaves beside every word ordinal << 33 | position << 1 | strand:
 * the ordinal says which sequence the word belongs to, and ordinals ascend with the text.  k_seq_profile<PROBE> walks the
 * words in tiles of PROFILE_TILE, consecutive lanes on consecutive words:
 *
 *   - PROBE: one find () per word in the bucket index (gt4hip_index.h), the stored count its value; !PROBE (-mm N): the value
 *     is read from the u32 array the k_query family (gt4hip_query.hip) filled for the same device words;
 *   - a lane holds (ordinal, hit, hit ? value : 0).  Runs of equal ordinal inside a wavefront are found with one ballot of
 *     head flags; a run's words are counted from the ballots alone, its hits and their values are added with the
 *     shuffle-down ladder of k_query, and only in wavefronts that have a hit at all;
 *   - a run with other ordinals on both sides inside its wavefront is the whole of its sequence in the tile (ordinals
 *     ascend): its head lane adds it to the sequence's sums.  The first and the last run of a wavefront may go on in the
 *     neighbours: they are posted to LDS, two entries per wavefront and round, 64 per tile in word order, and the tile's
 *     first wavefront folds those by the same ballot and ladder.  So a tile adds to a sequence's sums ONCE, however the
 *     sequence lies in it: a chromosome of 10^8 words is 10^8 / PROFILE_TILE adds on one address, a tile of short reads
 *     is one add per read on addresses of their own;
 *   - the adds are 64-bit integer atomics: exact, the order does not matter;
 *   - ordinal - first_ordinal is compared with n_seqs before anything is addressed with it; a word out of the range
 *     is dropped and, like an ordinal below its predecessor's, raises the flag word behind the sums (GT4HIP_EINVAL).
 *
 * The sums (three u64 per sequence: a gt4hip_seq_profile) and the flag are zeroed by k_seq_zero in the same call. */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"

#include <string.h>

namespace gt4 {
namespace {

constexpr int PROFILE_ROUNDS = GT4HIP_PROFILE_ROUNDS;
constexpr u64 PROFILE_TILE = (u64) MM_THREADS * PROFILE_ROUNDS; /* words per tile (counter "profile_tile") */
constexpr int PROFILE_ENTRIES = 2 * MM_WAVES * PROFILE_ROUNDS;  /* boundary runs a tile posts: the first and last of every wavefront and round */
static_assert (PROFILE_ENTRIES == WAVE, "one wavefront folds the boundary runs of a tile");
constexpr u64 NO_SEQ = ~0ull; /* the sequence of a lane without a word, or with one outside the range */

struct Profile {
  const u64 *words, *raw;
  const u32 *values; /* !PROBE: per word, from k_query */
  u64 n;
  u64 first_ordinal, n_seqs;
  u32 min_value, max_value;
  unsigned long long *acc; /* n_seqs x (words, hits, sum), then the flag word */
};

__global__ __launch_bounds__ (MM_THREADS) void k_seq_zero (unsigned long long *acc, u64 n)
{
  for (u64 i = (u64) blockIdx.x * MM_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * MM_THREADS) acc[i] = 0;
}

/* the last lane of the run this lane lies in; H: the head flags of the wavefront (bit 0 always set) */
__device__ __forceinline__ int run_end (u64 H, int lane)
{
  const u64 after = lane == WAVE - 1 ? 0 : H & (~0ull << (lane + 1));
  return after ? __builtin_ctzll (after) - 1 : WAVE - 1;
}

/* the head lane of a run gets the run's hits and values (k_query's ladder) */
__device__ __forceinline__ void run_sums (int lane, int end, u32 &hits, u64 &sum)
{
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const u32 oh = __shfl_down (hits, d, WAVE);
    const u32 lo = __shfl_down ((u32) sum, d, WAVE), hi = __shfl_down ((u32) (sum >> 32), d, WAVE);
    if (lane + d <= end) {
      hits += oh;
      sum += (u64) lo | ((u64) hi << 32);
    }
  }
}

__device__ __forceinline__ void add_run (unsigned long long *acc, u64 seq, u32 words, u32 hits, u64 sum)
{
  unsigned long long *a = acc + 3 * seq;
  if (words) atomicAdd (a, (unsigned long long) words);
  if (hits) atomicAdd (a + 1, (unsigned long long) hits);
  if (sum) atomicAdd (a + 2, (unsigned long long) sum);
}

template <bool PROBE>
__global__ __launch_bounds__ (MM_THREADS) void k_seq_profile (Profile P, Index ix, u64 n_tiles)
{
  __shared__ u64 b_seq[PROFILE_ENTRIES], b_sum[PROFILE_ENTRIES];
  __shared__ u32 b_words[PROFILE_ENTRIES], b_hits[PROFILE_ENTRIES];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  bool wrong = false;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
#pragma unroll 1
    for (int rd = 0; rd < PROFILE_ROUNDS; rd++) {
      const u64 i = t * PROFILE_TILE + (u64) rd * MM_THREADS + threadIdx.x;
      const bool valid = i < P.n;
      u64 seq = NO_SEQ, ord = 0, sum = 0;
      u32 hits = 0;
      if (valid) {
        ord = P.raw[i] >> 33;
        const u64 rel = ord - P.first_ordinal;
        if (ord >= P.first_ordinal && rel < P.n_seqs) seq = rel;
        else wrong = true;
        u32 val;
        bool found;
        if (PROBE) {
          const u64 j = find (ix, P.words[i]);
          found = j != ~0ull;
          val = found ? ix.rec[3 * j + 2] : 0u;
        } else {
          val = P.values[i];
          found = val != 0;
        }
        if (found && val >= P.min_value && val <= P.max_value) {
          hits = 1;
          sum = val;
        }
      }
      /* the ordinal before this lane's: the neighbour's, for lane 0 the word before the wavefront's first */
      u64 prev = shfl_up_u64 (ord, 1);
      if (lane == 0) prev = valid && i ? P.raw[i - 1] >> 33 : 0;
      if (valid && prev > ord) wrong = true;
      const u64 pseq = shfl_up_u64 (seq, 1);
      const u64 H = __builtin_amdgcn_ballot_w64 (lane == 0 || pseq != seq);
      const u64 V = __builtin_amdgcn_ballot_w64 (valid);
      const int end = run_end (H, lane);
      const u32 words = (u32) __popcll (V & (~0ull << lane) & (end == WAVE - 1 ? ~0ull : (2ull << end) - 1));
      if (__builtin_amdgcn_ballot_w64 (hits != 0)) run_sums (lane, end, hits, sum);
      if ((H >> lane) & 1) {
        const int last_head = WAVE - 1 - __builtin_clzll (H);
        const int e = 2 * (rd * MM_WAVES + wv);
        if (lane == 0 || lane == last_head) {
          const int at = lane == 0 ? e : e + 1;
          b_seq[at] = seq, b_words[at] = words, b_hits[at] = hits, b_sum[at] = sum;
          if (last_head == 0) b_seq[e + 1] = seq, b_words[e + 1] = 0, b_hits[e + 1] = 0, b_sum[e + 1] = 0; /* one run: nothing more to post */
        } else if (seq != NO_SEQ) {
          add_run (P.acc, seq, words, hits, sum);
        }
      }
    }
    __syncthreads ();
    if (wv == 0) { /* the boundary runs, in word order: equal sequences are neighbours */
      const u64 seq = b_seq[lane];
      u64 sum = b_sum[lane];
      u32 words = b_words[lane], hits = b_hits[lane];
      const u64 pseq = shfl_up_u64 (seq, 1);
      const u64 H = __builtin_amdgcn_ballot_w64 (lane == 0 || pseq != seq);
      const int end = run_end (H, lane);
      u64 wsum = words; /* (the ladder adds a u32 and a u64: the words ride in the second) */
      run_sums (lane, end, hits, wsum);
      u32 none = 0;
      run_sums (lane, end, none, sum);
      if (((H >> lane) & 1) && seq != NO_SEQ) add_run (P.acc, seq, (u32) wsum, hits, sum);
    }
    __syncthreads ();
  }
  if (__builtin_amdgcn_ballot_w64 (wrong) && lane == 0) atomicOr (&P.acc[3 * P.n_seqs], 1ull);
}

}  // namespace
}  // namespace gt4

using namespace gt4;

namespace {

/* The call's kernels on words and raw locations in device memory (the arguments are checked): the sums zeroed, with n_mm > 0
 * the values by the k_query family, k_seq_profile; the sums and the flag read back. */
int profile_device (gt4hip_context *ctx, const char *who, gt4hip_query_index *qi, const u64 *d_words, const u64 *d_raw, u64 n, u64 first_ordinal, u64 n_seqs,
                    const gt4hip_query_params *prm, u32 min_value, u32 max_value, gt4hip_seq_profile *profiles)
{
  gt4hip_query_index_set_ms (qi, 0);
  if (!n_seqs) return n ? gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: %llu words and no sequence for them", who, (unsigned long long) n) : GT4HIP_OK;
  if (n_seqs > (1ull << 56)) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "%s: %llu sequences", who, (unsigned long long) n_seqs);
  if (!n) {
    memset (profiles, 0, (size_t) n_seqs * sizeof *profiles);
    return GT4HIP_OK;
  }
  const u64 tiles = (n + PROFILE_TILE - 1) / PROFILE_TILE;
  TempBlocks blk;
  int rc;
  Profile P = { d_words, d_raw, NULL, n, first_ordinal, n_seqs, min_value, max_value, NULL };
  u32 *d_values = NULL;
  const u64 n_acc = 3 * n_seqs + 1;
  if ((rc = blk.get (ctx, (size_t) n_acc * 8, (void **) &P.acc))) return rc;
  if (prm->n_mm && (rc = blk.get (ctx, (size_t) n * 4, (void **) &d_values))) return rc;
  P.values = d_values;
  Index ix;
  size_index (gt4hip_query_index_list (qi), &ix);
  ix.off = (const u64 *) gt4hip_query_index_offsets (qi);
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], ctx->stream));
  hipLaunchKernelGGL (k_seq_zero, dim3 (gt4hip_grid (ctx, n_acc, MM_THREADS)), dim3 (MM_THREADS), 0, ctx->stream, P.acc, n_acc);
  HIPCHK (ctx, hipGetLastError ());
  if (prm->n_mm && (rc = gt4hip_query_lookup_device (ctx, who, qi, prm, (const uint64_t *) d_words, n, d_values, NULL))) return rc;
  const int grid = gt4hip_grid (ctx, tiles, 1);
  if (prm->n_mm) hipLaunchKernelGGL (k_seq_profile<false>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, P, ix, tiles);
  else hipLaunchKernelGGL (k_seq_profile<true>, dim3 (grid), dim3 (MM_THREADS), 0, ctx->stream, P, ix, tiles);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], ctx->stream));
  HIPCHK (ctx, hipMemcpyAsync (ctx->scratch_host, P.acc + 3 * n_seqs, 8, hipMemcpyDeviceToHost, ctx->stream));
  if ((rc = gt4hip_read_back (ctx, profiles, P.acc, (size_t) n_seqs * sizeof *profiles, "reading the sequences' sums back failed"))) return rc;
  float ms = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) gt4hip_query_index_set_ms (qi, ms);
  if (ctx->scratch_host[0])
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: the words' ordinals descend or leave [%llu, %llu + %llu)", who, (unsigned long long) first_ordinal,
                        (unsigned long long) first_ordinal, (unsigned long long) n_seqs);
  return GT4HIP_OK;
}

}  // namespace

static_assert (sizeof (gt4hip_seq_profile) == 24, "a sequence's three sums are read back as they lie on the device");

extern "C" int gt4hip_query_profile_words (gt4hip_context *ctx, gt4hip_query_index *qi, const uint64_t *d_words, const uint64_t *d_raw, uint64_t n,
                                           uint64_t first_ordinal, uint64_t n_seqs, const gt4hip_query_params *prm, uint32_t min_value, uint32_t max_value,
                                           gt4hip_seq_profile *profiles)
{
  const char *who = "gt4hip_query_profile_words";
  if (!ctx || !qi || !prm || (n && (!d_words || !d_raw)) || (n_seqs && !profiles)) return GT4HIP_EINVAL;
  const int rc = gt4hip_query_check_params (ctx, who, qi, prm);
  if (rc) return rc;
  if (((size_t) d_words | (size_t) d_raw) & 7) return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: device words must be 8-byte aligned", who);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  return profile_device (ctx, who, qi, (const u64 *) d_words, (const u64 *) d_raw, n, first_ordinal, n_seqs, prm, min_value, max_value, profiles);
}

extern "C" int gt4hip_query_profile_text (gt4hip_context *ctx, gt4hip_query_index *qi, const void *text, size_t n_bytes, unsigned flags,
                                          const gt4hip_query_params *prm, uint32_t min_value, uint32_t max_value, const gt4hip_locations_carry *in,
                                          gt4hip_locations_carry *out, gt4hip_locations_piece *piece, gt4hip_seq_profile *profiles, uint64_t capacity,
                                          uint64_t *n_profiles, uint64_t *error_offset)
{
  const char *who = "gt4hip_query_profile_text";
  if (!ctx || !qi || !prm || !out || !piece || !n_profiles || (capacity && !profiles) || (flags & ~(unsigned) GT4HIP_MAKER_TEXT_ON_DEVICE)) return GT4HIP_EINVAL;
  *n_profiles = 0;
  int rc = gt4hip_query_check_params (ctx, who, qi, prm);
  if (rc) return rc;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_query_index_set_ms (qi, 0);
  /* a word ends at a byte of its own: a piece holds no more words than bytes */
  TempBlocks blk;
  u64 *d_words = NULL;
  if (n_bytes >= ((size_t) 1 << 58)) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "%s: %zu bytes in one piece", who, n_bytes);
  if ((rc = blk.get (ctx, n_bytes * 16, (void **) &d_words))) return rc;
  u64 *d_raw = d_words + (n_bytes ? n_bytes : 1);
  rc = gt4hip_text_to_locations (ctx, text, n_bytes, gt4hip_query_index_list (qi)->word_length, flags, in, out, (uint64_t *) d_words, (uint64_t *) d_raw, n_bytes, piece, error_offset);
  if (rc) return rc;
  const u64 open = in && in->seq_open ? 1 : 0;
  const u64 first = (in ? in->n_subseqs : 0) - open;
  const u64 n_seqs = open + piece->n_subseqs;
  *n_profiles = n_seqs;
  if (n_seqs > capacity) return GT4HIP_OK;
  return profile_device (ctx, who, qi, d_words, d_raw, piece->n_words, first, n_seqs, prm, min_value, max_value, profiles);
}
