/* gt4hip_internal.h -- shared between the kernel file and the C-ABI implementation. */
#ifndef GT4HIP_INTERNAL_H
#define GT4HIP_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gt4hip_pair_variant.h"

/* The one compile-time switch of the device code: the diagnostics build (`make prof`, -DGT4_PROFILE_PHASES=<thread whose
 * phases are stamped>) keeps what PROF (...) encloses -- phase stamps, scanner and resolve statistics; the product build
 * drops it. */
#ifdef GT4_PROFILE_PHASES
#define PROF(...) __VA_ARGS__
#else
#define PROF(...)
#endif

namespace gt4 {

struct PairOutputs {
  uint32_t *rec[4];        /* packed 12-byte records as dwords; may be null in count mode */
};

/* Control block in device memory, zeroed before every launch. */
struct PairControl {
  unsigned long long n_words[4];
  unsigned long long total_count[4];
  unsigned int ticket;     /* dynamic dealing: next tile */
  unsigned int error;      /* non-zero: a bounded spin gave up / consistency check tripped */
  unsigned int role;       /* first workgroup to arrive becomes the scanner */
  unsigned int pad;
  unsigned long long phase_cycles[24];
  unsigned long long resolve_stats[8]; /* diagnostic builds: sampled resolve calls, spins, -, agg/carry not ready at first look; scanner rounds, rows retired on the first look, rows */ /* diagnostic builds (-DGT4_PROFILE_PHASES): shader cycles per phase, summed over workgroups */
};

/* What the partition launch zeroes for the merge launch behind it, in 16-byte chunks: ctl_chunks of the control block, and
 * for every stream in `ops` the words of the chained scan as k_pair_merge lays them out in desc for `rows` rows of 64
 * tiles: agg u32[4][rows * 64], carry u64[4][rows + 1], rowsum u64[4][rows] (a stream's carries and row sums widened to
 * whole chunks, into a neighbour stream's words: the merge either finds those zeroed too or never reads them).
 * ctl_chunks 0 and ops 0: nothing. */
struct PartZero {
  void *ctl;
  uint32_t ctl_chunks, ops;
  unsigned long long *desc;
  uint64_t rows;
};

/* A context's limit on the grids of its striding kernels: option "grid_cap" (tests; 0 = none) and counter "grid_capped". */
struct GridLimit {
  int64_t cap;
  uint64_t capped;
};

/* workgroups of a kernel that strides over `blocks` blocks of work: one each, at most `most` and at most the context's
 * "grid_cap", at least one; a launch that gets fewer than it has blocks is counted in "grid_capped" */
inline int strided_grid (GridLimit &lim, uint64_t blocks, uint64_t most)
{
  if (lim.cap > 0 && (uint64_t) lim.cap < most) most = (uint64_t) lim.cap;
  const uint64_t g = blocks < 1 ? 1 : blocks < most ? blocks : most;
  if (blocks > g) lim.capped++;
  return (int) g;
}

/* threads per workgroup of the list utilities at the end of gt4hip_kernels.hip (counter "list_threads") */
#define GT4HIP_LIST_THREADS 256

/* guided: the co-rank searches place their probes from the coarse neighbours (gt4hip_corank.h); false: plain bisection */
hipError_t launch_partition (hipStream_t s, const uint32_t *A, uint64_t nA, const uint32_t *B, uint64_t nB,
                             uint64_t num_tiles, uint64_t tile_records, uint64_t *part, bool guided, const PartZero &zero);
hipError_t launch_pair_merge (hipStream_t s, const PairVariant &v, int grid, const uint32_t *A, uint64_t nA,
                              const uint32_t *B, uint64_t nB, const uint64_t *part, uint64_t num_tiles,
                              const PairParams &p, const PairOutputs &o, unsigned long long *desc,
                              PairControl *ctl);
hipError_t launch_scan_tiles (hipStream_t s, unsigned long long *desc, uint64_t num_tiles,
                              unsigned long long *block_sums);
hipError_t launch_generate (hipStream_t s, GridLimit &lim, uint32_t *rec, uint64_t n, uint64_t stride, uint64_t seed,
                            uint64_t count_seed, uint32_t max_count, uint64_t mult, uint64_t add);
hipError_t launch_sum_counts (hipStream_t s, GridLimit &lim, const uint32_t *rec, uint64_t n, unsigned long long *sum);
hipError_t launch_check_sorted (hipStream_t s, GridLimit &lim, const uint32_t *rec, uint64_t n, unsigned int *bad);
hipError_t launch_lower_bound (hipStream_t s, const uint32_t *rec, uint64_t n, uint64_t key,
                               unsigned long long *idx);
hipError_t launch_extract_column (hipStream_t s, GridLimit &lim, const uint32_t *rec, uint64_t n, uint32_t *counts, uint32_t n_lists, uint32_t column);
hipError_t launch_extract_keys (hipStream_t s, GridLimit &lim, const uint32_t *rec, uint64_t n, unsigned long long *keys);
hipError_t launch_decode_index (hipStream_t s, GridLimit &lim, const unsigned long long *kmers, uint64_t n, uint64_t num_locations, uint32_t *rec);

int merge_blocks_per_cu (const PairVariant &v);

}  // namespace gt4

#endif
