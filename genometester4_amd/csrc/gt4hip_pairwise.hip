/*
 * gt4hip_pairwise.hip -- glistcompare L1 .. LN --pairwise: what every list shares with every other one.
 * gt4hip_table_pairwise reads a per-key count table as gt4hip_union_table leaves it, ragged or contiguous, and reduces it to
 * two n_lists x n_lists matrices: shared[i][j] = the words with a count other than 0 in list i and in list j, min_total[i][j] =
 * the sum over the words of the smaller of the two counts; gt4hip_pairwise_multi builds the table and hands it over.
 *
 * The table is walked in the segments gt4hip_table_select walks (gt4hip_table_walk.h); the keys are not read.  The list
 * columns are cut into BLOCKS of GT4HIP_PAIRWISE_BLOCK (32); a pass takes a pair of blocks (I, J), I <= J.  Up to 32 lists
 * are one block and one pass, in which every count is read exactly once; B blocks are B (B + 1) / 2 passes that read the
 * counts of B * B blocks between them: the table B times.  Two kernels live here:
 *   k_pairwise_partial<G, SAME>  one group of G lanes per row (G = the next power of two >= the block's columns, 2 .. 32),
 *                             consecutive lanes on consecutive dwords of the row, GT4HIP_PAIRWISE_UNROLL rows of a group in
 *                             flight.  Lane a keeps the diagonal of its own column in registers (SAME: I = J).  A ballot gives
 *                             every group the holders of its row in block J; lane a, where list a holds the word, walks the
 *                             holders b (SAME: b > a), gets their count from the lane that loaded it and adds 1 and
 *                             min (c_a, c_b) to the workgroup's G x G accumulators in LDS, 64 bits each: p holders cost
 *                             p (p - 1) / 2 updates, a row one list holds costs none.  At its end the workgroup writes its
 *                             accumulators to its own place in the workspace
 *   k_pairwise_reduce         sums the workgroups' partial matrices and writes both triangles of the block pair
 * No global atomic, and no word of the workspace or the matrices is read before the same call has written it.
 */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_table_walk.h"

#include <string.h>

namespace gt4 {
namespace {

constexpr int PW_THREADS = GT4HIP_PAIRWISE_THREADS;
constexpr int PW_UNR = GT4HIP_PAIRWISE_UNROLL; /* rows a lane group has in flight */
constexpr u32 PW_BLOCK = GT4HIP_PAIRWISE_BLOCK;
constexpr int PW_RED_THREADS = 1024;
constexpr int PW_RED_SLICES = PW_RED_THREADS / WAVE; /* the workgroups' partials are dealt to that many wavefronts */
static_assert (PW_BLOCK == 32, "a group's holders are a 32-bit mask");

/* a pass: the columns [col_i, col_i + n_i) against [col_j, col_j + n_j); the same block, or col_i < col_j */
struct PwPass {
  u32 col_i, n_i, col_j, n_j;
};

template <int G, bool SAME>
__global__ __launch_bounds__ (PW_THREADS) void k_pairwise_partial (SelTable t, PwPass b, u64 *__restrict__ ws)
{
  static_assert (G >= 2 && G <= 32 && (G & (G - 1)) == 0, "a power of two of lanes inside half a wavefront");
  constexpr u32 NG = PW_THREADS / G; /* groups, = rows a workgroup reads per step and row in flight */
  constexpr u32 GMASK = G == 32 ? 0xffffffffu : (1u << G) - 1u;
  __shared__ u64 acc_shared[G * G];
  __shared__ u64 acc_min[G * G];
  const u32 tid = threadIdx.x, grp = tid / G, j = tid % G;
  const u32 gshift = (tid & (WAVE - 1)) & ~(u32) (G - 1); /* the group's first lane in its wavefront */
  const bool has_i = j < b.n_i, has_j = j < b.n_j;
  for (u32 e = tid; e < (u32) (G * G); e += PW_THREADS) acc_shared[e] = acc_min[e] = 0;
  __syncthreads ();
  u64 d_shared = 0, d_min = 0; /* SAME: the diagonal of column j */
  for (u64 s = blockIdx.x; s < t.segments; s += gridDim.x) {
    u64 row_base, src_base;
    u32 rows;
    segment_of (t, s, row_base, src_base, rows);
    for (u32 base = 0; base < rows; base += NG * PW_UNR) { /* (the bound is the workgroup's: every lane reaches the ballots) */
      u32 ci[PW_UNR], cj[PW_UNR];
#pragma unroll
      for (int u = 0; u < PW_UNR; u++) {
        const u32 i = base + (u32) u * NG + grp;
        const bool valid = i < rows;
        const u32 *row = t.counts + (src_base + (valid ? i : 0u)) * t.n_lists;
        ci[u] = valid && has_i ? __builtin_nontemporal_load (row + b.col_i + j) : 0u;
        if (!SAME) cj[u] = valid && has_j ? __builtin_nontemporal_load (row + b.col_j + j) : 0u;
      }
#pragma unroll
      for (int u = 0; u < PW_UNR; u++) {
        const u32 a = ci[u], c = SAME ? ci[u] : cj[u];
        if (SAME) {
          d_shared += a != 0u;
          d_min += a;
        }
        u32 m = (u32) (__builtin_amdgcn_ballot_w64 (c != 0u) >> gshift) & GMASK; /* the holders of the group's row in block J */
        if (SAME) m &= ~((2u << j) - 1u);                                         /* ... above a */
        if (a == 0u) m = 0u;
        while (__builtin_amdgcn_ballot_w64 (m != 0u)) { /* (the wavefront's: every lane serves the reads of the others) */
          const u32 bb = m ? (u32) __builtin_ctz (m) : 0u;
          const u32 cb = (u32) __shfl ((int) c, (int) (gshift + bb), WAVE);
          if (m) {
            atomicAdd (&acc_shared[j * G + bb], (u64) 1);
            atomicAdd (&acc_min[j * G + bb], (u64) (a < cb ? a : cb));
            m &= m - 1u;
          }
        }
      }
    }
  }
  if (SAME && has_i) {
    atomicAdd (&acc_shared[j * G + j], d_shared);
    atomicAdd (&acc_min[j * G + j], d_min);
  }
  __syncthreads ();
  u64 *mine = ws + (u64) blockIdx.x * (2 * G * G);
  for (u32 e = tid; e < (u32) (G * G); e += PW_THREADS) {
    mine[e] = acc_shared[e];
    mine[G * G + e] = acc_min[e];
  }
}

/* cell e of the 2 x G x G partials (the shared matrix, then the sums), summed over the workgroups: 64 cells a workgroup,
 * the partials dealt to its wavefronts.  Writes [i][j] and [j][i] of the n x n matrices. */
__global__ __launch_bounds__ (PW_RED_THREADS) void k_pairwise_reduce (const u64 *__restrict__ ws, u32 n_wg, u32 g, PwPass b, u32 same, u32 n,
                                                                      u64 *__restrict__ out_shared, u64 *__restrict__ out_min)
{
  __shared__ u64 part[PW_RED_SLICES][WAVE];
  const u32 lane = threadIdx.x & (WAVE - 1), slice = threadIdx.x / WAVE;
  const u32 cells = g * g, e = blockIdx.x * WAVE + lane;
  u64 sum = 0;
  if (e < 2 * cells)
    for (u32 w = slice; w < n_wg; w += PW_RED_SLICES) sum += ws[(u64) w * (2 * cells) + e];
  part[slice][lane] = sum;
  __syncthreads ();
  if (slice != 0 || e >= 2 * cells) return;
  sum = 0;
  for (int q = 0; q < PW_RED_SLICES; q++) sum += part[q][lane];
  const u32 c = e % cells, a = c / g, bb = c % g;
  if (a >= b.n_i || bb >= b.n_j || (same && a > bb)) return;
  u64 *out = e < cells ? out_shared : out_min;
  const u64 i = b.col_i + a, k = b.col_j + bb;
  out[i * n + k] = sum;
  out[k * n + i] = sum;
}

}  // namespace
}  // namespace gt4

using namespace gt4;

namespace {

template <int G>
void launch_partial (bool same, dim3 grid, hipStream_t st, const SelTable &t, const PwPass &b, u64 *ws)
{
  if (same) hipLaunchKernelGGL ((k_pairwise_partial<G, true>), grid, dim3 (PW_THREADS), 0, st, t, b, ws);
  else if (G == 32) hipLaunchKernelGGL ((k_pairwise_partial<32, false>), grid, dim3 (PW_THREADS), 0, st, t, b, ws);
}

void zero_matrices (uint32_t n, uint64_t *host_shared, uint64_t *host_min_total, float *device_ms)
{
  memset (host_shared, 0, (size_t) n * n * 8);
  memset (host_min_total, 0, (size_t) n * n * 8);
  if (device_ms) *device_ms = 0;
}

int table_pairwise (gt4hip_context *ctx, const gt4hip_count_table *table, uint64_t *host_shared, uint64_t *host_min_total, float *device_ms)
{
  const u32 n = table->n_lists;
  if (!n) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_table_pairwise: a table of no lists");
  if (table->n_keys && (!table->device_keys || !table->device_counts))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_table_pairwise: a table of %llu keys without its arrays", (unsigned long long) table->n_keys);
  const SelTable t = table_walk (table);
  if (!t.n_keys || !t.segments) return zero_matrices (n, host_shared, host_min_total, device_ms), GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  hipStream_t st = ctx->stream;

  u32 g = 2; /* lanes per row: the next power of two that holds a block's columns */
  while (g < (n < PW_BLOCK ? n : PW_BLOCK)) g *= 2;
  const dim3 grid ((unsigned) gt4hip_grid (ctx, t.segments));
  const size_t cells = (size_t) n * n;
  TempBlocks blk;
  u64 *ws = NULL, *out = NULL;
  int rc = blk.get (ctx, (size_t) grid.x * 2 * g * g * 8, (void **) &ws);
  if (!rc) rc = blk.get (ctx, 2 * cells * 8, (void **) &out);
  if (rc) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_table_pairwise: the workspace of %u workgroups and the matrices of %u lists", grid.x, n);

  const u32 n_blocks = (n + PW_BLOCK - 1) / PW_BLOCK;
  const dim3 red_grid ((2 * g * g + WAVE - 1) / WAVE);
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], st));
  for (u32 bi = 0; bi < n_blocks; bi++)
    for (u32 bj = bi; bj < n_blocks; bj++) {
      const u32 ci = bi * PW_BLOCK, cj = bj * PW_BLOCK;
      const PwPass b = { ci, n - ci < PW_BLOCK ? n - ci : PW_BLOCK, cj, n - cj < PW_BLOCK ? n - cj : PW_BLOCK };
      const bool same = bi == bj;
      if (bi || bj) gt4hip_grid_again (ctx, t.segments, (int) grid.x);
      switch (g) {
        case 2: launch_partial<2> (same, grid, st, t, b, ws); break;
        case 4: launch_partial<4> (same, grid, st, t, b, ws); break;
        case 8: launch_partial<8> (same, grid, st, t, b, ws); break;
        case 16: launch_partial<16> (same, grid, st, t, b, ws); break;
        default: launch_partial<32> (same, grid, st, t, b, ws); break;
      }
      HIPCHK (ctx, hipGetLastError ());
      hipLaunchKernelGGL (k_pairwise_reduce, red_grid, dim3 (PW_RED_THREADS), 0, st, (const u64 *) ws, grid.x, g, b, same ? 1u : 0u, n, out, out + cells);
      HIPCHK (ctx, hipGetLastError ());
    }
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], st));
  if ((rc = gt4hip_read_back (ctx, host_shared, out, cells * 8, "reading the shared matrix back failed"))) return rc;
  if ((rc = gt4hip_read_back (ctx, host_min_total, out + cells, cells * 8, "reading the min_total matrix back failed"))) return rc;
  float ms = 0;
  HIPCHK (ctx, hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]));
  if (device_ms) *device_ms = ms;
  return GT4HIP_OK;
}

}  // namespace

extern "C" int gt4hip_table_pairwise (gt4hip_context *ctx, const gt4hip_count_table *table, uint64_t *host_shared, uint64_t *host_min_total, float *device_ms)
{
  if (!ctx || !table || !host_shared || !host_min_total) return GT4HIP_EINVAL;
  return table_pairwise (ctx, table, host_shared, host_min_total, device_ms);
}

extern "C" int gt4hip_pairwise_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, uint64_t *host_shared,
                                       uint64_t *host_min_total, float *device_ms)
{
  if (!ctx || !lists || !n_lists || !host_shared || !host_min_total) return GT4HIP_EINVAL;
  TempTable t;
  const int rc = gt4hip_union_table_checked (ctx, lists, n_lists, &t.table);
  if (rc) return rc;
  return table_pairwise (ctx, &t.table, host_shared, host_min_total, device_ms);
}
