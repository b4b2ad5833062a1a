/* gt4hip_nway_rows8.h -- up to EIGHT lists per launch: the partition's row kernels and k_nway_need (a partition row is
 * ten entries: a lane per entry, a thread per tile).  Included by gt4hip_nway_part.h (GT4_KM_ROWS). */
__global__ __launch_bounds__ (256) void k_nway_sample_counts (const u32 *__restrict__ merged, u64 m_total, u32 G, u64 n_brackets, u32 *__restrict__ cnt)
{
  const int lane = threadIdx.x & 63;
  const u64 br = (u64) blockIdx.x * 4 + (threadIdx.x >> 6);
  if (br >= n_brackets) return;
  const u64 first = br * NWAY_BRACKET * G, end = first + (u64) NWAY_BRACKET * G < m_total ? first + (u64) NWAY_BRACKET * G : m_total;
  u64 c0 = 0, c1 = 0; /* 16-bit fields: lists 0..3, 4..7 (a bracket has at most 64 * 32 samples) */
  for (u64 j = first + lane; j < end; j += WAVE) {
    const u32 id = merged[3 * j + 2];
    const u64 one = 1ull << (16 * (id & 3u));
    c0 += id < 4u ? one : 0ull;
    c1 += id < 4u ? 0ull : one;
  }
  c0 = wave_sum (c0);
  c1 = wave_sum (c1);
  if (lane < NWAY_MAX) cnt[br * NWAY_MAX + lane] = (u32) (((lane < 4 ? c0 : c1) >> (16 * (lane & 3))) & 0xffffu);
}

__global__ __launch_bounds__ (64 * NWAY_MAX) void k_nway_bracket_bases (u32 *__restrict__ cnt, u64 n_brackets)
{
  nway_bracket_prefix (cnt, n_brackets, threadIdx.x >> 6, threadIdx.x & 63); /* a wavefront per list */
}

constexpr u32 NWAY_G_MAX = 32; /* samples per tile the bracket's LDS copy has room for */

__global__ __launch_bounds__ (64) void k_nway_partition_rows (NwayParams p, const u32 *__restrict__ merged, u64 m_total, u32 G, u32 n_buckets, const u32 *__restrict__ bases,
                                                           u64 *__restrict__ part)
{
  __shared__ u32x4 smp4[NWAY_BRACKET * NWAY_G_MAX * 3 / 4]; /* the bracket's samples: read once, 16 bytes per lane and instruction */
  const u32 *const smp = reinterpret_cast<const u32 *> (smp4);
  const int lane = threadIdx.x;
  const u64 br = blockIdx.x;
  const u64 t = br * NWAY_BRACKET + lane;
  {
    const u64 f = br * NWAY_BRACKET * G;
    const u64 cnt = f >= m_total ? 0 : (m_total - f < (u64) NWAY_BRACKET * G ? m_total - f : (u64) NWAY_BRACKET * G);
    const u32 quads = (u32) ((3 * cnt + 3) / 4); /* (the list's allocation is a multiple of 16 bytes and f * 12 is one too) */
    const u32x4 *src = reinterpret_cast<const u32x4 *> (merged + 3 * f);
    for (u32 i = lane; i < quads; i += WAVE) smp4[i] = src[i];
    __syncthreads ();
  }
  const u64 nt = p.num_tiles;
  const bool row = t <= nt;
  /* boundary keys in front of this tile and behind it */
  const bool has_x = row && t > 0 && t < nt, has_y = row && t + 1 < nt;
  const u64 x = has_x ? nway_boundary_key (merged, m_total, G, p.num_tiles, t) : 0ull;
  const u64 y = has_y ? nway_boundary_key (merged, m_total, G, p.num_tiles, t + 1) : 0ull;
  /* the list the boundary sample came from: its cut is behind that very sample, no search */
  const u32 x_list = has_x ? merged[3 * (t == nt - 1 ? m_total - 1 : t * (u64) G - 1) + 2] : 0xffffffffu;
  /* the tile's key range and bucket function (as k_nway_partition) */
  u64 lo_key = 0, bk = 0;
  const bool tile = row && t < nt;
  u64 c0 = 0, c1 = 0; /* the tile's own samples per list: 16-bit fields, lists 0..3 and 4..7 */
  if (tile) {
    lo_key = t == 0 ? nway_first_key (p) : x + 1ull;
    const u64 hi = t + 1 == nt ? nway_last_key (p) : y;
    bk = nway_bucket_consts (lo_key, hi, n_buckets);
    /* the tile's own samples: counts per list, and whether the interpolation will work on them */
    const u64 first = t * (u64) G, end = first >= m_total ? first : (first + G < m_total ? first + G : m_total);
    NwayClusterTest test (lo_key, hi, bk);
    for (u64 j0 = first; j0 < end; j0 += 8) { /* (eight samples asked for at once) */
      u64 sk[8];
      u32 sid[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const u32 j = (u32) ((j0 + u < end ? j0 + u : end - 1) - br * NWAY_BRACKET * G);
        sk[u] = (u64) smp[3 * j] | ((u64) smp[3 * j + 1] << 32);
        sid[u] = smp[3 * j + 2];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (j0 + u >= end) continue;
        const u64 one = 1ull << (16 * (sid[u] & 3u));
        c0 += sid[u] < 4u ? one : 0ull;
        c1 += sid[u] < 4u ? 0ull : one;
        test.add (sk[u]);
      }
    }
    if (t + 1 < nt && test.clustered ()) bk |= 1ull << 9;
  }
  /* samples in front of the tile = the bracket's base + the earlier lanes' (every lane takes part) */
  c0 = wave_inclusive_scan (c0, lane) - c0;
  c1 = wave_inclusive_scan (c1, lane) - c1;
  if (tile) {
    u64 a[8];
    nway_cut_search8 (p, 0, t, x, x_list, bases + br * NWAY_MAX, c0, c1, a);
#pragma unroll
    for (int i = 0; i < NWAY_MAX; i++) part[t * NWAY_PSTRIDE + i] = a[i];
    part[t * NWAY_PSTRIDE + NWAY_MAX] = lo_key;
    part[t * NWAY_PSTRIDE + NWAY_MAX + 1] = bk;
  } else if (row) { /* t == num_tiles: the lists' ends */
    for (u32 i = 0; i < NWAY_MAX; i++) part[t * NWAY_PSTRIDE + i] = i < p.k ? p.n[i] : 0ull;
    part[t * NWAY_PSTRIDE + NWAY_MAX] = 0;
    part[t * NWAY_PSTRIDE + NWAY_MAX + 1] = 0;
  }
}

__device__ __forceinline__ u32 nway_tile_slots (const u64 *__restrict__ part, u64 t, bool *mono)
{
  u64 slots = 0;
  for (int i = 0; i < NWAY_MAX; i++) {
    const u64 a = part[t * NWAY_PSTRIDE + i], b = part[(t + 1) * NWAY_PSTRIDE + i];
    *mono &= b >= a;
    slots += (b - a + NWAY_HS - 1) / NWAY_HS;
  }
  return slots > 0xffffffffull ? 0xffffffffu : (u32) slots;
}

/* flag[0]: a tile needs more than two pieces (or the table is not monotone); flag[1]: tiles whose samples look
 * clustered; flag[2]: tiles cut in two */
__global__ __launch_bounds__ (NWAY_SPLIT_BLOCK) void k_nway_need (const u64 *__restrict__ part, u32 num_tiles, u32 nch, u32 *__restrict__ need, u32 *__restrict__ block_sums, u32 *flag)
{
  __shared__ u32 ws[NWAY_SPLIT_BLOCK / WAVE];
  const u64 t = (u64) blockIdx.x * NWAY_SPLIT_BLOCK + threadIdx.x;
  u32 v = 0;
  if (t < num_tiles) {
    bool mono = true;
    const u32 slots = nway_tile_slots (part, t, &mono);
    v = slots <= nch ? 1u : 2u;
    if (!mono || slots > 2 * nch - 2 * NWAY_MAX) atomicOr (flag, 1u); /* (each half rounds every run up once more) */
    if ((part[t * NWAY_PSTRIDE + NWAY_MAX + 1] >> 9) & 1ull) atomicAdd (flag + 1, 1u);
    if (v == 2u) atomicAdd (flag + 2, 1u);
    need[t] = v;
  }
  v = dpp_wave_sum_u32 (v);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x / WAVE] = v;
  __syncthreads ();
  if (threadIdx.x == 0) {
    u32 sum = 0;
    for (u32 w = 0; w < NWAY_SPLIT_BLOCK / WAVE; w++) sum += ws[w];
    block_sums[blockIdx.x] = sum;
  }
}
