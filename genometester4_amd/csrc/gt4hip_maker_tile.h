/* gt4hip_maker_tile.h -- the reader's tile geometry and the state of the reader at a thread's first byte of a tile: what the
 * kernels of gt4hip_maker.hip share with the statistics pass of gt4hip_gmer.hip (k_mk_text_counts) and the masking passes of
 * gt4hip_mask.hip (k_mask_ends, k_mask_apply), which run on the arrays a call of the reader has just filled; and where words
 * end among a thread's codes (load_word_ends).  Include after gt4hip_device.h and gt4hip_host.h; internal linkage throughout. */
#ifndef GT4HIP_MAKER_TILE_H
#define GT4HIP_MAKER_TILE_H

namespace gt4 {
namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_PER = 16;                              /* bytes (codes) per thread */
constexpr u64 MK_TILE = (u64) MK_THREADS * MK_PER;      /* bytes of text per tile; codes per tile of the emit stage */
constexpr int MK_HALO = 32;                             /* codes in front of the first: the carry of the piece before */
static_assert (MK_TILE == GT4HIP_MAKER_TILE, "what the counters maker_text_tile / maker_code_tile report");

/* what the kernels hand to the host, and k_mk_summary to the kernels behind it */
struct MakerInfo {
  u64 nul_pos;  /* offset of the first NUL (the reference's end of file), n when there is none */
  u64 err;      /* smallest (offset << 3 | GT4HIP_MAKER_ERR_*), ~0 when the text is well formed */
  u64 n_codes;  /* codes of the text in front of nul_pos */
  u64 n_words;
  u32 in_name, phase, at_line_start, pad; /* the carries behind the last byte */
  /* gt4hip_text_to_locations alone (behind what the kernels of gt4hip_text_to_words read and write) */
  u64 n_events;  /* name starts, sequence starts and (FastQ) sequence ends of the text */
  u64 max_pos;   /* largest position of a word */
  u64 overflow;  /* a word's ordinal or position does not fit its raw field */
};

/* 16 bytes of text at `off` as four dwords; bytes at `limit` and behind read as 0 */
__device__ __forceinline__ void load16 (const unsigned char *__restrict__ text, u64 limit, u64 off, u32 w[4])
{
  if (off + MK_PER <= limit) {
    const u32x4 v = *(const u32x4 *) (text + off);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  } else {
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (int i = 0; i < MK_PER; i++)
      if (off + i < limit) w[i >> 2] |= (u32) text[off + i] << (8 * (i & 3));
  }
}

#define MK_BYTE(w, j) (((w)[(j) >> 2] >> (8 * ((j) & 3))) & 0xffu)

/* a thread's 16 bytes: bytes >= ' ', '\n's, and whether a '>' stands behind the last '\n' (anywhere when there is none) */
__device__ __forceinline__ void scan16 (const u32 w[4], u32 *kept, u32 *nl, u32 *tail)
{
  u32 k = 0, l = 0, t = 0;
#pragma unroll
  for (int j = 0; j < MK_PER; j++) {
    const u32 c = MK_BYTE (w, j);
    k += c >= 0x20u;
    if (c == '\n') l++, t = 0;
    if (c == '>') t = 1;
  }
  *kept = k, *nl = l, *tail = t;
}

/* (has a '\n', '>' behind the last '\n') of the lanes of a wavefront taken together */
__device__ __forceinline__ void wave_line_state (u64 m_nl, u64 m_tail, u32 *has, u32 *tail)
{
  *has = m_nl != 0;
  *tail = m_nl ? (m_tail >> (63 - __builtin_clzll (m_nl))) != 0 : m_tail != 0;
}

/* v summed over the workgroup's threads in front of this one, and over all of them; s_sum: MK_THREADS / WAVE words of LDS
 * that are free again at the caller's next barrier */
struct BlockScan { u32 before, total; };
__device__ __forceinline__ BlockScan block_scan (u32 v, u32 *s_sum)
{
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const u32 incl = dpp_inclusive_scan_u32 (v);
  if (lane == WAVE - 1) s_sum[wv] = incl;
  __syncthreads ();
  BlockScan r = { incl - v, 0 };
  for (int i = 0; i < MK_THREADS / WAVE; i++) {
    if (i < wv) r.before += s_sum[i];
    r.total += s_sum[i];
  }
  return r;
}

/* The state of the reader (src/fasta.c's machine) at a thread's first byte of tile t, from the thread's bytes, the
 * workgroup's and the tile's carries: what k_mk_codes and k_mk_events start their byte loops from. */
struct TileHead {
  u32 w[4];               /* the thread's 16 bytes, 0 at n_eff and behind */
  u32 rank, n_codes;      /* bytes >= ' ' of the tile in front of the thread, and of the whole tile */
  u32 phase, name;        /* lines so far mod 4; in a name */
};
__device__ __forceinline__ TileHead tile_head (const unsigned char *__restrict__ text, u64 n_eff, u64 off, const u32 *tile_state, u32 *s_sum, u32 *s_has, u32 *s_tail)
{
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  TileHead h;
  u32 kept, nl, tail;
  load16 (text, n_eff, off, h.w);
  scan16 (h.w, &kept, &nl, &tail);
  const u64 m_nl = __builtin_amdgcn_ballot_w64 (nl != 0), m_tail = __builtin_amdgcn_ballot_w64 (tail != 0);
  u32 has, wt;
  wave_line_state (m_nl, m_tail, &has, &wt);
  if (lane == 0) s_has[wv] = has, s_tail[wv] = wt;
  const BlockScan sc = block_scan (kept | (nl << 16), s_sum); /* both at most 4096 per tile */
  const u32 st = *tile_state;
  h.name = st & 1u;
  for (int i = 0; i < MK_THREADS / WAVE; i++)
    if (i < wv) h.name = s_has[i] ? s_tail[i] : (h.name | s_tail[i]);
  const u64 below = ((u64) 1 << lane) - 1, b_nl = m_nl & below, b_tail = m_tail & below;
  h.name = b_nl ? (b_tail >> (63 - __builtin_clzll (b_nl))) != 0 : (h.name | (b_tail != 0));
  h.rank = sc.before & 0xffffu;
  h.phase = ((st >> 1) + (sc.before >> 16)) & 3u;
  h.n_codes = sc.total & 0xffffu;
  return h;
}

/* `buf`: the halo's MK_HALO codes, then the text's (16-byte aligned).  w = the thread's 16 codes from j0 on and the MK_HALO
 * in front of them (all 4 where the thread has none); returns bit i set iff a word ends at code j0 + i, that is iff
 * codes j0 + i - k + 1 .. j0 + i are bases. */
__device__ __forceinline__ u32 load_word_ends (const unsigned char *__restrict__ buf, u64 j0, u64 n_codes, u32 k, u32 w[12])
{
  if (j0 < n_codes) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      const u32x4 v = *(const u32x4 *) (buf + j0 + 16 * q);
      w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 12; q++) w[q] = 0x04040404u;
  }
  u32 len = 0, ends = 0;
#pragma unroll
  for (int i = 0; i < MK_HALO + MK_PER; i++) {
    len = MK_BYTE (w, i) < 4u ? len + 1u : 0u;
    if (i >= MK_HALO && j0 + (u64) (i - MK_HALO) < n_codes && len >= k) ends |= 1u << (i - MK_HALO);
  }
  return ends;
}

}  // namespace
}  // namespace gt4

#endif
