/* gt4hip_maker.hip -- glistmaker's front on the device: FastA / FastQ text in HBM -> packed k-mer words
 * (gt4hip_text_to_words), and with the table step of gt4hip_sort.hip behind it, text -> list (gt4hip_text_to_list).
 * gt4hip_text_to_locations is the same reader for glistmaker --index: beside every word where it stands, and the text's
 * name and sequence boundaries for the file block (the second half of the kernels below).
 *
 * The reader restated is fasta_reader_read_nwords (reference src/fasta.c:87-291), a byte-serial state machine.  Every
 * decision in it is local once two carries are known at the start of a tile of text: FastA "a '>' was seen on this line"
 * (every byte from the first '>' of a line to its '\n' is name), FastQ "lines so far mod 4" (name, sequence, '+' line,
 * quality).  Stages, each a streaming pass over tiles of MK_TILE bytes (16 per thread, text order inside a thread):
 *
 *   k_mk_summary     per tile: bytes >= ' ' (each becomes one code), '\n's, '>' behind the last '\n'; first NUL (atomicMin)
 *   k_tile_scan      (gt4hip_index.h) tile counts -> where each tile's codes start
 *   k_mk_state_scan  the two carries at the start of every tile (one workgroup; a name may cover whole tiles)
 *   k_mk_codes       classify + compact: one byte per text byte >= ' ', 0..3 = a base of a sequence line, 4 = anything that
 *                    resets the run (other characters, and every byte of a name, '+' or quality line: names and FastQ's
 *                    three other lines always hold such a byte, so the run ends there as in the reference); bytes < ' '
 *                    leave nothing, which is how words span line breaks (:258).  FastQ's tag checks (:201, :276) as the
 *                    smallest offending offset (atomicMin).  The tile that holds the last byte of the text writes the
 *                    carries out.
 *   k_mk_emit<0>     a word ends at code j iff codes j-k+1..j are bases: counted per tile of MK_TILE codes; every thread reads
 *                    its 16 codes and the 32 before them (k - 1 <= 31 are needed: no chain between threads or tiles)
 *   k_tile_scan      word counts -> where each tile's words start
 *   k_mk_emit<1>     the words (forward word masked to 2k bits, reverse complement rolled as :233-234, the smaller of the
 *                    two unless FORWARD_ONLY), staged in LDS and written out in order
 *
 * k_tile_count of gt4hip_index.h is not used: it counts a 4-byte flag per item, which would cost more traffic than
 * the text itself; the counts here come out of the classification.  Algorithmic bytes per text byte: 1 + 1 read, 1
 * written (codes), 1 read (emit, twice: count and write) and 8 written per word. */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"

#include <stdlib.h>
#include <string.h>

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

/* c2n of src/fasta.c:66-69, 4 for everything else */
__device__ __forceinline__ u32 nuc_code (u32 c)
{
  c |= 0x20u;
  return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : (c == 't' || c == 'u') ? 3u : 4u;
}

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

__global__ __launch_bounds__ (MK_THREADS) void k_mk_summary (const unsigned char *__restrict__ text, u64 n, u64 n_tiles, u32 *tile_cnt, u32 *tile_info,
                                                             MakerInfo *info)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE], s_has[MK_THREADS / WAVE], s_tail[MK_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[4], kept, nl, tail;
    load16 (text, n, off, w);
    scan16 (w, &kept, &nl, &tail);
    int z = MK_PER;
#pragma unroll
    for (int j = MK_PER - 1; j >= 0; j--)
      if (MK_BYTE (w, j) == 0 && off + j < n) z = j;
    if (z < MK_PER) atomicMin (&info->nul_pos, off + (u64) z);
    const u32 sum = dpp_wave_sum_u32 (kept | (nl << 16)); /* both at most 4096 per tile */
    u32 has, wt;
    wave_line_state (__builtin_amdgcn_ballot_w64 (nl != 0), __builtin_amdgcn_ballot_w64 (tail != 0), &has, &wt);
    if (lane == 0) s_sum[wv] = sum, s_has[wv] = has, s_tail[wv] = wt;
    __syncthreads ();
    if (threadIdx.x == 0) {
      u32 s = 0, tl = 0;
      for (int i = 0; i < MK_THREADS / WAVE; i++) {
        s += s_sum[i];
        tl = s_has[i] ? s_tail[i] : (tl | s_tail[i]);
      }
      tile_cnt[t] = s & 0xffffu;
      tile_info[t] = (s >> 16) | (tl << 31);
    }
    __syncthreads ();
  }
}

/* tile_state[t] = (in a name) | (lines so far mod 4) << 1 at the first byte of tile t; one workgroup, a stretch of tiles per thread */
__global__ __launch_bounds__ (1024) void k_mk_state_scan (const u32 *tile_info, u64 n_tiles, u32 in_name0, u32 phase0, u32 *tile_state)
{
  __shared__ u32 c_nl[1024], c_has[1024], c_tail[1024];
  const u64 per = (n_tiles + 1023) / 1024;
  const u64 first = (u64) threadIdx.x * per, last = first + per < n_tiles ? first + per : n_tiles;
  u32 nl = 0, has = 0, tail = 0;
  for (u64 t = first; t < last; t++) {
    const u32 v = tile_info[t], l = v & 0x7fffffffu, tl = v >> 31;
    nl += l;
    tail = l ? tl : (tail | tl);
    has |= l != 0;
  }
  c_nl[threadIdx.x] = nl, c_has[threadIdx.x] = has, c_tail[threadIdx.x] = tail;
  __syncthreads ();
  if (threadIdx.x == 0) {
    u32 name = in_name0, ph = phase0;
    for (int i = 0; i < 1024; i++) {
      const u32 l = c_nl[i], h = c_has[i], tl = c_tail[i];
      c_nl[i] = ph, c_tail[i] = name;
      ph = (ph + l) & 3u;
      name = h ? tl : (name | tl);
    }
  }
  __syncthreads ();
  u32 name = c_tail[threadIdx.x], ph = c_nl[threadIdx.x];
  for (u64 t = first; t < last; t++) {
    const u32 v = tile_info[t], l = v & 0x7fffffffu, tl = v >> 31;
    tile_state[t] = name | (ph << 1);
    ph = (ph + l) & 3u;
    name = l ? tl : (name | tl);
  }
}

/* `codes` is the code of the text's first byte >= ' ' (the halo lies in front of it) */
template <bool FASTQ>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_codes (const unsigned char *__restrict__ text, u64 n, u64 n_tiles, const u64 *tile_off, const u32 *tile_state,
                                                           u32 at_line_start0, unsigned char *codes, MakerInfo *info)
{
  __shared__ unsigned char out[MK_TILE];
  __shared__ u32 s_sum[MK_THREADS / WAVE], s_has[MK_THREADS / WAVE], s_tail[MK_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (t * MK_TILE >= n_eff) break; /* (uniform: every later tile of this workgroup lies behind the end as well) */
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[4], kept, nl, tail;
    load16 (text, n_eff, off, w);
    scan16 (w, &kept, &nl, &tail);
    const u32 incl = dpp_inclusive_scan_u32 (kept | (nl << 16));
    const u64 m_nl = __builtin_amdgcn_ballot_w64 (nl != 0), m_tail = __builtin_amdgcn_ballot_w64 (tail != 0);
    u32 has, wt;
    wave_line_state (m_nl, m_tail, &has, &wt);
    if (lane == WAVE - 1) s_sum[wv] = incl;
    if (lane == 0) s_has[wv] = has, s_tail[wv] = wt;
    __syncthreads ();
    const u32 st = tile_state[t];
    u32 before = 0, total = 0, name = st & 1u;
    for (int i = 0; i < MK_THREADS / WAVE; i++) {
      if (i < wv) {
        before += s_sum[i];
        name = s_has[i] ? s_tail[i] : (name | s_tail[i]);
      }
      total += s_sum[i];
    }
    const u32 excl = before + incl - (kept | (nl << 16));
    u32 rank = excl & 0xffffu;
    u32 phase = ((st >> 1) + (excl >> 16)) & 3u;
    {
      const u64 below = ((u64) 1 << lane) - 1, b_nl = m_nl & below, b_tail = m_tail & below;
      name = b_nl ? (b_tail >> (63 - __builtin_clzll (b_nl))) != 0 : (name | (b_tail != 0));
    }
    u32 pnl = 0;
    if (FASTQ && off < n_eff) pnl = off ? text[off - 1] == '\n' : at_line_start0;
#pragma unroll
    for (int j = 0; j < MK_PER; j++) {
      const u32 c = MK_BYTE (w, j);
      const u64 p = off + j;
      if (p < n_eff) {
        u32 code;
        if (FASTQ) {
          if (pnl && phase == 2u && c != '+') atomicMin (&info->err, (p << 3) | GT4HIP_MAKER_ERR_PLUS);
          if (pnl && phase == 0u && c != '@') atomicMin (&info->err, (p << 3) | GT4HIP_MAKER_ERR_AT);
          code = phase == 1u ? nuc_code (c) : 4u;
          pnl = c == '\n';
          if (pnl) phase = (phase + 1u) & 3u;
        } else {
          if (c == '\n') name = 0;
          if (c == '>') name = 1;
          code = name ? 4u : nuc_code (c);
        }
        if (c >= 0x20u) out[rank++] = (unsigned char) code;
        if (p == n_eff - 1) {
          info->in_name = name;
          info->phase = phase;
          info->at_line_start = c == '\n';
          info->n_codes = tile_off[t] + rank;
        }
      }
    }
    __syncthreads ();
    /* the tile's codes to their place: single bytes up to a dword boundary, dwords, single bytes */
    const u32 m = total & 0xffffu;
    unsigned char *dst = codes + tile_off[t];
    u32 head = (u32) (4u - ((size_t) dst & 3u)) & 3u;
    if (head > m) head = m;
    const u32 nd = (m - head) >> 2, rest = (m - head) & 3u;
    if (threadIdx.x < head) dst[threadIdx.x] = out[threadIdx.x];
    for (u32 j = threadIdx.x; j < nd; j += MK_THREADS) {
      const unsigned char *s = out + head + 4 * j;
      *(u32 *) (dst + head + 4 * j) = (u32) s[0] | ((u32) s[1] << 8) | ((u32) s[2] << 16) | ((u32) s[3] << 24);
    }
    if (threadIdx.x < rest) dst[head + 4 * nd + threadIdx.x] = out[head + 4 * nd + threadIdx.x];
    __syncthreads ();
  }
}

/* `buf`: the halo's MK_HALO codes, then the text's (16-byte aligned).  WRITE = false: tile_cnt[t] = words that end in tile t. */
template <bool WRITE>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_emit (const unsigned char *__restrict__ buf, const MakerInfo *info, u64 n_tiles, u32 k, u32 forward_only,
                                                          u32 *tile_cnt, const u64 *tile_off, u64 *words)
{
  __shared__ u64 stage[WRITE ? MK_TILE : 1];
  __shared__ u32 s_sum[MK_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const u64 n_codes = info->n_codes;
  const u64 mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 j0 = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[12];
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
    u32 len = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < MK_HALO + MK_PER; i++) {
      const u32 c = MK_BYTE (w, i);
      len = c < 4u ? len + 1u : 0u;
      if (i >= MK_HALO && j0 + (u64) (i - MK_HALO) < n_codes && len >= k) cnt++;
    }
    const u32 incl = dpp_inclusive_scan_u32 (cnt);
    if (lane == WAVE - 1) s_sum[wv] = incl;
    __syncthreads ();
    u32 before = 0, total = 0;
    for (int i = 0; i < MK_THREADS / WAVE; i++) {
      if (i < wv) before += s_sum[i];
      total += s_sum[i];
    }
    if (!WRITE) {
      if (threadIdx.x == 0) tile_cnt[t] = total;
    } else {
      u32 rank = before + incl - cnt;
      u64 fw = 0, rv = 0;
      len = 0;
#pragma unroll
      for (int i = 0; i < MK_HALO + MK_PER; i++) {
        const u32 c = MK_BYTE (w, i);
        fw = (fw << 2) | (c & 3u);
        rv = (rv >> 2) | ((u64) (~c & 3u) << (2 * (k - 1)));
        len = c < 4u ? len + 1u : 0u;
        if (i >= MK_HALO && j0 + (u64) (i - MK_HALO) < n_codes && len >= k) {
          const u64 f = fw & mask;
          stage[rank++] = forward_only || f < rv ? f : rv;
        }
      }
      __syncthreads ();
      u64 *dst = words + tile_off[t];
      for (u32 j = threadIdx.x; j < total; j += MK_THREADS) dst[j] = stage[j];
    }
    __syncthreads ();
  }
}

/* ---- locations (glistmaker --index): where every word stands, and the subsequences of the file block
 *
 * The reader's callbacks for an index (reference src/glistmaker.c:1031-1067) need three things per word: the ordinal of
 * its sequence within the file, its position -- bytes >= ' ' of the sequence in front of the word's first base (:1064,
 * src/fasta.c:254-264), which is the distance in codes from the sequence's start, since the codes of a sequence are
 * contiguous in the code stream -- and the strand.  So the text's *events* are compacted, in text order, each with the
 * index of the code that follows it:
 *   FastA  0 a '>' outside a name (the name starts behind it), 1 the '\n' that ends a name (the sequence starts behind it);
 *          they alternate, so event g of a file is a sequence start iff g is odd, and that sequence's ordinal is g / 2
 *   FastQ  1 the '\n' of a name line, 2 the '\n' of a sequence line (the sequence ends), 0 the '\n' of a quality line (a
 *          name starts two bytes on); event g is a sequence start iff g % 3 == 0, ordinal g / 3
 * A word that ends at code j lies in the sequence of the last event whose code index is <= j: every name and every
 * '+' / quality line holds a code that ends the run, so no other event can lie between a word and its sequence's start.
 * The host puts the 28-byte records of the file block together from the same events (a name or a sequence may cover any
 * number of tiles or pieces: the open record travels in the carry).
 *   k_mk_events<.., 0>  events per tile of text (the classification of k_mk_codes again, nothing written)
 *   k_tile_scan         -> where each tile's events go
 *   k_mk_events<.., 1>  (offset in the file << 2 | kind, index of the next code) per event
 *   k_mk_emit_loc       k_mk_emit<1> with, beside every word, ordinal << 33 | position << 1 | strand */
/* 1 when the byte c is x, as arithmetic: sixteen compares a thread would each hold a pair of scalar registers */
#define IS_BYTE(c, x) ((((c) ^ (u32) (x)) - 1u) >> 31)

template <bool FASTQ, bool WRITE>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_events (const unsigned char *__restrict__ text, u64 n, u64 n_tiles, const u64 *tile_off, const u32 *tile_state, u64 file_off,
                                                            u32 *ev_cnt, const u64 *ev_off, u64 *ev, const MakerInfo *info)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE], s_has[MK_THREADS / WAVE], s_tail[MK_THREADS / WAVE], s_ev[MK_THREADS / WAVE];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (t * MK_TILE >= n_eff) { /* (uniform) */
      if (!WRITE && threadIdx.x == 0) ev_cnt[t] = 0;
      continue;
    }
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[4], kept, nl, tail;
    load16 (text, n_eff, off, w);
    scan16 (w, &kept, &nl, &tail);
    const u32 incl = dpp_inclusive_scan_u32 (kept | (nl << 16));
    const u64 m_nl = __builtin_amdgcn_ballot_w64 (nl != 0), m_tail = __builtin_amdgcn_ballot_w64 (tail != 0);
    u32 has, wt;
    wave_line_state (m_nl, m_tail, &has, &wt);
    if (lane == WAVE - 1) s_sum[wv] = incl;
    if (lane == 0) s_has[wv] = has, s_tail[wv] = wt;
    __syncthreads ();
    const u32 st = tile_state[t];
    u32 before = 0, name = st & 1u;
    for (int i = 0; i < wv; i++) {
      before += s_sum[i];
      name = s_has[i] ? s_tail[i] : (name | s_tail[i]);
    }
    const u32 excl = before + incl - (kept | (nl << 16));
    u32 rank = excl & 0xffffu;
    u32 phase = ((st >> 1) + (excl >> 16)) & 3u;
    {
      const u64 below = ((u64) 1 << lane) - 1, b_nl = m_nl & below, b_tail = m_tail & below;
      name = b_nl ? (b_tail >> (63 - __builtin_clzll (b_nl))) != 0 : (name | (b_tail != 0));
    }
    /* this thread's events */
    u32 ne = 0;
    {
      u32 nm = name, ph = phase;
#pragma unroll
      for (int j = 0; j < MK_PER; j++) { /* (load16 gives 0 for the bytes behind n_eff: no event there) */
        const u32 c = MK_BYTE (w, j), is_nl = IS_BYTE (c, '\n'), is_gt = IS_BYTE (c, '>');
        if (FASTQ) {
          ne += is_nl & (ph != 2u);
          ph = (ph + is_nl) & 3u;
        } else {
          ne += (is_nl & nm) | (is_gt & (nm ^ 1u));
          nm = (nm | is_gt) & (is_nl ^ 1u);
        }
      }
    }
    const u32 einc = dpp_inclusive_scan_u32 (ne);
    if (lane == WAVE - 1) s_ev[wv] = einc;
    __syncthreads ();
    u32 ebefore = 0, etotal = 0;
    for (int i = 0; i < MK_THREADS / WAVE; i++) {
      if (i < wv) ebefore += s_ev[i];
      etotal += s_ev[i];
    }
    if (!WRITE) {
      if (threadIdx.x == 0) ev_cnt[t] = etotal;
    } else if (ne) {
      u64 slot = ev_off[t] + ebefore + einc - ne;
      const u64 code0 = tile_off[t];
#pragma unroll
      for (int j = 0; j < MK_PER; j++) {
        const u32 c = MK_BYTE (w, j), is_nl = IS_BYTE (c, '\n'), is_gt = IS_BYTE (c, '>');
        u32 kind, is_ev;
        if (FASTQ) {
          kind = (phase + 1u) & 3u; /* name line 1, sequence line 2, '+' line none, quality line 0 */
          is_ev = is_nl & (kind != 3u);
          phase = (phase + is_nl) & 3u;
        } else {
          kind = is_nl;
          is_ev = (is_nl & name) | (is_gt & (name ^ 1u));
          name = (name | is_gt) & (is_nl ^ 1u);
        }
        if (is_ev) {
          ev[2 * slot] = ((file_off + off + j) << 2) | kind;
          ev[2 * slot + 1] = code0 + rank;
          slot++;
        }
        if (c >= 0x20u) rank++;
      }
    }
    __syncthreads ();
  }
}

/* k_mk_emit<true> with the raw location beside every word.  ev: the piece's events, n_ev of them, the first is event g0
 * of the file; ord0 / codes0: the ordinal of the sequence the piece starts in and its codes in front of the piece. */
template <int PERIOD>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_emit_loc (const unsigned char *__restrict__ buf, MakerInfo *info, u64 n_tiles, u32 k, const u64 *tile_off, u64 *words,
                                                              u64 *raw, const u64 *__restrict__ ev, u64 n_ev, u64 g0, u64 ord0, u64 codes0)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE];
  __shared__ unsigned long long s_max, s_over;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const u64 n_codes = info->n_codes;
  const u64 mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 j0 = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    if (threadIdx.x == 0) s_max = 0, s_over = 0;
    u32 w[12];
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
    u32 len = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < MK_HALO + MK_PER; i++) {
      const u32 c = MK_BYTE (w, i);
      len = c < 4u ? len + 1u : 0u;
      if (i >= MK_HALO && j0 + (u64) (i - MK_HALO) < n_codes && len >= k) cnt++;
    }
    const u32 incl = dpp_inclusive_scan_u32 (cnt);
    if (lane == WAVE - 1) s_sum[wv] = incl;
    __syncthreads ();
    u32 before = 0;
    for (int i = 0; i < wv; i++) before += s_sum[i];
    if (cnt) {
      /* a thread's words and locations lie together (up to 128 bytes each), written from the thread: not staged in LDS as
       * k_mk_emit<true> stages the words, which would take the two streams through it one after the other */
      u64 at = tile_off[t] + before + incl - cnt;
      /* events whose code index is <= j0: the last of them is where the sequence of code j0 starts */
      u64 lo = 0, hi = n_ev;
      while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (ev[2 * mid + 1] <= j0) lo = mid + 1;
        else hi = mid;
      }
      u64 fw = 0, rv = 0, pmax = 0, over = 0;
      len = 0;
#pragma unroll
      for (int i = 0; i < MK_HALO + MK_PER; i++) {
        const u32 c = MK_BYTE (w, i);
        fw = (fw << 2) | (c & 3u);
        rv = (rv >> 2) | ((u64) (~c & 3u) << (2 * (k - 1)));
        len = c < 4u ? len + 1u : 0u;
        if (i >= MK_HALO && j0 + (u64) (i - MK_HALO) < n_codes && len >= k) {
          const u64 j = j0 + (u64) (i - MK_HALO);
          while (lo < n_ev && ev[2 * lo + 1] <= j) lo++;
          const u64 ord = lo ? (g0 + lo - 1) / PERIOD : ord0;
          const u64 pos = (lo ? j - ev[2 * lo - 1] : j + codes0) + 1 - k;
          const u64 f = fw & mask;
          words[at] = f < rv ? f : rv;
          raw[at] = (ord << 33) | ((pos & 0xffffffffull) << 1) | (u64) (rv < f);
          at++;
          pmax = pos > pmax ? pos : pmax;
          over |= (ord >> 31) | (pos >> 32);
        }
      }
      atomicMax (&s_max, (unsigned long long) pmax);
      if (over) s_over = 1;
    }
    __syncthreads ();
    if (threadIdx.x == 0) {
      if (s_max) atomicMax ((unsigned long long *) &info->max_pos, s_max);
      if (s_over) info->overflow = 1;
    }
    __syncthreads ();
  }
}

/* raw locations of one file -> the words of the location section (reference :1066): file | ordinal | position | strand */
__global__ __launch_bounds__ (256) void k_pack_locations (u64 *__restrict__ raw, u64 n, u64 file, u32 sb, u32 pb)
{
  for (u64 i = (u64) blockIdx.x * 256 + threadIdx.x; i < n; i += (u64) gridDim.x * 256) {
    const u64 r = raw[i];
    raw[i] = (file << (sb + pb + 1)) | ((r >> 33) << (pb + 1)) | (r & 0x1ffffffffull);
  }
}

}  // namespace
}  // namespace gt4

namespace {

/* the error that holds if the text ends where this carry was taken (src/fasta.c:200-213), or 0 */
uint32_t end_error (const gt4hip_maker_carry *c)
{
  if (c->file_type != GT4HIP_MAKER_FASTQ || c->line_phase != 2) return 0;
  return c->at_line_start ? GT4HIP_MAKER_ERR_PLUS : GT4HIP_MAKER_ERR_PLUS_EOF;
}

const char *error_text (uint32_t kind)
{
  switch (kind) {
    case GT4HIP_MAKER_ERR_START: return "invalid start tag (neither '>' nor '@')";
    case GT4HIP_MAKER_ERR_PLUS: return "FastQ tag '+' missing";
    case GT4HIP_MAKER_ERR_AT: return "FastQ tag '@' missing";
    case GT4HIP_MAKER_ERR_PLUS_EOF: return "the text ends inside a FastQ '+' line";
    default: return "malformed text";
  }
}

int format_error (gt4hip_context *ctx, gt4hip_maker_carry *out, uint32_t kind, uint64_t offset, uint64_t *error_offset)
{
  out->error = kind;
  if (error_offset) *error_offset = offset;
  return gt4hip_fail (ctx, GT4HIP_EFORMAT, "gt4hip_text_to_words: %s at byte %llu", error_text (kind), (unsigned long long) offset);
}

}  // namespace

/* The words of a call are a pooled block that the context owns, like its workspaces: one at a time. */
extern "C" void gt4hip_words_free (gt4hip_context *ctx, uint64_t *d_words)
{
  if (!ctx || !ctx->maker_words || (d_words && (void *) d_words != ctx->maker_words->dev)) return;
  gt4hip_list_free (ctx->maker_words);
  ctx->maker_words = NULL;
}

extern "C" int gt4hip_words_download (gt4hip_context *ctx, const uint64_t *d_words, uint64_t n_words, uint64_t *host_words)
{
  if (!ctx || (n_words && (!d_words || !host_words))) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!n_words) return GT4HIP_OK;
  return gt4hip_read_back (ctx, host_words, d_words, (size_t) n_words * 8, "gt4hip_words_download failed");
}

namespace {

/* what gt4hip_text_to_locations adds to a call of the reader */
struct LocCall {
  const gt4hip_locations_carry *in;
  u64 *dst_words, *dst_raw; /* the caller's device arrays */
  uint64_t capacity;
  gt4hip_locations_piece *piece;
  gt4hip_locations_carry *out;
};

int finish_locations (gt4hip_context *ctx, LocCall *loc, const gt4hip_maker_carry *reader, const u64 *d_ev, uint64_t n_ev, uint64_t n_codes, uint64_t end_offset, uint64_t max_pos);

/* gt4hip_text_to_words; with `loc`, gt4hip_text_to_locations: the same kernels up to the words' count, then the events and
 * k_mk_emit_loc into the caller's arrays instead of k_mk_emit<true> into a block of the context */
int text_to_words (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_maker_carry *in,
                   gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words, uint64_t *error_offset, LocCall *loc)
{
  if (!ctx || !d_words || !n_words || (n_bytes && !text) || !word_length || word_length > 32 ||
      (flags & ~(unsigned) (GT4HIP_MAKER_FORWARD_ONLY | GT4HIP_MAKER_TEXT_ON_DEVICE)))
    return GT4HIP_EINVAL;
  if ((flags & GT4HIP_MAKER_TEXT_ON_DEVICE) && ((size_t) text & 15)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: device text must be 16-byte aligned");
  if (in && (in->file_type > GT4HIP_MAKER_FASTQ || in->line_phase > 3)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: carry not from this library");
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!loc) gt4hip_words_free (ctx, NULL); /* (the words of the call before, if the caller still left them) */
  *d_words = NULL;
  *n_words = 0;
  if (error_offset) *error_offset = 0;
  gt4hip_maker_carry c;
  if (in) {
    c = *in;
  } else {
    memset (&c, 0, sizeof c);
    memset (c.codes, 4, sizeof c.codes);
    c.at_line_start = 1;
  }
  c.error = 0;
  gt4hip_maker_carry dummy;
  if (!out) out = &dummy;
  *out = c;
  if (!n_bytes || c.ended) return loc ? finish_locations (ctx, loc, out, NULL, 0, 0, loc->in ? loc->in->offset : 0, 0) : GT4HIP_OK;
  hipStream_t st = ctx->stream;
  Blocks blk;
  int rc;
  /* the text */
  const unsigned char *d_text = (const unsigned char *) text;
  if (!(flags & GT4HIP_MAKER_TEXT_ON_DEVICE)) {
    void *p = NULL;
    if ((rc = blk.get (ctx, n_bytes, &p))) return rc;
    HIPCHK (ctx, hipMemcpyAsync (p, text, n_bytes, hipMemcpyHostToDevice, st));
    d_text = (const unsigned char *) p;
  }
  /* the first byte of a file decides its type (:128-138); a NUL there is an empty file */
  if (!c.file_type) {
    unsigned char first = 0;
    if (flags & GT4HIP_MAKER_TEXT_ON_DEVICE) {
      if ((rc = gt4hip_read_back (ctx, &first, d_text, 1, "reading the first byte of the text failed"))) return rc;
    } else {
      first = *(const unsigned char *) text;
    }
    if (!first) {
      hipStreamSynchronize (st); /* (the upload reads the caller's text) */
      out->ended = 1;
      return loc ? finish_locations (ctx, loc, out, NULL, 0, 0, loc->in ? loc->in->offset : 0, 0) : GT4HIP_OK;
    }
    if (first != '>' && first != '@') {
      hipStreamSynchronize (st);
      return format_error (ctx, out, GT4HIP_MAKER_ERR_START, 0, error_offset);
    }
    c.file_type = first == '>' ? GT4HIP_MAKER_FASTA : GT4HIP_MAKER_FASTQ;
  }
  const uint64_t tiles = (n_bytes + MK_TILE - 1) / MK_TILE;
  if (tiles >= (1ull << 32)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: %zu bytes in one piece", n_bytes);
  MakerInfo *info = NULL;
  u32 *tile_cnt = NULL, *tile_info = NULL, *tile_state = NULL;
  u64 *tile_off = NULL;
  unsigned char *buf = NULL;
  if ((rc = blk.get (ctx, sizeof (MakerInfo), (void **) &info))) return rc;
  if ((rc = blk.get (ctx, tiles * 4, (void **) &tile_cnt))) return rc;
  if ((rc = blk.get (ctx, tiles * 4, (void **) &tile_info))) return rc;
  if ((rc = blk.get (ctx, tiles * 4, (void **) &tile_state))) return rc;
  if ((rc = blk.get (ctx, tiles * 8, (void **) &tile_off))) return rc;
  if ((rc = blk.get (ctx, tiles * MK_TILE + MK_HALO + 64, (void **) &buf))) return rc;
  /* with locations the codes' offsets are still read after the words are counted: the emit stage gets arrays of its own */
  u32 *emit_cnt = tile_cnt, *ev_cnt = NULL;
  u64 *emit_off = tile_off, *ev_off = NULL;
  if (loc) {
    if ((rc = blk.get (ctx, tiles * 4, (void **) &emit_cnt))) return rc;
    if ((rc = blk.get (ctx, tiles * 8, (void **) &emit_off))) return rc;
    if ((rc = blk.get (ctx, tiles * 4, (void **) &ev_cnt))) return rc;
    if ((rc = blk.get (ctx, tiles * 8, (void **) &ev_off))) return rc;
  }
  const bool fastq = c.file_type == GT4HIP_MAKER_FASTQ;
  const u64 file_off = loc && loc->in ? loc->in->offset : 0;
  MakerInfo h;
  memset (&h, 0, sizeof h);
  h.nul_pos = n_bytes;
  h.err = ~0ull;
  h.in_name = c.in_name, h.phase = c.line_phase, h.at_line_start = c.at_line_start;
  HIPCHK (ctx, hipMemcpyAsync (info, &h, sizeof h, hipMemcpyHostToDevice, st));
  HIPCHK (ctx, hipMemcpyAsync (buf, c.codes, MK_HALO, hipMemcpyHostToDevice, st));
  const int grid = grid_for (ctx, tiles, 1);
  hipEventRecord (ctx->ev[0], st);
  hipLaunchKernelGGL (k_mk_summary, dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_cnt, tile_info, info);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, tile_cnt, (u64) tiles, tile_off, &info->n_words);
  hipLaunchKernelGGL (k_mk_state_scan, dim3 (1), dim3 (1024), 0, st, tile_info, (u64) tiles, c.in_name, c.line_phase, tile_state);
  if (c.file_type == GT4HIP_MAKER_FASTQ)
    hipLaunchKernelGGL (k_mk_codes<true>, dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, c.at_line_start, buf + MK_HALO, info);
  else
    hipLaunchKernelGGL (k_mk_codes<false>, dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, c.at_line_start, buf + MK_HALO, info);
  /* (tile_cnt and tile_off now serve the emit stage: at most as many codes as bytes, so at most as many tiles) */
  hipLaunchKernelGGL (k_mk_emit<false>, dim3 (grid), dim3 (MK_THREADS), 0, st, buf, info, (u64) tiles, word_length, 0u, emit_cnt, emit_off, (u64 *) NULL);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, emit_cnt, (u64) tiles, emit_off, &info->n_words);
  if (loc) {
    if (fastq)
      hipLaunchKernelGGL ((k_mk_events<true, false>), dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, file_off, ev_cnt, ev_off, (u64 *) NULL, info);
    else
      hipLaunchKernelGGL ((k_mk_events<false, false>), dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, file_off, ev_cnt, ev_off, (u64 *) NULL, info);
    hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, ev_cnt, (u64) tiles, ev_off, &info->n_events);
  }
  hipEventRecord (ctx->ev[1], st);
  HIPCHK (ctx, hipGetLastError ());
  if ((rc = gt4hip_read_back (ctx, &h, info, sizeof h, "reading the extraction's totals back failed"))) return rc;
  /* what the next piece starts from */
  out->file_type = c.file_type;
  out->in_name = h.in_name, out->line_phase = h.phase, out->at_line_start = h.at_line_start;
  out->ended = h.nul_pos < n_bytes;
  HIPCHK (ctx, hipMemcpyAsync (out->codes, buf + h.n_codes, MK_HALO, hipMemcpyDeviceToHost, st)); /* the last 32 codes, halo included */
  HIPCHK (ctx, hipStreamSynchronize (st));
  if (h.err != ~0ull) return format_error (ctx, out, (uint32_t) (h.err & 7u), h.err >> 3, error_offset);
  if (out->ended && end_error (out)) return format_error (ctx, out, end_error (out), h.nul_pos, error_offset);
  if (loc) {
    if (h.n_words > loc->capacity)
      return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_text_to_locations: %llu words, room for %llu", (unsigned long long) h.n_words, (unsigned long long) loc->capacity);
    u64 *ev = NULL;
    if ((rc = blk.get (ctx, (size_t) h.n_events * 16, (void **) &ev))) return rc;
    hipEventRecord (ctx->ev[2], st);
    if (h.n_events) {
      if (fastq)
        hipLaunchKernelGGL ((k_mk_events<true, true>), dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, file_off, ev_cnt, ev_off, ev, info);
      else
        hipLaunchKernelGGL ((k_mk_events<false, true>), dim3 (grid), dim3 (MK_THREADS), 0, st, d_text, (u64) n_bytes, (u64) tiles, tile_off, tile_state, file_off, ev_cnt, ev_off, ev, info);
    }
    if (h.n_words) {
      const u64 g0 = loc->in ? loc->in->n_events : 0, ord0 = loc->in && loc->in->n_subseqs ? loc->in->n_subseqs - 1 : 0, codes0 = loc->in ? loc->in->seq_codes : 0;
      if (fastq)
        hipLaunchKernelGGL (k_mk_emit_loc<3>, dim3 (grid), dim3 (MK_THREADS), 0, st, buf, info, (u64) tiles, word_length, emit_off, loc->dst_words, loc->dst_raw, ev, h.n_events, g0, ord0, codes0);
      else
        hipLaunchKernelGGL (k_mk_emit_loc<2>, dim3 (grid), dim3 (MK_THREADS), 0, st, buf, info, (u64) tiles, word_length, emit_off, loc->dst_words, loc->dst_raw, ev, h.n_events, g0, ord0, codes0);
    }
    hipEventRecord (ctx->ev[3], st);
    HIPCHK (ctx, hipGetLastError ());
    if ((rc = gt4hip_read_back (ctx, &h, info, sizeof h, "reading the locations' totals back failed"))) return rc;
    float ms = 0, ms2 = 0;
    if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess && hipEventElapsedTime (&ms2, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->extract_ms = ms + ms2;
    if (h.overflow) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_locations: a sequence ordinal of 2^31 or a position of 2^32 or more does not fit a raw location");
    if (h.n_words) *d_words = (uint64_t *) loc->dst_words;
    *n_words = h.n_words;
    return finish_locations (ctx, loc, out, ev, h.n_events, h.n_codes, file_off + (out->ended ? h.nul_pos : n_bytes), h.max_pos);
  }
  if (h.n_words) {
    void *w = NULL, *owner = NULL;
    if (gt4hip_block_alloc (ctx, (size_t) h.n_words * 8, &w, &owner))
      return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_text_to_words: %llu words", (unsigned long long) h.n_words);
    ctx->maker_words = (gt4hip_list *) owner;
    hipEventRecord (ctx->ev[2], st);
    hipLaunchKernelGGL (k_mk_emit<true>, dim3 (grid), dim3 (MK_THREADS), 0, st, buf, info, (u64) tiles, word_length, (u32) ((flags & GT4HIP_MAKER_FORWARD_ONLY) != 0),
                        tile_cnt, tile_off, (u64 *) w);
    hipError_t e = hipGetLastError ();
    hipEventRecord (ctx->ev[3], st);
    if (e == hipSuccess) e = hipStreamSynchronize (st);
    if (e != hipSuccess) {
      gt4hip_words_free (ctx, (uint64_t *) w);
      return gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_text_to_words: %s", hipGetErrorString (e));
    }
    /* the kernels alone: neither the read-back of the totals nor the allocation of the words between the two spans */
    float ms = 0, ms2 = 0;
    if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess && hipEventElapsedTime (&ms2, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->extract_ms = ms + ms2;
    *d_words = (uint64_t *) w;
    *n_words = h.n_words;
  }
  return GT4HIP_OK;
}

/* the piece's events -> its subsequence records and the carry behind it (reference start_sequence_index / end_sequence_index,
 * src/glistmaker.c:1031-1052); `reader`: the reader's carry behind the piece, end_offset: where the piece (or the text) ends */
int finish_locations (gt4hip_context *ctx, LocCall *loc, const gt4hip_maker_carry *reader, const u64 *d_ev, uint64_t n_ev, uint64_t n_codes, uint64_t end_offset, uint64_t max_pos)
{
  gt4hip_locations_carry c;
  if (loc->in) {
    c = *loc->in;
  } else {
    memset (&c, 0, sizeof c);
    c.name_pos = 1; /* (a FastQ file's first name has no event) */
  }
  gt4hip_locations_piece *pc = loc->piece;
  memset (pc, 0, sizeof *pc);
  std::vector<u64> ev (2 * n_ev);
  if (n_ev) {
    const int rc = gt4hip_read_back (ctx, ev.data (), d_ev, (size_t) n_ev * 16, "reading the text's events back failed");
    if (rc) return rc;
  }
  uint64_t n_new = 0;
  for (uint64_t i = 0; i < n_ev; i++) n_new += (ev[2 * i] & 3u) == 1u;
  gt4hip_locations_free (ctx);
  gt4hip_subseq *recs = NULL;
  if (n_new) {
    recs = (gt4hip_subseq *) malloc (n_new * sizeof *recs);
    if (!recs) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_text_to_locations: %llu subsequence records", (unsigned long long) n_new);
    ctx->maker_subseqs = recs;
  }
  const bool fastq = reader->file_type == GT4HIP_MAKER_FASTQ;
  uint64_t n = 0, last_start = ~0ull;
  auto close_at = [&] (uint64_t at) {
    if (!c.seq_open) return;
    if (n) recs[n - 1].seq_len = at - recs[n - 1].seq_pos;
    else pc->closed = 1, pc->closed_seq_len = at - c.seq_pos;
    c.seq_open = 0;
  };
  for (uint64_t i = 0; i < n_ev; i++) {
    const uint64_t at = ev[2 * i] >> 2;
    switch (ev[2 * i] & 3u) {
      case 0: /* a name starts: behind the '>', or two bytes behind a quality line's '\n' */
        if (!fastq) close_at (at);
        c.name_pos = at + (fastq ? 2 : 1);
        break;
      case 1: /* the sequence starts behind this '\n' */
        recs[n].name_pos = c.name_pos, recs[n].name_len = at - c.name_pos, recs[n].seq_pos = at + 1, recs[n].seq_len = 0;
        n++;
        c.seq_open = 1, c.seq_pos = at + 1;
        last_start = ev[2 * i + 1];
        break;
      default: close_at (at); break; /* a FastQ sequence line ends */
    }
  }
  if (reader->ended) close_at (end_offset); /* (src/fasta.c:109: a NUL ends the sequence as the end of the file does) */
  c.reader = *reader;
  c.offset = end_offset;
  c.n_events += n_ev;
  c.n_subseqs += n;
  c.seq_codes = last_start != ~0ull ? n_codes - last_start : c.seq_codes + n_codes;
  if (max_pos > c.max_position) c.max_position = max_pos;
  pc->n_subseqs = n;
  pc->subseqs = recs;
  if (loc->out) *loc->out = c;
  return GT4HIP_OK;
}

}  // namespace

extern "C" void gt4hip_locations_free (gt4hip_context *ctx)
{
  if (!ctx) return;
  free (ctx->maker_subseqs);
  ctx->maker_subseqs = NULL;
}

extern "C" int gt4hip_text_to_words (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_maker_carry *in,
                                     gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words, uint64_t *error_offset)
{
  return text_to_words (ctx, text, n_bytes, word_length, flags, in, out, d_words, n_words, error_offset, NULL);
}

extern "C" int gt4hip_text_to_locations (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_locations_carry *in,
                                         gt4hip_locations_carry *out, uint64_t *d_words, uint64_t *d_raw, uint64_t capacity, gt4hip_locations_piece *piece, uint64_t *error_offset)
{
  if (!ctx || !out || !piece || (capacity && (!d_words || !d_raw)) || (flags & GT4HIP_MAKER_FORWARD_ONLY)) return GT4HIP_EINVAL;
  LocCall loc = { in, (u64 *) d_words, (u64 *) d_raw, capacity, piece, out };
  memset (piece, 0, sizeof *piece);
  gt4hip_maker_carry reader;
  uint64_t *w = NULL, n = 0;
  if (in) *out = *in;
  else memset (out, 0, sizeof *out);
  const int rc = text_to_words (ctx, text, n_bytes, word_length, flags, in ? &in->reader : NULL, &reader, &w, &n, error_offset, &loc);
  if (rc) out->reader = reader; /* (the kind of a GT4HIP_EFORMAT) */
  else piece->n_words = n;
  return rc;
}

extern "C" int gt4hip_pack_locations (gt4hip_context *ctx, uint64_t *d_raw, uint64_t n, uint64_t file, unsigned subseq_bits, unsigned pos_bits)
{
  if (!ctx || (n && !d_raw)) return GT4HIP_EINVAL;
  if (!subseq_bits || !pos_bits || pos_bits > 32 || subseq_bits > 31 || subseq_bits + pos_bits + 1 > 63 || (file >> (63 - subseq_bits - pos_bits)))
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_pack_locations: file %llu with %u + %u + 1 bits behind it does not fit 64 bits", (unsigned long long) file, subseq_bits, pos_bits);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!n) return GT4HIP_OK;
  hipLaunchKernelGGL (k_pack_locations, dim3 (grid_for (ctx, n, 256)), dim3 (256), 0, ctx->stream, (u64 *) d_raw, (u64) n, (u64) file, subseq_bits, pos_bits);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

/* The pairs of an index -- every word of every input and its location -- are one pooled block of the context. */
extern "C" void gt4hip_pairs_release (gt4hip_context *ctx)
{
  if (!ctx || !ctx->index_pairs) return;
  gt4hip_list_free (ctx->index_pairs);
  ctx->index_pairs = NULL;
}

extern "C" int gt4hip_pairs_reserve (gt4hip_context *ctx, uint64_t n_pairs, uint64_t **d_words, uint64_t **d_values)
{
  if (!ctx || !d_words || !d_values) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_pairs_release (ctx);
  *d_words = *d_values = NULL;
  if (!n_pairs) return GT4HIP_OK;
  void *p = NULL, *owner = NULL;
  if (n_pairs >= (1ull << 59) || gt4hip_block_alloc (ctx, (size_t) n_pairs * 16, &p, &owner))
    return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_pairs_reserve: %llu pairs need %llu bytes of device memory", (unsigned long long) n_pairs, (unsigned long long) n_pairs * 16);
  ctx->index_pairs = (gt4hip_list *) owner;
  *d_words = (uint64_t *) p;
  *d_values = (uint64_t *) p + n_pairs;
  return GT4HIP_OK;
}

extern "C" int gt4hip_text_to_list (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, gt4hip_list **out)
{
  if (!ctx || !out) return GT4HIP_EINVAL;
  *out = NULL;
  gt4hip_maker_carry end;
  uint64_t *words = NULL, n = 0, at = 0;
  int rc = gt4hip_text_to_words (ctx, text, n_bytes, word_length, flags, NULL, &end, &words, &n, &at);
  /* the text ends here: what a reader that runs into the end of the file reports */
  if (!rc && !end.ended && end_error (&end)) rc = format_error (ctx, &end, end_error (&end), n_bytes, NULL);
  if (!rc) rc = gt4hip_device_words_to_list (ctx, words, n, word_length, out);
  gt4hip_words_free (ctx, words);
  return rc;
}
