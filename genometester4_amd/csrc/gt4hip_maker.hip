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
 * What sibling kernels share is written once, as inline functions: tile_head (the reader's state at a thread's first byte:
 * k_mk_codes, k_mk_events), load_word_ends and for_each_word (where words end, and the walk over them: k_mk_emit,
 * k_mk_emit_loc), block_scan (all of them and k_mk_summary).  The tile geometry, tile_head, block_scan and load_word_ends
 * live in gt4hip_maker_tile.h, which gt4hip_gmer.hip's statistics pass and gt4hip_mask.hip's two passes share.  The host half
 * is one MakerCall handed through stages.
 *
 * k_tile_count of gt4hip_index.h is not used: it counts a 4-byte flag per item, which would cost more traffic than
 * the text itself; the counts here come out of the classification.  Algorithmic bytes per text byte: 1 + 1 read, 1
 * written (codes), 1 read (emit, twice: count and write) and 8 written per word. */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"
#include "gt4hip_maker_tile.h"

#include <stdlib.h>
#include <string.h>

namespace gt4 {
namespace {

/* c2n of src/fasta.c:66-69, 4 for everything else */
__device__ __forceinline__ u32 nuc_code (u32 c)
{
  c |= 0x20u;
  return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : (c == 't' || c == 'u') ? 3u : 4u;
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
    u32 has, wt;
    wave_line_state (__builtin_amdgcn_ballot_w64 (nl != 0), __builtin_amdgcn_ballot_w64 (tail != 0), &has, &wt);
    if (lane == 0) s_has[wv] = has, s_tail[wv] = wt;
    const u32 s = block_scan (kept | (nl << 16), s_sum).total; /* both at most 4096 per tile */
    if (threadIdx.x == 0) {
      u32 tl = 0;
      for (int i = 0; i < MK_THREADS / WAVE; i++) tl = s_has[i] ? s_tail[i] : (tl | s_tail[i]);
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
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (t * MK_TILE >= n_eff) break; /* (uniform: every later tile of this workgroup lies behind the end as well) */
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    const TileHead h = tile_head (text, n_eff, off, tile_state + t, s_sum, s_has, s_tail);
    u32 rank = h.rank, phase = h.phase, name = h.name;
    u32 pnl = 0;
    if (FASTQ && off < n_eff) pnl = off ? text[off - 1] == '\n' : at_line_start0;
#pragma unroll
    for (int j = 0; j < MK_PER; j++) {
      const u32 c = MK_BYTE (h.w, j);
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
    const u32 m = h.n_codes;
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

/* f (j, forward word masked to 2k bits, reverse complement) for every word of `ends`, j the index of its last code, in order */
template <typename F>
__device__ __forceinline__ void for_each_word (const u32 w[12], u32 ends, u64 j0, u32 k, F f)
{
  const u64 mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
  u64 fw = 0, rv = 0;
#pragma unroll
  for (int i = 0; i < MK_HALO + MK_PER; i++) {
    const u32 c = MK_BYTE (w, i);
    fw = (fw << 2) | (c & 3u);
    rv = (rv >> 2) | ((u64) (~c & 3u) << (2 * (k - 1)));
    if (i >= MK_HALO && (ends >> (i - MK_HALO) & 1u)) f (j0 + (u64) (i - MK_HALO), fw & mask, rv);
  }
}

/* WRITE = false: tile_cnt[t] = words that end in tile t. */
template <bool WRITE>
__global__ __launch_bounds__ (MK_THREADS) void k_mk_emit (const unsigned char *__restrict__ buf, const MakerInfo *info, u64 n_tiles, u32 k, u32 forward_only,
                                                          u32 *tile_cnt, const u64 *tile_off, u64 *words)
{
  __shared__ u64 stage[WRITE ? MK_TILE : 1];
  __shared__ u32 s_sum[MK_THREADS / WAVE];
  const u64 n_codes = info->n_codes;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 j0 = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[12];
    const u32 ends = load_word_ends (buf, j0, n_codes, k, w), cnt = (u32) __popc (ends);
    const BlockScan sc = block_scan (cnt, s_sum);
    if (!WRITE) {
      if (threadIdx.x == 0) tile_cnt[t] = sc.total;
    } else {
      u32 rank = sc.before;
      for_each_word (w, ends, j0, k, [&] (u64, u64 f, u64 rv) { stage[rank++] = forward_only || f < rv ? f : rv; });
      __syncthreads ();
      u64 *dst = words + tile_off[t];
      for (u32 j = threadIdx.x; j < sc.total; j += MK_THREADS) dst[j] = stage[j];
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
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    if (t * MK_TILE >= n_eff) { /* (uniform) */
      if (!WRITE && threadIdx.x == 0) ev_cnt[t] = 0;
      continue;
    }
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    const TileHead h = tile_head (text, n_eff, off, tile_state + t, s_sum, s_has, s_tail);
    u32 rank = h.rank, phase = h.phase, name = h.name;
    /* this thread's events */
    u32 ne = 0;
    {
      u32 nm = name, ph = phase;
#pragma unroll
      for (int j = 0; j < MK_PER; j++) { /* (load16 gives 0 for the bytes behind n_eff: no event there) */
        const u32 c = MK_BYTE (h.w, j), is_nl = IS_BYTE (c, '\n'), is_gt = IS_BYTE (c, '>');
        if (FASTQ) {
          ne += is_nl & (ph != 2u);
          ph = (ph + is_nl) & 3u;
        } else {
          ne += (is_nl & nm) | (is_gt & (nm ^ 1u));
          nm = (nm | is_gt) & (is_nl ^ 1u);
        }
      }
    }
    const BlockScan es = block_scan (ne, s_ev);
    if (!WRITE) {
      if (threadIdx.x == 0) ev_cnt[t] = es.total;
    } else if (ne) {
      u64 slot = ev_off[t] + es.before;
      const u64 code0 = tile_off[t];
#pragma unroll
      for (int j = 0; j < MK_PER; j++) {
        const u32 c = MK_BYTE (h.w, j), is_nl = IS_BYTE (c, '\n'), is_gt = IS_BYTE (c, '>');
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
  const u64 n_codes = info->n_codes;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 j0 = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    if (threadIdx.x == 0) s_max = 0, s_over = 0;
    u32 w[12];
    const u32 ends = load_word_ends (buf, j0, n_codes, k, w), cnt = (u32) __popc (ends);
    const BlockScan sc = block_scan (cnt, s_sum);
    if (cnt) {
      /* a thread's words and locations lie together (up to 128 bytes each), written from the thread: not staged in LDS as
       * k_mk_emit<true> stages the words, which would take the two streams through it one after the other */
      u64 at = tile_off[t] + sc.before;
      /* events whose code index is <= j0: the last of them is where the sequence of code j0 starts */
      u64 lo = 0, hi = n_ev;
      while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (ev[2 * mid + 1] <= j0) lo = mid + 1;
        else hi = mid;
      }
      u64 pmax = 0, over = 0;
      for_each_word (w, ends, j0, k, [&] (u64 j, u64 f, u64 rv) {
        while (lo < n_ev && ev[2 * lo + 1] <= j) lo++;
        const u64 ord = lo ? (g0 + lo - 1) / PERIOD : ord0;
        const u64 pos = (lo ? j - ev[2 * lo - 1] : j + codes0) + 1 - k;
        words[at] = f < rv ? f : rv;
        raw[at] = (ord << 33) | ((pos & 0xffffffffull) << 1) | (u64) (rv < f);
        at++;
        pmax = pos > pmax ? pos : pmax;
        over |= (ord >> 31) | (pos >> 32);
      });
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
__global__ __launch_bounds__ (GT4HIP_PACK_THREADS) void k_pack_locations (u64 *__restrict__ raw, u64 n, u64 file, u32 sb, u32 pb)
{
  for (u64 i = (u64) blockIdx.x * GT4HIP_PACK_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * GT4HIP_PACK_THREADS) {
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

struct TypeKernels {
  decltype (&k_mk_codes<false>) codes;
  decltype (&k_mk_events<false, false>) count_events, write_events;
  decltype (&k_mk_emit_loc<2>) emit_loc;
};

/* One call of the reader: its arguments and what the stages hand on.  A stage returns GT4HIP_OK, an error, or MK_DONE. */
struct MakerCall {
  gt4hip_context *ctx;
  const void *text;
  size_t n_bytes;
  unsigned k, flags;
  gt4hip_maker_carry *out;
  uint64_t **d_words, *n_words, *error_offset;
  LocCall *loc;            /* NULL: gt4hip_text_to_words */
  gt4hip_maker_carry c;    /* what the piece starts from */
  TempBlocks blk;
  const unsigned char *d_text;
  const TypeKernels *kern;
  u64 file_off, tiles;     /* where the piece starts in its file (locations); its tiles of text */
  int grid;
  MakerInfo *info, h;      /* on the device, and as last read back */
  u64 *tile_off, *emit_off, *ev_off, *ev;
  u32 *tile_cnt, *tile_info, *tile_state, *emit_cnt, *ev_cnt;
  unsigned char *buf;      /* the halo, then the codes */
};
constexpr int MK_DONE = -1; /* not an error: there is no text to read (no bytes, behind a NUL, or a NUL first) */

/* the kernels that are instantiated by file type, [0] for FastA and [1] for FastQ: the one place that names both */
const TypeKernels MK_KERNELS[2] = { { k_mk_codes<false>, k_mk_events<false, false>, k_mk_events<false, true>, k_mk_emit_loc<2> },
                                    { k_mk_codes<true>, k_mk_events<true, false>, k_mk_events<true, true>, k_mk_emit_loc<3> } };

/* arguments, the carry in and its copy out, the text on the device, the file's type */
int maker_begin (MakerCall &m, const gt4hip_maker_carry *in)
{
  gt4hip_context *const ctx = m.ctx;
  if (!ctx || !m.d_words || !m.n_words || (m.n_bytes && !m.text) || !m.k || m.k > 32 || (m.flags & ~(unsigned) (GT4HIP_MAKER_FORWARD_ONLY | GT4HIP_MAKER_TEXT_ON_DEVICE)))
    return GT4HIP_EINVAL;
  if ((m.flags & GT4HIP_MAKER_TEXT_ON_DEVICE) && ((size_t) m.text & 15)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: device text must be 16-byte aligned");
  if (in && (in->file_type > GT4HIP_MAKER_FASTQ || in->line_phase > 3)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: carry not from this library");
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!m.loc) gt4hip_words_free (ctx, NULL); /* (the words of the call before, if the caller still left them) */
  *m.d_words = NULL;
  *m.n_words = 0;
  if (m.error_offset) *m.error_offset = 0;
  if (in) {
    m.c = *in;
  } else {
    memset (&m.c, 0, sizeof m.c);
    memset (m.c.codes, 4, sizeof m.c.codes);
    m.c.at_line_start = 1;
  }
  m.c.error = 0;
  *m.out = m.c;
  if (!m.n_bytes || m.c.ended) return MK_DONE;
  m.d_text = (const unsigned char *) m.text;
  if (!(m.flags & GT4HIP_MAKER_TEXT_ON_DEVICE)) {
    const int rc = m.blk.get (ctx, m.n_bytes, (void **) &m.d_text);
    if (rc) return rc;
    HIPCHK (ctx, hipMemcpyAsync ((void *) m.d_text, m.text, m.n_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  /* the first byte of a file decides its type (:128-138); a NUL there is an empty file */
  if (!m.c.file_type) {
    const bool on_device = (m.flags & GT4HIP_MAKER_TEXT_ON_DEVICE) != 0;
    unsigned char first = on_device ? 0 : *(const unsigned char *) m.text;
    const int rc = on_device ? gt4hip_read_back (ctx, &first, m.d_text, 1, "reading the first byte of the text failed") : GT4HIP_OK;
    if (rc) return rc;
    if (first != '>' && first != '@') {
      hipStreamSynchronize (ctx->stream); /* (the upload reads the caller's text) */
      if (first) return format_error (ctx, m.out, GT4HIP_MAKER_ERR_START, 0, m.error_offset);
      m.out->ended = 1;
      return MK_DONE;
    }
    m.c.file_type = first == '>' ? GT4HIP_MAKER_FASTA : GT4HIP_MAKER_FASTQ;
  }
  m.kern = &MK_KERNELS[m.c.file_type == GT4HIP_MAKER_FASTQ];
  m.file_off = m.loc && m.loc->in ? m.loc->in->offset : 0;
  return GT4HIP_OK;
}

/* The first span of the extraction.  The call's device arrays; classify: text -> codes by summary, the two scans and k_mk_codes */
int maker_classify_count (MakerCall &m)
{
  gt4hip_context *const ctx = m.ctx;
  hipStream_t st = ctx->stream;
  const u64 tiles = m.tiles = (m.n_bytes + MK_TILE - 1) / MK_TILE;
  if (tiles >= (1ull << 32)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_words: %zu bytes in one piece", m.n_bytes);
  /* per tile three offsets and five counts.  The emit stage has arrays of its own (tiles of codes: at most as many as tiles
   * of text): with locations tile_off is still read after the words are counted. */
  int rc;
  if ((rc = m.blk.get (ctx, sizeof (MakerInfo), (void **) &m.info))) return rc;
  if ((rc = m.blk.get (ctx, tiles * (3 * 8 + 5 * 4), (void **) &m.tile_off))) return rc;
  if ((rc = m.blk.get (ctx, tiles * MK_TILE + MK_HALO + 64, (void **) &m.buf))) return rc;
  m.emit_off = m.tile_off + tiles, m.ev_off = m.emit_off + tiles, m.tile_cnt = (u32 *) (m.ev_off + tiles);
  m.tile_info = m.tile_cnt + tiles, m.tile_state = m.tile_info + tiles, m.emit_cnt = m.tile_state + tiles, m.ev_cnt = m.emit_cnt + tiles;
  m.h = MakerInfo { m.n_bytes, ~0ull, 0, 0, m.c.in_name, m.c.line_phase, m.c.at_line_start }; /* (the rest 0) */
  HIPCHK (ctx, hipMemcpyAsync (m.info, &m.h, sizeof m.h, hipMemcpyHostToDevice, st));
  HIPCHK (ctx, hipMemcpyAsync (m.buf, m.c.codes, MK_HALO, hipMemcpyHostToDevice, st));
  m.grid = gt4hip_grid (ctx, tiles, 1);
  hipEventRecord (ctx->ev[0], st);
  hipLaunchKernelGGL (k_mk_summary, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.d_text, (u64) m.n_bytes, tiles, m.tile_cnt, m.tile_info, m.info);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, m.tile_cnt, tiles, m.tile_off, &m.info->n_words);
  hipLaunchKernelGGL (k_mk_state_scan, dim3 (1), dim3 (1024), 0, st, m.tile_info, tiles, m.c.in_name, m.c.line_phase, m.tile_state);
  gt4hip_grid_again (ctx, tiles, m.grid);
  hipLaunchKernelGGL (m.kern->codes, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.d_text, (u64) m.n_bytes, tiles, m.tile_off, m.tile_state, m.c.at_line_start, m.buf + MK_HALO, m.info);
  /* count: words per tile of codes and where each tile's go; with locations the same for the events of each tile of text */
  gt4hip_grid_again (ctx, tiles, m.grid);
  hipLaunchKernelGGL (k_mk_emit<false>, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.buf, m.info, m.tiles, m.k, 0u, m.emit_cnt, m.emit_off, (u64 *) NULL);
  hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, m.emit_cnt, m.tiles, m.emit_off, &m.info->n_words);
  if (m.loc) {
    gt4hip_grid_again (ctx, tiles, m.grid);
    hipLaunchKernelGGL (m.kern->count_events, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.d_text, (u64) m.n_bytes, m.tiles, m.tile_off, m.tile_state, m.file_off, m.ev_cnt, m.ev_off, m.ev, m.info);
    hipLaunchKernelGGL (k_tile_scan, dim3 (1), dim3 (1024), 0, st, m.ev_cnt, m.tiles, m.ev_off, &m.info->n_events);
  }
  hipEventRecord (ctx->ev[1], st);
  return GT4HIP_OK;
}

/* the one read-back of the totals, what the next piece starts from, and the text's format errors */
int maker_totals (MakerCall &m)
{
  gt4hip_context *const ctx = m.ctx;
  gt4hip_maker_carry *const out = m.out;
  const MakerInfo &h = m.h;
  HIPCHK (ctx, hipGetLastError ());
  const int rc = gt4hip_read_back (ctx, &m.h, m.info, sizeof h, "reading the extraction's totals back failed");
  if (rc) return rc;
  out->file_type = m.c.file_type;
  out->in_name = h.in_name, out->line_phase = h.phase, out->at_line_start = h.at_line_start;
  out->ended = h.nul_pos < m.n_bytes;
  HIPCHK (ctx, hipMemcpyAsync (out->codes, m.buf + h.n_codes, MK_HALO, hipMemcpyDeviceToHost, ctx->stream)); /* the last 32 codes, halo included */
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  if (h.err != ~0ull) return format_error (ctx, out, (uint32_t) (h.err & 7u), h.err >> 3, m.error_offset);
  if (out->ended && end_error (out)) return format_error (ctx, out, end_error (out), h.nul_pos, m.error_offset);
  return GT4HIP_OK;
}

/* gmer_counter's statistics of the piece (k_mk_text_counts, gt4hip_gmer.hip), behind the totals: the codes are in place */
int maker_text_counts (MakerCall &m, uint64_t counts[3])
{
  gt4hip_context *const ctx = m.ctx;
  unsigned long long *d = NULL;
  const int rc = m.blk.get (ctx, 3 * 8, (void **) &d);
  if (rc) return rc;
  HIPCHK (ctx, hipMemsetAsync (d, 0, 3 * 8, ctx->stream));
  gt4hip_grid_again (ctx, m.tiles, m.grid);
  gt4hip_launch_text_counts (ctx->stream, m.grid, m.c.file_type == GT4HIP_MAKER_FASTQ, m.d_text, m.n_bytes, m.tiles, m.tile_state, m.buf + MK_HALO, m.info, d);
  HIPCHK (ctx, hipGetLastError ());
  return gt4hip_read_back (ctx, counts, d, 3 * 8, "reading the text's statistics back failed");
}

/* the kernels alone: events 0 to 1 and 2 to 3, neither the read-back of the totals nor the allocation of the words between them */
void record_extract_ms (gt4hip_context *ctx)
{
  float ms = 0, ms2 = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess && hipEventElapsedTime (&ms2, ctx->ev[2], ctx->ev[3]) == hipSuccess) ctx->extract_ms = ms + ms2;
}

/* the words into a block of the context */
int maker_emit_words (MakerCall &m)
{
  gt4hip_context *const ctx = m.ctx;
  hipStream_t st = ctx->stream;
  if (!m.h.n_words) return GT4HIP_OK;
  void *w = NULL, *owner = NULL;
  if (gt4hip_block_alloc (ctx, (size_t) m.h.n_words * 8, &w, &owner))
    return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_text_to_words: %llu words", (unsigned long long) m.h.n_words);
  ctx->maker_words = (gt4hip_list *) owner;
  hipEventRecord (ctx->ev[2], st);
  gt4hip_grid_again (ctx, m.tiles, m.grid);
  hipLaunchKernelGGL (k_mk_emit<true>, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.buf, m.info, m.tiles, m.k, (u32) ((m.flags & GT4HIP_MAKER_FORWARD_ONLY) != 0), m.emit_cnt, m.emit_off, (u64 *) w);
  hipError_t e = hipGetLastError ();
  hipEventRecord (ctx->ev[3], st);
  if (e == hipSuccess) e = hipStreamSynchronize (st);
  if (e != hipSuccess) {
    gt4hip_words_free (ctx, (uint64_t *) w);
    return gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_text_to_words: %s", hipGetErrorString (e));
  }
  record_extract_ms (ctx);
  *m.d_words = (uint64_t *) w;
  *m.n_words = m.h.n_words;
  return GT4HIP_OK;
}

/* the events, then the words and their raw locations into the caller's arrays, then the records of the file block */
int maker_emit_locations (MakerCall &m)
{
  gt4hip_context *const ctx = m.ctx;
  hipStream_t st = ctx->stream;
  LocCall *const loc = m.loc;
  MakerInfo &h = m.h;
  if (h.n_words > loc->capacity)
    return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_text_to_locations: %llu words, room for %llu", (unsigned long long) h.n_words, (unsigned long long) loc->capacity);
  int rc;
  if ((rc = m.blk.get (ctx, (size_t) h.n_events * 16, (void **) &m.ev))) return rc;
  hipEventRecord (ctx->ev[2], st);
  if (h.n_events) {
    gt4hip_grid_again (ctx, m.tiles, m.grid);
    hipLaunchKernelGGL (m.kern->write_events, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.d_text, (u64) m.n_bytes, m.tiles, m.tile_off, m.tile_state, m.file_off, m.ev_cnt, m.ev_off, m.ev, m.info);
  }
  if (h.n_words) {
    const u64 g0 = loc->in ? loc->in->n_events : 0, ord0 = loc->in && loc->in->n_subseqs ? loc->in->n_subseqs - 1 : 0, codes0 = loc->in ? loc->in->seq_codes : 0;
    gt4hip_grid_again (ctx, m.tiles, m.grid);
    hipLaunchKernelGGL (m.kern->emit_loc, dim3 (m.grid), dim3 (MK_THREADS), 0, st, m.buf, m.info, m.tiles, m.k, m.emit_off, loc->dst_words, loc->dst_raw, m.ev, h.n_events, g0, ord0, codes0);
  }
  hipEventRecord (ctx->ev[3], st);
  HIPCHK (ctx, hipGetLastError ());
  if ((rc = gt4hip_read_back (ctx, &h, m.info, sizeof h, "reading the locations' totals back failed"))) return rc;
  record_extract_ms (ctx);
  if (h.overflow) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_text_to_locations: a sequence ordinal of 2^31 or a position of 2^32 or more does not fit a raw location");
  if (h.n_words) *m.d_words = (uint64_t *) loc->dst_words;
  *m.n_words = h.n_words;
  return finish_locations (ctx, loc, m.out, m.ev, h.n_events, h.n_codes, m.file_off + (m.out->ended ? h.nul_pos : m.n_bytes), h.max_pos);
}

/* gt4hip_text_to_words; with `loc`, gt4hip_text_to_locations: the same stages up to the words' count, then the events and
 * k_mk_emit_loc into the caller's arrays instead of k_mk_emit<true> into a block of the context */
int text_to_words (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_maker_carry *in,
                   gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words, uint64_t *error_offset, LocCall *loc, uint64_t *counts = NULL,
                   gt4hip_reader_then then = NULL, void *then_arg = NULL)
{
  gt4hip_maker_carry dummy;
  MakerCall m = { ctx, text, n_bytes, word_length, flags, out ? out : &dummy, d_words, n_words, error_offset, loc };
  if (counts) counts[0] = counts[1] = counts[2] = 0;
  int rc = maker_begin (m, in);
  if (rc == MK_DONE) return loc ? finish_locations (ctx, loc, m.out, NULL, 0, 0, loc->in ? loc->in->offset : 0, 0) : GT4HIP_OK;
  if (rc || (rc = maker_classify_count (m)) || (rc = maker_totals (m))) return rc;
  if (counts && (rc = maker_text_counts (m, counts))) return rc;
  if (loc) return maker_emit_locations (m);
  if ((rc = maker_emit_words (m)) || !then) return rc;
  /* gt4hip_mask.hip's passes, on the arrays of this call */
  const gt4hip_reader_view view = { m.d_text, m.n_bytes, m.tiles, (const uint64_t *) m.tile_off, (const uint64_t *) m.emit_off, m.buf, m.info, m.h.nul_pos, m.h.n_codes, *m.d_words, *m.n_words };
  return then (ctx, &view, then_arg);
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

int gt4hip_text_to_words_counted (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_maker_carry *in,
                                  gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words, uint64_t *error_offset, uint64_t counts[3])
{
  return text_to_words (ctx, text, n_bytes, word_length, flags, in, out, d_words, n_words, error_offset, NULL, counts);
}

int gt4hip_text_to_words_then (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags, const gt4hip_maker_carry *in,
                               gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words, uint64_t *error_offset, gt4hip_reader_then then, void *arg)
{
  return text_to_words (ctx, text, n_bytes, word_length, flags, in, out, d_words, n_words, error_offset, NULL, NULL, then, arg);
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
  hipLaunchKernelGGL (k_pack_locations, dim3 (gt4hip_grid (ctx, n, GT4HIP_PACK_THREADS)), dim3 (GT4HIP_PACK_THREADS), 0, ctx->stream, (u64 *) d_raw, (u64) n, (u64) file, subseq_bits, pos_bits);
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
