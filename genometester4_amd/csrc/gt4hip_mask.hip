/* gt4hip_mask.hip -- glistquery --mask on the device, gfx950, wave64: every base of a text that lies inside a word of a
 * resident list is replaced (not in the reference as a program: what its `glistquery -s` prints says which words hit).
 *
 * The reader (gt4hip_text_to_words, gt4hip_maker.hip) leaves, while its call lasts, the piece's codes (one byte per text
 * byte >= ' ', the halo of the piece before in front of them), the codes in front of every tile of text, the words in text
 * order and the words in front of every tile of codes.  Two streaming passes run on those arrays (gt4hip_reader_then):
 *
 *   k_mask_ends<PROBE>  over tiles of MK_TILE codes, 16 per thread: where words end among the thread's codes
 *                       (load_word_ends), the index of each of those words (the emit stage's tile offsets and a block scan
 *                       of the popcounts), the hit test -- PROBE: one find () per word in the bucket index, !PROBE (-mm N):
 *                       the value the k_query family left for the word -- and ONE BIT PER CODE, "a hit word ends here",
 *                       16 bits per thread.  n_hits: one add per wavefront.  back: a hit word that ends at code j < k - 1
 *                       of the piece covers k - 1 - j codes in front of it; the largest of those (atomicMax; only the
 *                       first two threads of the first tile can have one).
 *   k_mask_apply<SOFT>  over tiles of MK_TILE text bytes, 16 per thread: the rank of the thread's first byte >= ' ' among
 *                       the codes (the reader's tile offsets and a block scan), the 16 + k - 1 end bits from that rank on as
 *                       one 64-bit extract, cover = OR over d < k of (ends >> d) by doubling shifts, and the walk over the
 *                       16 bytes: every byte >= ' ' takes the next cover bit.  Only bases are ever covered (all k codes of
 *                       a word are bases), so no name or line state is needed.  Bytes at and behind the first NUL are
 *                       copied.  n_covered: one add per wavefront.
 *
 * Bytes per text byte: k_mask_ends reads 1 (codes; 3 with the halo of every thread, from cache) and 8 per word (PROBE: and
 * the probe's records; !PROBE: 4 per word), writes 1/8; k_mask_apply reads 1 + 1/8 (+ 1/2 per thread from cache) and writes 1. */
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"
#include "gt4hip_index.h"
#include "gt4hip_maker_tile.h"

#include <string.h>

namespace gt4 {
namespace {

/* what the two kernels add up (zeroed by the call): ctx->scratch */
struct MaskTotals {
  unsigned long long n_hits, n_covered;
  u32 back, pad;
};

/* end_bits: one u16 per thread and tile of codes, bit i: a hit word ends at code t * MK_TILE + 16 * thread + i */
template <bool PROBE>
__global__ __launch_bounds__ (MK_THREADS) void k_mask_ends (const unsigned char *__restrict__ buf, const MakerInfo *info, u64 n_tiles, u32 k, const u64 *emit_off,
                                                            const u64 *__restrict__ words, const u32 *__restrict__ values, u64 n_words, Index ix, u32 min_value,
                                                            u32 max_value, unsigned short *__restrict__ end_bits, MaskTotals *tot)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE];
  const u64 n_codes = info->n_codes;
  u32 n_hits = 0;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 j0 = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[12];
    const u32 ends = load_word_ends (buf, j0, n_codes, k, w);
    const BlockScan sc = block_scan ((u32) __popc (ends), s_sum);
    u64 at = emit_off[t] + sc.before;
    u32 hit = 0;
    for (u32 e = ends; e && at < n_words; e &= e - 1, at++) {
      u32 val;
      bool found;
      if (PROBE) {
        const u64 j = find (ix, words[at]);
        found = j != ~0ull;
        val = found ? ix.rec[3 * j + 2] : 0u;
      } else {
        val = values[at];
        found = val != 0;
      }
      if (found && val >= min_value && val <= max_value) hit |= e & (0u - e);
    }
    end_bits[t * MK_THREADS + threadIdx.x] = (unsigned short) hit;
    n_hits += (u32) __popc (hit);
    if (hit && j0 + (u32) __builtin_ctz (hit) + 1 < k) atomicMax (&tot->back, k - 1u - (u32) j0 - (u32) __builtin_ctz (hit)); /* (j0 is 0 or 16 here) */
    __syncthreads ();
  }
  n_hits = dpp_wave_sum_u32 (n_hits);
  if ((threadIdx.x & (WAVE - 1)) == 0 && n_hits) atomicAdd (&tot->n_hits, (unsigned long long) n_hits);
}

/* end_bits read as u64: bit j & 63 of word j >> 6 is code j's; the words behind the last code's are 0 */
template <bool SOFT>
__global__ __launch_bounds__ (MK_THREADS) void k_mask_apply (const unsigned char *__restrict__ text, u64 n, u64 n_tiles, const u64 *tile_off, const MakerInfo *info,
                                                             const u64 *__restrict__ end_bits, u32 k, u32 mask_byte, unsigned char *__restrict__ out, MaskTotals *tot)
{
  __shared__ u32 s_sum[MK_THREADS / WAVE];
  const u64 nul = info->nul_pos, n_eff = nul < n ? nul : n;
  u32 n_cov = 0;
  for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const u64 off = t * MK_TILE + (u64) threadIdx.x * MK_PER;
    u32 w[4], kept, nl, tail;
    load16 (text, n, off, w);
    scan16 (w, &kept, &nl, &tail);
    const BlockScan sc = block_scan (kept, s_sum);
    u32 cover = 0;
    if (kept && off < n_eff) {
      const u64 r = tile_off[t] + sc.before;
      const u32 s = (u32) r & 63u;
      const u64 lo = end_bits[r >> 6], hi = end_bits[(r >> 6) + 1];
      u64 x = ((lo >> s) | (s ? hi << (64u - s) : 0ull)) & ((1ull << (MK_PER + k - 1u)) - 1ull);
      for (u32 span = 1; span < k;) { /* x = OR over d < span of (ends >> d) */
        const u32 d = span < k - span ? span : k - span;
        x |= x >> d;
        span += d;
      }
      cover = (u32) x & 0xffffu;
    }
    if (cover) {
      u32 ci = 0;
#pragma unroll
      for (int j = 0; j < MK_PER; j++) {
        const u32 c = MK_BYTE (w, j);
        if (c >= 0x20u) {
          if (((cover >> ci) & 1u) && off + j < n_eff) {
            const u32 to = SOFT ? (c | 0x20u) : mask_byte;
            w[j >> 2] = (w[j >> 2] & ~(0xffu << (8 * (j & 3)))) | (to << (8 * (j & 3)));
            n_cov++;
          }
          ci++;
        }
      }
    }
    if (off + MK_PER <= n) {
      u32x4 v;
      v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
      *(u32x4 *) (out + off) = v;
    } else {
#pragma unroll
      for (int j = 0; j < MK_PER; j++)
        if (off + j < n) out[off + j] = (unsigned char) MK_BYTE (w, j);
    }
    __syncthreads ();
  }
  n_cov = dpp_wave_sum_u32 (n_cov);
  if ((threadIdx.x & (WAVE - 1)) == 0 && n_cov) atomicAdd (&tot->n_covered, (unsigned long long) n_cov);
}

}  // namespace
}  // namespace gt4

using namespace gt4;

namespace {

struct MaskCall {
  const char *who;
  gt4hip_query_index *qi;
  const gt4hip_query_params *prm;
  u32 k, min_value, max_value, mask_byte;
  bool soft;
  unsigned char *d_masked; /* n_bytes of device memory */
  gt4hip_mask_piece *piece;
  bool ran;
};

/* the two passes on the arrays of the reader's call (gt4hip_reader_then) */
int mask_then (gt4hip_context *ctx, const gt4hip_reader_view *v, void *arg)
{
  MaskCall *const c = (MaskCall *) arg;
  hipStream_t st = ctx->stream;
  c->ran = true;
  TempBlocks blk;
  int rc;
  /* a u16 per thread and tile, and two u64 behind them that k_mask_apply's extract may read */
  const size_t bits_bytes = (size_t) v->tiles * MK_THREADS * 2;
  unsigned char *d_bits = NULL;
  u32 *d_values = NULL;
  if ((rc = blk.get (ctx, bits_bytes + 16, (void **) &d_bits))) return rc;
  if (c->prm->n_mm && v->n_words && (rc = blk.get (ctx, (size_t) v->n_words * 4, (void **) &d_values))) return rc;
  MaskTotals *tot = (MaskTotals *) ctx->scratch;
  Index ix;
  size_index (gt4hip_query_index_list (c->qi), &ix);
  ix.off = (const u64 *) gt4hip_query_index_offsets (c->qi);
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], st));
  HIPCHK (ctx, hipMemsetAsync (tot, 0, sizeof *tot, st));
  HIPCHK (ctx, hipMemsetAsync (d_bits + bits_bytes, 0, 16, st));
  if (d_values && (rc = gt4hip_query_lookup_device (ctx, c->who, c->qi, c->prm, (const uint64_t *) v->d_words, v->n_words, d_values, NULL))) return rc;
  const int grid = gt4hip_grid (ctx, v->tiles, 1);
  if (c->prm->n_mm)
    hipLaunchKernelGGL (k_mask_ends<false>, dim3 (grid), dim3 (MK_THREADS), 0, st, v->buf, (const MakerInfo *) v->info, (u64) v->tiles, c->k, (const u64 *) v->emit_off, (const u64 *) v->d_words,
                        d_values, (u64) v->n_words, ix, c->min_value, c->max_value, (unsigned short *) d_bits, tot);
  else
    hipLaunchKernelGGL (k_mask_ends<true>, dim3 (grid), dim3 (MK_THREADS), 0, st, v->buf, (const MakerInfo *) v->info, (u64) v->tiles, c->k, (const u64 *) v->emit_off, (const u64 *) v->d_words,
                        d_values, (u64) v->n_words, ix, c->min_value, c->max_value, (unsigned short *) d_bits, tot);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], st));
  gt4hip_grid_again (ctx, v->tiles, grid);
  if (c->soft)
    hipLaunchKernelGGL (k_mask_apply<true>, dim3 (grid), dim3 (MK_THREADS), 0, st, v->d_text, (u64) v->n_bytes, (u64) v->tiles, (const u64 *) v->tile_off, (const MakerInfo *) v->info,
                        (const u64 *) d_bits, c->k, c->mask_byte, c->d_masked, tot);
  else
    hipLaunchKernelGGL (k_mask_apply<false>, dim3 (grid), dim3 (MK_THREADS), 0, st, v->d_text, (u64) v->n_bytes, (u64) v->tiles, (const u64 *) v->tile_off, (const MakerInfo *) v->info,
                        (const u64 *) d_bits, c->k, c->mask_byte, c->d_masked, tot);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[2], st));
  if ((rc = gt4hip_read_scratch (ctx, 3))) return rc;
  MaskTotals h;
  memcpy (&h, ctx->scratch_host, sizeof h);
  float ms = 0, ms2 = 0;
  if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess && hipEventElapsedTime (&ms2, ctx->ev[1], ctx->ev[2]) == hipSuccess) {
    ctx->mask_ends_ms = ms, ctx->mask_apply_ms = ms2;
    gt4hip_query_index_set_ms (c->qi, ms + ms2);
  }
  c->piece->n_words = v->n_words;
  c->piece->n_hits = h.n_hits;
  c->piece->n_covered = h.n_covered;
  c->piece->back = h.back;
  return GT4HIP_OK;
}

}  // namespace

static_assert (sizeof (MaskTotals) == 24, "the totals are the first three of the context's scratch words");

extern "C" int gt4hip_query_mask_text (gt4hip_context *ctx, gt4hip_query_index *qi, const void *text, size_t n_bytes, unsigned flags, const gt4hip_query_params *prm,
                                       uint32_t min_value, uint32_t max_value, unsigned char mask_byte, const gt4hip_maker_carry *in, gt4hip_maker_carry *out,
                                       void *masked, gt4hip_mask_piece *piece, uint64_t *error_offset)
{
  const char *who = "gt4hip_query_mask_text";
  if (!ctx || !qi || !prm || !out || !piece || (n_bytes && (!text || !masked)) || (flags & ~(unsigned) (GT4HIP_MAKER_TEXT_ON_DEVICE | GT4HIP_MASK_SOFT))) return GT4HIP_EINVAL;
  memset (piece, 0, sizeof *piece);
  int rc = gt4hip_query_check_params (ctx, who, qi, prm);
  if (rc) return rc;
  const bool on_device = (flags & GT4HIP_MAKER_TEXT_ON_DEVICE) != 0;
  if (on_device && ((size_t) masked & 15)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: device memory for the masked text must be 16-byte aligned", who);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_query_index_set_ms (qi, 0);
  ctx->mask_ends_ms = ctx->mask_apply_ms = 0;
  TempBlocks blk;
  MaskCall c = { who, qi, prm, gt4hip_query_index_list (qi)->word_length, min_value, max_value, mask_byte, (flags & GT4HIP_MASK_SOFT) != 0, (unsigned char *) masked, piece, false };
  if (!on_device && n_bytes && (rc = blk.get (ctx, n_bytes, (void **) &c.d_masked))) return rc;
  uint64_t *d_words = NULL, n_words = 0;
  rc = gt4hip_text_to_words_then (ctx, text, n_bytes, c.k, flags & GT4HIP_MAKER_TEXT_ON_DEVICE, in, out, &d_words, &n_words, error_offset, mask_then, &c);
  gt4hip_words_free (ctx, NULL);
  if (rc || !n_bytes) return rc;
  if (!c.ran) { /* nothing for the reader: a piece behind a NUL, or a NUL as the first byte of a file */
    if (!on_device) {
      memcpy (masked, text, n_bytes);
    } else {
      HIPCHK (ctx, hipMemcpyAsync (masked, text, n_bytes, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
    }
    return GT4HIP_OK;
  }
  if (!on_device) return gt4hip_read_back (ctx, masked, c.d_masked, n_bytes, "reading the masked text back failed");
  return GT4HIP_OK;
}
