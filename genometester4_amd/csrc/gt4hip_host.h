/* gt4hip_host.h -- host-side internals shared by the C-ABI implementation files: the context and list objects, the
 * owners of a call's temporaries (TempLists, TempBlocks, TempTable), the grid size of the striding kernels, and what the
 * units of the library host (gt4hip_api.hip, gt4hip_pair.hip, gt4hip_multi.hip, gt4hip_table.hip, gt4hip_nway.hip) and
 * gt4hip_io / _comm / _sort / _maker / _mismatch / _query / _seqprofile / _mask / _gmer / _subset / _select / _pairwise.hip call in one another. */
#ifndef GT4HIP_HOST_H
#define GT4HIP_HOST_H

#include "../../include/gt4hip.h"
#include "gt4hip_internal.h"

#include <stddef.h>
#include <algorithm>
#include <utility>
#include <vector>

struct gt4hip_io; /* gt4hip_io.hip: pinned staging + copy threads, created on first use */

struct gt4hip_context {
  int device;
  hipStream_t stream;
  hipEvent_t ev[4];
  int n_cus;
  int two_pass;
  int64_t grid_override;
  uint32_t spin_limit;       /* option "spin_limit": bound of the single-pass kernel's waits (0 = default) */
  int a_rows;      /* option "a_rows": A-only single-pass kernels: 0 the A-rows body for every tile whose A records fit half the position rows, -1 never */
  int part_guided; /* option "part_guided": the pair partition's co-rank searches: 0 guided by the coarse neighbours (gt4hip_corank.h), -1 plain bisection */
  double partition_ms; /* counter "partition_us": the partition launch of the last pair call (HIP events 0 -> 1 of gt4hip_run_pair) */
  int dynamic;     /* option "dynamic": tiles of the single-pass kernels dealt by a ticket counter: 0 automatic, 1 always, -1 never (round-robin) */
  int scan_group;  /* option "scan_group": 0 automatic, 1 always the scanner group, -1 always one wavefront per stream */
  int force_geom; /* options "geom1" / "geom0": force the large / small geometry for every call (experiments); 0 = automatic */
  uint64_t single_pass_fallbacks; /* calls that had to be rerun on the two-pass path */
  /* freed list storage kept for reuse: hipMalloc / hipFree of tens of GB cost far more than the
   * merges themselves (an 8-way union tree allocates seven outputs per call) */
  std::vector<std::pair<void *, size_t>> *pool;
  int pool_enabled;
  size_t pool_bytes;         /* bytes the pool holds right now */
  size_t pool_cap;           /* most it may hold (option "pool_cap_mb"; default: half of the device memory) */
  /* workspace, grown on demand */
  uint64_t *part;
  size_t part_bytes;
  unsigned long long *desc;
  size_t desc_bytes;
  unsigned long long *block_sums;
  size_t block_sums_bytes;
  gt4::PairControl *ctl;          /* device */
  gt4::PairControl *ctl_host;     /* pinned */
  unsigned long long *scratch;      /* device, 4 x u64 */
  unsigned long long *scratch_host; /* pinned */
  /* N-way tile kernel (gt4hip_nway.hip) */
  uint64_t *kway_part;       /* tile boundaries, [tiles + 1][8] */
  size_t kway_part_bytes;
  void *kway_cnt;            /* samples of every list per bracket of 64 tiles */
  size_t kway_cnt_bytes;
  uint64_t *kway_part2;      /* the boundaries with the tiles that would not fit LDS cut in two (the table the tile kernel reads) */
  size_t kway_part2_bytes;
  void *kway_need;           /* tiles each nominal tile becomes (u32), block sums (u32) */
  size_t kway_need_bytes;
  uint64_t kway_splits;      /* counter "kway_splits": tiles cut in two by the last N-way call */
  int kway_enabled;          /* option "kway": 0 = always the pairwise tree, 1 = the one-pass kernel unless the keys are clustered, 2 = always, also for two lists, 3 = always (three lists and more) */
  int kway_max;              /* option "kway_max": lists per launch of the tile kernel, 32 (default: unless the lists share most keys), 8, or 33 (= 32 whatever the keys) */
  uint64_t kway_width;       /* counter "kway_width": lists per launch the last N-way union took (8 or 32) */
  uint64_t kway_shared_x100; /* counter "kway_shared_x100": 100 x the mean number of lists a probed key lies in (last union of more than eight lists) */
  int64_t kway_g;            /* option "kway_g": samples per tile (0 = automatic) */
  int64_t kway_vt;           /* option "kway_vt": positions per thread in a merge pass, at least (0 = default) */
  uint64_t kway_overflows;   /* calls that fell back to the tree because a tile would not fit LDS */
  uint64_t kway_calls;       /* N-way unions done by the one-pass kernel */
  uint64_t kway_declined;    /* ... handed to the pairwise tree because the keys are clustered (option "kway" = 1) */
  double table_ms;           /* the last gt4hip_union_table, wall time of the call */
  double sort_ms, fold_ms;   /* the last gt4hip_device_words_to_list: radix sort and fold (HIP events) */
  double extract_ms;         /* the last gt4hip_text_to_words that gave words: its kernels (HIP events around them alone) */
  struct gt4hip_list *maker_words; /* the words of the last gt4hip_text_to_words, until gt4hip_words_free or the next call */
  struct gt4hip_list *index_kmers; /* the k-mer section of the last gt4hip_pairs_to_index, until gt4hip_index_free or the next call */
  struct gt4hip_list *index_pairs; /* the block of gt4hip_pairs_reserve, until gt4hip_pairs_release or the next call */
  gt4hip_subseq *maker_subseqs;    /* host: the records of the last gt4hip_text_to_locations, until gt4hip_locations_free or the next call */
  double nway_kernel_ms;     /* the last one-pass launch's kernel time (HIP events on the library's stream) and tiles */
  uint64_t nway_tiles;
  uint64_t nway_sample_tiles; /* counter "nway_sample_tiles": the most tiles of a sample-level launch of the last N-way call (0: it had none) */
  int last_multi_one_pass;   /* the last gt4hip_union_multi was done by the one-pass tile kernel (counter "nway_one_pass") */
  gt4hip_io *io;            /* file <-> HBM staging (gt4hip_io.hip), NULL until first used */
  gt4hip_mismatch_stats mm_stats; /* the last gt4hip_compare_mismatch (gt4hip_mismatch.hip) */
  uint64_t mm_wide_levels;      /* counter "mm_wide_levels": its levels, both sides added, that ran the 64-bit unranking (k_level<true>) */
  uint64_t mm_unskipped_levels; /* counter "mm_unskipped_levels": ... that ran without the early exit (early == 0) */
  uint64_t query_wide;          /* counter "query_wide": the last gt4hip_query_lookup launched k_query<true> */
  uint64_t subset_passes;       /* counter "subset_passes": passes of the last gt4hip_list_subset (gt4hip_subset.hip) */
  double subset_ms;             /* counter "subset_us": its kernels (HIP events) */
  double mask_ends_ms, mask_apply_ms; /* counters "mask_ends_us", "mask_apply_us": the last gt4hip_query_mask_text (gt4hip_mask.hip) */
  int select_vec;               /* option "select_vec": gt4hip_table_select reads rows of a multiple of four counts 16 bytes per lane (0) / every row a dword per lane (-1) */
  uint64_t select_wide;         /* counter "select_wide": the last gt4hip_table_select read 16 bytes per lane */
  gt4::GridLimit grid_limit;    /* option "grid_cap" (tests): workgroups at most of every kernel that strides over its work, 0 = the built-in caps alone; counter "grid_capped": launches whose grid had fewer workgroups than blocks of work */
  int poison;                   /* option "poison" (tests): every device block handed out, new or from the pool, is filled with 0xA5 bytes first */
  uint64_t caller_piece;        /* option "caller_piece" (tests): markers per piece of gt4hip_caller_probabilities, 0 = 2^22, with all 15 likelihoods 2^20 */
  void *caller_tab;             /* gt4hip_caller.hip: the log-factorial table, the workgroups' partial sums and their ticket; NULL until a set is made */
  char err[512];
  char info[256];
};

struct gt4hip_list {
  gt4hip_context *ctx;
  void *dev;
  size_t bytes; /* size of the allocation behind dev when owned */
  uint64_t n_words;
  uint64_t capacity;
  uint32_t word_length;
  int owns;
};

/* what only the library's own translation units call is kept out of its exported symbols */
#define GT4HIP_LOCAL __attribute__ ((visibility ("hidden")))
/* ---- gt4hip_api.hip */
int gt4hip_fail (gt4hip_context *ctx, int code, const char *fmt, ...);
/* every device allocation of the library: gives the pooled blocks back and retries when the driver is out of memory */
hipError_t gt4hip_dev_alloc (gt4hip_context *ctx, void **p, size_t bytes);
/* a workspace buffer of the context grown to `need` bytes and an eighth: the stream is drained before the old one goes */
GT4HIP_LOCAL int gt4hip_grow (gt4hip_context *ctx, void **p, size_t *have, size_t need);
int gt4hip_list_new (gt4hip_context *ctx, uint64_t capacity, uint32_t word_length, gt4hip_list **out);
/* a list of no records that owns nothing (the second operand where a call has only one) */
GT4HIP_LOCAL gt4hip_list gt4hip_empty_list (gt4hip_context *ctx, uint32_t word_length);
/* device -> host copy of `bytes` on the context's stream, then the stream is drained; fails with "<what>: <HIP error>" */
GT4HIP_LOCAL int gt4hip_read_back (gt4hip_context *ctx, void *host, const void *dev, size_t bytes, const char *what);
/* the first n u64 of ctx->scratch -> ctx->scratch_host, as above */
GT4HIP_LOCAL inline int gt4hip_read_scratch (gt4hip_context *ctx, unsigned n) { return gt4hip_read_back (ctx, ctx->scratch_host, ctx->scratch, n * 8, "reading the scratch words back failed"); }

/* Device lists that exist for one call: what the owner still holds when it goes out of scope is freed, in the order adopted
 * (the block pool hands out the best-fitting block and evicts the oldest: that order decides what the next call reuses). */
struct GT4HIP_LOCAL TempLists {
  std::vector<gt4hip_list *> lists;
  TempLists () {}
  TempLists (const TempLists &) = delete;
  void operator= (const TempLists &) = delete;
  ~TempLists () { clear (); }
  gt4hip_list *adopt (gt4hip_list *l) { return lists.push_back (l), l; }
  void release () { lists.clear (); } /* (they are the caller's now) */
  void clear ()
  {
    for (gt4hip_list *l : lists) gt4hip_list_free (l);
    lists.clear ();
  }
  /* A level of a merge tree is complete (`level`: its results, `next`: what the level above reads): the lists of the level
   * below are freed, except those carried over as they are; this owner then holds `level`'s lists followed by the carried. */
  void next_level (TempLists &level, const std::vector<const gt4hip_list *> &next)
  {
    for (gt4hip_list *l : lists) {
      if (std::find (next.begin (), next.end (), l) != next.end ()) level.lists.push_back (l);
      else gt4hip_list_free (l);
    }
    lists.clear ();
    lists.swap (level.lists);
  }
};

/* gt4hip_table.hip: device memory from the context's block pool; the owner is what gt4hip_block_free takes */
int gt4hip_block_alloc (gt4hip_context *ctx, size_t bytes, void **dev, void **owner);
void gt4hip_block_free (void *owner);

/* Device blocks that exist for one call, freed like TempLists' lists: in the order acquired.  A block that ends up in an
 * object that outlives the call is not taken here: gt4hip_block_alloc gives its owner to the object directly. */
struct GT4HIP_LOCAL TempBlocks {
  std::vector<void *> owners;
  TempBlocks () {}
  TempBlocks (const TempBlocks &) = delete;
  void operator= (const TempBlocks &) = delete;
  ~TempBlocks () { clear (); }
  /* *p = a block of `bytes` bytes (of 16 where that is 0) */
  int get (gt4hip_context *ctx, size_t bytes, void **p)
  {
    void *owner = NULL;
    const int rc = gt4hip_block_alloc (ctx, bytes ? bytes : 16, p, &owner);
    if (!rc) owners.push_back (owner);
    return rc;
  }
  void clear ()
  {
    for (void *o : owners) gt4hip_block_free (o);
    owners.clear ();
  }
};

/* workgroups of a kernel that strides over `blocks` blocks of work: one each, at most eight per compute unit and at most
 * option "grid_cap", at least one (gt4::strided_grid, which also keeps counter "grid_capped").  Only for kernels whose
 * workgroups never wait for one another: under "grid_cap" = 1 a single workgroup does all the work. */
inline int gt4hip_grid (gt4hip_context *ctx, uint64_t blocks) { return gt4::strided_grid (ctx->grid_limit, blocks, (uint64_t) (ctx->n_cus > 0 ? ctx->n_cus : 256) * 8); }
/* one more launch with the grid gt4hip_grid gave for `blocks` blocks of work: counted in "grid_capped" as the first was */
inline void gt4hip_grid_again (gt4hip_context *ctx, uint64_t blocks, int grid) { ctx->grid_limit.capped += blocks > (uint64_t) grid; }
/* ... over `items` items, `per_block` to a block */
inline int gt4hip_grid (gt4hip_context *ctx, uint64_t items, uint64_t per_block) { return gt4hip_grid (ctx, (items + per_block - 1) / per_block); }

/* *out = the caller's list `given` if it holds `need` records (an error if not; `s`: the output stream named in the
 * text, < 0 where the call has one output), else a new list of that capacity, which `made` then owns */
GT4HIP_LOCAL int gt4hip_output_list (gt4hip_context *ctx, int s, gt4hip_list *given, uint64_t need, uint32_t word_length, TempLists &made, gt4hip_list **out);

/* ---- gt4hip_pair.hip */
struct PairRun {
  uint64_t n_words[4];
  uint64_t total_count[4];
  double merge_ms, device_ms;
  uint64_t tiles;
};
/* the merge of (A, B) with fully resolved kernel parameters, waited for; dst[s]: non-null for every requested stream unless count_only */
GT4HIP_LOCAL int gt4hip_run_pair (gt4hip_context *ctx, const uint32_t *A, uint64_t nA, const uint32_t *B, uint64_t nB, const gt4::PairParams &p,
                                  bool count_only, uint32_t *const dst[4], PairRun *run, bool force_two_pass = false);
/* The same on lists: out[s] is the caller's list or NULL (then one of the worst-case size is made and returned there);
 * sets the outputs' n_words.  Nothing is made, and out[] is as it was, when the call fails. */
GT4HIP_LOCAL int gt4hip_pair_with_outputs (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, const gt4::PairParams &p, bool count_only,
                                           gt4hip_list *out[4], PairRun *run);
/* the parameters of a step of an N-way operation or a table column: one stream, one rule for it, no subtract */
GT4HIP_LOCAL gt4::PairParams gt4hip_nway_params (uint32_t op_bit, uint32_t rule, uint32_t cutoff, uint32_t ovr, uint32_t filter);
/* bytes of the chained scan's descriptors (gt4hip_device.h): agg u32[4][rows * 64], carry u64[4][rows + 1], rowsum u64[4][rows] */
GT4HIP_LOCAL size_t gt4hip_lookback_desc_bytes (uint64_t tiles);

/* ---- gt4hip_nway.hip, gt4hip_table.hip, gt4hip_io.hip, gt4hip_maker.hip */
int gt4hip_nway_union (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t k, uint32_t rule, uint32_t cutoff, uint32_t ovr,
                       uint32_t filter, bool count_only, gt4hip_list *out, uint64_t *n_words, uint64_t *total_count, double *device_ms, int *used);
int gt4hip_nway_table (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t k, const uint32_t cols[], gt4hip_count_table *table, int probe,
                       int presence, int *used);
int gt4hip_table_alloc (gt4hip_context *ctx, gt4hip_count_table *table, uint64_t n, uint32_t n_lists);
/* ragged tables (gt4hip_count_table.ragged): the index of `tiles` tiles -- rows before every tile (compact) and where
 * the tile's rows lie in the arrays (padded), tiles + 1 device u64 each */
int gt4hip_table_set_ragged (gt4hip_context *ctx, gt4hip_count_table *table, uint64_t tiles);
void *gt4hip_table_compact_bases (gt4hip_count_table *table);
void *gt4hip_table_padded_bases (gt4hip_count_table *table);
/* ... and the number of tiles (0: the table is contiguous) */
uint64_t gt4hip_table_ragged_tiles (const gt4hip_count_table *table);
/* A count table that exists for one call (gt4hip_select_multi, gt4hip_pairwise_multi) */
struct GT4HIP_LOCAL TempTable {
  gt4hip_count_table table;
  TempTable () : table () {}
  TempTable (const TempTable &) = delete;
  void operator= (const TempTable &) = delete;
  ~TempTable () { gt4hip_table_free (&table); }
};
/* gt4hip_union_table of lists that must all be there (GT4HIP_EINVAL) and of one word length (GT4HIP_EWORDLEN) */
GT4HIP_LOCAL int gt4hip_union_table_checked (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, gt4hip_count_table *table);
/* gt4hip_select.hip: rows the emit kernel ranks, stages and writes at a time, and rows per segment of a contiguous table
 * (a ragged table's segments are the rows of its tiles) */
#define GT4HIP_SELECT_TILE 1024u
#define GT4HIP_SELECT_SEGMENT 4096u
/* gt4hip_pairwise.hip: threads per workgroup of the partial kernel, rows a group of lanes has in flight, and list columns per
 * block (a workgroup reads THREADS / lanes per row x UNROLL rows per step; gt4hip_table_walk.h: the segments both walk) */
#define GT4HIP_PAIRWISE_THREADS 256u
#define GT4HIP_PAIRWISE_UNROLL 4u
#define GT4HIP_PAIRWISE_BLOCK 32u
void gt4hip_io_destroy (gt4hip_context *ctx);
/* threads per workgroup, which is items per block of work, of the item loops of gt4hip_query / _mismatch / _gmer.hip and
 * gt4hip_index.h (counter "mm_threads") and of gt4hip_caller.hip (counter "caller_threads"); workgroups of k_caller_mlogl
 * at most (counter "caller_max_grid"); words per block of the radix sort's histogram kernel (counter "sort_hist_chunk") */
#define GT4HIP_MM_THREADS 256
/* items per thread and tile of the compaction and hit passes (counter "mm_tile": items per tile), locations per thread and
 * tile of the gather (counter "gather_tile"), and the most bins gt4hip_list_count_histogram keeps in LDS (counter "hist_lds_bins") */
#define GT4HIP_MM_ROUNDS 8
#define GT4HIP_GATHER_ROUNDS 8
#define GT4HIP_HIST_LDS_BINS 4096u
/* words per thread and tile of gt4hip_seqprofile.hip's kernel (counter "profile_tile": words per tile) */
#define GT4HIP_PROFILE_ROUNDS 8
#define GT4HIP_CALLER_THREADS 256
#define GT4HIP_CALLER_MAX_GRID 1024
#define GT4HIP_SORT_HIST_THREADS 256
#define GT4HIP_SORT_HIST_ITEMS 16
/* bytes of text, and codes, per tile of gt4hip_maker.hip's kernels (counters "maker_text_tile", "maker_code_tile") */
#define GT4HIP_MAKER_TILE 4096u
/* items per tile of gt4hip_subset.hip's decision kernels (counter "subset_tile") and elements per thread of its scans
 * (counter "subset_scan_tile": elements per tile of a scan, 256 threads' worth) */
#define GT4HIP_SUBSET_TILE 4096u
#define GT4HIP_SUBSET_SCAN_V 8
/* raw locations per block of k_pack_locations (counter "pack_threads") */
#define GT4HIP_PACK_THREADS 256
/* gt4hip_text_to_words (gt4hip_maker.hip) for gt4hip_gmer.hip: with `counts`, one more pass over the piece's bytes and codes
 * sets counts[0..2] = 'N' / 'n' among the bytes the reference's reader loop takes (all in front of a NUL but FastQ '+'
 * lines), bases of sequence lines, and C / G among those (read_character and read_nucleotide, src/gmer_counter.c:917-936) */
GT4HIP_LOCAL int gt4hip_text_to_words_counted (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags,
                                               const gt4hip_maker_carry *in, gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words,
                                               uint64_t *error_offset, uint64_t counts[3]);
/* gt4hip_gmer.hip: k_mk_text_counts on the arrays of a reader call (text, tile states, codes, MakerInfo); out: three zeroed device words */
GT4HIP_LOCAL void gt4hip_launch_text_counts (hipStream_t stream, int grid, bool fastq, const unsigned char *d_text, size_t n_bytes, uint64_t tiles,
                                             const uint32_t *tile_state, const unsigned char *codes, const void *info, unsigned long long *out);
/* gt4hip_text_to_words for gt4hip_mask.hip: what a call of the reader has on the device while it lasts.  `then` runs behind
 * the words' kernel (the stream is drained, the totals are read back), before the call's blocks go back to the pool; it is
 * not called when the call fails or has nothing to read (no bytes, a piece behind a NUL, a NUL as the first byte of a file) */
struct gt4hip_reader_view {
  const unsigned char *d_text;  /* the piece on the device */
  size_t n_bytes;
  uint64_t tiles;               /* of GT4HIP_MAKER_TILE bytes of text; the tiles of codes are no more */
  const uint64_t *tile_off;     /* codes in front of each tile of text */
  const uint64_t *emit_off;     /* words that end in front of each tile of codes */
  const unsigned char *buf;     /* the halo's 32 codes, then the piece's (16-byte aligned, 64 readable bytes behind the last) */
  const void *info;             /* the device's MakerInfo (gt4hip_maker_tile.h) */
  uint64_t nul_pos, n_codes;    /* of it, as read back */
  const uint64_t *d_words;      /* NULL when there is none */
  uint64_t n_words;
};
typedef int (*gt4hip_reader_then) (gt4hip_context *ctx, const gt4hip_reader_view *view, void *arg);
GT4HIP_LOCAL int gt4hip_text_to_words_then (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags,
                                            const gt4hip_maker_carry *in, gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words,
                                            uint64_t *error_offset, gt4hip_reader_then then, void *arg);
/* gt4hip_query.hip for gt4hip_seqprofile.hip and gt4hip_mask.hip.  The argument rules of the lookups (`who` in the message); the list an index
 * was made of and its bucket offsets; the device time a call on the index reports (gt4hip_query_index_last_ms) */
GT4HIP_LOCAL int gt4hip_query_check_params (gt4hip_context *ctx, const char *who, const gt4hip_query_index *qindex, const gt4hip_query_params *params);
GT4HIP_LOCAL const gt4hip_list *gt4hip_query_index_list (const gt4hip_query_index *qindex);
GT4HIP_LOCAL const uint64_t *gt4hip_query_index_offsets (const gt4hip_query_index *qindex);
GT4HIP_LOCAL void gt4hip_query_index_set_ms (gt4hip_query_index *qindex, double ms);
/* The kernels of gt4hip_query_lookup on n > 0 words in DEVICE memory, enqueued on the context's stream and not waited for:
 * d_values[i] (and d_found[i]; may be NULL where n_mm > 0) as gt4hip_query_lookup defines them.  Sets counter "query_wide". */
GT4HIP_LOCAL int gt4hip_query_lookup_device (gt4hip_context *ctx, const char *who, gt4hip_query_index *qindex, const gt4hip_query_params *params,
                                             const uint64_t *d_words, uint64_t n, uint32_t *d_values, unsigned char *d_found);
int gt4hip_io_download (gt4hip_context *ctx, const void *dev, void *host, size_t bytes);
/* host memory (a file mapping, say) -> device memory, waited for: large extents in pieces through the staging threads */
int gt4hip_io_upload (gt4hip_context *ctx, const void *host, void *dev, size_t bytes);

#define HIPCHK(ctx, call)                                                                               \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return gt4hip_fail ((ctx), e_ == hipErrorOutOfMemory ? GT4HIP_ENOMEM : GT4HIP_EHIP, \
                                              "%s failed: %s", #call, hipGetErrorString (e_));          \
  } while (0)

#endif
