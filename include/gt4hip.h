/*
 * gt4hip.h -- C ABI of the MI355X (gfx950) sorted k-mer list set-operation engine.
 *
 * This is the drop-in boundary between a C host -- the glistcompare CLI in
 * genometester4_amd/csrc/gt4_glistcompare_cli.c, or GenomeTester4's own glistcompare.c / glistmaker.c /
 * glistquery.c with the binding shown in INTEGRATION.md -- and the hand-written HIP kernels.
 * Plain C types only; nothing here throws, exits or prints.  Every function returns
 * GT4HIP_OK (0) or a GT4HIP_E* code; gt4hip_last_error() gives the message.
 *
 * A "list" is an array of packed 12-byte records (u64 key LE + u32 count LE), strictly ascending
 * by key, resident in HBM -- the record layout of a GenomeTester4 .list file body
 * (reference src/word-map.h:89-99, src/word-list.h:61-72).
 *
 * Threading: one host thread per context.  The context owns its HIP stream and workspace;
 * callers never manage streams.  Inputs are borrowed for the duration of a call (the reference
 * maps them PROT_READ, src/utils.c:54); outputs belong to the caller and are released with
 * gt4hip_list_free().
 *
 * There is NO CPU fallback behind this interface: without a usable gfx950 device every entry
 * point fails with GT4HIP_ENODEVICE.
 */
#ifndef GT4HIP_H
#define GT4HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GT4HIP_RECORD_BYTES 12u

enum {
  GT4HIP_OK = 0,
  GT4HIP_EINVAL = 1,      /* bad argument                                   */
  GT4HIP_ENODEVICE = 2,   /* no usable GPU / HIP runtime failure at init     */
  GT4HIP_ENOMEM = 3,      /* device or host allocation failed                */
  GT4HIP_ERULE = 4,       /* rule not allowed for this operation (the reference returns 1:
                             src/glistcompare.c:518-523, :622-627)           */
  GT4HIP_EHIP = 5,        /* a HIP call or kernel failed                     */
  GT4HIP_EWORDLEN = 6,    /* lists of different word length                  */
  GT4HIP_EINTERNAL = 7,   /* in-kernel consistency check tripped             */
  GT4HIP_ECALLBACK = 8,   /* (internal) walk stopped by the caller's callback */
  GT4HIP_EIO = 9,         /* reading or writing a file descriptor failed       */
  GT4HIP_ECOMM = 10,      /* RCCL could not be loaded / a collective failed    */
  GT4HIP_EFORMAT = 11     /* sequence text that is neither FastA nor FastQ, or malformed FastQ; an index whose
                             sections contradict each other (gt4hip_location_index_create) */
};

/* enum Rules of the reference, src/glistcompare.c:45-54 (same numeric values) */
enum {
  GT4HIP_RULE_DEFAULT = 0,
  GT4HIP_RULE_ADD = 1,
  GT4HIP_RULE_SUBTRACT = 2,
  GT4HIP_RULE_MIN = 3,
  GT4HIP_RULE_MAX = 4,
  GT4HIP_RULE_FIRST = 5,
  GT4HIP_RULE_SECOND = 6,
  GT4HIP_RULE_NUMBER = 7
};

/* the four outputs of compare_wordmaps, src/glistcompare.c:814-834; also the index order */
enum {
  GT4HIP_OP_UNION = 1,   /* index 0: <out>_<k>_union.list   */
  GT4HIP_OP_INTRSEC = 2, /* index 1: <out>_<k>_intrsec.list */
  GT4HIP_OP_DIFF1 = 4,   /* index 2: <out>_<k>_0_diff1.list */
  GT4HIP_OP_DIFF2 = 8    /* index 3: <out>_<k>_0_diff2.list */
};

typedef struct gt4hip_context gt4hip_context;
typedef struct gt4hip_list gt4hip_list;

/* ---------------------------------------------------------------- (i) init / teardown */

/* Binds a context to HIP device `device` (>= 0), creating its stream and workspace. */
int gt4hip_create (int device, gt4hip_context **ctx);
void gt4hip_destroy (gt4hip_context *ctx);
/* Message of the last failure on this context (or of the last failed gt4hip_create when ctx is
 * NULL).  Valid until the next call on the same context. */
const char *gt4hip_last_error (const gt4hip_context *ctx);
const char *gt4hip_strerror (int code);
/* Number of HIP devices visible; 0 when there is none or the runtime is unusable. */
int gt4hip_device_count (void);
/* The device a context lives on, and: give the context's pooled (freed, kept for reuse) blocks back to the driver. */
int gt4hip_context_device (const gt4hip_context *ctx);
int gt4hip_trim (gt4hip_context *ctx);
/* Free and total bytes of the context's device memory right now (hipMemGetInfo). */
int gt4hip_device_memory (gt4hip_context *ctx, uint64_t *free_bytes, uint64_t *total_bytes);
/* "name|gcnArch|CUs|HBM bytes" of the context's device, for logs. */
const char *gt4hip_device_info (const gt4hip_context *ctx);

/* ---------------------------------------------------------------- lists in HBM */

/* Copies n_words packed records from host memory (pageable or pinned) into a new HBM list.
 * Replaces gt4_word_map_new's mmap (src/word-map.c:165-241) as the way a list becomes readable. */
int gt4hip_list_upload (gt4hip_context *ctx, const void *host_records, uint64_t n_words,
                        uint32_t word_length, gt4hip_list **out);
/* The same from the k-mer table of a GT4I index file (what gt4_index_map_new exposes through the
 * sorted-list interface, reference src/index-map.c:123-175): n_words 16-byte (word, first location)
 * entries; the count of entry i is entry i+1's first location minus its own, the last one's
 * num_locations minus its own, truncated to 32 bits.  Decoded on the device. */
int gt4hip_list_upload_index (gt4hip_context *ctx, const void *host_kmers, uint64_t n_words, uint64_t num_locations,
                              uint32_t word_length, gt4hip_list **out);
/* Wraps records already in device memory (4-byte aligned, as the body of a .list file and every
 * gt4hip_list_slice are); the storage is not freed by gt4hip_list_free. */
int gt4hip_list_wrap (gt4hip_context *ctx, void *device_records, uint64_t n_words,
                      uint32_t word_length, gt4hip_list **out);
/* Uninitialised list with room for `capacity` records (n_words = capacity until set). */
int gt4hip_list_alloc (gt4hip_context *ctx, uint64_t capacity, uint32_t word_length, gt4hip_list **out);
/* A view of records [first, first+count) of `list` (shares storage; used for key-range shards). */
int gt4hip_list_slice (gt4hip_context *ctx, const gt4hip_list *list, uint64_t first, uint64_t count,
                       gt4hip_list **out);
/* File <-> HBM transfers (replace gt4_mmap + scout, src/utils.c:35-99, and the
 * fwrite / write output loops, src/glistcompare.c:491-496, :579-582).  The body of a list moves in
 * 8 MiB pieces through pinned staging buffers owned by the context (set up once, on first use) on
 * GT4HIP_IO_THREADS (default 8) copy threads, each with its own HIP stream: pread -> pinned -> HBM
 * and HBM -> pinned -> pwrite overlap piece by piece.  `fd` needs no particular file position.
 *   _upload_fd  new list from n_words records at byte `file_offset` of `fd`
 *   _load_fd    the same into an existing list (capacity >= n_words; sets n_words)
 *   _load       the same from host memory (large pageable buffers go through the staging threads)
 *   _write_fd   records [first, first+count) of `list` to `fd` at byte `file_offset` (pwrite: several
 *               writers -- threads or processes -- may fill disjoint extents of one file) */
int gt4hip_list_upload_fd (gt4hip_context *ctx, int fd, uint64_t file_offset, uint64_t n_words, uint32_t word_length,
                           gt4hip_list **out);
int gt4hip_list_load_fd (gt4hip_context *ctx, gt4hip_list *list, int fd, uint64_t file_offset, uint64_t n_words);
int gt4hip_list_load (gt4hip_context *ctx, gt4hip_list *list, const void *host_records, uint64_t n_words);
int gt4hip_list_write_fd (gt4hip_context *ctx, const gt4hip_list *list, uint64_t first, uint64_t count, int fd,
                          uint64_t file_offset);
/* Up to four lists to four files in one go (the outputs of one compare_wordmaps pass): the copy threads
 * are dealt to the files, because several writers of ONE file serialise on its inode lock. */
int gt4hip_lists_write_fd (gt4hip_context *ctx, uint32_t n, const gt4hip_list *const lists[], const uint64_t first[],
                           const uint64_t count[], const int fds[], const uint64_t file_offsets[]);
/* Copies the records back to host memory (n_words * 12 bytes). */
int gt4hip_list_download (gt4hip_context *ctx, const gt4hip_list *list, void *host_records);
/* Copies records [first, first+count) back to host memory. */
int gt4hip_list_download_range (gt4hip_context *ctx, const gt4hip_list *list, uint64_t first,
                                uint64_t count, void *host_records);
/* Lists return their storage to their context's pool: free every list BEFORE gt4hip_destroy of the
 * context it came from (a list must not outlive its context). */
void gt4hip_list_free (gt4hip_list *list);

uint64_t gt4hip_list_n_words (const gt4hip_list *list);      /* GT4WordSListInstance.num_words   */
uint32_t gt4hip_list_word_length (const gt4hip_list *list);  /* GT4WordSListInstance.word_length */
void *gt4hip_list_device_ptr (const gt4hip_list *list);
int gt4hip_list_set_n_words (gt4hip_list *list, uint64_t n_words);
/* Sum of counts (GT4WordSListInstance.sum_counts), computed on the device. */
int gt4hip_list_sum_counts (gt4hip_context *ctx, const gt4hip_list *list, uint64_t *sum);
/* 1 if keys are strictly ascending (the precondition of every merge below), else 0. */
int gt4hip_list_is_sorted (gt4hip_context *ctx, const gt4hip_list *list, int *sorted);
/* Index of the first record with key >= `key` (binary search on the device; shard splitters). */
int gt4hip_list_lower_bound (gt4hip_context *ctx, const gt4hip_list *list, uint64_t key, uint64_t *index);
/* GT4WordSArray get_word(idx), src/word-array-sorted.h:41-49 */
int gt4hip_list_get_word (gt4hip_context *ctx, const gt4hip_list *list, uint64_t idx, uint64_t *word,
                          uint32_t *count);

/* ---------------------------------------------------------------- (ii) pair operation */

/* Arguments of compare_wordmaps (src/glistcompare.c:789-790), minus the file naming. */
typedef struct {
  uint32_t ops;            /* mask of GT4HIP_OP_*: which of the four outputs to produce      */
  int32_t rule;            /* GT4HIP_RULE_*; DEFAULT resolves per output as the reference does */
  uint32_t cutoff;         /* -c / --cutoff (default 1)                                       */
  int32_t subtract;        /* -du: diff1 keeps keys with equal counts (src/glistcompare.c:480) */
  uint32_t count_override; /* the integer given to -r (RULE_NUMBER)                           */
  int32_t count_only;      /* --count_only: totals only, no records materialised              */
} gt4hip_compare_params;

typedef struct {
  uint64_t n_words[4];     /* records per output (header n_words), 0 for outputs not requested */
  uint64_t total_count[4]; /* sum of counts per output (header total_count)                    */
  /* In: NULL, or a caller-provided list (gt4hip_list_alloc) with enough capacity to receive the
   * output -- ZERO the struct before the call (memset) unless outputs are provided: a garbage
   * pointer here is taken for a caller's list.  Out: the output records (a new list when NULL was passed; NULL for count_only and
   * for outputs not requested).  Worst-case capacities: union na+nb, intrsec min(na,nb),
   * diff1 na, diff2 nb. */
  gt4hip_list *out[4];
  double merge_kernel_ms;  /* device time of the merge kernel alone (HIP events on the stream)  */
  double device_ms;        /* device time of everything the call enqueued                        */
  uint64_t merge_tiles;    /* tiles the merge kernel processed                                   */
} gt4hip_compare_result;

/* One pass over the merged key sequence of a and b producing up to four outputs
 * (compare_wordmaps hot loop, src/glistcompare.c:843-905). */
int gt4hip_compare (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b,
                    const gt4hip_compare_params *params, gt4hip_compare_result *result);

/* ---------------------------------------------------------------- (ii b) difference up to N mismatches */

/* Arguments of compare_wordmaps_mm (glistcompare -mm N, src/glistcompare.c:958-1093). */
typedef struct {
  uint32_t ops;          /* GT4HIP_OP_DIFF1 and/or GT4HIP_OP_DIFF2 only             */
  uint32_t cutoff;
  int32_t  subtract;     /* -du                                                    */
  uint32_t n_mismatch;   /* N >= 1                                                 */
  int32_t  count_only;
} gt4hip_mismatch_params;

/* Per-call measurements of the last gt4hip_compare_mismatch on a context (gt4hip_mismatch_stats_get). */
#define GT4HIP_MM_MAX_LEVELS 32
typedef struct {
  uint64_t prepass_words[2];                    /* table sizes after the pre-pass: diff1, diff2 (0 if not requested) */
  double prepass_ms;                            /* device time of the pre-pass (= result.merge_kernel_ms)          */
  uint32_t n_levels;                            /* levels run: min(n_mismatch, GT4HIP_MM_MAX_LEVELS)               */
  double level_ms[GT4HIP_MM_MAX_LEVELS];        /* device time of level c + 1, both tables                         */
  uint64_t level_words[GT4HIP_MM_MAX_LEVELS];   /* words that entered level c + 1, both tables                     */
  uint64_t level_probes[GT4HIP_MM_MAX_LEVELS];  /* index lookups level c + 1 performed (after early exits)          */
  uint64_t probes;                              /* all lookups of the call, the pre-pass's included                */
} gt4hip_mismatch_stats;

/* The difference of a and b "up to N mismatches" (fetch_relevant_words, src/glistcompare.c:1134-1168): the
 * pre-pass table of compare_wordmaps_mm, then levels c = 1..N in which a word survives while the number of its
 * exactly-c-substitution variants (canonicalised) PRESENT in the other list -- not their counts -- stays below the
 * cutoff (with subtract: present in b and not in a count -1 each, and any variant in b but not in a drops the word).
 * Results go to slots 2 and 3 of `result` under the rules of gt4hip_compare (caller-provided lists, count_only);
 * merge_kernel_ms is the pre-pass, device_ms the whole call.  An empty lookup list holds no neighbour (the
 * reference crashes there).  Any op bit other than DIFF1 / DIFF2, or n_mismatch 0, is GT4HIP_EINVAL. */
int gt4hip_compare_mismatch (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b,
                             const gt4hip_mismatch_params *params, gt4hip_compare_result *result);
/* The measurements of the context's last successful gt4hip_compare_mismatch. */
int gt4hip_mismatch_stats_get (gt4hip_context *ctx, gt4hip_mismatch_stats *stats);

/* ---------------------------------------------------------------- (ii c) glistquery: lookups and list statistics */

/* The bucket index of a resident list (windows of ~8 records, at most 32 MiB), built once and used by every batch.
 * The index reads the list's records: keep the list alive and unchanged until gt4hip_query_index_free. */
typedef struct gt4hip_query_index gt4hip_query_index;
int gt4hip_query_index_create (gt4hip_context *ctx, const gt4hip_list *list, gt4hip_query_index **qindex);
void gt4hip_query_index_free (gt4hip_query_index *qindex);
/* Device time (HIP events) of the kernels of the last lookup call on this index, copies excluded. */
double gt4hip_query_index_last_ms (const gt4hip_query_index *qindex);

/* Arguments of gt4_word_dict_lookup_mm (src/word-dict.c:74-106) as search_one_word passes them. */
typedef struct {
  uint32_t n_mm;      /* -mm: substitutions allowed, 0..32; n_mm + pm_3 <= word length when n_mm > 0     */
  uint32_t pm_3;      /* -p: base positions 0..pm_3 - 1 (bits 2i, 2i + 1: the LAST bases) never change;
                         ignored when n_mm == 0                                                        */
  int32_t canonize;   /* non-zero (the reference's only mode): the query and every variant are replaced
                         by min (w, reverse complement); 0: words are looked up as they are            */
} gt4hip_query_params;

/* Variants per query, V = sum over c = 0..n_mm of C(k - pm_3, c) 3^c; GT4HIP_EINVAL when it does not fit 64 bits. */
int gt4hip_query_variants (uint32_t word_length, const gt4hip_query_params *params, uint64_t *n_variants);
/* The XOR mask of variant `rank` (0 <= rank < V): rank 0 is the word itself, then every variant with one
 * substitution, with two, ...  A substitution at base position i with m in 1..3 is m << 2i. */
int gt4hip_query_variant_mask (uint32_t word_length, const gt4hip_query_params *params, uint64_t rank, uint64_t *mask);

/* `words`: n_queries packed k-mers in HOST memory; `values` (u32) and `found` (one byte) per query, HOST memory too:
 * the call copies in, runs on the context's stream, copies out and returns when the results are there.
 * n_mm == 0: found = the (canonical) word is in the list, value = its count (a stored count of 0 is still found).
 * n_mm > 0: value = sum of the counts of all V variants found, each canonicalised before it is looked up, in uint32_t
 * arithmetic that wraps; two variants with the same canonical word count twice; found = value != 0.
 * n_queries x V must fit 64 bits (GT4HIP_EINVAL with a message otherwise). */
int gt4hip_query_lookup (gt4hip_context *ctx, gt4hip_query_index *qindex, const uint64_t *words, uint64_t n_queries,
                         const gt4hip_query_params *params, uint32_t *values, uint8_t *found);

typedef struct {
  uint64_t query;     /* number of the query in the batch                  */
  uint64_t rank;      /* the variant (gt4hip_query_variant_mask)           */
  uint64_t word;      /* the word that was found: the canonical variant    */
  uint32_t count;     /* its stored count (may be 0)                       */
  uint32_t reserved;
} gt4hip_query_hit;

/* The --all form: every variant that is in the list, in (query, rank) order.  Two passes on the device (count, then
 * fill): *n_hits is always the number of hits; `hits` (HOST memory, room for `capacity`) is filled only when
 * *n_hits <= capacity -- call with capacity 0 to size a buffer, or with a guess and again when *n_hits exceeds it. */
int gt4hip_query_lookup_all (gt4hip_context *ctx, gt4hip_query_index *qindex, const uint64_t *words, uint64_t n_queries,
                             const gt4hip_query_params *params, gt4hip_query_hit *hits, uint64_t capacity, uint64_t *n_hits);

/* ---- glistquery --locations: a GT4I index resident with its location section.
 * gt4hip_location_index_create takes the two sections of a mapped index file (include/gt4_listfile.h: index_kmers,
 * index_location_words) and keeps on the device: the k-mer section decoded to a list (gt4hip_location_index_list: what
 * gt4hip_query_index_create and every statistic take; it lives as long as the location index), the first location of
 * every k-mer, the packed locations, and the three bit sizes.  Both sections are copied from host memory in pieces.
 * The k-mer section is checked ON THE DEVICE in the same pass that decodes it: first locations that descend, or
 * one above num_locations, are GT4HIP_EFORMAT and nothing is made -- no kernel ever reads the location array through
 * an unchecked offset.  Bit sizes with n_file_bits + n_subseq_bits + n_pos_bits + 1 > 64 are GT4HIP_EFORMAT too.  An
 * index that does not fit the device is GT4HIP_ENOMEM. */
typedef struct gt4hip_location_index gt4hip_location_index;
int gt4hip_location_index_create (gt4hip_context *ctx, const void *host_kmers, uint64_t n_words, const void *host_locations,
                                  uint64_t num_locations, uint32_t word_length, uint32_t n_file_bits, uint32_t n_subseq_bits,
                                  uint32_t n_pos_bits, gt4hip_location_index **lindex);
void gt4hip_location_index_free (gt4hip_location_index *lindex);
const gt4hip_list *gt4hip_location_index_list (const gt4hip_location_index *lindex);
uint64_t gt4hip_location_index_n_locations (const gt4hip_location_index *lindex);

/* One place a word occurs, decoded (index_map_get_location, src/index-map.c:197-208): 16 bytes. */
typedef struct {
  uint64_t pos_dir;   /* position << 1 | strand (1: the canonical word is the reverse complement of the text) */
  uint32_t file;      /* number of the file ...                                                               */
  uint32_t seq;       /* ... and of the sequence in it, each in 32 bits as the reference holds them           */
} gt4hip_location;

/* gt4hip_query_lookup_all with the locations of every hit.  `qindex` must have been made of
 * gt4hip_location_index_list (lindex).  The hits are the same records in (query, rank) order; count is the number of
 * locations of the word in 32 bits (the reference's n_locations).  The locations of hit h are
 * locations[sum of the counts of the hits before h ... + its count), in the order of the index.  Two variants of a
 * query with the same canonical word are two hits, and the word's locations are copied twice, as the reference prints
 * them twice.  Both totals are always returned; the two HOST arrays are filled only when *n_hits <= hit_capacity AND
 * *n_locations <= loc_capacity, and are left untouched otherwise.  The device holds 16 bytes per location for the
 * call: a batch too large for it is GT4HIP_ENOMEM -- split it. */
int gt4hip_query_lookup_locations (gt4hip_context *ctx, gt4hip_query_index *qindex, const gt4hip_location_index *lindex,
                                   const uint64_t *words, uint64_t n_queries, const gt4hip_query_params *params,
                                   gt4hip_query_hit *hits, uint64_t hit_capacity, uint64_t *n_hits,
                                   gt4hip_location *locations, uint64_t loc_capacity, uint64_t *n_locations);
/* Device time of the gather kernel alone in the last gt4hip_query_lookup_locations on this index (HIP events). */
double gt4hip_query_index_gather_ms (const gt4hip_query_index *qindex);

/* One streaming pass over the records each (glistquery --median, --distribution, --gc; src/glistquery.c:831-932).
 * Smallest and largest count (0xffffffff and 0 for an empty list). */
int gt4hip_list_count_stats (gt4hip_context *ctx, const gt4hip_list *list, uint32_t *min, uint32_t *max);
/* Records with count < med and with count > med: one step of print_median's bisection. */
int gt4hip_list_count_split (gt4hip_context *ctx, const gt4hip_list *list, uint32_t med, uint64_t *below, uint64_t *above);
/* hist[c - 1] = records with count c, for 1 <= c <= max (`max` entries of host memory; counts of 0 are skipped). */
int gt4hip_list_count_histogram (gt4hip_context *ctx, const gt4hip_list *list, uint32_t max, uint64_t *hist);
/* Sum over the records of count x (G and C bases of the word). */
int gt4hip_list_gc (gt4hip_context *ctx, const gt4hip_list *list, uint64_t *weighted_gc_bases);

/* ---------------------------------------------------------------- (ii d) glistcompare --subset: random subsets */

/* The three methods of subset () (src/glistcompare.c:719-787).  The ITEMS the reference walks are the records of the
 * list (rand_unique, rand_weighted_unique) or their occurrences (rand: record i is count_i items). */
enum { GT4HIP_SUBSET_RAND = 0, GT4HIP_SUBSET_RAND_UNIQUE = 1, GT4HIP_SUBSET_RAND_WEIGHTED_UNIQUE = 2 };
typedef struct {
  uint32_t method;    /* GT4HIP_SUBSET_*                                                                        */
  uint64_t size;      /* SIZE: items to select                                                                  */
  uint64_t state48;   /* X0 of drand48's generator: srand48 (seed) sets ((uint32_t) seed << 16) | 0x330E        */
} gt4hip_subset_params;

/* The list the reference writes for the same list, method, SIZE and generator state, record for record: item i is
 * selected iff fewer than SIZE items were selected before it and draw i of drand48 is <= (double) out / in
 * (rand_weighted_unique: (double) count * out / in), evaluated in IEEE double as the C expression stands.  The serial
 * walk is solved as a fixed point on the device; the input is only read.  *out is a new list (the
 * caller's, gt4hip_list_free) with *n_words records whose counts add up to *total_count; for rand a record carries the
 * number of its selected occurrences.  SIZE 0 or an empty list give an empty list.  Where fewer than SIZE items are
 * selected behind the last item (rand with SIZE above the sum of the counts, the unique methods with SIZE above the
 * number of records, a rand_weighted_unique walk that falls short) the reference does not terminate or writes the last
 * record twice: here that is GT4HIP_EINVAL, the message names the method, SIZE and the number reached, and no list is
 * made.  Device memory, all sized from the call: 8 bytes per record (not for rand_unique), 24 bytes per tile of
 * "subset_tile" items, for rand 12 more bytes per record; GT4HIP_ENOMEM when that does not fit -- nothing is chunked.
 * Counters: "subset_passes", "subset_tile", "subset_us". */
int gt4hip_list_subset (gt4hip_context *ctx, const gt4hip_list *list, const gt4hip_subset_params *params,
                        gt4hip_list **out, uint64_t *n_words, uint64_t *total_count);
/* The generator's state `position` steps behind state48, by the jump-ahead table the kernels' threads start from
 * (48 affine maps, one per power of two; host code, no device needed).  Draw i of drand48 is (the state at position i + 1) / 2^48. */
uint64_t gt4hip_subset_state_at (uint64_t state48, uint64_t position);

/* ---------------------------------------------------------------- (iii) N-way operations */

typedef struct {
  uint64_t n_words;
  uint64_t total_count;
  gt4hip_list *out;        /* as gt4hip_compare_result.out: optional in, result out */
  double device_ms;
  uint64_t records_read;    /* records the pairwise merges of this call read (all levels) ...      */
  uint64_t records_written; /* ... and wrote: 12 bytes each, the HBM traffic the call really caused */
} gt4hip_multi_result;

/* union_multi, src/glistcompare.c:500-603: rule in {DEFAULT(=ADD), ADD, MAX, NUMBER}, cutoff
 * applied to the RESULTING count.  Empty lists are skipped. */
int gt4hip_union_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                        uint32_t cutoff, int32_t rule, uint32_t count_override, int32_t count_only,
                        gt4hip_multi_result *result);
/* intersect_multi, src/glistcompare.c:605-717: rule in {DEFAULT(=MIN), MIN, MAX, ADD, NUMBER}. */
int gt4hip_intersect_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                            uint32_t cutoff, int32_t rule, uint32_t count_override, int32_t count_only,
                            gt4hip_multi_result *result);

/* Per-key count table of an N-way union: for every distinct key ascending, counts[j] = count in
 * list j or 0 (what gt4_union hands to its callback, src/set-operations.c:161-179).  Up to 32 non-empty lists:
 * one launch of the N-way tile kernel (a ragged table, see below; nine and more lists: its 32-list instance -- 32 lists of
 * 2e7 entries, 3.4e8 rows: 13.6 ms against 540 ms by merges, profiles/round5); more than 32, option "kway_max" = 8 beyond
 * eight, or a ragged table that does not fit the device: by merges -- the N-way union gives the keys, and each column is
 * one more streaming merge of the key list with list j (rule SECOND keeps list j's count, absent keys get 0).
 * keys_out: n_keys u64; counts_out: n_keys * n_lists u32, row-major.  Both are device buffers
 * owned by the result; release with gt4hip_table_free. */
typedef struct {
  uint64_t n_keys;
  uint32_t n_lists;
  void *device_keys;
  void *device_counts;
  void *owner[2]; /* library-private: the pooled device blocks behind the two arrays */
  /* Non-NULL: the table is RAGGED.  gt4hip_union_table of up to 32 lists writes the table in ONE launch of the
   * N-way tile kernel: a tile of the merged key sequence puts its rows where its RECORDS start (it has at most as many
   * distinct keys as records), so the two arrays are allocated for the lists' records and hold unused rows behind
   * every tile's.  gt4hip_table_download gathers the rows asked for; gt4hip_table_compact turns the table into the
   * contiguous form (n_keys rows, ragged = NULL) for callers that read the device arrays themselves. */
  void *ragged;
} gt4hip_count_table;
int gt4hip_union_table (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                        gt4hip_count_table *table);
/* The same table restricted to the keys of lists[0] (what gt4_is_union walks,
 * src/set-operations.c:207-226): n_keys = n_words of lists[0], column 0 = its own counts. */
int gt4hip_probe_table (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                        gt4hip_count_table *table);
/* The same with `presence` != 0: column j holds 1 where list j contains the key and 0 where it does
 * not (a list may hold a key with count 0): what search_lists_multi needs beside the counts
 * (reference src/glistquery.c:776-812). */
int gt4hip_probe_table_ex (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, int presence,
                           gt4hip_count_table *table);
/* Makes a ragged table contiguous on the device (a gather into new arrays; a no-op for a contiguous one). */
int gt4hip_table_compact (gt4hip_context *ctx, gt4hip_count_table *table);
/* Copies rows [first, first+count) of the table to host memory. */
int gt4hip_table_download (gt4hip_context *ctx, const gt4hip_count_table *table, uint64_t first,
                           uint64_t count, uint64_t *host_keys, uint32_t *host_counts);
void gt4hip_table_free (gt4hip_count_table *table);

/* glistcompare -u --min_lists M --max_lists X (not in the reference): the records of the N-way union whose word lies in M to
 * X of the N lists.  For a word, p is the number of lists that hold it with a count other than 0 (a record with count 0 does
 * not make its list a holder: the count table cannot tell it from absence); the result is the subsequence of what
 * gt4hip_union_multi gives for the same lists, rule, cutoff and override with min_lists <= p <= max_lists, record for record.
 * min_lists 1 and max_lists n_lists: the union itself (where every stored count is at least 1); both n_lists: the key set of
 * the intersection.  Rules as gt4hip_union_multi (anything else: GT4HIP_ERULE); an empty list counts towards n_lists and holds
 * nothing; 1 <= min_lists <= max_lists <= n_lists, else GT4HIP_EINVAL with a message.  `result` as gt4hip_union_multi:
 * result->out may bring a list of enough capacity (the kept records; n_keys of the table always suffice), device_ms is the
 * select kernels alone, records_read the table's rows, records_written the kept ones.
 * gt4hip_select_multi builds the table with gt4hip_union_table (one launch for up to 32 non-empty lists, by merges beyond)
 * and hands it to gt4hip_table_select, which takes a table as it is, ragged or contiguous, and leaves it unchanged: every row
 * is read once, (8 + 4 n_lists) bytes, plus 5 bytes of workspace written and read per row; 12 bytes are written per kept
 * record.  A list gt4hip_table_select makes itself says word length 32: a table does not know its own. */
int gt4hip_select_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                         uint32_t min_lists, uint32_t max_lists, uint32_t cutoff, int32_t rule,
                         uint32_t count_override, int32_t count_only, gt4hip_multi_result *result);
int gt4hip_table_select (gt4hip_context *ctx, const gt4hip_count_table *table, uint32_t min_lists, uint32_t max_lists,
                         uint32_t cutoff, int32_t rule, uint32_t count_override, int32_t count_only,
                         gt4hip_multi_result *result);

/* glistcompare L1 .. LN --pairwise (not in the reference): what every list shares with every other one.  With c_i (w) the
 * count of word w in list i, 0 where it is absent (a record with count 0 is the same as absence: the count table cannot tell
 * the two apart), two matrices of n_lists x n_lists numbers, row-major:
 *   host_shared[i * n_lists + j]     the words w with c_i (w) > 0 and c_j (w) > 0
 *   host_min_total[i * n_lists + j]  the sum over all words of min (c_i (w), c_j (w))
 * Both are symmetric and filled in full, both triangles and the diagonal, which holds a list's words with a count other than
 * 0 and the sum of its counts.  For i != j the two numbers are the NUnique and NTotal lines of `glistcompare Li Lj -i
 * --count_only` under the default rule; the union's size is shared[i][i] + shared[j][j] - shared[i][j], the two differences'
 * shared[i][i] - shared[i][j] and shared[j][j] - shared[i][j].  An empty list counts towards n_lists, its row and column are
 * 0; n_lists = 1 is valid; lists of different word lengths: GT4HIP_EWORDLEN.  device_ms (may be NULL) is the time of the
 * pairwise kernels alone.
 * gt4hip_pairwise_multi builds the table with gt4hip_union_table, hands it to gt4hip_table_pairwise and frees it.
 * gt4hip_table_pairwise takes a table as it is, ragged or contiguous, and leaves it unchanged: up to 32 lists, every row's
 * counts are read exactly once, 4 n_lists bytes (the keys are not read); beyond that the list columns are taken in blocks of
 * 32 and the table is read ceil (n_lists / 32) times.  A row that p lists hold costs p (p - 1) / 2 updates. */
int gt4hip_table_pairwise (gt4hip_context *ctx, const gt4hip_count_table *table,
                           uint64_t *host_shared, uint64_t *host_min_total, float *device_ms);
int gt4hip_pairwise_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists,
                           uint64_t *host_shared, uint64_t *host_min_total, float *device_ms);

/* ---------------------------------------------------------------- (e) key-range shards across GPUs */

/* Every set operation above is key-local, so the key space can be cut into contiguous ranges: shard
 * g merges only the records of its range (cut out of every input with a lower_bound), and the shards'
 * outputs concatenated in shard order are the sorted result.  One process per GPU.
 * First key of shard g of n_shards equal-width ranges of the 4^word_length key space (2^64 for
 * k = 32); shard g covers [first(g), first(g+1)), the last one everything from first(n_shards-1). */
uint64_t gt4hip_shard_first_key (uint32_t word_length, uint32_t n_shards, uint32_t g);
/* SAMPLED cuts for lists resident in HBM (equal-width ranges balance only uniformly spread keys: the packed word IS
 * the sequence, reference src/sequence.c:116-130): first_keys[g], g < n_shards, is the first key of shard g
 * (first_keys[0] = 0) such that the shards hold about the same number of INPUT records of the n lists together
 * (every (total / 65536)-th key of every list, merged).  Deterministic: ranks holding the same lists get the same cuts. */
int gt4hip_shard_cuts (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n, uint32_t n_shards, uint64_t *first_keys);

/* The exchange step: gatherv of the shards' records on `root` over RCCL (xGMI inside a node), as
 * grouped ncclSend / ncclRecv (RCCL has no native gatherv).  librccl.so is loaded by the first call
 * of this group only.  The communicator id is made by ONE rank (gt4hip_comm_unique_id) and handed
 * to the others by whatever the host has (shared memory after fork, a file, MPI, torch.distributed). */
#define GT4HIP_COMM_ID_BYTES 128
typedef struct gt4hip_comm gt4hip_comm;
int gt4hip_comm_unique_id (void *id_out);
int gt4hip_comm_create (gt4hip_context *ctx, const void *id, int n_ranks, int rank, gt4hip_comm **comm);
void gt4hip_comm_destroy (gt4hip_comm *comm);
int gt4hip_comm_rank (const gt4hip_comm *comm);
int gt4hip_comm_size (const gt4hip_comm *comm);
/* Message of the last failed gt4hip_comm_unique_id (no context yet at that point). */
const char *gt4hip_comm_last_error (void);
/* The other exchange of a sharded step: every rank's (n_words, total_count) to every rank (header totals, output
 * offsets): one ncclAllGather of two 64-bit words per rank on the library's stream, one synchronisation.
 * totals[2 r], totals[2 r + 1] = rank r's pair (2 * gt4hip_comm_size words). */
int gt4hip_comm_allgather_totals (gt4hip_comm *c, uint64_t n_words, uint64_t total_count, uint64_t *totals);
/* ... n <= 8 words per rank (the totals of every output of a pair operation at once): all[n r + i] = word i of rank r */
int gt4hip_comm_allgather_u64 (gt4hip_comm *c, const uint64_t *mine, uint32_t n, uint64_t *all);

/* counts[r] = records rank r contributes (every rank passes the same array: the all-gathered header
 * totals).  Rank r sends the first counts[r] records of `local`; on `root`, `gathered` (capacity >=
 * the sum) receives them in rank order and its n_words is set; other ranks pass NULL.  Blocks until
 * this rank's part is done. */
int gt4hip_comm_gatherv (gt4hip_comm *comm, const gt4hip_list *local, const uint64_t counts[], int root,
                         gt4hip_list *gathered);

/* ---------------------------------------------------------------- glistmaker's table step */

/* Sorts n_words packed 64-bit k-mer words (device memory) ascending, in place: the reference's
 * wordtable_sort (src/word-table.c:217-231; hybridInPlaceRadixSort256, src/utils.c:127-198) as an LSD
 * radix sort over the 2 * word_length significant bits (8- and 9-bit digits; one histogram kernel, then one
 * chained-scan scatter kernel per digit).  Needs n_words * 8 bytes of scratch + 4 KB of scan state per
 * 8192 words (0.5 GB per 10^9 words).  n_words < 2^56 and fewer than 2^32 tiles of 8192 words (n_words <
 * 2^45); more is GT4HIP_EINVAL.  The scans' waits are bounded (option "spin_limit"): one that gives up
 * -- a device shared with a stuck process -- makes the call return GT4HIP_EHIP. */
int gt4hip_sort_words (gt4hip_context *ctx, void *device_words, uint64_t n_words, uint32_t word_length);
/* Sort + wordtable_find_frequencies (src/word-table.c:233-260): host words (any order, repeats
 * allowed) -> a new list of (word, number of occurrences) records, ascending -- what glistmaker writes
 * to its temporary lists before gt4_write_union collates them (src/glistmaker.c:914-924, :333, :814). */
int gt4hip_words_to_list (gt4hip_context *ctx, const uint64_t *host_words, uint64_t n_words, uint32_t word_length,
                          gt4hip_list **out);
/* The same for words already in device memory.  The words are scratch from the call on: their buffer
 * holds the sorted words or the last pass's input afterwards, whichever the number of passes leaves. */
int gt4hip_device_words_to_list (gt4hip_context *ctx, void *device_words, uint64_t n_words, uint32_t word_length,
                                 gt4hip_list **out);

/* ---------------------------------------------------------------- glistmaker --index: words with a value each */

/* gt4hip_sort_words for (word, value) pairs: n_pairs words and as many 64-bit values (two device arrays), both in
 * place, ascending by word over its 2 * word_length significant bits.  The same digits and chained scan; every pass
 * moves 32 bytes per pair.  Stable: the values of equal words stay in the order they came, so values that ascend in
 * the input -- packed locations in text order -- ascend within every word afterwards (the order the reference sorts
 * them into, src/glistmaker.c:569).  Needs n_pairs * 16 bytes of scratch + the scan state of gt4hip_sort_words. */
int gt4hip_sort_pairs (gt4hip_context *ctx, void *device_words, void *device_values, uint64_t n_pairs,
                       uint32_t word_length);

/* The two arrays behind the file block of a GT4I index (reference src/glistmaker.c:425-574), in device memory. */
typedef struct {
  uint64_t n_kmers;             /* words kept by the cut-offs                                                        */
  uint64_t n_locations;         /* values of the kept words: what the index header calls n_locations                 */
  uint64_t n_values;            /* values in d_locations: all of them, the cut-offs do not filter this section (:568) */
  const uint64_t *d_kmers;      /* n_kmers x (word, index of its first value counting the kept words' values only)   */
  const uint64_t *d_locations;  /* the caller's values, sorted by word, in text order within a word                   */
} gt4hip_index_arrays;

/* write_kmers + write_locations (:425-574) for pairs in device memory: gt4hip_sort_pairs, equal words folded, words
 * with fewer than min_locations or more than max_locations values dropped from the k-mer section (:486).  Start
 * indices advance over the kept words only, and the values stay unfiltered, as in the reference: with cut-offs the two
 * sections do not agree, and a reader gets what the reference's file gives it.  Both input arrays are sorted in place;
 * d_locations is device_values.  d_kmers is the context's, one at a time: it lasts until gt4hip_index_free, the
 * context's next gt4hip_pairs_to_index or gt4hip_destroy.  Download either with gt4hip_words_download.  A word's values are
 * counted in 32 bits, as the reference counts them (:459): a word with 2^32 or more is GT4HIP_EINVAL, nothing is returned. */
int gt4hip_pairs_to_index (gt4hip_context *ctx, void *device_words, void *device_values, uint64_t n_pairs,
                           uint32_t word_length, uint32_t min_locations, uint32_t max_locations,
                           gt4hip_index_arrays *out);
void gt4hip_index_free (gt4hip_context *ctx);

/* ---------------------------------------------------------------- glistmaker's front: sequence text -> words */

enum {
  GT4HIP_MAKER_FORWARD_ONLY = 1,   /* the forward word as it stands, not min (word, reverse complement)              */
  GT4HIP_MAKER_TEXT_ON_DEVICE = 2  /* `text` is device memory (16-byte aligned); else host memory, copied in by the call */
};
enum { GT4HIP_MAKER_FASTA = 1, GT4HIP_MAKER_FASTQ = 2 };
/* what GT4HIP_EFORMAT stands for (gt4hip_maker_carry.error), with the reference's message in src/fasta.c */
enum {
  GT4HIP_MAKER_ERR_START = 1,    /* :136 the first byte of a file is neither '>' nor '@'                              */
  GT4HIP_MAKER_ERR_PLUS = 2,     /* :202 the line behind a FastQ sequence line does not start with '+' (or is missing) */
  GT4HIP_MAKER_ERR_AT = 3,       /* :277 the byte behind a FastQ quality line is neither '@' nor the end of the text  */
  GT4HIP_MAKER_ERR_PLUS_EOF = 4  /* :211 the text ends inside a FastQ '+' line                                        */
};

/* The reader's state between two pieces of one file: hand the `out` of a piece to the next piece as `in`; NULL starts a
 * file.  A piece may be cut anywhere. */
typedef struct {
  uint32_t file_type;      /* 0: nothing read yet; GT4HIP_MAKER_FASTA / _FASTQ, decided by the first byte of the file */
  uint32_t in_name;        /* FastA: the piece ended inside a name                                                    */
  uint32_t line_phase;     /* FastQ: '\n's so far mod 4 (0 name, 1 sequence, 2 '+' line, 3 quality)                   */
  uint32_t at_line_start;  /* the last byte was a '\n' (or there was none yet)                                        */
  uint32_t ended;          /* a NUL byte ended the text (the reference's end of file): later pieces give nothing      */
  uint32_t error;          /* GT4HIP_MAKER_ERR_* when the call returned GT4HIP_EFORMAT                                */
  uint8_t codes[32];       /* the last codes (0..3 a base, 4 none): the word_length - 1 bases a word of the next piece may begin with */
} gt4hip_maker_carry;

/* fasta_reader_read_nwords (src/fasta.c:87-291) as glistmaker runs it (canonising, src/listmaker-queue.c:196) on
 * `n_bytes` of FastA / FastQ text: every word of `word_length` bases, in text order, into a new device buffer
 * (*d_words, *n_words; NULL and 0 when there is none).  The buffer is the context's, one at a time: it is scratch for
 * gt4hip_device_words_to_list and lasts until gt4hip_words_free (d_words NULL: whatever the context holds), the
 * context's next gt4hip_text_to_words or gt4hip_destroy.  Bytes < ' ' are skipped, so words span line breaks; any other byte that is no base
 * ends the run; a NUL byte ends the text.  Malformed text is GT4HIP_EFORMAT with the offending byte's offset in
 * *error_offset (may be NULL) and the kind in out->error; what the end of the file makes of a FastQ text that stops
 * behind a sequence line or inside a '+' line is the caller's to report, unless a NUL ended it (gt4hip_text_to_list does). */
int gt4hip_text_to_words (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags,
                          const gt4hip_maker_carry *in, gt4hip_maker_carry *out, uint64_t **d_words, uint64_t *n_words,
                          uint64_t *error_offset);
/* Gives the context's word buffer back.  The context holds exactly one: `d_words` is that buffer's address or NULL
 * ("whatever the context holds"); any other pointer is ignored.  A d_words of an earlier gt4hip_text_to_words is
 * invalid from the moment the context's next gt4hip_text_to_words is entered, also when that call fails or gives no
 * words: finish with the words of a piece (gt4hip_device_words_to_list, gt4hip_words_download) before the next piece. */
void gt4hip_words_free (gt4hip_context *ctx, uint64_t *d_words);
/* n_words words of such a buffer -> host memory */
int gt4hip_words_download (gt4hip_context *ctx, const uint64_t *d_words, uint64_t n_words, uint64_t *host_words);
/* One whole text -> the list glistmaker writes for it: gt4hip_text_to_words, then gt4hip_device_words_to_list. */
int gt4hip_text_to_list (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags,
                         gt4hip_list **out);

/* ---------------------------------------------------------------- glistmaker --index: where every word stands */

/* One sequence of a file as the file block of a GT4I index records it (reference src/glistmaker.c:659-692): byte offsets
 * in the file; seq_len runs to the next name's tag or the end of the file (FastA, line breaks included) or to the end of
 * the sequence line (FastQ).  The file holds name_len in 32 bits. */
typedef struct {
  uint64_t name_pos, name_len, seq_pos, seq_len;
} gt4hip_subseq;

/* gt4hip_maker_carry for gt4hip_text_to_locations: hand the `out` of a piece to the next piece as `in`; NULL starts a file. */
typedef struct {
  gt4hip_maker_carry reader;
  uint64_t offset;        /* bytes of the file in front of the next piece                                               */
  uint64_t n_events;      /* name starts, sequence starts and FastQ sequence ends so far                                */
  uint64_t n_subseqs;     /* sequences begun so far: the ordinal of the next one                                        */
  uint64_t seq_codes;     /* bytes >= ' ' since the last sequence began                                                 */
  uint64_t max_position;  /* largest position of a word so far (the reference's max_lpos)                               */
  uint64_t name_pos;      /* of the name begun last                                                                     */
  uint64_t seq_pos;       /* of the sequence begun last                                                                 */
  uint32_t seq_open;      /* that sequence has not ended: at the end of the file its seq_len is file size - seq_pos     */
  uint32_t pad;
} gt4hip_locations_carry;

/* what a piece gave beside its words */
typedef struct {
  uint64_t n_words;
  uint64_t n_subseqs;            /* sequences that begin in the piece                                                   */
  const gt4hip_subseq *subseqs;  /* host memory of the context: until gt4hip_locations_free, the context's next
                                    gt4hip_text_to_locations or gt4hip_destroy.  seq_len is 0 where the sequence -- the
                                    last one -- is still open behind the piece (out->seq_open)                          */
  uint64_t closed_seq_len;       /* closed: the sequence that was open in front of the piece ended in it, this long     */
  uint32_t closed, pad;
} gt4hip_locations_piece;

/* gt4hip_text_to_words that also says where every word stands (read_word_index, src/glistmaker.c:1054-1067): word i of
 * the piece into d_words[i] and ordinal << 33 | position << 1 | strand into d_raw[i] -- the ordinal of its sequence
 * within the file, the bytes >= ' ' of that sequence in front of the word (:1064), and 1 when the canonical word is the
 * reverse complement.  d_words and d_raw are the caller's device arrays of `capacity` words each (gt4hip_pairs_reserve,
 * or any device memory): a piece with more words is GT4HIP_ENOMEM and writes nothing.  An ordinal of 2^31 or a position
 * of 2^32 or more is GT4HIP_EINVAL.  GT4HIP_MAKER_FORWARD_ONLY is not accepted.  Errors of the text as in gt4hip_text_to_words,
 * the kind in out->reader.error. */
int gt4hip_text_to_locations (gt4hip_context *ctx, const void *text, size_t n_bytes, unsigned word_length, unsigned flags,
                              const gt4hip_locations_carry *in, gt4hip_locations_carry *out, uint64_t *d_words,
                              uint64_t *d_raw, uint64_t capacity, gt4hip_locations_piece *piece, uint64_t *error_offset);
void gt4hip_locations_free (gt4hip_context *ctx);
/* n raw locations of file number `file` (device memory, in place) -> the words of an index's location section:
 * file << (subseq_bits + pos_bits + 1) | ordinal << (pos_bits + 1) | position << 1 | strand (:1066).  The bit sizes are
 * known behind the last file only, hence a step of its own.  Sizes that do not fit 64 bits together are GT4HIP_EINVAL. */
int gt4hip_pack_locations (gt4hip_context *ctx, uint64_t *d_raw, uint64_t n, uint64_t file, unsigned subseq_bits,
                           unsigned pos_bits);
/* Device memory for n_pairs words and as many values, one block of the context (one at a time): until
 * gt4hip_pairs_release, the context's next gt4hip_pairs_reserve or gt4hip_destroy.  GT4HIP_ENOMEM names the bytes. */
int gt4hip_pairs_reserve (gt4hip_context *ctx, uint64_t n_pairs, uint64_t **d_words, uint64_t **d_values);
void gt4hip_pairs_release (gt4hip_context *ctx);

/* ---------------------------------------------------------------- glistquery --per_sequence: the hits of every sequence of a text */

/* The words of a text looked up in a list (gt4hip_query_index, above) and the results added up per sequence.
 * value (w) is what gt4hip_query_lookup gives for the word (n_mm == 0: the stored count; n_mm > 0: the wrapping 32-bit sum
 * over the variants found) and `found` its found; a word is a HIT when it is found and min_value <= value <= max_value.
 * With n_mm == 0 an absent word is never a hit, also with min_value 0; a stored count of 0 is found.  n_hits counts the
 * hits of a sequence, sum adds their values in 64 bits, n_words counts every word. */
typedef struct { uint64_t n_words, n_hits, sum; } gt4hip_seq_profile;

/* words and raw locations already on the device (what gt4hip_text_to_locations leaves): the words' ordinals
 * (raw >> 33) ascend and lie in [first_ordinal, first_ordinal + n_seqs); profiles[s] (HOST, n_seqs entries) is
 * SET to what the words of ordinal first_ordinal + s give; a sequence without words gives {0, 0, 0}.  The words are looked
 * up as they stand (the reader's words are canonical); the word length is the index's list's.  Ordinals that descend or
 * leave the range are GT4HIP_EINVAL: the kernel checks every ordinal before it addresses anything with it and raises one
 * flag word.  The device holds 24 bytes per sequence for the call, with n_mm > 0 four more per word.  One kernel over tiles of
 * "profile_tile" words: a tile adds to a sequence's three sums once, with 64-bit integer adds, so the
 * result does not depend on the order; the sums are zeroed by a launch of the call.  gt4hip_query_index_last_ms: the call's kernels. */
int gt4hip_query_profile_words (gt4hip_context *ctx, gt4hip_query_index *qindex, const uint64_t *d_words, const uint64_t *d_raw,
                                uint64_t n_words, uint64_t first_ordinal, uint64_t n_seqs, const gt4hip_query_params *params,
                                uint32_t min_value, uint32_t max_value, gt4hip_seq_profile *profiles);

/* one piece of a file: gt4hip_text_to_locations into a block of the call, then the above.  Entry 0 is what the piece
 * adds to the sequence left open by the piece before (only when in && in->seq_open); then one entry per sequence
 * that begins in the piece (piece->n_subseqs).  *n_profiles is always set; the array is filled only when it fits `capacity`.
 * `flags`: GT4HIP_MAKER_TEXT_ON_DEVICE.  The carry, `piece` (its records last as gt4hip_text_to_locations says), the errors
 * of the text and the reader's limits are gt4hip_text_to_locations's.  The device holds 16 bytes per byte of the piece. */
int gt4hip_query_profile_text (gt4hip_context *ctx, gt4hip_query_index *qindex, const void *text, size_t n_bytes, unsigned flags,
                               const gt4hip_query_params *params, uint32_t min_value, uint32_t max_value,
                               const gt4hip_locations_carry *in, gt4hip_locations_carry *out, gt4hip_locations_piece *piece,
                               gt4hip_seq_profile *profiles, uint64_t capacity, uint64_t *n_profiles, uint64_t *error_offset);

/* ---------------------------------------------------------------- glistquery --mask: the bases a list's words cover */

/* what a piece gave: words that END in the piece and the hits among them (as gt4hip_seq_profile counts them), the piece's
 * own covered bases, and how many of the last bytes >= ' ' IN FRONT of the piece a hit word of this piece covers */
typedef struct { uint64_t n_words, n_hits, n_covered; uint32_t back, pad; } gt4hip_mask_piece;
enum { GT4HIP_MASK_SOFT = 4 }; /* beside GT4HIP_MAKER_TEXT_ON_DEVICE, which here also says that `masked` is device memory (16-byte aligned) */

/* One piece of a file with every covered base replaced.  The text's words are gt4hip_text_to_words's (canonising); a word is
 * a HIT by the rule of gt4hip_seq_profile above (found, and min_value <= value <= max_value, under params' n_mm / pm_3); a
 * base is COVERED when it is one of the word_length bases of at least one hit word.  masked[0 .. n_bytes) = the piece with
 * its covered bases written as mask_byte, with GT4HIP_MASK_SOFT as byte | 0x20; every other byte, and every byte from a NUL
 * on, as it is.  A hit word that ends in this piece may begin in front of it: piece->back (0 .. word_length - 1, never more
 * than the bases the carry holds) says how many of the last bytes >= ' ' in front of the piece it covers -- a suffix of
 * them, all bases --, which the caller patches; they are not counted in n_covered.  The carry, the errors of the text and
 * *error_offset are gt4hip_text_to_words's; after an error `masked` holds nothing.  The context's word buffer is released.
 * On the device the call holds, per byte of the piece: 1 (the codes) + 1/8 (one bit per code) + 8 per word (at most one per
 * byte), for host text 2 more (the text and the masked text), with n_mm > 0 4 more per word: 11 1/8 bytes at most, 15 1/8 with
 * mismatches.  gt4hip_query_index_last_ms: the lookups and the two masking kernels. */
int gt4hip_query_mask_text (gt4hip_context *ctx, gt4hip_query_index *qindex, const void *text, size_t n_bytes, unsigned flags,
                            const gt4hip_query_params *params, uint32_t min_value, uint32_t max_value, unsigned char mask_byte,
                            const gt4hip_maker_carry *in, gt4hip_maker_carry *out, void *masked, gt4hip_mask_piece *piece,
                            uint64_t *error_offset);

/* ---------------------------------------------------------------- gmer_counter: database k-mers counted in reads */

/* A k-mer database resident in HBM (reference src/database.c, src/gmer_counter.c:751-815, without the trie): the
 * canonical words sorted into 12-byte list records that carry the k-mer's index where a list keeps its count, the bucket
 * index of those records, and one 64-bit counter per k-mer.  Counters never saturate here: clamping to 16 or 32 bits is the
 * caller's (the reference stops at 65535, or at 0xffffffff with -32). */
typedef struct gt4hip_gmer_db gt4hip_gmer_db;
enum {
  GT4HIP_GMER_ON_DEVICE = 2,     /* `words` / `text` is device memory (the bit of GT4HIP_MAKER_TEXT_ON_DEVICE)                   */
  GT4HIP_GMER_PLAIN_ATOMICS = 4  /* every hit its own atomic; default: a wavefront whose hits all fall on ONE k-mer adds their
                                    number with one atomic (a read of one repeated base), any other wavefront one atomic per hit */
};
/* Word i of host_words (n_kmers < 2^32 words below 4^word_length, any order, either strand) owns counter i.  On the device:
 * canonicalised, sorted with the index as the value (gt4hip_sort_pairs), packed and indexed; the counters start at 0.  Two
 * words with the same canonical form (a word and its own reverse complement too) are GT4HIP_EINVAL -- the message names
 * both indices -- found by the kernel that packs the sorted words; nothing is made then.  Free the db before its context. */
int gt4hip_gmer_db_create (gt4hip_context *ctx, const uint64_t *host_words, uint64_t n_kmers, uint32_t word_length, gt4hip_gmer_db **db);
void gt4hip_gmer_db_free (gt4hip_gmer_db *db);
uint64_t gt4hip_gmer_db_n_kmers (const gt4hip_gmer_db *db);
/* One probe of the bucket index per word, the words looked up as they stand (canonical already, as the reader leaves them);
 * a hit is one 64-bit atomic add on its k-mer's counter.  *n_hits (may be NULL): words found; *kmer_gc (may be NULL): the
 * sum over the hits of (w ^ w >> 1) & 1 -- what the reference's n_kmer_gc gains per hit, divided by the word length
 * (src/gmer_counter.c:799-803 reloads the word inside its loop).  Both are reduced per wavefront, one atomic each per
 * wavefront and launch.  `flags`: GT4HIP_GMER_ON_DEVICE, GT4HIP_GMER_PLAIN_ATOMICS. */
int gt4hip_gmer_count_words (gt4hip_context *ctx, gt4hip_gmer_db *db, const uint64_t *words, uint64_t n_words, unsigned flags,
                             uint64_t *n_hits, uint64_t *kmer_gc);
/* Device time (HIP events) of the counting kernel of the last gt4hip_gmer_count_words / _count_text on this db. */
double gt4hip_gmer_db_last_ms (const gt4hip_gmer_db *db);

/* what a piece of text gave (gmer_counter --stats, src/gmer_counter.c:412-419, :767-804) */
typedef struct {
  uint64_t n_n;        /* 'N' / 'n' among the bytes the reader's loop takes: every byte in front of a NUL but FastQ '+' lines  */
  uint64_t n_nucl;     /* bases of sequence lines (the reader's codes 0..3)                                                    */
  uint64_t n_gc;       /* ... that are C or G                                                                                  */
  uint64_t n_words;    /* words read                                                                                           */
  uint64_t n_hits;     /* ... found in the database                                                                            */
  uint64_t n_kmer_gc;  /* word length x the kmer_gc of gt4hip_gmer_count_words: the reference's n_kmer_gc                      */
} gt4hip_gmer_stats;

/* gt4hip_text_to_words on a piece of a file, then the counting kernel on its words, which never leave the device.  The carry
 * and the errors of the text are gt4hip_text_to_words's.  `stats` (may be NULL) is SET to what this piece gave; its first
 * three fields cost one more streaming pass over the piece's bytes and codes, with the reader's own classification: pieces
 * cut anywhere add up to what the whole text gives.  `flags`: GT4HIP_GMER_ON_DEVICE (16-byte aligned), GT4HIP_GMER_PLAIN_ATOMICS. */
int gt4hip_gmer_count_text (gt4hip_context *ctx, gt4hip_gmer_db *db, const void *text, size_t n_bytes, unsigned flags,
                            const gt4hip_maker_carry *carry_in, gt4hip_maker_carry *carry_out, gt4hip_gmer_stats *stats,
                            uint64_t *error_offset);
/* Counters [first, first + n) -> host memory; all counters back to 0. */
int gt4hip_gmer_counts_download (gt4hip_context *ctx, const gt4hip_gmer_db *db, uint64_t first, uint64_t n, uint64_t *host_counts);
int gt4hip_gmer_counts_reset (gt4hip_context *ctx, gt4hip_gmer_db *db);

/* ---------------------------------------------------------------- gmer_caller: genotype likelihoods of k-mer count pairs */

/* The model of genotype_probabilities (reference src/genotypes.c:9-124), as gmer_caller holds it: seven `float`
 * parameters and the B allele frequency.  They are promoted to double where C promotes them in the reference. */
typedef struct {
  float l_viga;  /* mean count of a k-mer that is not in the genome (errors)   */
  float p_0, p_1, p_2;  /* probability of 0, 1, 2 copies                        */
  float lambda;  /* mean count of a k-mer of two copies (the coverage)          */
  float size, size2;  /* negative-binomial size = size + size2 x mean           */
  float pB;      /* frequency of the B allele                                   */
} gt4hip_caller_model;
#define GT4HIP_CALLER_GENOTYPES 15u  /* -, A, B, AA, AB, BB, AAA, AAB, BBA, BBB, AAAA, AAAB, BBBA, AABB, BBBB */

/* The markers of a run resident in HBM: n pairs (a_counts[i], b_counts[i]), uploaded once; every call below reads them
 * there.  Free the set before its context. */
typedef struct gt4hip_caller_set gt4hip_caller_set;
int gt4hip_caller_set_create (gt4hip_context *ctx, const uint32_t *a_counts, const uint32_t *b_counts, uint64_t n, gt4hip_caller_set **set);
void gt4hip_caller_set_free (gt4hip_caller_set *set);
uint64_t gt4hip_caller_set_n (const gt4hip_caller_set *set);
/* Device time (HIP events) of the kernel of the last gt4hip_caller_mlogl / of the kernels of the last
 * gt4hip_caller_probabilities on this set, copies excluded. */
double gt4hip_caller_set_last_ms (const gt4hip_caller_set *set);

/* mlogL3 (src/gmer_caller.c:821-843) over markers [first, first + n): *sum = -(sum over the markers of
 * log (max (a[0] + ... + a[14], 1e-30))), a[] the 15 likelihoods of the marker under `m`.  What depends on the model alone
 * (the 15 priors, and per mean the size, p, log p, size x log (1 - p), lgamma (size) and the "size <= 0 or mean <= 0 gives
 * 0" verdict) is computed by the call on the host with libm; per marker the device computes ten negative-binomial terms
 * and the 15 products q0 * q1 * p[j].  One launch and one read-back of 8 bytes.  The sum is reproducible bit for bit: the
 * grid depends on n alone, a thread adds its markers in ascending order, a workgroup adds its threads by a fixed tree, and
 * the workgroup that finishes last adds the workgroups' sums in index order by the same tree; no floating-point atomics.
 * n = 0 gives -0.0, as the reference's loop does. */
int gt4hip_caller_mlogl (gt4hip_context *ctx, gt4hip_caller_set *set, uint64_t first, uint64_t n, const gt4hip_caller_model *m, double *sum);

/* calc_run (src/gmer_caller.c:365-388) over markers [first, first + n), into HOST arrays of n entries: best[i] = the index
 * of the largest likelihood (the first of equals: a strict > scan from 0, so 0 where all are NaN), a_best[i] that
 * likelihood, a_sum[i] = a[0] + ... + a[14] in that order, and where a_all is not NULL a_all[15 i + j] = a[j].  Large n
 * goes through the device in pieces sized to what the context's pool gives. */
int gt4hip_caller_probabilities (gt4hip_context *ctx, gt4hip_caller_set *set, uint64_t first, uint64_t n, const gt4hip_caller_model *m,
                                 uint8_t *best, double *a_best, double *a_sum, double *a_all);

/* ---------------------------------------------------------------- synthetic lists (bench) */

/* Fills `list` (capacity >= n) with n strictly ascending keys < 4^word_length and counts in
 * [1, max_count]: record i gets key i*stride + (hash(seed,i) mod stride) with
 * stride = floor(keyspace / n); counts from hash(seed+1,i).  Same (seed, n, word_length) =>
 * same list on every device (tests regenerate it on the CPU). */
int gt4hip_generate (gt4hip_context *ctx, gt4hip_list *list, uint64_t n, uint64_t seed, uint32_t max_count);
/* General form: key_i = (i*stride + hash(key_seed,i) mod stride) * mult + add with
 * stride = floor(keyspace / mult / n) and add < mult, counts from hash(count_seed,i).  Lists made
 * with different `add` under one `mult` are disjoint; lists sharing key_seed share keys.  The
 * bench builds A = S u PA, B = S' u PB from three disjoint residue classes this way, which fixes
 * |A n B| = |S| exactly.  gt4hip_generate is (seed, seed+1, mult 1, add 0). */
int gt4hip_generate_ex (gt4hip_context *ctx, gt4hip_list *list, uint64_t n, uint64_t key_seed, uint64_t count_seed,
                        uint32_t max_count, uint64_t mult, uint64_t add);

/* Blocks until everything enqueued on the context's stream has finished. */
int gt4hip_synchronize (gt4hip_context *ctx);

/* Tuning / debugging knobs (not part of the reference surface):
 *   "two_pass" = 1     count + scan + write instead of the single-pass kernel
 *   "pool" = 0         release freed list storage to the driver instead of pooling it
 *   "pool_cap_mb" = n  most the pool may hold (default: half of the device memory); every device
 *                      allocation that fails gives the pooled blocks back and retries
 *   "grid" = n         workgroups of the merge kernels, pair and N-way, in every launch of a call, pass 2 of the two-pass
 *                      path included (0: one per resident slot).  A launch never gets more than it has tiles (and a
 *                      scanner), and a single-pass launch that writes records never fewer than two: its first workgroup
 *                      to arrive is the scanner, so n = 1 runs one worker there as n = 2 does
 *   "kway" = 0 / 1 / 2 / 3  N-way unions of three and more lists by the pairwise tree of the pair kernel / by
 *                      the one-pass tile kernel (gt4hip_nway.hip) unless a probe of the keys or the tiles' own
 *                      samples show them clustered -- stretches of adjacent keys between wide gaps, which the
 *                      tile kernel orders two to three times slower: the tree is faster then (the default;
 *                      counter "kway_declined") / always by the tile kernel, two-list unions of the N-way
 *                      entry points too / always by the tile kernel (three lists and more); count tables
 *                      follow the same switch (and are never declined).
 *                      "kway_g": samples per tile of its first partition attempt; "kway_vt" (tests):
 *                      97 tile boundaries by searches over whole brackets, 98 every tile bucketed by
 *                      its pivot run, 99 every tile on the search path
 *   "spin_limit" = n   bound of the single-pass kernel's inter-workgroup waits (0: default, ~seconds)
 *   "dynamic" = 1 / -1 tiles of the single-pass kernel always / never dealt by a ticket counter
 *                      (0: automatic -- the record-writing kernels except a complement alone)
 *   "scan_group" = 1 / -1  the scanner as a group of wavefronts always / never (0: by launch size)
 *   "a_rows" = 0 / -1  single-pass intersection and first complement: a tile whose first-list records fit half
 *                      of the workgroup's position rows is ranked by the body compiled for those rows alone /
 *                      every tile by the general body (experiments, tests)
 *   "part_guided" = 0 / -1  the pair partition's co-rank searches place their first probes from the coarse
 *                      neighbours' ranks and the probed keys (gt4hip_corank.h: fewer scattered reads on keys that
 *                      are locally uniform, never more than bisection's and four) / plain bisection; the tile
 *                      ranges are the same either way
 *   "select_vec" = 0 / -1  gt4hip_table_select reads rows of a multiple of four counts (in 16-byte aligned arrays) 16 bytes
 *                      per lane / every row a dword per lane, as all other rows are read (bench, tests)
 *   "grid_cap" = n     (tests) every kernel that walks its work in a loop stepping by its grid -- items, tiles or segments:
 *                      the query, per-sequence profile, mismatch, maker, gmer, subset, select, pairwise and caller kernels, the radix sort's
 *                      histogram, the list utilities -- is launched with n workgroups at most, so that small inputs take the
 *                      second and later trips of those loops; 0 (default): the built-in caps alone.  Results do not change.
 *                      Not followed by kernels launched one workgroup per tile or whose workgroups wait for one another
 *                      (the merge and N-way kernels keep "grid"; radix scatter, fold, index and partition kernels), nor
 *                      by gt4hip_caller_mlogl, whose grid is a function of the number of markers alone
 *   "poison" = 1       (tests) every device block the library hands out, new or from its pool, is filled with 0xA5 bytes
 *                      first: a block from the pool holds what an earlier call left there, often the very results the
 *                      next call is to compute, and an item a kernel skips would keep them
 *   "caller_piece" = n (tests) markers per piece of gt4hip_caller_probabilities (0: 2^22, with all 15 likelihoods 2^20)
 *   "geom0" / "geom1"  force the 512- / 1024-thread geometry (experiments). */
int gt4hip_set_option (gt4hip_context *ctx, const char *name, int64_t value);
/* Diagnostic counters of a context.  "single_pass_fallbacks": calls whose single-pass merge gave up a
 * bounded wait (a worker not resident: shared device) and were rerun on the two-pass path;
 * "partition_us": the partition launch of the context's last pair merge (HIP events around it; it also zeroes the merge's workspace);
 * "kway_declined": N-way unions handed to the pairwise tree because their keys are clustered;
 * "kway_calls" / "kway_overflows": N-way unions (and count tables) done by the one-pass tile kernel /
 * partitions repeated with fewer samples per tile because a tile would not have fit LDS;
 * "nway_kernel_us", "nway_tiles": the last N-way call's tile kernel (its last launch); "nway_sample_tiles": the most tiles
 * among that call's launches over sample levels, 0 if it had none; "nway_one_pass": 1 when the last
 * gt4hip_union_multi took the one-pass tile kernel, 0 when it took the pairwise tree; "sort_us", "fold_us", "table_us":
 * the last gt4hip_device_words_to_list / gt4hip_union_table call; "extract_us": the kernels of the last gt4hip_text_to_words
 * that gave words (HIP events around the kernels alone: the call's read-back of its totals and the allocation of the
 * words lie between two spans and are not in it; a kernel trace sums the same kernels); "maker_text_tile",
 * "maker_code_tile": bytes of text, and codes (one per text byte >= ' '), per tile of that call's kernels;
 * "query_wide": 1 when the context's last gt4hip_query_lookup ran the kernel with 64-bit variant ranks, else 0;
 * "mm_wide_levels": levels of the last gt4hip_compare_mismatch, both tables added, run with 64-bit variant ranks;
 * "mm_unskipped_levels": levels of it run without the early exit of decided words (more than 2^32 - 1 variants a word, no subtract);
 * "subset_passes": passes of the last gt4hip_list_subset until a scan changed no tile's carry-in (0: it had nothing to walk);
 * "subset_tile": items per tile of its kernels; "subset_us": its device time (HIP events around the kernels, the one
 * word read back per pass included); "mask_ends_us", "mask_apply_us": the two spans of the last gt4hip_query_mask_text (HIP
 * events: the lookups with k_mask_ends, and k_mask_apply); "select_wide": 1 when the context's last gt4hip_table_select (gt4hip_select_multi's too)
 * read 16 bytes per lane, else 0; "grid_capped": launches of the context, since it was made, of a kernel that strides over its
 * work with fewer workgroups than blocks of work (by option "grid_cap" or by a built-in cap): the loops of those took a second
 * trip.  Sizes the tests build their inputs from: "mm_threads": items per block of work of the item loops of the query,
 * mismatch and gmer kernels (a quarter of the records per block of the list statistics); "mm_tile": items per tile of the
 * hit and compaction passes; "profile_tile": words per tile of gt4hip_query_profile_words' kernel (its sums are zeroed in blocks of
 * "mm_threads" words, three per sequence and one more); "gather_tile": locations per tile of gt4hip_query_lookup_locations' gather; "hist_lds_bins": the
 * most bins gt4hip_list_count_histogram keeps in LDS; "list_threads": records per block of gt4hip_generate, _list_sum_counts,
 * _list_is_sorted, _list_upload_index and the count table's column kernels; "sort_hist_chunk": words per block of the
 * radix sort's histogram; "select_segment": rows per segment of a contiguous count table; "subset_scan_tile": elements per tile of
 * gt4hip_list_subset's scans; "pack_threads": locations per block of gt4hip_pack_locations; "caller_threads": markers per
 * block of the caller kernels; "caller_max_grid": workgroups of gt4hip_caller_mlogl at most. */
int gt4hip_get_counter (gt4hip_context *ctx, const char *name, uint64_t *value);
/* Diagnostic: the partition launch of a pair merge alone, with tiles of tile_records merged records (any length: tests cut
 * small lists into many tiles).  host_part receives 2 x (tiles + 1) words, tiles = ceil ((|a| + |b|) / tile_records):
 * boundary t = {records of a, records of b} before tile t, first list first on equal keys, the second list's record of a
 * pair that the diagonal cuts pulled into the earlier tile.  Follows option "part_guided". */
int gt4hip_pair_partition (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, uint64_t tile_records, uint64_t *host_part);

#ifdef __cplusplus
}
#endif
#endif
