/*
 * gt4_glistquery_cli.c -- `glistquery`, the drop-in command line for looking words up in a list and for
 * the list statistics.  Host C; every lookup and every pass over a list's counts runs in the HIP kernels
 * behind include/gt4hip.h (gt4hip_query.hip), the multi-list forms in those behind
 * include/gt4_set_operations.h.
 *
 * Same argv grammar, defaults, validation order, messages, stdout and exit codes as the reference's
 * main() (reference src/glistquery.c:108-437; search_one_word :543-568, search_n_query_strings :609-662,
 * print_median :831-889, print_distro :891-909, print_gc :911-932; the FastA / FastQ state machine of
 * src/fasta.c:87-300 for plain text).  Query words are collected on the host in batches of QUERY_BATCH,
 * looked up in one call per batch and printed in input order.
 * Deliberate differences, all loud:
 *   - gzip-compressed sequence files (-s) are refused: error + exit 1;
 *   - --locations with a plain .list on the command line is refused: error + exit 1, no device opened (the reference
 *     ignores the option there).  --files and --sequences on anything but one index are the reference's own errors,
 *     with a second line that names the option.  Without --locations a GT4I index is read as the sorted k-mer list it
 *     contains, as glistcompare here does;
 *   - --sequences reads the names out of the source files on the host, as the reference does; a source that cannot be
 *     mapped gives the reference's message and an EMPTY name (the reference prints an uninitialised buffer), and a name
 *     is cut at the end of its source file (the reference reads past it);
 *   - -l X.index is refused as the reference refuses it (it streams the query list, which takes a .list only:
 *     "invalid or corrupted", exit 1); earlier versions of this program read the index as the list it holds;
 *   - an index whose sections do not fit its file, or whose k-mer section points outside its location section, is
 *     refused (gt4_indexfile_open, gt4hip_location_index_create): error + exit 1;
 *   - --bloom and --disable_scouts are accepted and ignored;
 *   - --distribution skips a record whose count is 0 (the reference writes before its array there);
 *   - more than 1024 lists are an error (the reference overruns its array);
 *   - -D prints "List ... loaded" and print_median's trace lines, nothing else is promised;
 *   - --stat reads headers only and -v / -h nothing at all: they work without a GPU.  The dump of ONE
 *     list (no query option) is file I/O: it prints the mapped records and opens no device either, with --locations
 *     too; so are --files and --sequences.
 *     Everything else fails without a usable GPU: there is no CPU path;
 *   - the list must fit one device (as for glistcompare -mm); larger is an out-of-memory error;
 *   - --words-only (not in the reference) prints the packed query words -q / -f / -s / -l would look up,
 *     one decimal number per line, and opens no device: for tests of the parsers;
 *   - -s FILE --per_sequence [--min_hits H] (not in the reference) prints one line per sequence of FILE, in file order:
 *     NAME, the number of its words, the number of those that hit, and the sum of the hits' values (64 bits), tab-separated.
 *     A word's value is what -s looks up for it under the same -mm / -p; it is a hit when max (-min, 1) <= value <= -max:
 *     the lines the reference prints for that sequence alone with `-min max (A, 1) -max B`.  NAME runs from behind the tag to
 *     the first byte <= ' '.  --min_hits H keeps the sequences with at least H hits.  The file is mapped and goes through the
 *     device in pieces of GT4HIP_QUERY_CHUNK=<bytes>[K|M|G] (default: 1/64 of the free device memory, 1 MiB to 1 GiB), cut
 *     anywhere: the reader, the lookups and the sums per sequence run there (gt4hip_query_profile_text) and a sequence is
 *     printed when the next one begins.  After a reader error the sequences read so far are printed with the words in
 *     front of the error, as -s prints those words, then the reader's message; the exit status is -s's.  Refused with one
 *     "Error:" line and exit 1 in front of any device: --per_sequence without -s, with another query or a statistics
 *     option, with --all or --locations, with more than one list; --min_hits without --per_sequence.  -h stays the
 *     reference's usage screen byte for byte (it is a golden transcript): these two options are described here and in README.md.
 *   - -s FILE --mask [--soft_mask] (not in the reference; its authors' stub is src/gmasker.c) writes FILE to stdout byte for byte,
 *     except that every base that lies inside a word of the list is written as N, with --soft_mask as its lower-case letter
 *     (U becomes u, a lower-case base stays).  The words are -s's, a word counts when max (-min, 1) <= value <= -max under the
 *     same -mm / -p (--per_sequence's rule), and a base is covered when it is one of the k bases of such a word.  Names, '+' and
 *     quality lines, '\r', control and high bytes and runs shorter than k stay as they are; so does everything from a NUL
 *     on.  The file goes through the device in pieces of GT4HIP_QUERY_CHUNK as for --per_sequence (gt4hip_query_mask_text);
 *     the output is a stream, so the tail a later piece may still cover -- from the (k - 1)-th last byte >= ' ' on -- is held
 *     back (GT4MaskTail, gt4_cli.c) and the result does not depend on where the cuts fall.  After a reader error stdout holds the
 *     masked bytes in front of the offending byte, then comes the reader's message and -s's exit status.  Refused with one
 *     "Error:" line and exit 1 in front of any device: --mask without -s, with -q / -f / -l, --all, --locations, --files,
 *     --sequences, --per_sequence, --min_hits or a statistics option, with more than one list, with a gzip file; --soft_mask
 *     without --mask.  Neither option is on the -h screen.
 * With --locations the queries go through gt4hip_query_lookup_locations, batch by batch: every hit is printed as
 * WORD, count, REVERSE and one line per location (search_one_word / cb_print / print_index_info, :469-476, :528-568).
 * REVERSE is the reference's sticky flag: set by the first query whose reverse complement is the smaller word and never
 * cleared, so every later query of the run prints 1 and flipped strands; the host carries it across batches in input
 * order.  On the device a lookup takes 16 bytes per location and 56 per hit (the 40-byte record and two 8-byte offsets):
 * a batch may hold at most B = A QUARTER OF THE FREE DEVICE MEMORY / 72 locations and as many hits (gt4hip_device_memory,
 * read once behind the upload of the index; never fewer than 2^16 each), which is a quarter of that memory at worst.  A
 * batch with more of either, or one the library still answers with out-of-memory, is cut in two halves that are looked
 * up one after the other (and those again); a single query over the budget is an out-of-memory error.
 * Argv is read in parse_argv() alone.  One environment variable is read here, for tests only:
 * GT4_GLISTQUERY_LOCATION_BUDGET = the most locations a batch may hold, in place of B (the hits keep theirs).  GT4HIP_DEVICE
 * picks the device of the library's default context, GT4HIP_HBM_LIMIT and GT4HIP_VERBOSE act inside the multi-list
 * calls (gt4_setops.c).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "gt4_cli.h"
#include "gt4_listfile.h"
#include "gt4_set_operations.h"
#include "gt4hip.h"

#define MAX_LISTS 1024
#define QUERY_BATCH (1u << 20)
/* device bytes of a location lookup per location (the 16-byte record) plus per hit (the 40-byte hit, its two 8-byte offsets) */
#define LOOKUP_BYTES (sizeof (gt4hip_location) + sizeof (gt4hip_query_hit) + 16)

enum { CMD_QUERY, CMD_STATS, CMD_GC, CMD_MEDIAN, CMD_DISTRO, CMD_FILES, CMD_SEQUENCES };

enum { OPT_VERSION, OPT_HELP, OPT_SEQFILE, OPT_LISTFILE, OPT_QUERYFILE, OPT_QUERY, OPT_PM, OPT_MM, OPT_MIN, OPT_MAX, OPT_DEBUG, OPT_ALL,
       OPT_STATS, OPT_MEDIAN, OPT_DISTRO, OPT_GC, OPT_FILES, OPT_SEQUENCES, OPT_LOCATIONS, OPT_3P, OPT_5P, OPT_HEADER, OPT_BLOOM,
       OPT_IS_UNION, OPT_NOSCOUTS, OPT_WORDS_ONLY, OPT_PER_SEQUENCE, OPT_MIN_HITS, OPT_MASK, OPT_SOFT_MASK };

static const GT4CliOption OPTIONS[] = {
  { "-v", OPT_VERSION }, { "--version", OPT_VERSION }, { "-h", OPT_HELP }, { "--help", OPT_HELP }, { "-?", OPT_HELP },
  { "-s", OPT_SEQFILE }, { "--seqfile", OPT_SEQFILE }, { "-l", OPT_LISTFILE }, { "--listfile", OPT_LISTFILE },
  { "-f", OPT_QUERYFILE }, { "--queryfile", OPT_QUERYFILE }, { "-q", OPT_QUERY }, { "--query", OPT_QUERY },
  { "-p", OPT_PM }, { "--perfectmatch", OPT_PM }, { "-mm", OPT_MM }, { "--mismatch", OPT_MM },
  { "-min", OPT_MIN }, { "--minfreq", OPT_MIN }, { "-max", OPT_MAX }, { "--maxfreq", OPT_MAX }, { "-D", OPT_DEBUG },
  { "--all", OPT_ALL }, { "-all", OPT_ALL }, { "--stats", OPT_STATS }, { "--stat", OPT_STATS }, { "-stat", OPT_STATS },
  { "--median", OPT_MEDIAN }, { "-median", OPT_MEDIAN }, { "--distribution", OPT_DISTRO }, { "-distribution", OPT_DISTRO },
  { "-gc", OPT_GC }, { "--gc", OPT_GC }, { "--files", OPT_FILES }, { "--sequences", OPT_SEQUENCES }, { "--locations", OPT_LOCATIONS },
  { "--3p", OPT_3P }, { "--5p", OPT_5P }, { "--header", OPT_HEADER }, { "--bloom", OPT_BLOOM }, { "--is_union", OPT_IS_UNION },
  { "--disable_scouts", OPT_NOSCOUTS },
  { "--words-only", OPT_WORDS_ONLY }, /* not in the reference: print the parsed query words, no device */
  { "--per_sequence", OPT_PER_SEQUENCE }, { "--min_hits", OPT_MIN_HITS }, /* not in the reference: -s, summed per sequence */
  { "--mask", OPT_MASK }, { "--soft_mask", OPT_SOFT_MASK },               /* not in the reference: -s, the covered bases masked */
};

static const char *const HELP_LINES[] = {
  "Usage: glistquery INPUT_LIST [OPTIONS]",
  "Options:",
  "    -v, --version             - print version information and exit",
  "    -h, --help                - print this usage screen and exit",
  "    -stat, --stats            - print statistics of the list file and exit",
  "    --median                  - print min/max/median/average and exit",
  "    --distribution MAX        - print distribution up to MAX",
  "    --gc                      - print average GC content of all words",
  "    -q, --query               - single query word",
  "    -f, --queryfile           - list of query words in a file",
  "    -s, --seqfile             - FastA/FastQ file",
  "    -l, --listfile            - list file made by glistmaker",
  "    -mm, --mismatch NUMBER    - specify number of mismatches (0-16; default 0)",
  "    -p, --perfectmatch NUMBER - specify number of 3' perfect matches (0-32; default 0)",
  "    -min, --minfreq NUMBER    - minimum frequency of the printed words (default 0)",
  "    -max, --maxfreq NUMBER    - maximum frequency of the printed words (default MAX_UINT)",
  "    --files                   - Print indexed files",
  "    --sequences               - Print indexed subsequences",
  "    --bloom                   - use bloom filter to speed up lookups",
  "    --all                     - in case of mismatches prints all found words",
  "    --locations               - in case of index print all word locations",
  "    --3p                      - if query is longer than word use 3' end",
  "    --5p                      - if query is longer than word use 5' end",
  "    -D                        - increase debug level",
};

/* What argv decides.  parse_argv fills it, validate and open_inputs check it; the jobs only read it. */
typedef struct {
  const char *lists[MAX_LISTS];
  unsigned int n_lists;
  const char *querystring, *queryfilename, *seqfilename, *querylistfilename;
  unsigned int nmm, pm3, minfreq, maxfreq, distro, command;
  int printall, print_header, locations, is_union, use_3p, use_5p, words_only, debug;
  int per_sequence, have_min_hits; /* --per_sequence, --min_hits H */
  int mask, soft_mask;             /* --mask, --soft_mask */
  uint64_t min_hits;
} Options;

static void print_help (int exit_value)
{
  gt4_cli_print_help (stderr, "glistquery", HELP_LINES, sizeof HELP_LINES / sizeof HELP_LINES[0]);
  exit (exit_value);
}

/* ------------------------------------------------------------------ words */

/* get_nucl_value, src/sequence.c:43-52: any character maps to two bits */
static uint64_t nucl_value (char nucl)
{
  if (nucl & 4) return (uint64_t) (((nucl >> 4) | 2) & 3);
  return (uint64_t) ((nucl & 6) >> 1);
}

/* string_to_word, src/sequence.c:116-130 */
static uint64_t string_to_word (const char *s, unsigned int wordlength)
{
  const unsigned int l = wordlength < 32 ? wordlength : 32;
  uint64_t word = 0;
  for (unsigned int i = 0; i < l; i++) {
    if (strchr ("ACGTUacgtu", s[i]) == NULL) fprintf (stderr, "Invalid character %c in string!\n", s[i]);
    word = (word << 2) | nucl_value (s[i]);
  }
  return word;
}

static uint64_t reverse_complement (uint64_t w, unsigned int k)
{
  uint64_t r = 0;
  w = ~w;
  for (unsigned int i = 0; i < k; i++) {
    r = (r << 2) | (w & 3);
    w >>= 2;
  }
  return r;
}

static uint64_t canonical_word (uint64_t w, unsigned int k)
{
  const uint64_t r = reverse_complement (w, k);
  return r < w ? r : w;
}

/* ------------------------------------------------------------------ the lists on the command line */

typedef struct {
  const char *name;
  int is_index;
  GT4ListFile file;
  uint32_t version_major, version_minor;
} Input;

static uint64_t input_word (const Input *in, uint64_t i)
{
  uint64_t w;
  memcpy (&w, in->is_index ? in->file.index_kmers + 16 * i : in->file.records + 12 * i, 8);
  return w;
}

static uint32_t input_count (const Input *in, uint64_t i)
{
  if (!in->is_index) {
    uint32_t c;
    memcpy (&c, in->file.records + 12 * i + 8, 4);
    return c;
  }
  uint64_t here, next = in->file.index_locations;
  memcpy (&here, in->file.index_kmers + 16 * i + 8, 8);
  if (i + 1 < in->file.header.n_words) memcpy (&next, in->file.index_kmers + 16 * (i + 1) + 8, 8);
  return (uint32_t) (next - here);
}

/* 0: mapped; 1: the reference's "invalid" state */
static int input_open (Input *in, const char *name, uint32_t code)
{
  memset (in, 0, sizeof *in);
  in->name = name;
  in->is_index = code == GT4_INDEX_CODE_VALUE;
  if (in->is_index ? gt4_indexfile_open (name, GT4_VERSION_MAJOR, &in->file) : gt4_listfile_open (name, GT4_VERSION_MAJOR, &in->file)) return 1;
  in->version_major = in->file.header.version_major;
  in->version_minor = in->file.header.version_minor;
  if (in->is_index && in->file.file_size >= 12) {
    memcpy (&in->version_major, in->file.file_map + 4, 4);
    memcpy (&in->version_minor, in->file.file_map + 8, 4);
  }
  return 0;
}

static void print_list_header (const Input *in)
{
  fprintf (stdout, "%s %s: built with glistmaker version %d.%d\n", in->is_index ? "Index" : "List", in->name, (int) in->version_major, (int) in->version_minor);
  fprintf (stdout, "Wordlength\t%u\n", in->file.header.word_length);
  fprintf (stdout, "NUnique\t%llu\n", (unsigned long long) in->file.header.n_words);
  fprintf (stdout, "NTotal\t%llu\n", (unsigned long long) in->file.header.total_count);
}

/* p, or exit 1 after "Error: out of memory (<what>)"; the compiler checks `what` against its arguments */
__attribute__ ((format (printf, 2, 3))) static void *or_oom (void *p, const char *what, ...)
{
  if (p) return p;
  va_list ap;
  va_start (ap, what);
  fprintf (stderr, "Error: out of memory (");
  vfprintf (stderr, what, ap);
  fprintf (stderr, ")\n");
  exit (1);
}

/* the list in device memory, or exit 1; `ctx` and `dev` may be NULL where the caller needs the object alone */
static GT4HipWordList *to_device (const char *name, gt4hip_context **ctx, const gt4hip_list **dev)
{
  gt4hip_context *c = gt4_hip_default_context ();
  if (!c) exit (1);
  if (ctx) *ctx = c;
  GT4HipWordList *l = gt4_hip_word_list_new (name, GT4_VERSION_MAJOR);
  if (!l) {
    fprintf (stderr, "Error: %s could not be loaded into device memory\n", name);
    exit (1);
  }
  if (dev) {
    *dev = gt4_hip_word_list_device (l);
    if (!*dev) {
      fprintf (stderr, "Error: %s does not fit the device memory (out of memory)\n", name);
      exit (1);
    }
  }
  return l;
}

/* ------------------------------------------------------------------ statistics */

static void print_median (const Input *in, gt4hip_context *ctx, const gt4hip_list *dev, int debug)
{
  const uint64_t num_words = in->file.header.n_words;
  uint32_t min, max, med, gmin, gmax;
  if (debug > 0) fprintf (stderr, "Finding min/max...");
  CHK (ctx, gt4hip_list_count_stats (ctx, dev, &gmin, &gmax));
  if (debug > 0) fprintf (stderr, "done (%u %u)\n", gmin, gmax);
  min = gmin;
  max = gmax;
  med = (uint32_t) (((uint64_t) min + max) / 2);
  /* the reference's bisection, step for step (it does not always end on the true median) */
  while (max > min) {
    uint64_t above = 0, below = 0, equal;
    CHK (ctx, gt4hip_list_count_split (ctx, dev, med, &below, &above));
    equal = num_words - above - below;
    if (debug > 0) fprintf (stderr, "Trying median %u - equal %llu, below %llu, above %llu\n", med, (unsigned long long) equal, (unsigned long long) below,
                            (unsigned long long) above);
    if (max == min + 1) {
      if (above > below + equal) med = max;
      break;
    }
    if (above > below) {
      if (above - below < equal) break;
      min = med;
    } else if (below > above) {
      if (below - above < equal) break;
      max = med;
    } else {
      break;
    }
    med = (min + max) / 2; /* 32-bit, as the reference */
  }
  print_list_header (in);
  fprintf (stdout, "Min %u Max %u Median %u Average %.2f\n", gmin, gmax, med, (double) in->file.header.total_count / num_words);
}

static void print_distro (gt4hip_context *ctx, const gt4hip_list *dev, unsigned int max)
{
  uint64_t *d = (uint64_t *) or_oom (calloc (max ? max : 1, 8), "distribution of %u", max);
  CHK (ctx, gt4hip_list_count_histogram (ctx, dev, max, d));
  for (unsigned int i = 0; i < max; i++) fprintf (stdout, "%u\t%llu\n", i + 1, (unsigned long long) d[i]);
  free (d);
}

static void print_gc (const Input *in, gt4hip_context *ctx, const gt4hip_list *dev)
{
  uint64_t count = 0;
  CHK (ctx, gt4hip_list_gc (ctx, dev, &count));
  printf ("GC\t%g\n", (double) count / (in->file.header.total_count * in->file.header.word_length));
}

/* ------------------------------------------------------------------ multi-list forms (include/gt4_set_operations.h) */

/* the callbacks' `data`: word length and number of lists; multi_cb's open line (one per word, "\t<list>:<count>" per list) and its word */
typedef struct { unsigned int wlen, n_lists; int open; uint64_t last; } PrintState;

static unsigned int dump_cb (uint64_t word, uint32_t *counts, void *data)
{
  const PrintState *st = (const PrintState *) data;
  char b[64];
  gt4_word2string (b, word, st->wlen);
  fputs (b, stdout);
  for (unsigned int j = 0; j < st->n_lists; j++) fprintf (stdout, "\t%u", counts[j]);
  fputc ('\n', stdout);
  return 0;
}

static unsigned int multi_cb (uint64_t word, unsigned int list, uint32_t count, void *data)
{
  PrintState *st = (PrintState *) data;
  if (!st->open || word != st->last) {
    char b[64];
    if (st->open) fputc ('\n', stdout);
    gt4_word2string (b, word, st->wlen);
    fputs (b, stdout);
    st->open = 1;
    st->last = word;
  }
  fprintf (stdout, "\t%u:%u", list, count);
  return 0;
}

static unsigned int zipper_cb (uint64_t word, uint32_t count, void *data)
{
  char b[64];
  gt4_word2string (b, word, ((const PrintState *) data)->wlen);
  fprintf (stdout, "%s\t%u\n", b, count);
  return 0;
}

/* ------------------------------------------------------------------ batched lookups */

typedef struct {
  gt4hip_context *ctx;
  gt4hip_query_index *qindex;
  gt4hip_query_params prm;
  const Options *o; /* min / max frequency, --all, --3p, --5p, --words-only */
  unsigned int k;
  uint64_t *words; /* canonical query words of the batch */
  uint64_t n;
  uint32_t *values;
  uint8_t *found;
  gt4hip_query_hit *hits;
  uint64_t hit_capacity;
  /* --locations */
  const gt4hip_location_index *lindex;
  gt4hip_location *locs;
  uint64_t loc_capacity, loc_budget, hit_budget; /* the most locations, and hits, a batch may hold */
  uint8_t *reverse;       /* per query of the batch: the sticky flag as it stood behind that query */
  uint32_t *query_counts; /* the zipper (-l without mismatches): the QUERY list's count of every word */
  int sticky, zipper;
} Searcher;

/* The place of a variant in the pre-order of gt4_word_table_generate_mismatches (src/word-table.c:360-382): the
 * substitutions (position i ascending, XOR value m) as bytes 4 i + m, compared as strings: a prefix sorts before
 * its extensions. */
typedef struct {
  unsigned char key[36];
  const gt4hip_query_hit *hit;
  uint64_t first_location; /* --locations: of the hit, in the batch's locations */
} OrderedHit;

static int ordered_cmp (const void *a, const void *b) { return strcmp ((const char *) ((const OrderedHit *) a)->key, (const char *) ((const OrderedHit *) b)->key); }

/* print_index_info, :469-477 */
static void print_locations (const gt4hip_location *l, uint64_t n, unsigned int reverse)
{
  for (uint64_t i = 0; i < n; i++)
    fprintf (stdout, "%u\t%u\t%llu\t%u\n", l[i].file, l[i].seq, (unsigned long long) (l[i].pos_dir >> 1), (unsigned int) (l[i].pos_dir & 1) ^ reverse);
}

static void print_hits (Searcher *s, uint64_t first, uint64_t n, uint64_t n_hits, const gt4hip_location *locs);
static void flush_locations (Searcher *s, uint64_t first, uint64_t n);

static void flush_batch (Searcher *s)
{
  char b[64];
  if (!s->n) return;
  if (s->o->words_only) {
    for (uint64_t i = 0; i < s->n; i++) fprintf (stdout, "%llu\n", (unsigned long long) s->words[i]);
    s->n = 0;
    return;
  }
  if (s->lindex) {
    flush_locations (s, 0, s->n);
    s->n = 0;
    return;
  }
  if (!s->o->printall) {
    CHK (s->ctx, gt4hip_query_lookup (s->ctx, s->qindex, s->words, s->n, &s->prm, s->values, s->found));
    for (uint64_t i = 0; i < s->n; i++) {
      if (s->found[i]) {
        if (s->values[i] < s->o->minfreq || s->values[i] > s->o->maxfreq) continue;
        gt4_word2string (b, s->words[i], s->k);
        fprintf (stdout, "%s\t%u\n", b, s->values[i]);
      } else if (!s->o->minfreq) {
        gt4_word2string (b, s->words[i], s->k);
        fprintf (stdout, "%s\t0\n", b);
      }
    }
    s->n = 0;
    return;
  }
  uint64_t n_hits = 0;
  CHK (s->ctx, gt4hip_query_lookup_all (s->ctx, s->qindex, s->words, s->n, &s->prm, s->hits, s->hit_capacity, &n_hits));
  if (n_hits > s->hit_capacity) {
    free (s->hits);
    s->hit_capacity = n_hits;
    s->hits = (gt4hip_query_hit *) or_oom (malloc ((size_t) n_hits * sizeof (gt4hip_query_hit)), "%llu hits", (unsigned long long) n_hits);
    CHK (s->ctx, gt4hip_query_lookup_all (s->ctx, s->qindex, s->words, s->n, &s->prm, s->hits, s->hit_capacity, &n_hits));
  }
  print_hits (s, 0, s->n, n_hits, NULL);
  s->n = 0;
}

/* The hits of queries [first, first + n) of the batch (hit.query counts from `first`), query by query in the reference's
 * order.  locs == NULL: WORD, count.  Else WORD, count, REVERSE and the locations of the hit, which lie in `locs` hit by hit. */
static void print_hits (Searcher *s, uint64_t first, uint64_t n, uint64_t n_hits, const gt4hip_location *locs)
{
  char b[64];
  OrderedHit *ord = NULL;
  size_t ord_cap = 0;
  uint64_t h = 0, at = 0;
  for (uint64_t i = 0; i < n; i++) {
    uint64_t e = h;
    while (e < n_hits && s->hits[e].query == i) e++;
    const size_t m = (size_t) (e - h);
    if (m > ord_cap) {
      ord_cap = m * 2;
      ord = (OrderedHit *) or_oom (realloc (ord, ord_cap * sizeof *ord), "%llu hits of one query", (unsigned long long) m);
    }
    uint32_t sum = 0;
    for (size_t j = 0; j < m; j++) {
      uint64_t mask = 0;
      CHK (s->ctx, gt4hip_query_variant_mask (s->k, &s->prm, s->hits[h + j].rank, &mask));
      unsigned int len = 0;
      for (unsigned int p = 0; p < s->k; p++) {
        const unsigned int x = (unsigned int) (mask >> (2 * p)) & 3u;
        if (x) ord[j].key[len++] = (unsigned char) (4 * p + x);
      }
      ord[j].key[len] = 0;
      ord[j].hit = &s->hits[h + j];
      ord[j].first_location = at;
      at += s->hits[h + j].count;
      sum += s->hits[h + j].count;
    }
    if (m > 1) qsort (ord, m, sizeof *ord, ordered_cmp);
    for (size_t j = 0; j < m; j++) {
      gt4_word2string (b, ord[j].hit->word, s->k);
      if (!locs) {
        fprintf (stdout, "%s\t%u\n", b, ord[j].hit->count);
        continue;
      }
      const unsigned int rev = s->zipper ? 0 : s->reverse[first + i];
      fprintf (stdout, "%s\t%u\t%u\n", b, s->zipper ? s->query_counts[first + i] : ord[j].hit->count, rev);
      print_locations (locs + ord[j].first_location, ord[j].hit->count, rev);
    }
    /* the reference's return value: with mismatches the summed count, without them "found" */
    const int none = s->prm.n_mm ? sum == 0 : m == 0;
    if (none && !s->o->minfreq && !s->zipper) {
      gt4_word2string (b, s->words[first + i], s->k);
      fprintf (stdout, "%s\t0\n", b);
    }
    h = e;
  }
  free (ord);
}

/* queries [first, first + n) of the batch with their locations; more locations than a batch may hold: by halves */
static void flush_locations (Searcher *s, uint64_t first, uint64_t n)
{
  uint64_t n_hits = 0, n_locs = 0;
  int rc = gt4hip_query_lookup_locations (s->ctx, s->qindex, s->lindex, s->words + first, n, &s->prm, s->hits, s->hit_capacity, &n_hits, s->locs, s->loc_capacity,
                                          &n_locs);
  const int fits = n_locs <= s->loc_budget && n_hits <= s->hit_budget;
  if (rc == GT4HIP_OK && fits && (n_hits > s->hit_capacity || n_locs > s->loc_capacity)) {
    if (n_hits > s->hit_capacity) {
      free (s->hits);
      s->hit_capacity = n_hits;
      s->hits = (gt4hip_query_hit *) or_oom (malloc ((size_t) n_hits * sizeof (gt4hip_query_hit)), "%llu hits", (unsigned long long) n_hits);
    }
    if (n_locs > s->loc_capacity) {
      free (s->locs);
      s->loc_capacity = n_locs;
      s->locs = (gt4hip_location *) or_oom (malloc ((size_t) n_locs * sizeof (gt4hip_location)), "%llu locations", (unsigned long long) n_locs);
    }
    rc = gt4hip_query_lookup_locations (s->ctx, s->qindex, s->lindex, s->words + first, n, &s->prm, s->hits, s->hit_capacity, &n_hits, s->locs, s->loc_capacity,
                                        &n_locs);
  }
  /* over the budget, or the device ran out all the same (the budget is an estimate): by halves */
  if ((rc == GT4HIP_OK && !fits) || rc == GT4HIP_ENOMEM) {
    if (n == 1) {
      char b[64];
      gt4_word2string (b, s->words[first], s->k);
      if (rc == GT4HIP_OK)
        fprintf (stderr, "Error: out of memory: the %llu hits and %llu locations of the query %s alone are more than a batch may hold (%llu and %llu)\n",
                 (unsigned long long) n_hits, (unsigned long long) n_locs, b, (unsigned long long) s->hit_budget, (unsigned long long) s->loc_budget);
      else fprintf (stderr, "Error: out of memory: the query %s alone does not fit the device: %s\n", b, gt4hip_last_error (s->ctx));
      exit (1);
    }
    flush_locations (s, first, n / 2);
    flush_locations (s, first + n / 2, n - n / 2);
    return;
  }
  if (rc != GT4HIP_OK) {
    fprintf (stderr, "Error: gt4hip_query_lookup_locations: %s\n", gt4hip_last_error (s->ctx));
    exit (1);
  }
  print_hits (s, first, n, n_hits, s->locs);
}

/* search_one_word: the query is looked up as its canonical form; REVERSE is set where that is the reverse complement
 * and stays set (:548-551) */
static void search_one_word (Searcher *s, uint64_t word)
{
  const uint64_t cw = s->zipper ? word : canonical_word (word, s->k);
  if (cw != word) s->sticky = 1;
  if (s->reverse) s->reverse[s->n] = (uint8_t) s->sticky;
  s->words[s->n++] = s->o->words_only ? word : cw;
  if (s->n == QUERY_BATCH) flush_batch (s);
}

/* the length rules of search_one_query_string / search_n_query_strings; 0: *word set */
static int query_string_word (const char *who, const char *c, const Searcher *s, uint64_t *word)
{
  const unsigned int len = (unsigned int) strlen (c), k = s->k;
  if (len != k) {
    if (len < k) {
      fprintf (stderr, "%s: Word too short (%u < %u)\n", who, k, len);
      return 1;
    } else if (s->o->use_3p) {
      *word = string_to_word (c + (len - k), k);
    } else if (s->o->use_5p) {
      *word = string_to_word (c, k);
    } else {
      fprintf (stderr, "%s: Wrong query length (%u != %u) - use --3p or --5p\n", who, k, len);
      return 1;
    }
  } else {
    *word = string_to_word (c, k);
  }
  return 0;
}

static int search_n_query_strings (Searcher *s, const char *queryfile)
{
  FILE *ifs = fopen (queryfile, "r");
  if (ifs == NULL) {
    fprintf (stderr, "search_n_query_strings: Cannot open file %s.\n", queryfile);
    return 1;
  }
  int val = fgetc (ifs);
  while (val > 0) {
    char c[256];
    unsigned int i = 0;
    uint64_t word;
    while (val > 0 && i < 255 && val != '\n') {
      c[i++] = (char) val;
      val = fgetc (ifs);
    }
    c[i] = 0;
    while (val > 0 && val != '\n') val = fgetc (ifs);
    while (val > 0 && val < 'A') val = fgetc (ifs);
    if (query_string_word ("search_n_query_strings", c, s, &word)) {
      flush_batch (s); /* what the reference had printed before it stopped */
      return 1;        /* (the reference leaves the file open too) */
    }
    search_one_word (s, word);
  }
  fclose (ifs);
  return 0;
}

/* The reader of src/fasta.c:87-300 for plain text: forward words only.  Returns what fasta_reader_read_nwords
 * returns (0, or -1 after its message). */
static int search_fasta (Searcher *s, const char *fname)
{
  enum { ST_NONE, ST_NAME, ST_SEQUENCE, ST_QUALITY } state = ST_NONE;
  FILE *ifs = fopen (fname, "r");
  if (!ifs) {
    fprintf (stderr, "search_fasta: Cannot open %s\n", fname);
    return 1;
  }
  const int c0 = fgetc (ifs), c1 = fgetc (ifs);
  if (gt4_cli_refuse_gzip (fname, c0, c1)) {
    fclose (ifs);
    return 1;
  }
  rewind (ifs);
  const unsigned int k = s->k;
  const uint64_t mask = k >= 32 ? ~0ull : (1ull << (2 * k)) - 1;
  int fastq = 0;
  uint64_t wordfw = 0, cpos = 0;
  unsigned int currentlength = 0;
  int result = 0;
#define READ() ((cval = fgetc (ifs)) < 0 ? (cval = 0) : cval) /* a sequence source returns 0 at the end */
  for (;;) {
    int cval;
    READ ();
    if (cval == 0) break;
    switch (state) {
    case ST_NONE:
      if (cval == '>') fastq = 0;
      else if (cval == '@') fastq = 1;
      else {
        fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid start tag '%c'\n", fname, cval);
        result = -1;
        goto done;
      }
      state = ST_NAME;
      cpos += 1;
      break;
    case ST_NAME:
      if (cval == '\n') {
        state = ST_SEQUENCE;
        wordfw = 0;
        currentlength = 0;
      }
      cpos += 1;
      break;
    case ST_SEQUENCE:
      if (!fastq && cval == '>') {
        state = ST_NAME;
      } else if (fastq && cval == '\n') {
        READ ();
        if (cval != '+') {
          fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '+' missing, found '%c' instead at %llu\n", fname, cval, (unsigned long long) cpos);
          result = -1;
          goto done;
        }
        cpos += 1;
        READ ();
        cpos += 1;
        while (cval != '\n') {
          if (cval <= 0) {
            fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid character '%c' after '+' %llu\n", fname, cval, (unsigned long long) cpos);
            result = -1;
            goto done;
          }
          READ ();
          cpos += 1;
        }
        state = ST_QUALITY;
      } else {
        unsigned int nuclval = 4;
        switch (cval) {
        case 'A': case 'a': nuclval = 0; break;
        case 'C': case 'c': nuclval = 1; break;
        case 'G': case 'g': nuclval = 2; break;
        case 'T': case 't': case 'U': case 'u': nuclval = 3; break;
        }
        if (nuclval <= 3) {
          wordfw = (wordfw << 2) | nuclval;
          currentlength += 1;
          if (currentlength > k) {
            wordfw &= mask;
            currentlength = k;
          }
          if (currentlength == k) search_one_word (s, wordfw);
        } else if (cval >= ' ') {
          wordfw = 0;
          currentlength = 0;
        }
      }
      cpos += 1;
      break;
    case ST_QUALITY:
      if (cval == '\n') {
        READ ();
        if (cval == 0) goto done;
        if (cval != '@') {
          fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '@' missing, found '%c' instead at %llu\n", fname, cval, (unsigned long long) cpos);
          result = -1;
          goto done;
        }
        cpos += 1;
        state = ST_NAME;
      }
      cpos += 1;
      break;
    }
  }
#undef READ
done:
  fclose (ifs);
  return result;
}

/* ------------------------------------------------------------------ argv, validation, inputs */

/* the value of -min / -max; NULL at the end of argv: a warning, and the default stays */
static void parse_frequency (const char *value, const char *which, unsigned int *freq)
{
  char *end;
  if (!value) {
    fprintf (stderr, "Warning: No %s frequency specified! Using the default value: %d.\n", which, *freq);
    return;
  }
  *freq = (unsigned int) strtol (value, &end, 10);
  if (*end != 0) {
    fprintf (stderr, "Error: Invalid %s frequency: %s! Must be a positive integer.\n", which, value);
    print_help (1);
  }
}

/* argv (reference :124-252; every quirk of its hand-rolled loop is kept) */
static void parse_argv (int argc, const char *argv[], Options *o)
{
  char *end;
  o->maxfreq = UINT_MAX; /* every other default is 0, CMD_QUERY among them */
  for (int argidx = 1; argidx < argc; argidx++) {
    const char *arg = argv[argidx];
    const int opt = gt4_cli_find_option (OPTIONS, sizeof OPTIONS / sizeof OPTIONS[0], arg);
    switch (opt) {
    case OPT_VERSION:
      gt4_cli_print_version (stdout, "glistquery");
      exit (0);
    case OPT_HELP: print_help (0); break;
    case OPT_SEQFILE:
    case OPT_LISTFILE:
    case OPT_QUERYFILE:
    case OPT_QUERY:
      if (!argv[argidx + 1] || argv[argidx + 1][0] == '-') {
        fprintf (stderr, "Warning: No %s specified!\n", opt == OPT_SEQFILE ? "sequence file name" : opt == OPT_LISTFILE ? "query list file name"
                                                        : opt == OPT_QUERYFILE ? "query file name" : "query");
        argidx += 1;
        continue;
      }
      if (opt == OPT_SEQFILE) o->seqfilename = argv[argidx + 1];
      else if (opt == OPT_LISTFILE) o->querylistfilename = argv[argidx + 1];
      else if (opt == OPT_QUERYFILE) o->queryfilename = argv[argidx + 1];
      else o->querystring = argv[argidx + 1];
      argidx += 1;
      break;
    case OPT_PM:
    case OPT_MM: {
      argidx += 1;
      if (argidx >= argc) print_help (1);
      const unsigned int val = (unsigned int) strtol (argv[argidx], &end, 10);
      if (*end || val > (opt == OPT_PM ? 32u : 16u)) print_help (1);
      if (opt == OPT_PM) o->pm3 = val;
      else o->nmm = val;
      break;
    }
    case OPT_MIN: parse_frequency (argv[++argidx], "minimum", &o->minfreq); break;
    case OPT_MAX: parse_frequency (argv[++argidx], "maximum", &o->maxfreq); break;
    case OPT_DEBUG: o->debug += 1; break;
    case OPT_ALL: o->printall = 1; break;
    case OPT_STATS: o->command = CMD_STATS; break;
    case OPT_MEDIAN: o->command = CMD_MEDIAN; break;
    case OPT_DISTRO:
      if (argidx + 1 >= argc) print_help (1);
      argidx += 1;
      o->distro = (unsigned int) strtol (argv[argidx], &end, 10);
      o->command = CMD_DISTRO;
      break;
    case OPT_GC: o->command = CMD_GC; break;
    case OPT_FILES: o->command = CMD_FILES; break;
    case OPT_SEQUENCES: o->command = CMD_SEQUENCES; break;
    case OPT_LOCATIONS: o->locations = 1; break;
    case OPT_3P: o->use_3p = 1; break;
    case OPT_5P: o->use_5p = 1; break;
    case OPT_HEADER: o->print_header = 1; break;
    case OPT_BLOOM:
    case OPT_NOSCOUTS: break; /* accepted and ignored */
    case OPT_IS_UNION: o->is_union = 1; break;
    case OPT_WORDS_ONLY: o->words_only = 1; break;
    case OPT_PER_SEQUENCE: o->per_sequence = 1; break;
    case OPT_MASK: o->mask = 1; break;
    case OPT_SOFT_MASK: o->soft_mask = 1; break;
    case OPT_MIN_HITS:
      argidx += 1;
      if (argidx >= argc || !argv[argidx][0] || argv[argidx][0] == '-') {
        fprintf (stderr, "Error: --min_hits needs a number\n");
        exit (1);
      }
      o->min_hits = strtoull (argv[argidx], &end, 10);
      if (*end) {
        fprintf (stderr, "Error: Invalid number of hits: %s\n", argv[argidx]);
        exit (1);
      }
      o->have_min_hits = 1;
      break;
    default:
      if (arg[0] != '-') {
        if (o->n_lists == MAX_LISTS) {
          fprintf (stderr, "Error: more than %d lists\n", MAX_LISTS);
          exit (1);
        }
        o->lists[o->n_lists++] = arg;
      } else {
        fprintf (stderr, "Error: Unknown argument: %s!\n", arg);
        print_help (1);
      }
    }
  }
}

static void validate (const Options *o)
{
  if (!o->n_lists) {
    fprintf (stderr, "No list/index files specified!\n");
    print_help (1);
  }
  /* --mask and --per_sequence stand with -s alone; one line, in front of every file and device */
  const char *with = NULL, *what = o->mask ? "--mask" : "--per_sequence";
  if (o->soft_mask && !o->mask) {
    fprintf (stderr, "Error: --soft_mask needs --mask\n");
    exit (1);
  }
  if (o->have_min_hits && !o->per_sequence) {
    fprintf (stderr, o->mask ? "Error: --mask cannot be combined with --min_hits\n" : "Error: --min_hits needs --per_sequence\n");
    exit (1);
  }
  if (!o->per_sequence && !o->mask) return;
  if (o->mask && o->per_sequence) with = "--per_sequence";
  else if (o->querystring) with = "-q";
  else if (o->queryfilename) with = "-f";
  else if (o->querylistfilename) with = "-l";
  else if (o->printall) with = "--all";
  else if (o->locations) with = "--locations";
  else if (o->command == CMD_FILES) with = "--files";
  else if (o->command == CMD_SEQUENCES) with = "--sequences";
  else if (o->command != CMD_QUERY) with = "the statistics options";
  else if (o->words_only) with = "--words-only";
  if (with) fprintf (stderr, "Error: %s cannot be combined with %s\n", what, with);
  else if (!o->seqfilename) fprintf (stderr, "Error: %s needs a sequence file (-s)\n", what);
  else if (o->n_lists != 1) fprintf (stderr, "Error: %s takes one list or index, %u were given\n", what, o->n_lists);
  else return;
  exit (1);
}

/* what needs an index, checked behind open_inputs and in front of every device */
static void validate_index_options (const Options *o, const Input *maps)
{
  const Input *list = NULL;
  for (unsigned int i = 0; i < o->n_lists && !list; i++)
    if (!maps[i].is_index) list = &maps[i];
  if (o->command == CMD_FILES || o->command == CMD_SEQUENCES) {
    if (!list && o->n_lists == 1) return;
    fprintf (stderr, "Error: %s can only be queried from single index\n", o->command == CMD_FILES ? "Files" : "Sequences");
    fprintf (stderr, "Error: %s needs one index", o->command == CMD_FILES ? "--files" : "--sequences");
    if (list) fprintf (stderr, ": %s is a list\n", list->name);
    else fprintf (stderr, ": %u were given\n", o->n_lists);
    exit (1);
  }
  if (o->locations && list) {
    fprintf (stderr, "Error: --locations needs an index: %s is a list\n", list->name);
    exit (1);
  }
}

/* The magic number of a list.  1: the file cannot be opened; a file shorter than the number has code 0 */
static int list_code (const char *name, uint32_t *code)
{
  FILE *ifs = fopen (name, "r");
  if (!ifs) return 1;
  if (fread (code, 4, 1, ifs) != 1) *code = 0;
  fclose (ifs);
  return 0;
}

/* Maps every list / index and the -l query list (headers only so far) and returns the word length.  A list that cannot
 * be opened ends the program at once; every other fault is reported for every file, then exit 1. */
static unsigned int open_inputs (const Options *o, Input *maps, Input *query_input)
{
  unsigned int wlen = 0, invalid = 0;
  for (unsigned int i = 0; i < o->n_lists; i++) {
    uint32_t code = 0;
    int ok = 0;
    if (list_code (o->lists[i], &code)) {
      fprintf (stderr, "Cannot open list %s\n", o->lists[i]);
      exit (1);
    }
    if (code == GT4_LIST_CODE_VALUE || code == GT4_INDEX_CODE_VALUE) {
      ok = !input_open (&maps[i], o->lists[i], code);
      if (ok && o->debug && code == GT4_LIST_CODE_VALUE) fprintf (stderr, "List %s loaded\n", o->lists[i]);
    } else {
      fprintf (stderr, "Error: %s is not a valid GenomeTester4 list/index file\n", o->lists[i]);
      invalid = 1;
    }
    if (!ok) {
      fprintf (stderr, "Error: %s is invalid or corrupted\n", o->lists[i]);
      invalid = 1;
    } else if (!wlen) {
      wlen = maps[i].file.header.word_length;
    } else if (maps[i].file.header.word_length != wlen) {
      fprintf (stderr, "Error: %s has different word length %u (first list had %u)\n", o->lists[i], maps[i].file.header.word_length, wlen);
      invalid = 1;
    }
  }
  if (o->querylistfilename) {
    uint32_t code = 0;
    /* the reference streams the query list (gt4_word_list_stream_new), which takes a .list only: an index is refused */
    const int unreadable = list_code (o->querylistfilename, &code);
    if (!unreadable && code == GT4_INDEX_CODE_VALUE)
      fprintf (stderr, "gt4_word_list_stream_new: invalid file tag (%x, should be %x)\n", code, GT4_LIST_CODE_VALUE);
    if (unreadable || code != GT4_LIST_CODE_VALUE || input_open (query_input, o->querylistfilename, code)) {
      fprintf (stderr, "Error: %s is invalid or corrupted\n", o->querylistfilename);
      invalid = 1;
    } else if (query_input->file.header.word_length != wlen) {
      fprintf (stderr, "Error: %s has different word length %u (first list had %u)\n", o->querylistfilename, query_input->file.header.word_length, wlen);
      invalid = 1;
    }
  }
  if (invalid) exit (1);
  return wlen;
}

/* ------------------------------------------------------------------ the jobs; each returns the exit code */

/* --stat: the headers, no device */
static int run_stat (const Options *o, const Input *maps)
{
  for (unsigned int i = 0; i < o->n_lists; i++) print_list_header (&maps[i]);
  return 0;
}

/* --median / --distribution / --gc, list by list */
static int run_statistics (const Options *o, const Input *maps)
{
  for (unsigned int i = 0; i < o->n_lists; i++) {
    gt4hip_context *ctx;
    const gt4hip_list *dev;
    GT4HipWordList *l = to_device (o->lists[i], &ctx, &dev);
    if (o->command == CMD_MEDIAN) print_median (&maps[i], ctx, dev, o->debug);
    else if (o->command == CMD_DISTRO) print_distro (ctx, dev, o->distro + 1);
    else print_gc (&maps[i], ctx, dev);
    gt4_hip_word_list_delete (l);
  }
  return 0;
}

/* one packed location of an index (index_map_get_location, src/index-map.c:197-208) as print_index_info prints it */
static void print_packed_location (const GT4ListFile *f, uint64_t code)
{
  const unsigned int fb = f->index_file_bits, sb = f->index_subseq_bits, pb = f->index_pos_bits;
#define FIELD(shift, bits) ((shift) >= 64 || !(bits) ? 0 : (code >> (shift)) & ((bits) >= 64 ? ~0ull : (1ull << (bits)) - 1))
  fprintf (stdout, "%u\t%u\t%llu\t%u\n", (unsigned int) FIELD (sb + pb + 1, fb), (unsigned int) FIELD (pb + 1, sb), (unsigned long long) FIELD (1, pb),
           (unsigned int) (code & 1));
#undef FIELD
}

/* no query option, one list: the mapped records, no device; with --locations every place of every word of an index
 * (print_full_map, :481-510).  A first location outside the location section ends the dump with an error. */
static int run_dump (const Input *in, int locations)
{
  char b[64];
  for (uint64_t i = 0; i < in->file.header.n_words; i++) {
    const uint32_t count = input_count (in, i);
    gt4_word2string (b, input_word (in, i), in->file.header.word_length);
    fprintf (stdout, "%s\t%u\n", b, count);
    if (!locations) continue;
    uint64_t at, code;
    memcpy (&at, in->file.index_kmers + 16 * i + 8, 8);
    if (at > in->file.index_locations || count > in->file.index_locations - at) {
      fflush (stdout);
      fprintf (stderr, "Error: %s is corrupted: the locations of word %llu lie outside its %llu locations\n", in->name, (unsigned long long) i,
               (unsigned long long) in->file.index_locations);
      return 1;
    }
    for (uint32_t j = 0; j < count; j++) {
      memcpy (&code, in->file.index_location_words + 8 * (at + j), 8);
      print_packed_location (&in->file, code);
    }
  }
  return 0;
}

/* --files (print_files, :439-449): file I/O on the mapping */
static int run_files (const Input *in)
{
  for (uint32_t i = 0; i < in->file.index_n_files; i++) {
    GT4IndexFile f;
    if (gt4_indexfile_file (&in->file, i, &f)) return 1;
    fprintf (stdout, "%u\t%s\t%llu\t%llu\n", i, f.name, (unsigned long long) f.size, (unsigned long long) f.n_sequences);
  }
  return 0;
}

/* --sequences (print_sequences, :451-467): the names come out of the source files, mapped by their stored names
 * (gt4_index_map_get_sequence_name, src/index-map.c:249-314): at most 1023 bytes, up to the first NUL.  The reference
 * tries to map a missing source again for every sequence, with a message each time. */
static int run_sequences (const Input *in)
{
  for (uint32_t i = 0; i < in->file.index_n_files; i++) {
    GT4IndexFile f;
    if (gt4_indexfile_file (&in->file, i, &f)) return 1;
    const unsigned char *src = NULL;
    uint64_t src_size = 0;
    for (uint64_t j = 0; j < f.n_sequences; j++) {
      GT4IndexSequence q;
      char name[1024];
      unsigned int len = 0;
      gt4_indexfile_sequence (&f, j, &q);
      if (!src) {
        struct stat st;
        const int fd = open (f.name, O_RDONLY);
        const int open_errno = errno;
        if (fd >= 0 && fstat (fd, &st) == 0 && st.st_size > 0) {
          src = (const unsigned char *) mmap (NULL, (size_t) st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
          if (src == MAP_FAILED) src = NULL;
          else src_size = (uint64_t) st.st_size;
        }
        if (!src) {
          fflush (stdout);
          fprintf (stderr, "gt4_mmap (%s): %s\n", fd < 0 ? "open" : "mmap", fd < 0 ? strerror (open_errno) : "the file cannot be mapped");
          fprintf (stderr, "imap_map_src: could not mmap file %s\n", f.name);
        }
        if (fd >= 0) close (fd);
      }
      if (src)
        while (len < 1023 && len < q.name_len && q.name_pos < src_size && len < src_size - q.name_pos && src[q.name_pos + len]) len++;
      if (len) memcpy (name, src + q.name_pos, len);
      name[len] = 0;
      fprintf (stdout, "%u\t%llu\t%s\t%llu\t%llu\t%llu\n", i, (unsigned long long) j, name, (unsigned long long) q.name_pos, (unsigned long long) q.seq_pos,
               (unsigned long long) q.seq_len);
    }
    if (src) munmap ((void *) src, (size_t) src_size);
  }
  return 0;
}

/* no query option, several lists: every word of their union (--is_union: gt4_is_union) with its count in each */
static int run_union_dump (const Options *o, unsigned int wlen)
{
  static GT4HipWordList *objs[MAX_LISTS];
  PrintState st = { .wlen = wlen, .n_lists = o->n_lists };
  if (o->print_header) {
    fprintf (stdout, "KMER");
    for (unsigned int i = 0; i < o->n_lists; i++) fprintf (stdout, "\t%s", o->lists[i]);
    fprintf (stdout, "\n");
  }
  for (unsigned int i = 0; i < o->n_lists; i++) objs[i] = to_device (o->lists[i], NULL, NULL);
  const unsigned int r = (o->is_union ? gt4_is_union : gt4_union) (objs, o->n_lists, dump_cb, &st);
  if (r) fprintf (stderr, "Error: the union of the lists failed (%u)\n", r);
  return r != 0;
}

/* -l against several lists; the query list goes to the device first */
static int run_multi_search (const Options *o, unsigned int wlen)
{
  static GT4HipWordList *objs[MAX_LISTS];
  PrintState st = { .wlen = wlen, .n_lists = o->n_lists };
  if (o->nmm || o->pm3) {
    fprintf (stderr, "Error: Searching multiple lists is incompatible with mismatches\n");
    return 1;
  }
  GT4HipWordList *q = to_device (o->querylistfilename, NULL, NULL);
  for (unsigned int i = 0; i < o->n_lists; i++) objs[i] = to_device (o->lists[i], NULL, NULL);
  const unsigned int result = gt4_search_lists_multi (q, objs, o->n_lists, multi_cb, &st);
  if (st.open) fputc ('\n', stdout);
  return (int) result;
}

/* -l against one list without mismatches: the list goes to the device first (min / max / --all do not apply, as in the reference) */
static int run_zipper (const Options *o, unsigned int wlen)
{
  PrintState st = { .wlen = wlen, .n_lists = 1 };
  GT4HipWordList *l = to_device (o->lists[0], NULL, NULL);
  GT4HipWordList *q = to_device (o->querylistfilename, NULL, NULL);
  const unsigned int r = gt4_search_list_zipper (l, q, zipper_cb, &st);
  if (r) fprintf (stderr, "Error: the search of %s in %s failed (%u)\n", o->querylistfilename, o->lists[0], r);
  return r != 0;
}

/* -q / -f / -s / -l against one list, in batches; --words-only prints the words and opens no device */
static int run_lookups (const Options *o, unsigned int wlen, const Input *index, const Input *query_input)
{
  int v = 0;
  Searcher s = { .o = o, .k = wlen, .prm = { .n_mm = o->nmm, .pm_3 = o->pm3, .canonize = 1 } };
  const int locations = o->locations && !o->words_only;
  gt4hip_location_index *lindex = NULL;
  /* the zipper with locations (search_list_zipper, :702-717): the words of the query list as they are, the QUERY list's
   * count, REVERSE 0, nothing for a word that is not there */
  s.zipper = locations && !o->querystring && !o->queryfilename && !o->seqfilename && !o->nmm;
  if (s.zipper) s.prm.canonize = 0;
  s.words = (uint64_t *) or_oom (malloc ((size_t) QUERY_BATCH * 8), "query batch");
  s.values = (uint32_t *) or_oom (malloc ((size_t) QUERY_BATCH * 4), "query batch");
  s.found = (uint8_t *) or_oom (malloc (QUERY_BATCH), "query batch");
  s.hit_capacity = o->printall || locations ? QUERY_BATCH : 0;
  s.hits = s.hit_capacity ? (gt4hip_query_hit *) or_oom (malloc ((size_t) s.hit_capacity * sizeof (gt4hip_query_hit)), "query batch") : NULL;
  GT4HipWordList *l = NULL;
  if (locations) {
    const GT4ListFile *f = &index->file;
    uint64_t free_bytes = 0, total_bytes = 0;
    s.reverse = (uint8_t *) or_oom (malloc (QUERY_BATCH), "query batch");
    s.loc_capacity = QUERY_BATCH;
    s.locs = (gt4hip_location *) or_oom (malloc ((size_t) s.loc_capacity * sizeof (gt4hip_location)), "query batch");
    if (s.zipper) s.query_counts = (uint32_t *) or_oom (malloc ((size_t) QUERY_BATCH * 4), "query batch");
    s.ctx = gt4_hip_default_context ();
    if (!s.ctx) exit (1);
    CHK (s.ctx, gt4hip_location_index_create (s.ctx, f->index_kmers, f->header.n_words, f->index_location_words, f->index_locations, wlen, f->index_file_bits,
                                              f->index_subseq_bits, f->index_pos_bits, &lindex));
    s.lindex = lindex;
    CHK (s.ctx, gt4hip_query_index_create (s.ctx, gt4hip_location_index_list (lindex), &s.qindex));
    CHK (s.ctx, gt4hip_device_memory (s.ctx, &free_bytes, &total_bytes));
    s.loc_budget = s.hit_budget = free_bytes / 4 / LOOKUP_BYTES;
    if (s.loc_budget < (1u << 16)) s.loc_budget = s.hit_budget = 1u << 16;
    const char *e = getenv ("GT4_GLISTQUERY_LOCATION_BUDGET"); /* tests: the halving of a batch */
    if (e && *e) s.loc_budget = strtoull (e, NULL, 10);
  } else if (!o->words_only) {
    const gt4hip_list *dev = NULL;
    l = to_device (o->lists[0], &s.ctx, &dev);
    CHK (s.ctx, gt4hip_query_index_create (s.ctx, dev, &s.qindex));
  }
  if (o->querystring) {
    uint64_t word;
    v = query_string_word ("search_one_query_string", o->querystring, &s, &word);
    if (!v) search_one_word (&s, word);
  } else if (o->queryfilename) {
    v = search_n_query_strings (&s, o->queryfilename);
  } else if (o->seqfilename) {
    v = search_fasta (&s, o->seqfilename);
  } else if (o->querylistfilename) {
    for (uint64_t i = 0; i < query_input->file.header.n_words; i++) {
      if (s.zipper) s.query_counts[s.n] = input_count (query_input, i);
      search_one_word (&s, input_word (query_input, i));
    }
  }
  flush_batch (&s); /* what was looked up before a parser error is printed all the same */
  fflush (stdout);
  if (s.qindex) gt4hip_query_index_free (s.qindex);
  gt4hip_location_index_free (lindex);
  if (l) gt4_hip_word_list_delete (l);
  free (s.locs);
  free (s.reverse);
  free (s.query_counts);
  free (s.words);
  free (s.values);
  free (s.found);
  free (s.hits);
  return v;
}

/* ------------------------------------------------------------------ -s FILE --per_sequence */

/* the sequence whose line is still to come: its words may go on in the next piece */
typedef struct {
  const Options *o;
  const unsigned char *data; /* the mapped file */
  uint64_t size;
  int have;
  uint64_t name_pos;
  gt4hip_seq_profile sum;
} PendingSequence;

static void pending_print (PendingSequence *p)
{
  if (!p->have) return;
  p->have = 0;
  if (p->sum.n_hits < p->o->min_hits) return;
  fwrite (p->data + p->name_pos, 1, gt4_cli_name_length (p->data, p->size, p->name_pos), stdout);
  fprintf (stdout, "\t%llu\t%llu\t%llu\n", (unsigned long long) p->sum.n_words, (unsigned long long) p->sum.n_hits, (unsigned long long) p->sum.sum);
}

/* the reference's line for a reader error (src/fasta.c:136, :202, :211, :277), as search_fasta prints them */
static void print_reader_error (const char *fname, const unsigned char *data, uint64_t size, uint32_t kind, uint64_t at)
{
  const int found = at < size ? data[at] : 0;
  const unsigned long long cpos = at ? at - 1 : 0;
  switch (kind) {
    case GT4HIP_MAKER_ERR_START: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid start tag '%c'\n", fname, found); break;
    case GT4HIP_MAKER_ERR_PLUS: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '+' missing, found '%c' instead at %llu\n", fname, found, cpos); break;
    case GT4HIP_MAKER_ERR_AT: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '@' missing, found '%c' instead at %llu\n", fname, found, cpos); break;
    default: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid character '%c' after '+' %llu\n", fname, found, (unsigned long long) at); break;
  }
}

/* One piece through gt4hip_query_profile_text, its sums into `pend` and onto stdout.  0, or the library's code with the
 * reader's error in next->reader.error and its offset in the piece in *at; `prof` grows to what a piece needs. */
static int profile_piece (gt4hip_context *ctx, gt4hip_query_index *qindex, const Options *o, const unsigned char *text, size_t len, const gt4hip_locations_carry *carry,
                          gt4hip_locations_carry *next, gt4hip_seq_profile **prof, uint64_t *prof_cap, PendingSequence *pend, uint64_t *at, uint64_t *n_words)
{
  const gt4hip_query_params prm = { .n_mm = o->nmm, .pm_3 = o->pm3, .canonize = 1 };
  const uint32_t lo = o->minfreq > 1 ? o->minfreq : 1;
  gt4hip_locations_piece piece;
  uint64_t n = 0;
  int rc = gt4hip_query_profile_text (ctx, qindex, text, len, 0, &prm, lo, o->maxfreq, carry, next, &piece, *prof, *prof_cap, &n, at);
  if (!rc && n > *prof_cap) {
    free (*prof);
    *prof_cap = n + n / 2;
    *prof = (gt4hip_seq_profile *) or_oom (malloc ((size_t) *prof_cap * sizeof **prof), "%llu sequences of one piece", (unsigned long long) n);
    rc = gt4hip_query_profile_text (ctx, qindex, text, len, 0, &prm, lo, o->maxfreq, carry, next, &piece, *prof, *prof_cap, &n, at);
  }
  if (rc) return rc;
  uint64_t e = 0;
  if (carry && carry->seq_open) {
    pend->sum.n_words += (*prof)[0].n_words, pend->sum.n_hits += (*prof)[0].n_hits, pend->sum.sum += (*prof)[0].sum;
    e = 1;
  }
  for (uint64_t i = 0; i < piece.n_subseqs; i++) {
    pending_print (pend);
    pend->have = 1;
    pend->name_pos = piece.subseqs[i].name_pos;
    pend->sum = (*prof)[e + i];
  }
  *n_words = piece.n_words;
  return GT4HIP_OK;
}

/* ---- what --per_sequence and --mask share: the file of -s mapped whole, the list and its index on the device, the pieces */

typedef struct {
  const char *name;
  const unsigned char *data;
  uint64_t size;
} SeqFile;

/* 0: mapped (size 0: there is nothing to read); 1 after a message: the file cannot be opened or mapped, or is gzip-compressed */
static int seqfile_map (const char *fname, SeqFile *f)
{
  struct stat st;
  const int fd = open (fname, O_RDONLY);
  if (fd < 0 || fstat (fd, &st)) {
    fprintf (stderr, "search_fasta: Cannot open %s\n", fname);
    if (fd >= 0) close (fd);
    return 1;
  }
  f->name = fname, f->data = NULL, f->size = (uint64_t) st.st_size;
  if (f->size) {
    void *m = mmap (NULL, (size_t) f->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      fprintf (stderr, "Error: cannot map %s: %s\n", fname, strerror (errno));
      close (fd);
      return 1;
    }
    f->data = (const unsigned char *) m;
  }
  close (fd);
  return gt4_cli_refuse_gzip (fname, f->size > 0 ? f->data[0] : EOF, f->size > 1 ? f->data[1] : EOF);
}

typedef struct {
  gt4hip_context *ctx;
  gt4hip_query_index *qindex;
  GT4HipWordList *list;
  uint64_t chunk; /* bytes of a piece: GT4HIP_QUERY_CHUNK, or 1/64 of the free device memory, 1 MiB to 1 GiB */
  int verbose;
  unsigned int pieces;
  double reader_ms, device_ms;
} Streamer;

static void streamer_open (const Options *o, Streamer *s)
{
  int device = 0;
  const gt4hip_list *dev = NULL;
  memset (s, 0, sizeof *s);
  gt4_cli_read_environment (&device, &s->verbose);
  s->list = to_device (o->lists[0], &s->ctx, &dev);
  CHK (s->ctx, gt4hip_query_index_create (s->ctx, dev, &s->qindex));
  s->chunk = gt4_cli_parse_bytes (getenv ("GT4HIP_QUERY_CHUNK"));
  if (!s->chunk) {
    uint64_t free_b = 0, total_b = 0;
    CHK (s->ctx, gt4hip_device_memory (s->ctx, &free_b, &total_b));
    s->chunk = free_b / 64;
    if (s->chunk > (1ull << 30)) s->chunk = 1ull << 30;
    if (s->chunk < (1ull << 20)) s->chunk = 1ull << 20;
  }
  if (s->verbose) fprintf (stderr, "Device: %s; pieces of %llu bytes\n", gt4hip_device_info (s->ctx), (unsigned long long) s->chunk);
}

/* bytes of the piece that starts at `pos`: a chunk, cut behind the last '\n' of its second half where there is one */
static size_t piece_length (const SeqFile *f, uint64_t pos, uint64_t chunk)
{
  size_t len = (size_t) (f->size - pos);
  if (len > chunk) {
    len = (size_t) chunk;
    const unsigned char *nl = (const unsigned char *) memrchr (f->data + pos + len / 2, '\n', len - len / 2);
    if (nl) len = (size_t) (nl - (f->data + pos)) + 1;
  }
  return len;
}

/* GT4HIP_VERBOSE: the piece that ends at `pos`; `what`: what the device did behind the reader */
static void piece_done (Streamer *s, const SeqFile *f, uint64_t pos, uint64_t n_words, const char *what)
{
  s->pieces++;
  if (!s->verbose) return;
  uint64_t us = 0;
  const double ms = gt4hip_query_index_last_ms (s->qindex);
  gt4hip_get_counter (s->ctx, "extract_us", &us);
  s->device_ms += ms, s->reader_ms += us / 1000.0;
  fprintf (stderr, "%s: piece %u ends at byte %llu: %llu words, reader %.3f ms, %s %.3f ms\n", f->name, s->pieces, (unsigned long long) pos,
           (unsigned long long) n_words, us / 1000.0, what, ms);
}

/* the end of the file behind a FastQ sequence line or inside a '+' line (src/fasta.c:200-213): -1 after the reader's line, else 0 */
static int end_of_file_error (const SeqFile *f, const gt4hip_maker_carry *c)
{
  if (c->ended || c->file_type != GT4HIP_MAKER_FASTQ || c->line_phase != 2) return 0;
  print_reader_error (f->name, f->data, f->size, c->at_line_start ? GT4HIP_MAKER_ERR_PLUS : GT4HIP_MAKER_ERR_PLUS_EOF, f->size);
  return -1;
}

static void streamer_close (Streamer *s, const SeqFile *f, const char *what)
{
  if (s->verbose)
    fprintf (stderr, "%s: %llu bytes in %u piece(s); reader %.3f ms, %s %.3f ms\n", f->name, (unsigned long long) f->size, s->pieces, s->reader_ms, what, s->device_ms);
  gt4hip_query_index_free (s->qindex);
  gt4_hip_word_list_delete (s->list);
  munmap ((void *) f->data, (size_t) f->size);
}

static int run_per_sequence (const Options *o)
{
  SeqFile f;
  if (seqfile_map (o->seqfilename, &f)) return 1;
  if (!f.size) return 0;
  const char *fname = f.name;
  const unsigned char *data = f.data;
  const uint64_t size = f.size;
  Streamer s;
  streamer_open (o, &s);
  gt4hip_context *ctx = s.ctx;
  gt4hip_query_index *qindex = s.qindex;
  PendingSequence pend = { .o = o, .data = data, .size = size };
  gt4hip_locations_carry carry, next;
  gt4hip_seq_profile *prof = NULL;
  uint64_t prof_cap = 0, pos = 0;
  int have = 0, result = 0;
  while (pos < size) {
    const size_t len = piece_length (&f, pos, s.chunk);
    uint64_t at = 0, n_words = 0;
    int rc = profile_piece (ctx, qindex, o, data + pos, len, have ? &carry : NULL, &next, &prof, &prof_cap, &pend, &at, &n_words);
    if (rc == GT4HIP_EFORMAT) {
      /* the words in front of the error count, as -s looks them up: the piece again, up to the offending byte */
      const uint32_t kind = next.reader.error;
      uint64_t none = 0;
      if (at && (rc = profile_piece (ctx, qindex, o, data + pos, (size_t) at, have ? &carry : NULL, &next, &prof, &prof_cap, &pend, &none, &n_words))) {
        fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
        exit (1);
      }
      pending_print (&pend);
      fflush (stdout);
      print_reader_error (fname, data, size, kind, pos + at);
      result = -1;
      break;
    }
    if (rc) {
      fflush (stdout);
      fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
      exit (1);
    }
    carry = next;
    have = 1;
    pos += len;
    piece_done (&s, &f, pos, n_words, "lookups and sums");
    if (carry.reader.ended) break;
  }
  if (!result) {
    pending_print (&pend);
    fflush (stdout);
    if (have) result = end_of_file_error (&f, &carry.reader);
  }
  free (prof);
  gt4hip_locations_free (ctx);
  streamer_close (&s, &f, "lookups and sums");
  return result;
}

/* ------------------------------------------------------------------ -s FILE --mask [--soft_mask] */

static int write_stdout (const void *bytes, size_t n, void *arg)
{
  (void) arg;
  return fwrite (bytes, 1, n, stdout) != n;
}

static void mask_or_exit (int failed)
{
  if (!failed) return;
  fflush (stdout);
  fprintf (stderr, "Error: the masked text could not be written: %s\n", errno ? strerror (errno) : "out of memory");
  exit (1);
}

/* The file goes through gt4hip_query_mask_text piece by piece; what a later piece may still cover is held back (GT4MaskTail). */
static int run_mask (const Options *o)
{
  SeqFile f;
  if (seqfile_map (o->seqfilename, &f)) return 1;
  if (!f.size) return 0;
  Streamer s;
  streamer_open (o, &s);
  gt4hip_context *ctx = s.ctx;
  const gt4hip_query_params prm = { .n_mm = o->nmm, .pm_3 = o->pm3, .canonize = 1 };
  const uint32_t lo = o->minfreq > 1 ? o->minfreq : 1;
  const unsigned int flags = o->soft_mask ? GT4HIP_MASK_SOFT : 0, k = gt4hip_list_word_length (gt4_hip_word_list_device (s.list));
  unsigned char *masked = (unsigned char *) or_oom (malloc ((size_t) (f.size < s.chunk ? f.size : s.chunk)), "a piece of %llu bytes", (unsigned long long) s.chunk);
  GT4MaskTail tail;
  gt4_mask_tail_init (&tail, o->soft_mask, 'N', write_stdout, NULL);
  gt4hip_maker_carry carry, next;
  gt4hip_mask_piece piece;
  uint64_t pos = 0;
  int have = 0, result = 0;
  while (pos < f.size) {
    const size_t len = piece_length (&f, pos, s.chunk);
    uint64_t at = 0;
    int rc = gt4hip_query_mask_text (ctx, s.qindex, f.data + pos, len, flags, &prm, lo, o->maxfreq, 'N', have ? &carry : NULL, &next, masked, &piece, &at);
    if (rc == GT4HIP_EFORMAT) {
      /* the words in front of the error count, as -s looks them up: the piece again, up to the offending byte */
      const uint32_t kind = next.error;
      uint64_t none = 0;
      if (at) {
        if (gt4hip_query_mask_text (ctx, s.qindex, f.data + pos, (size_t) at, flags, &prm, lo, o->maxfreq, 'N', have ? &carry : NULL, &next, masked, &piece, &none)) {
          fflush (stdout);
          fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
          exit (1);
        }
        mask_or_exit (gt4_mask_tail_push (&tail, masked, (size_t) at, piece.back, k));
      }
      mask_or_exit (gt4_mask_tail_finish (&tail));
      fflush (stdout);
      print_reader_error (f.name, f.data, f.size, kind, pos + at);
      result = -1;
      break;
    }
    if (rc) {
      fflush (stdout);
      fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
      exit (1);
    }
    mask_or_exit (gt4_mask_tail_push (&tail, masked, len, piece.back, k));
    carry = next;
    have = 1;
    pos += len;
    piece_done (&s, &f, pos, piece.n_words, "lookups and masking");
    if (carry.ended) break;
  }
  if (!result) {
    /* the end of the file, or a NUL: nothing more is covered; the rest of the file as it is */
    mask_or_exit (gt4_mask_tail_finish (&tail));
    if (pos < f.size) mask_or_exit (write_stdout (f.data + pos, (size_t) (f.size - pos), NULL));
    mask_or_exit (fflush (stdout) != 0);
    if (have) result = end_of_file_error (&f, &carry);
  }
  free (masked);
  streamer_close (&s, &f, "lookups and masking");
  return result;
}

int main (int argc, const char *argv[])
{
  static Options o;
  static Input maps[MAX_LISTS], query_input;
  parse_argv (argc, argv, &o);
  validate (&o);
  const unsigned int wlen = open_inputs (&o, maps, &query_input);
  validate_index_options (&o, maps);
  if (o.command == CMD_STATS) return run_stat (&o, maps);
  if (o.command == CMD_FILES) return run_files (&maps[0]);
  if (o.command == CMD_SEQUENCES) return run_sequences (&maps[0]);
  if (o.command != CMD_QUERY) return run_statistics (&o, maps); /* median, distribution or gc */
  if (!o.seqfilename && !o.querylistfilename && !o.queryfilename && !o.querystring)
    return o.n_lists > 1 ? run_union_dump (&o, wlen) : run_dump (&maps[0], o.locations);
  if (o.querylistfilename && o.n_lists > 1) return run_multi_search (&o, wlen);
  if (o.n_lists > 1) {
    fprintf (stderr, "Error: Query is incompatible with multiple lists/indices\n");
    return 1;
  }
  if (o.nmm + o.pm3 > wlen) {
    fprintf (stderr, "Error: Number of mismatches (%u) and 3' perfect match (%u) are longer than word length %u\n", o.nmm, o.pm3, wlen);
    return 1;
  }
  if (o.per_sequence) return run_per_sequence (&o);
  if (o.mask) return run_mask (&o);
  if (!o.querystring && !o.queryfilename && !o.seqfilename && !o.nmm && !o.words_only && !o.locations) return run_zipper (&o, wlen);
  return run_lookups (&o, wlen, &maps[0], &query_input);
}
