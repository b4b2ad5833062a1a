/*
 * gt4_glistmaker_cli.c -- `glistmaker`, the drop-in command line that turns FastA / FastQ text into a k-mer list.
 * Host C; the text is read into HBM and everything behind that -- classifying the bytes, putting the canonical words
 * together, sorting and counting them, collating the pieces -- runs in the HIP kernels behind include/gt4hip.h
 * (gt4hip_maker.hip, gt4hip_sort.hip, the N-way union).
 *
 * Same argv grammar, defaults, validation order, messages, help text on stderr, -v, output name (`<out>_<k>.list`,
 * written as `.tmp`, then renamed) and exit codes as the reference's main() (reference src/glistmaker.c:138-353).
 * --num_threads, --max_tables, --table_size (which swallows the argument behind its value, :210), --tmpdir, --stream
 * and -D are parsed and validated as there and otherwise ignored: there is no task queue and there are no temporary
 * files.  -c / --cutoff / --min and --max are validated as there and, as there, do nothing to a list: the reference
 * hands cutoff 1 to gt4_write_union (:333, :814) and reads min / max for index output only (:486).
 * A text larger than a chunk goes through the device in pieces, cut behind a '\n' where the second half of the chunk has
 * one; each piece becomes a list and the lists are collated by ADD unions of at most 32 (gt4_write_union): as soon as 32
 * lists of a level exist they become one list of the level above, so at most 31 lists per level are resident while the
 * files are read.  The reference keeps such lists in temporary files; here they stay in device memory, so the collated
 * lists of the levels (in the end: the result) have to fit there.  Several input files pool their words; a run of bases
 * never crosses from one file into the next.
 * --index writes `<out>_<k>.index` instead (reference write_index, :366-782): every word of every input with where it
 * stands stays in device memory -- 16 bytes a word, sized from the inputs' bytes -- until one sort by word behind the last
 * file, since the bit sizes of a location are known only then; the sort needs as much again.  What does not fit is an
 * error that names --index and the bytes, and no file is written.  Offsets in the file block count from the start of the
 * file throughout (the reference cuts files above 10^8 bytes into blocks and counts seq_pos from the block's start).
 * Deliberate differences, all an error message + exit 1:
 *   - --index with standard input (the file block records a file's name and size);
 *   - input that starts with the gzip magic (the reference goes by the name's .gz): decompress it first;
 *   - without a usable GPU the program fails: there is no CPU path;
 *   - malformed text (a first byte that is neither '>' nor '@'; FastQ without its '+' line or its '@'): the reference's
 *     message for the first offending byte, then "Error: ..."; no output file is written.  (The reference carries on
 *     behind a reader error and writes whatever it still finds.)
 * Environment, all of it read in read_environment():
 *   GT4HIP_MAKER_CHUNK=<bytes>[K|M|G]  bytes of text per piece (default: 1/64 of the free device memory, at most 1 GiB);
 *   GT4HIP_DEVICE=N                    the device (default 0);
 *   GT4HIP_VERBOSE=1                   prints the device, the pieces (where each ends) and the kernel times on stderr.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "gt4_cli.h"
#include "gt4_listfile.h"
#include "gt4hip.h"

#define MAX_FILES 1024
#define MAX_TABLES 256
#define UNION_WIDTH 32 /* FILE_MERGE_SIZE, src/glistmaker.c:68 */
#define MAX_LEVELS 13  /* 32^13 pieces: more than a text of 2^64 bytes has */

static const char *const HELP_LINES[] = {
  "Usage: glistmaker <INPUTFILES> [OPTIONS]",
  "Options:",
  "    -v, --version           - print version information and exit",
  "    -h, --help              - print this usage screen and exit",
  "    -w, --wordlength NUMBER - specify index wordsize (1-32)",
  "    -o, --outputname STRING - specify output name (default \"out\")",
  "    --index                 - create index instead of list",
  "    --num_threads           - number of threads (default 8)",
  "    --max_tables            - maximum number of temporary tables (default 4096)",
  "    --table_size            - maximum size of the temporary table (default 1048576)",
  "    --tmpdir                - directory for temporary files (may need an order of magnitude more space than the size of the final list)",
  "    --stream                - read files as streams instead of memory-mapping (slower but uses less virtual memory)",
  "    --index                 - creates indexed list (larger and slower)",
  "    -D                      - increase debug level",
};

typedef struct {
  const char *fnames[MAX_FILES];
  unsigned int nfiles;
  unsigned int wordlength, min, max, nthreads, ntables, stream, create_index, debug;
  long long tablesize;
  const char *outputname, *tmpdir;
  /* environment */
  uint64_t chunk;
  int device, verbose;
} Options;

static void print_help (int exit_value)
{
  gt4_cli_print_help (stderr, "glistmaker", HELP_LINES, sizeof HELP_LINES / sizeof HELP_LINES[0]);
  exit (exit_value);
}

/* every environment variable of the program, once */
static void read_environment (Options *o)
{
  o->chunk = gt4_cli_parse_bytes (getenv ("GT4HIP_MAKER_CHUNK"));
  gt4_cli_read_environment (&o->device, &o->verbose);
}

/* the value of a numeric option, or the reference's message + help */
static long long number_arg (int argc, const char *argv[], int *i, const char *what)
{
  char *end;
  if (++*i >= argc) print_help (1);
  const long long v = strtoll (argv[*i], &end, 10);
  if (*end != 0) {
    fprintf (stderr, "Error: Invalid %s: %s! Must be an integer.\n", what, argv[*i]);
    print_help (1);
  }
  return v;
}

/* argv (reference :158-228) */
static void parse_argv (int argc, const char *argv[], Options *o)
{
  o->min = 1;
  o->max = 0xffffffffu;
  o->nthreads = 8;
  o->ntables = 32 * 128;
  o->tablesize = 1024 * 1024;
  o->outputname = "out";
  o->tmpdir = ".";
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp (a, "-v") || !strcmp (a, "--version")) {
      gt4_cli_print_version (stdout, "glistmaker");
      exit (0);
    } else if (!strcmp (a, "-h") || !strcmp (a, "--help") || !strcmp (a, "-?")) {
      print_help (0);
    } else if (!strcmp (a, "-o") || !strcmp (a, "--outputname")) {
      if (++i >= argc) print_help (1);
      o->outputname = argv[i];
    } else if (!strcmp (a, "-w") || !strcmp (a, "--wordlength")) {
      o->wordlength = (unsigned int) (long) number_arg (argc, argv, &i, "word-length");
    } else if (!strcmp (a, "-c") || !strcmp (a, "--cutoff") || !strcmp (a, "--min")) {
      o->min = (unsigned int) (long) number_arg (argc, argv, &i, "frequency cut-off");
    } else if (!strcmp (a, "--max")) {
      o->max = (unsigned int) (long) number_arg (argc, argv, &i, "frequency cut-off");
    } else if (!strcmp (a, "--num_threads")) {
      o->nthreads = (unsigned int) (long) number_arg (argc, argv, &i, "num-threads");
    } else if (!strcmp (a, "--max_tables")) {
      o->ntables = (unsigned int) (long) number_arg (argc, argv, &i, "max_tables");
    } else if (!strcmp (a, "--table_size")) {
      o->tablesize = number_arg (argc, argv, &i, "table-size");
      i += 1; /* the reference skips the argument behind the value as well */
    } else if (!strcmp (a, "--tmpdir")) {
      if (++i >= argc) print_help (1);
      o->tmpdir = argv[i];
    } else if (!strcmp (a, "--stream")) {
      o->stream = 1;
    } else if (!strcmp (a, "--index")) {
      o->create_index = 1;
    } else if (!strcmp (a, "-D")) {
      o->debug += 1;
    } else {
      if (a[0] == '-' && a[1]) print_help (1);
      if (o->nfiles >= MAX_FILES) continue;
      o->fnames[o->nfiles++] = a;
    }
  }
}

/* reference :230-264 */
static void validate (Options *o)
{
  if (o->ntables > MAX_TABLES) o->ntables = MAX_TABLES;
  if (!o->nfiles) {
    fprintf (stderr, "Error: No FastA/FastQ file specified!\n");
    print_help (1);
  }
  if (o->wordlength < 1 || o->wordlength > 32) {
    fprintf (stderr, "Error: Invalid word-length %d (must be 1 - 32)!\n", (int) o->wordlength);
    print_help (1);
  }
  if (o->min < 1) {
    fprintf (stderr, "Error: Invalid frequency cut-off: %d! Must be positive.\n", (int) o->min);
    print_help (1);
  }
  if (o->max < o->min) {
    fprintf (stderr, "Error: Invalid frequency range: %u-%u!\n", o->min, o->max);
    print_help (1);
  }
  if (strlen (o->outputname) > 200) {
    fprintf (stderr, "Error: Output name exceeds the 200 character limit.");
    exit (1);
  }
  for (unsigned int i = 0; i < o->nfiles; i++) {
    struct stat s;
    if (!strcmp (o->fnames[i], "-")) continue;
    if (stat (o->fnames[i], &s)) {
      fprintf (stderr, "main: No such file (cannot stat): %s\n", o->fnames[i]);
      exit (1);
    }
  }
}

/* ------------------------------------------------------------------ input text */

typedef struct {
  const unsigned char *data;
  size_t size;
  int mapped;
  char id[1100]; /* the reader's name in the reference's messages */
} Text;

static void text_open (const Options *o, const char *name, Text *t)
{
  memset (t, 0, sizeof *t);
  if (!strcmp (name, "-")) {
    snprintf (t->id, sizeof t->id, "STDIN");
    size_t cap = 1u << 20, n = 0;
    unsigned char *b = (unsigned char *) malloc (cap);
    while (b) {
      const size_t got = fread (b + n, 1, cap - n, stdin);
      n += got;
      if (n < cap) break;
      b = (unsigned char *) realloc (b, cap *= 2);
    }
    if (!b) {
      fprintf (stderr, "Error: out of memory (standard input)\n");
      exit (1);
    }
    t->data = b;
    t->size = n;
    return;
  }
  if (o->stream) snprintf (t->id, sizeof t->id, "%.1024s", name);
  else snprintf (t->id, sizeof t->id, "%.1024s block 0", name);
  const int fd = open (name, O_RDONLY);
  struct stat s;
  if (fd < 0 || fstat (fd, &s)) {
    fprintf (stderr, "Error: cannot open %s: %s\n", name, strerror (errno));
    exit (1);
  }
  t->size = (size_t) s.st_size;
  if (t->size) {
    void *p = mmap (NULL, t->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) {
      fprintf (stderr, "Error: cannot map %s: %s\n", name, strerror (errno));
      exit (1);
    }
    t->data = (const unsigned char *) p;
    t->mapped = 1;
  }
  close (fd);
  if (t->size >= 2 && gt4_cli_refuse_gzip (name, t->data[0], t->data[1])) exit (1);
}

static void text_close (Text *t)
{
  if (t->mapped) munmap ((void *) t->data, t->size);
  else free ((void *) t->data);
}

/* the reference's line for a reader error (src/fasta.c:136, :202, :211, :277), then ours; exit 1 */
static void format_error_exit (const Text *t, uint32_t kind, uint64_t at)
{
  const int found = at < t->size ? t->data[at] : 0;
  const unsigned long long cpos = at ? at - 1 : 0;
  switch (kind) {
    case GT4HIP_MAKER_ERR_START: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid start tag '%c'\n", t->id, found); break;
    case GT4HIP_MAKER_ERR_PLUS: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '+' missing, found '%c' instead at %llu\n", t->id, found, cpos); break;
    case GT4HIP_MAKER_ERR_AT: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '@' missing, found '%c' instead at %llu\n", t->id, found, cpos); break;
    default: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid character '%c' after '+' %llu\n", t->id, found, (unsigned long long) at); break;
  }
  fprintf (stderr, "Error: %s is not well-formed FastA / FastQ text (byte %llu): no list written\n", t->id, (unsigned long long) at);
  exit (1);
}

/* ------------------------------------------------------------------ text -> lists -> one list */

/* the lists not yet collated: level 0 holds the pieces' own, level i + 1 unions of UNION_WIDTH lists of level i */
typedef struct {
  gt4hip_list *v[MAX_LEVELS][UNION_WIDTH];
  unsigned int n[MAX_LEVELS];
} Lists;

/* gt4_write_union (reference :333, :814): cnt lists -> one, by ADD with cutoff 1; the inputs are freed */
static gt4hip_list *union_lists (gt4hip_context *ctx, gt4hip_list *const *v, unsigned int cnt)
{
  if (cnt == 1) return v[0];
  gt4hip_multi_result res;
  memset (&res, 0, sizeof res);
  CHK (ctx, gt4hip_union_multi (ctx, (const gt4hip_list *const *) v, cnt, 1, GT4HIP_RULE_ADD, 1, 0, &res));
  for (unsigned int i = 0; i < cnt; i++) gt4hip_list_free (v[i]);
  return res.out;
}

/* a full level becomes one list of the level above at once */
static void lists_push (gt4hip_context *ctx, Lists *ls, gt4hip_list *l)
{
  for (unsigned int level = 0; level < MAX_LEVELS; level++) {
    ls->v[level][ls->n[level]++] = l;
    if (ls->n[level] < UNION_WIDTH || level + 1 == MAX_LEVELS) return;
    l = union_lists (ctx, ls->v[level], UNION_WIDTH);
    ls->n[level] = 0;
  }
}

/* one file through the device, a piece at a time: a list per piece that holds a word */
static void file_to_lists (const Options *o, gt4hip_context *ctx, const Text *t, uint64_t chunk, Lists *ls)
{
  gt4hip_maker_carry carry, next;
  int have = 0;
  size_t pos = 0;
  unsigned int pieces = 0;
  double extract_us = 0, sort_us = 0;
  while (pos < t->size) {
    size_t len = t->size - pos;
    if (len > chunk) {
      len = (size_t) chunk;
      /* behind the last '\n' of the chunk's second half, where there is one */
      const unsigned char *nl = (const unsigned char *) memrchr (t->data + pos + len / 2, '\n', len - len / 2);
      if (nl) len = (size_t) (nl - (t->data + pos)) + 1;
    }
    uint64_t *words = NULL, n_words = 0, at = 0;
    const int rc = gt4hip_text_to_words (ctx, t->data + pos, len, o->wordlength, 0, have ? &carry : NULL, &next, &words, &n_words, &at);
    if (rc == GT4HIP_EFORMAT) format_error_exit (t, next.error, pos + at);
    if (rc) {
      fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
      exit (1);
    }
    if (n_words) {
      gt4hip_list *l = NULL;
      uint64_t us = 0;
      CHK (ctx, gt4hip_device_words_to_list (ctx, words, n_words, o->wordlength, &l));
      gt4hip_words_free (ctx, words);
      lists_push (ctx, ls, l);
      if (!gt4hip_get_counter (ctx, "extract_us", &us)) extract_us += (double) us;
      if (!gt4hip_get_counter (ctx, "sort_us", &us)) sort_us += (double) us;
    }
    carry = next;
    have = 1;
    pos += len;
    pieces++;
    if (o->verbose && pos < t->size) fprintf (stderr, "%s: piece %u ends at byte %zu\n", t->id, pieces, pos);
    if (carry.ended) break;
  }
  /* the end of the file behind a FastQ sequence line or inside a '+' line (src/fasta.c:200-213) */
  if (have && !carry.ended && carry.file_type == GT4HIP_MAKER_FASTQ && carry.line_phase == 2)
    format_error_exit (t, carry.at_line_start ? GT4HIP_MAKER_ERR_PLUS : GT4HIP_MAKER_ERR_PLUS_EOF, t->size);
  if (o->verbose) fprintf (stderr, "%s: %zu bytes in %u piece(s); extraction %.3f ms, radix sort %.3f ms\n", t->id, t->size, pieces, extract_us / 1000.0, sort_us / 1000.0);
}

/* what the levels still hold -> one list (NULL: there was no word), from the lowest level up */
static gt4hip_list *collate (gt4hip_context *ctx, Lists *ls)
{
  gt4hip_list *up = NULL;
  for (unsigned int level = 0; level < MAX_LEVELS; level++) {
    if (up) ls->v[level][ls->n[level]++] = up; /* (a level in use holds at most UNION_WIDTH - 1) */
    up = ls->n[level] ? union_lists (ctx, ls->v[level], ls->n[level]) : NULL;
    ls->n[level] = 0;
  }
  return up;
}

/* ------------------------------------------------------------------ --index: text -> pairs -> index file */

_Static_assert (sizeof (GT4IndexSubseq) == sizeof (gt4hip_subseq), "the library's records are handed to the writer as they are");

static unsigned int bit_size (uint64_t v) /* get_bitsize, reference :116-126 */
{
  unsigned int n = 1;
  while (v >>= 1) n++;
  return n;
}

static void index_no_room (uint64_t text_bytes, uint64_t need)
{
  fprintf (stderr, "Error: --index: the words of %llu bytes of text and their locations need %llu bytes of device memory, which do not fit: no index written\n",
           (unsigned long long) text_bytes, (unsigned long long) need);
  exit (1);
}

/* one file through the device, a piece at a time: its words and raw locations behind the `at` pairs there are, its records into `in` */
static uint64_t file_to_pairs (const Options *o, gt4hip_context *ctx, const Text *t, uint64_t chunk, uint64_t *d_words, uint64_t *d_raw, uint64_t at, uint64_t capacity,
                               GT4IndexInput *in, uint64_t *max_pos)
{
  gt4hip_locations_carry carry, next;
  GT4IndexSubseq *subs = NULL;
  uint64_t n_subs = 0, cap_subs = 0, n_words = 0;
  int have = 0;
  size_t pos = 0;
  unsigned int pieces = 0;
  while (pos < t->size) {
    size_t len = t->size - pos;
    if (len > chunk) {
      len = (size_t) chunk;
      const unsigned char *nl = (const unsigned char *) memrchr (t->data + pos + len / 2, '\n', len - len / 2);
      if (nl) len = (size_t) (nl - (t->data + pos)) + 1;
    }
    gt4hip_locations_piece piece;
    uint64_t err_at = 0;
    const int rc = gt4hip_text_to_locations (ctx, t->data + pos, len, o->wordlength, 0, have ? &carry : NULL, &next, d_words + at + n_words, d_raw + at + n_words,
                                             capacity - at - n_words, &piece, &err_at);
    if (rc == GT4HIP_EFORMAT) format_error_exit (t, next.reader.error, pos + err_at);
    if (rc) {
      fprintf (stderr, "Error: --index: %s\n", gt4hip_last_error (ctx));
      exit (1);
    }
    if (piece.closed && n_subs) subs[n_subs - 1].seq_len = piece.closed_seq_len;
    if (n_subs + piece.n_subseqs > cap_subs) {
      cap_subs = (n_subs + piece.n_subseqs) * 2;
      subs = (GT4IndexSubseq *) realloc (subs, cap_subs * sizeof *subs);
      if (!subs) {
        fprintf (stderr, "Error: out of memory (%llu sequence records)\n", (unsigned long long) cap_subs);
        exit (1);
      }
    }
    if (piece.n_subseqs) memcpy (subs + n_subs, piece.subseqs, piece.n_subseqs * sizeof *subs);
    n_subs += piece.n_subseqs;
    n_words += piece.n_words;
    carry = next;
    have = 1;
    pos += len;
    pieces++;
    if (o->verbose && pos < t->size) fprintf (stderr, "%s: piece %u ends at byte %zu\n", t->id, pieces, pos);
    if (carry.reader.ended) break;
  }
  if (have && !carry.reader.ended && carry.reader.file_type == GT4HIP_MAKER_FASTQ && carry.reader.line_phase == 2)
    format_error_exit (t, carry.reader.at_line_start ? GT4HIP_MAKER_ERR_PLUS : GT4HIP_MAKER_ERR_PLUS_EOF, t->size);
  if (have && carry.seq_open && n_subs) subs[n_subs - 1].seq_len = t->size - subs[n_subs - 1].seq_pos; /* (src/fasta.c:109) */
  if (have && carry.max_position > *max_pos) *max_pos = carry.max_position;
  if (o->verbose) fprintf (stderr, "%s: %zu bytes in %u piece(s); %llu words in %llu sequences\n", t->id, t->size, pieces, (unsigned long long) n_words, (unsigned long long) n_subs);
  in->n_subseqs = n_subs;
  in->subseqs = subs;
  return n_words;
}

/* n 64-bit words of device memory behind what the file holds */
static int write_device_words (gt4hip_context *ctx, FILE *f, const uint64_t *d, uint64_t n, uint64_t *buf)
{
  for (uint64_t first = 0; first < n; first += DOWNLOAD_CHUNK) {
    const uint64_t cnt = n - first < DOWNLOAD_CHUNK ? n - first : DOWNLOAD_CHUNK;
    if (gt4hip_words_download (ctx, d + first, cnt, buf)) {
      fprintf (stderr, "Error: reading results back from the GPU failed: %s\n", gt4hip_last_error (ctx));
      return 1;
    }
    if (fwrite (buf, 8, cnt, f) != cnt) return 1;
  }
  return 0;
}

static int make_index (const Options *o, gt4hip_context *ctx, Text *texts, uint64_t chunk)
{
  uint64_t text_bytes = 0, free_b = 0, total_b = 0;
  for (unsigned int i = 0; i < o->nfiles; i++) text_bytes += texts[i].size;
  /* a word per byte at the most: 16 bytes each resident, as much again for the sort's other side, and the pieces' staging */
  gt4hip_device_memory (ctx, &free_b, &total_b);
  if (text_bytes > (~0ull >> 6) || text_bytes * 16 > free_b) index_no_room (text_bytes, text_bytes * 16);
  uint64_t *d_words = NULL, *d_raw = NULL;
  if (gt4hip_pairs_reserve (ctx, text_bytes, &d_words, &d_raw)) index_no_room (text_bytes, text_bytes * 16);
  static GT4IndexInput inputs[MAX_FILES];
  static uint64_t first_word[MAX_FILES + 1];
  uint64_t n_pairs = 0, max_pos = 0, max_sub = 0;
  for (unsigned int i = 0; i < o->nfiles; i++) {
    inputs[i].name = o->fnames[i];
    inputs[i].size = texts[i].size;
    first_word[i] = n_pairs;
    n_pairs += file_to_pairs (o, ctx, &texts[i], chunk, d_words, d_raw, n_pairs, text_bytes, &inputs[i], &max_pos);
    if (inputs[i].n_subseqs && inputs[i].n_subseqs - 1 > max_sub) max_sub = inputs[i].n_subseqs - 1;
    text_close (&texts[i]);
  }
  first_word[o->nfiles] = n_pairs;
  const unsigned int fb = bit_size (o->nfiles - 1), sb = bit_size (max_sub), pb = bit_size (max_pos);
  if (fb + sb + pb + 1 > 64) {
    fprintf (stderr, "Error: --index: %u file, %u sequence and %u position bits and the strand do not fit the 64 bits of a location: no index written\n", fb, sb, pb);
    return 1;
  }
  gt4hip_index_arrays idx;
  memset (&idx, 0, sizeof idx);
  if (n_pairs) {
    for (unsigned int i = 0; i < o->nfiles; i++)
      CHK (ctx, gt4hip_pack_locations (ctx, d_raw + first_word[i], first_word[i + 1] - first_word[i], i, sb, pb));
    gt4hip_device_memory (ctx, &free_b, &total_b);
    if (n_pairs * 16 > free_b) index_no_room (text_bytes, text_bytes * 16 + n_pairs * 16);
    if (gt4hip_pairs_to_index (ctx, d_words, d_raw, n_pairs, o->wordlength, o->min, o->max, &idx)) {
      fprintf (stderr, "Error: --index: %s\n", gt4hip_last_error (ctx));
      return 1;
    }
  }
  void *head = NULL;
  size_t head_bytes = 0;
  if (gt4_index_head_build (o->wordlength, n_pairs != 0, idx.n_kmers, idx.n_locations, fb, sb, pb, inputs, o->nfiles, &head, &head_bytes)) {
    fprintf (stderr, "Error: out of memory (file block)\n");
    return 1;
  }
  char out_name[1024], tmp_name[1100];
  snprintf (out_name, sizeof out_name, "%s_%u.index", o->outputname, o->wordlength);
  snprintf (tmp_name, sizeof tmp_name, "%s.tmp", out_name);
  FILE *f = fopen (tmp_name, "wb");
  if (!f) {
    fprintf (stderr, "Cannot create output file %s\n", tmp_name);
    return 1;
  }
  const uint64_t most = idx.n_values > 2 * idx.n_kmers ? idx.n_values : 2 * idx.n_kmers;
  uint64_t *buf = (uint64_t *) malloc ((size_t) (most < DOWNLOAD_CHUNK ? most + 1 : DOWNLOAD_CHUNK) * 8);
  int bad = !buf || fwrite (head, 1, head_bytes, f) != head_bytes;
  if (!bad) bad = write_device_words (ctx, f, idx.d_kmers, 2 * idx.n_kmers, buf);
  if (!bad) bad = write_device_words (ctx, f, idx.d_locations, idx.n_values, buf);
  bad |= fclose (f) != 0;
  free (buf);
  free (head);
  if (bad) {
    fprintf (stderr, "Error: writing %s failed\n", tmp_name);
    unlink (tmp_name);
    return 1;
  }
  if (rename (tmp_name, out_name)) fprintf (stderr, "Cannot rename %s to %s\n", tmp_name, out_name);
  gt4hip_index_free (ctx);
  gt4hip_pairs_release (ctx);
  gt4hip_locations_free (ctx);
  for (unsigned int i = 0; i < o->nfiles; i++) free ((void *) inputs[i].subseqs);
  gt4hip_destroy (ctx);
  return 0;
}

int main (int argc, const char *argv[])
{
  static Options o;
  read_environment (&o);
  parse_argv (argc, argv, &o);
  validate (&o);
  if (o.create_index)
    for (unsigned int i = 0; i < o.nfiles; i++)
      if (!strcmp (o.fnames[i], "-")) {
        fprintf (stderr, "Error: --index does not read standard input: the index records every input file's name and size\n");
        return 1;
      }
  static Text texts[MAX_FILES];
  for (unsigned int i = 0; i < o.nfiles; i++) text_open (&o, o.fnames[i], &texts[i]);
  gt4hip_context *ctx = NULL;
  if (gt4hip_create (o.device, &ctx)) {
    fprintf (stderr, "Error: %sno usable GPU: %s\n", o.create_index ? "--index: " : "", gt4hip_last_error (NULL));
    return 1;
  }
  uint64_t chunk = o.chunk;
  if (!chunk) {
    uint64_t free_b = 0, total_b = 0;
    gt4hip_device_memory (ctx, &free_b, &total_b);
    chunk = free_b / 64;
    if (chunk > (1ull << 30)) chunk = 1ull << 30;
    if (chunk < (1ull << 20)) chunk = 1ull << 20;
  }
  if (o.verbose) fprintf (stderr, "Device: %s; pieces of %llu bytes\n", gt4hip_device_info (ctx), (unsigned long long) chunk);
  if (o.create_index) return make_index (&o, ctx, texts, chunk);
  static Lists ls;
  for (unsigned int i = 0; i < o.nfiles; i++) {
    file_to_lists (&o, ctx, &texts[i], chunk, &ls);
    text_close (&texts[i]);
  }
  gt4hip_list *result = collate (ctx, &ls);
  char out_name[1024];
  snprintf (out_name, sizeof out_name, "%s_%u.list", o.outputname, o.wordlength);
  /* no word at all: a header alone (reference :341-348); a rename that fails is reported and the run ends with 0, as there */
  const uint64_t n_words = result ? gt4hip_list_n_words (result) : 0;
  uint64_t total_count = 0;
  if (n_words && gt4hip_list_sum_counts (ctx, result, &total_count)) return 1;
  if (gt4_cli_write_list_file (ctx, result, o.wordlength, n_words, total_count, out_name, 0666, "") == 1) return 1;
  if (result) gt4hip_list_free (result);
  gt4hip_destroy (ctx);
  return 0;
}
