/*
 * gt4_gmer_counter_cli.c -- `gmer_counter`, the drop-in command line that counts the k-mers of a database in FastA /
 * FastQ reads (the counting half of FastGT; reference src/gmer_counter.c, src/database.c:20-282).  Host C; the reads go
 * through HBM in pieces and everything behind that -- the reader, the lookup of every word, the counters, the --stats
 * sums -- runs in the HIP kernels behind include/gt4hip.h (gt4hip_maker.hip, gt4hip_gmer.hip).
 *
 * Stages: parse argv; parse the database text on the host (names, node table, words); create the context and the
 * device db; stream every file in pieces; download, clamp and print.  Same argv grammar, messages, header lines,
 * columns and exit codes as the reference's main() (:135-450) and print_counts (:625-711).  The counters are 64-bit on
 * the device and are clamped here to 65535, or to 0xffffffff with -32, which is where the reference stops counting
 * (:791-795).  --num_threads, --prefetch, -D and -DDB are accepted and do nothing (the -D timing lines on stderr are not
 * reproduced).  The database parser restates the reference's, its line counter's comparison of a BYTE with the file
 * size included (src/database.c:68): a database under 256 bytes is "not text-format" there unless all its bytes are
 * smaller than its size, and so it is here.
 * Deliberate differences, all one "Error: ..." line + exit 1, before any device is touched:
 *   - -dbb, -w, --compile_index, --export_reads, --dump_index, --count_trie_allocations: binary databases (a 2 GB trie
 *     image whatever the database holds) and the read index are not built;
 *   - sequence files without -db (the reference dereferences a null database);
 *   - the same canonical k-mer twice in the database (the reference loses most counts behind "Count too big");
 *   - a node line with fewer k-mers than it declares, or a k-mer shorter than the word length or with a character that
 *     is no base (the reference goes on with shifted node numbers, or with whatever the bytes encode);
 *   - a first node line without a k-mer, a word length above 32, a database whose last byte is no newline (the
 *     reference reads behind the file);
 *   - --double_median with an odd number of k-mers in the last node (the reference reads behind its counters);
 *   - gzip input (by its magic bytes) and standard input ('-').
 * A reader error is fatal with the reference's two lines; --recover is accepted, but the reference's carrying on behind
 * the error is not reproduced: one more line says so.  Without a usable GPU the program fails: there is no CPU path.
 * Environment, all of it read in read_environment():
 *   GT4HIP_GMER_CHUNK=<bytes>[K|M|G]  bytes of text per piece (default: 1/64 of the free device memory, at most 1 GiB),
 *                                     cut behind a '\n' where the second half of the chunk has one;
 *   GT4HIP_DEVICE=N, GT4HIP_VERBOSE=1 as in the other tools.
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

static const char *const HELP_LINES[] = {
  "Usage:",
  "  gmer_counter ARGUMENTS SEQUENCES...",
  "Arguments:",
  "    -v | --version   - Print version information and exit",
  "    -db DATABASE     - SNP/KMER database file",
  "    -dbb DBBINARY    - binary database file",
  "    -w FILENAME      - write binary database to file",
  "    -32              - use 32-bit integeres for counts (default 16-bit)",
  "    --max_kmers NUM  - maximum number of kmers per node",
  "    --silent         - do not print kmer counts (default for index and binary database compilation)",
  "    --verbose        - print kmer counts (default for counting)",
  "    --header         - print header row",
  "    --total          - print the total number of kmers per node",
  "    --unique         - print the number of nonzero kmers per node",
  "    --kmers          - print individual kmer counts (default if no other output)",
  "    --compile_index FILENAME - Add read index to database and write it to file",
  "    --distribution NUM  - print kmer distribution (up to given number)",
  "    --num_threads    - number of worker threads (default 24)",
  "    --prefetch       - prefetch memory mapped files (faster on high-memory systems)",
  "    --recover        - recover from FastA/FastQ errors (useful for corrupted streams)",
  "    --stats          - print some statistics about sequence and kmers",
  "    -D               - increase debug level",
  "    -DDB             - increase database debug level",
};

typedef struct {
  const char *seqnames[MAX_FILES];
  unsigned int nseqs;
  const char *db_name, *dbb, *wdb, *index_name;
  const char *refused; /* the first option given that this program does not implement */
  unsigned int max_kmers_per_node;
  unsigned int silent, verbose, big, dm, header, total, unique, kmers, distro, recover, stats;
  /* environment */
  uint64_t chunk;
  int device, env_verbose;
} Options;

static void print_usage (FILE *to) { gt4_cli_print_help (to, "gmer_counter", HELP_LINES, sizeof HELP_LINES / sizeof HELP_LINES[0]); }

/* every environment variable of the program, once */
static void read_environment (Options *o)
{
  o->chunk = gt4_cli_parse_bytes (getenv ("GT4HIP_GMER_CHUNK"));
  gt4_cli_read_environment (&o->device, &o->env_verbose);
}

/* the value behind an option, or the usage on stderr and exit 1 (reference :165-168) */
static const char *value_arg (int argc, const char *argv[], int *i)
{
  if (++*i >= argc) {
    print_usage (stderr);
    exit (1);
  }
  return argv[*i];
}

/* argv (reference :155-257) */
static void parse_argv (int argc, const char *argv[], Options *o)
{
  o->max_kmers_per_node = 1000000000;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp (a, "-v") || !strcmp (a, "--version")) {
      gt4_cli_print_version (stdout, "gmer_counter");
      exit (0);
    } else if (!strcmp (a, "-h") || !strcmp (a, "--help")) {
      print_usage (stdout);
      exit (0);
    } else if (!strcmp (a, "-db")) {
      o->db_name = value_arg (argc, argv, &i);
    } else if (!strcmp (a, "-dbb")) {
      o->dbb = value_arg (argc, argv, &i);
      if (!o->refused) o->refused = a;
    } else if (!strcmp (a, "-w")) {
      o->wdb = value_arg (argc, argv, &i);
      if (!o->refused) o->refused = a;
    } else if (!strcmp (a, "--max_kmers")) {
      o->max_kmers_per_node = (unsigned int) strtol (value_arg (argc, argv, &i), NULL, 10);
    } else if (!strcmp (a, "--silent")) {
      o->silent = 1;
    } else if (!strcmp (a, "--verbose")) {
      o->verbose = 1;
    } else if (!strcmp (a, "--header")) {
      o->header = 1;
    } else if (!strcmp (a, "--total")) {
      o->total = 1;
    } else if (!strcmp (a, "--unique")) {
      o->unique = 1;
    } else if (!strcmp (a, "--kmers")) {
      o->kmers = 1;
    } else if (!strcmp (a, "-32")) {
      o->big = 1;
    } else if (!strcmp (a, "--double_median")) {
      o->dm = 1;
    } else if (!strcmp (a, "--compile_index")) {
      o->index_name = value_arg (argc, argv, &i);
      if (!o->refused) o->refused = a;
    } else if (!strcmp (a, "--export_reads") || !strcmp (a, "--count_trie_allocations") || !strcmp (a, "--dump_index")) {
      if (!o->refused) o->refused = a;
    } else if (!strcmp (a, "--distribution")) {
      o->distro = (unsigned int) strtol (value_arg (argc, argv, &i), NULL, 10);
    } else if (!strcmp (a, "--num_threads")) {
      (void) value_arg (argc, argv, &i);
    } else if (!strcmp (a, "--prefetch") || !strcmp (a, "-D") || !strcmp (a, "-DDB")) {
      /* accepted, nothing to do */
    } else if (!strcmp (a, "--recover")) {
      o->recover = 1;
    } else if (!strcmp (a, "--stats") || !strcmp (a, "-stat")) {
      o->stats = 1;
    } else {
      if (o->nseqs >= MAX_FILES) {
        fprintf (stderr, "Maximum number of input sequence files is 1024\n");
        exit (1);
      }
      o->seqnames[o->nseqs++] = a;
    }
  }
}

/* reference :259-282, then what this program refuses */
static void validate (Options *o)
{
  if (!o->nseqs && !o->wdb) {
    fprintf (stderr, "Nothing to do!\n");
    print_usage (stderr);
    exit (1);
  }
  if (o->db_name && o->dbb) {
    fprintf (stderr, "Both text and binary database specifed\n");
    print_usage (stderr);
    exit (1);
  }
  if (o->dbb && o->wdb) {
    fprintf (stderr, "Binary database read and written\n");
    print_usage (stderr);
    exit (1);
  }
  if (!o->total && !o->unique && !o->distro) o->kmers = 1;
  if (o->distro > 65536) o->distro = 65536;
  if (o->refused) {
    fprintf (stderr, "Error: %s is not supported: binary databases and the read index are not built by this program (use -db with a text database)\n", o->refused);
    exit (1);
  }
  if (!o->db_name) {
    fprintf (stderr, "Error: no database: give -db DATABASE (sequence files alone cannot be counted)\n");
    exit (1);
  }
  for (unsigned int i = 0; i < o->nseqs; i++)
    if (!strcmp (o->seqnames[i], "-")) {
      fprintf (stderr, "Error: - (standard input) is not read: give the sequence files by name\n");
      exit (1);
    }
}

/* ------------------------------------------------------------------ the text database */

typedef struct {
  unsigned int wordsize;
  uint64_t n_nodes, n_kmers;
  char *names;          /* the names, each with its NUL */
  uint64_t *name;       /* per node: where its name starts */
  uint64_t *first;      /* per node: index of its first k-mer */
  unsigned int *nkmers; /* per node */
  uint64_t *words;      /* per k-mer, as written (either strand) */
} Db;

static void db_refuse (const char *db_name, const char *fmt, unsigned long long a, unsigned long long b)
{
  fprintf (stderr, "Error: %s: ", db_name);
  fprintf (stderr, fmt, a, b);
  fprintf (stderr, "\n");
  exit (1);
}

/* split_line (reference src/utils.c:233-248): up to `max` tokens of the line at c + s, parted by any byte < ' ' */
static unsigned int split_line (const unsigned char *c, uint64_t s, uint64_t n, uint64_t tok[], unsigned int len[], unsigned int max)
{
  unsigned int i = 0;
  while (i < max && c[s] != '\n') {
    uint64_t e = s;
    tok[i] = s;
    while (e < n && c[e] >= ' ') e++;
    len[i] = (unsigned int) (e - s);
    i++;
    s = e;
    if (c[s] != '\n') s++;
  }
  return i;
}

static unsigned int get_bits (unsigned int value)
{
  unsigned int bits = 0;
  for (; value > 0; value /= 2) bits++;
  return bits;
}

static int base_value (unsigned char ch)
{
  switch (ch | 0x20) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't':
    case 'u': return 3;
    default: return -1;
  }
}

static uint64_t reverse_complement (uint64_t w, unsigned int k)
{
  uint64_t r = 0;
  for (unsigned int i = 0; i < k; i++, w >>= 2) r = (r << 2) | (~w & 3);
  return r;
}

typedef struct { uint64_t word, idx; } WordIdx;
static int cmp_word_idx (const void *a, const void *b)
{
  const WordIdx *x = (const WordIdx *) a, *y = (const WordIdx *) b;
  if (x->word != y->word) return x->word < y->word ? -1 : 1;
  return x->idx < y->idx ? -1 : x->idx > y->idx;
}

/* gt4_gmer_db_new_from_text (reference src/database.c:94-282).  0: made; 1: the reference's "db == NULL" (its messages
 * are printed, the caller adds its own); what the reference misreads is refused with exit 1.
 * c holds n bytes and a NUL behind them; c[n - 1] == '\n' is checked first, so no line runs into the end. */
static int parse_db (const char *db_name, const unsigned char *c, uint64_t n, unsigned int max_kmers_per_node, Db *db)
{
  memset (db, 0, sizeof *db);
  if (n < 8) return 1;
  if (!c[5] || !c[7]) return 1;
  if (c[n - 1] != '\n') db_refuse (db_name, "the database does not end with a newline (byte %llu of %llu)", n - 1, n);
  /* count_lines_from_text (:20-82), the byte < csize comparison of :68 as it stands */
  uint64_t tok[3];
  unsigned int len[3];
  unsigned int n_lines = 0, wordsize = 0, sum_kmers = 0, max_kmers = 0;
  for (uint64_t cpos = 0; cpos < n;) {
    if (c[cpos] == '#') {
      while (cpos < n && c[cpos] != '\n') cpos++;
      if (cpos < n) cpos++;
      continue;
    }
    const unsigned int ntok = split_line (c, cpos, n, tok, len, 3);
    if (ntok < 2) {
      fprintf (stderr, "Line %u has <2 (%u) tokens\n", n_lines, ntok);
      n_lines = 0;
      break;
    }
    if (!n_lines) {
      if (ntok < 3 || !len[2]) db_refuse (db_name, "the first node line holds no k-mer: the word length is the length of its third token", 0, 0);
      if (len[2] > 32) db_refuse (db_name, "k-mers of %llu bases: at most 32 fit a word", len[2], 0);
      wordsize = len[2];
    }
    const unsigned int node_n_kmers = (unsigned int) strtol ((const char *) c + tok[1], NULL, 10);
    sum_kmers += node_n_kmers;
    if (node_n_kmers > max_kmers) max_kmers = node_n_kmers;
    while (c[cpos] < n && c[cpos] != '\n') cpos++;
    if (cpos < n) cpos++;
    n_lines++;
  }
  (void) sum_kmers;
  if (!n_lines) {
    fprintf (stderr, "File is not text-format kmer database (maybe binary?)\n");
    return 1;
  }
  if (max_kmers > max_kmers_per_node) max_kmers = max_kmers_per_node;
  const unsigned int node_bits = get_bits (n_lines + 1), kmer_bits = get_bits (max_kmers);
  if (node_bits + kmer_bits > 31) {
    fprintf (stderr, "Too many nodes and kmers (%u (%u bits), %u (%u bits)\n", n_lines + 1, node_bits, max_kmers, kmer_bits);
    return 1;
  }
  /* the fill pass (:164-259): lines, not bytes, from here on */
  uint64_t lines = 0, kmers = 0, names_size = 0;
  for (uint64_t cpos = 0; cpos < n;) {
    if (c[cpos] != '#') {
      const unsigned int ntok = split_line (c, cpos, n, tok, len, 3);
      if (ntok < 2) db_refuse (db_name, "node line %llu has fewer than 2 tokens", lines, 0);
      const long nk = strtol ((const char *) c + tok[1], NULL, 10);
      if (nk < 0) db_refuse (db_name, "node line %llu declares a negative number of k-mers", lines, 0);
      kmers += (uint64_t) nk < max_kmers_per_node ? (uint64_t) nk : max_kmers_per_node;
      names_size += len[0] + 1;
      lines++;
    }
    while (c[cpos] != '\n') cpos++;
    cpos++;
  }
  if (kmers >= (1ull << 32)) db_refuse (db_name, "%llu k-mers: more than 2^32 - 1", kmers, 0);
  db->wordsize = wordsize;
  db->names = (char *) calloc (names_size + 1, 1);
  db->name = (uint64_t *) malloc ((lines + 1) * sizeof (uint64_t));
  db->first = (uint64_t *) malloc ((lines + 1) * sizeof (uint64_t));
  db->nkmers = (unsigned int *) malloc ((lines + 1) * sizeof (unsigned int));
  db->words = (uint64_t *) malloc ((kmers + 1) * sizeof (uint64_t));
  if (!db->names || !db->name || !db->first || !db->nkmers || !db->words) db_refuse (db_name, "out of memory (%llu nodes, %llu k-mers)", lines, kmers);
  uint64_t idx = 0, kpos = 0, npos = 0;
  for (uint64_t cpos = 0; cpos < n;) {
    if (c[cpos] != '#') {
      const unsigned int ntok = split_line (c, cpos, n, tok, len, 3);
      const long nk = strtol ((const char *) c + tok[1], NULL, 10);
      const unsigned int nkm = (uint64_t) nk < max_kmers_per_node ? (unsigned int) nk : max_kmers_per_node;
      db->name[idx] = npos;
      memcpy (db->names + npos, c + tok[0], len[0]);
      npos += len[0] + 1;
      db->first[idx] = kpos;
      db->nkmers[idx] = nkm;
      if (ntok > 2) cpos = tok[2];
      for (unsigned int i = 0; i < nkm; i++) {
        while (c[cpos] < ' ' && c[cpos] != '\n') cpos++;
        if (ntok < 3 || c[cpos] == '\n') db_refuse (db_name, "node %llu holds %llu k-mers, fewer than it declares", idx, i);
        uint64_t w = 0;
        for (unsigned int j = 0; j < wordsize; j++) {
          const int v = base_value (c[cpos + j]); /* ('\n' and the NUL behind the text are no bases) */
          if (v < 0) db_refuse (db_name, "node %llu, k-mer %llu: shorter than the word length, or a character that is no base", idx, i);
          w = (w << 2) | (uint64_t) v;
        }
        db->words[kpos++] = w;
        while (c[cpos] >= ' ') cpos++;
      }
      idx++;
    }
    while (c[cpos] != '\n') cpos++;
    cpos++;
  }
  db->n_nodes = idx;
  db->n_kmers = kpos;
  /* the same canonical word twice */
  if (kpos) {
    WordIdx *s = (WordIdx *) malloc (kpos * sizeof *s);
    if (!s) db_refuse (db_name, "out of memory (%llu k-mers)", kpos, 0);
    for (uint64_t i = 0; i < kpos; i++) {
      const uint64_t w = db->words[i], r = reverse_complement (w, wordsize);
      s[i].word = r < w ? r : w;
      s[i].idx = i;
    }
    qsort (s, kpos, sizeof *s, cmp_word_idx);
    for (uint64_t i = 1; i < kpos; i++)
      if (s[i].word == s[i - 1].word) db_refuse (db_name, "k-mers %llu and %llu (counted from 0 over the whole database) are the same canonical word", s[i - 1].idx, s[i].idx);
    free (s);
  }
  return 0;
}

/* the database file with a NUL behind it; the reference's messages for a file that cannot be mapped (gt4_mmap, src/utils.c:36-64) */
static unsigned char *read_db_file (const char *name, uint64_t *size)
{
  struct stat st;
  if (stat (name, &st) < 0) {
    fprintf (stderr, "gt4_mmap (stat): %s\n", strerror (errno));
    return NULL;
  }
  const int fd = open (name, O_RDONLY);
  if (fd < 0) {
    fprintf (stderr, "gt4_mmap (open): %s\n", strerror (errno));
    return NULL;
  }
  if (!st.st_size) {
    close (fd);
    fprintf (stderr, "gt4_mmap (mmap): %s\n", strerror (EINVAL));
    return NULL;
  }
  unsigned char *b = (unsigned char *) malloc ((size_t) st.st_size + 1);
  size_t got = 0;
  while (b && got < (size_t) st.st_size) {
    const ssize_t r = read (fd, b + got, (size_t) st.st_size - got);
    if (r <= 0) break;
    got += (size_t) r;
  }
  close (fd);
  if (!b || got != (size_t) st.st_size) {
    fprintf (stderr, "gt4_mmap (mmap): %s\n", strerror (b ? EIO : ENOMEM));
    free (b);
    return NULL;
  }
  b[got] = 0;
  *size = got;
  return b;
}

/* ------------------------------------------------------------------ the reads */

typedef struct {
  const unsigned char *data;
  size_t size;
  const char *id; /* the reader's name in the reference's messages: the file's */
} Text;

static void reader_error_exit (const Options *o, const Text *t)
{
  fprintf (stderr, "read_file: Fasta reader %s returned 4294967295\n", t->id);
  if (o->recover) fprintf (stderr, "Error: --recover is not honoured: nothing is counted behind a reader error\n");
  exit (1);
}

static void text_open (const Options *o, const char *name, Text *t)
{
  memset (t, 0, sizeof *t);
  t->id = name;
  const int fd = open (name, O_RDONLY);
  struct stat s;
  if (fd < 0 || fstat (fd, &s)) {
    fprintf (stderr, "fasta_reader_read_nwords: Reader %s read error (-1) at 0\n", name);
    reader_error_exit (o, t);
  }
  t->size = (size_t) s.st_size;
  if (t->size) {
    void *p = mmap (NULL, t->size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (p == MAP_FAILED) {
      fprintf (stderr, "Error: cannot map %s: %s\n", name, strerror (errno));
      exit (1);
    }
    t->data = (const unsigned char *) p;
  }
  close (fd);
  if (t->size >= 2 && gt4_cli_refuse_gzip (name, t->data[0], t->data[1])) exit (1);
}

/* the reference's line for a reader error (src/fasta.c:136, :202, :211, :277) and read_file's behind it; exit 1 */
static void format_error_exit (const Options *o, const Text *t, uint32_t kind, uint64_t at)
{
  const int found = at < t->size ? t->data[at] : 0;
  const unsigned long long cpos = at ? at - 1 : 0;
  switch (kind) {
    case GT4HIP_MAKER_ERR_START: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid start tag '%c'\n", t->id, found); break;
    case GT4HIP_MAKER_ERR_PLUS: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '+' missing, found '%c' instead at %llu\n", t->id, found, cpos); break;
    case GT4HIP_MAKER_ERR_AT: fprintf (stderr, "fasta_reader_read_nwords: Reader %s tag '@' missing, found '%c' instead at %llu\n", t->id, found, cpos); break;
    default: fprintf (stderr, "fasta_reader_read_nwords: Reader %s invalid character '%c' after '+' %llu\n", t->id, found, (unsigned long long) at); break;
  }
  reader_error_exit (o, t);
}

/* one file through the device, a piece at a time; what the pieces gave is added to `sum` */
static void count_file (const Options *o, gt4hip_context *ctx, gt4hip_gmer_db *gdb, const Text *t, uint64_t chunk, gt4hip_gmer_stats *sum)
{
  gt4hip_maker_carry carry, next;
  int have = 0;
  size_t pos = 0;
  unsigned int pieces = 0;
  while (pos < t->size) {
    size_t len = t->size - pos;
    if (len > chunk) {
      len = (size_t) chunk;
      /* behind the last '\n' of the chunk's second half, where there is one */
      const unsigned char *nl = (const unsigned char *) memrchr (t->data + pos + len / 2, '\n', len - len / 2);
      if (nl) len = (size_t) (nl - (t->data + pos)) + 1;
    }
    gt4hip_gmer_stats st;
    uint64_t at = 0;
    memset (&st, 0, sizeof st);
    const int rc = gt4hip_gmer_count_text (ctx, gdb, t->data + pos, len, 0, have ? &carry : NULL, &next, &st, &at);
    if (rc == GT4HIP_EFORMAT) format_error_exit (o, t, next.error, pos + at);
    if (rc) {
      fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
      exit (1);
    }
    sum->n_n += st.n_n, sum->n_nucl += st.n_nucl, sum->n_gc += st.n_gc;
    sum->n_words += st.n_words, sum->n_hits += st.n_hits, sum->n_kmer_gc += st.n_kmer_gc;
    carry = next;
    have = 1;
    pos += len;
    pieces++;
    if (o->env_verbose && pos < t->size) fprintf (stderr, "%s: piece %u ends at byte %zu\n", t->id, pieces, pos);
    if (carry.ended) break;
  }
  /* the end of the file behind a FastQ sequence line or inside a '+' line (src/fasta.c:200-213) */
  if (have && !carry.ended && carry.file_type == GT4HIP_MAKER_FASTQ && carry.line_phase == 2)
    format_error_exit (o, t, carry.at_line_start ? GT4HIP_MAKER_ERR_PLUS : GT4HIP_MAKER_ERR_PLUS_EOF, t->size);
  if (o->env_verbose) fprintf (stderr, "%s: %zu bytes in %u piece(s)\n", t->id, t->size, pieces);
}

/* ------------------------------------------------------------------ output */

/* the counters as the reference holds them: kmers_16 and kmers_32 are one union (src/database.h:38-41) */
typedef struct {
  unsigned int count_bits;
  uint64_t n;
  unsigned short *k16; /* count_bits 32: the same bytes as k32, which is how --unique reads them (:655-659) */
  unsigned int *k32;
} Counts;

static unsigned int count_at (const Counts *c, uint64_t i) { return c->count_bits == 16 ? c->k16[i] : c->k32[i]; }

static int compare_counts (const void *lhs, const void *rhs)
{
  const unsigned int a = *(const unsigned int *) lhs, b = *(const unsigned int *) rhs;
  return a < b ? -1 : a > b;
}

/* get_pair_median (reference :945-1005) */
static unsigned int get_pair_median (const Db *db, const Counts *c)
{
  unsigned int total = 0, min = 0xffffffff, max = 0, med;
  for (uint64_t i = 0; i < db->n_nodes; i++) {
    total += db->nkmers[i] / 2;
    for (unsigned int j = 0; j < db->nkmers[i]; j += 2) {
      const unsigned int sum = count_at (c, db->first[i] + j) + count_at (c, db->first[i] + j + 1);
      if (sum > max) max = sum;
      if (sum < min) min = sum;
    }
  }
  med = (min + max) / 2;
  while (max > min) {
    unsigned int above = 0, below = 0, equal;
    for (uint64_t i = 0; i < db->n_nodes; i++)
      for (unsigned int j = 0; j < db->nkmers[i]; j += 2) {
        const unsigned int sum = count_at (c, db->first[i] + j) + count_at (c, db->first[i] + j + 1);
        if (sum > med) above += 1;
        if (sum < med) below += 1;
      }
    equal = total - above - below;
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
    med = (min + max) / 2;
  }
  return med;
}

/* print_counts (reference :625-711) */
static void print_counts (const Options *o, const Db *db, const Counts *c)
{
  if (o->header) {
    fprintf (stdout, "NODE\tN_KMERS");
    if (o->total) fprintf (stdout, "\tTOTAL");
    if (o->unique) fprintf (stdout, "\tUNIQUE");
    if (o->kmers) fprintf (stdout, "\tKMERS");
    if (o->distro) fprintf (stdout, "\tDISTRIBUTION");
    fprintf (stdout, "\n");
  }
  unsigned int *sorted = NULL, sorted_len = 0;
  for (uint64_t i = 0; i < db->n_nodes; i++) {
    const unsigned int nk = db->nkmers[i];
    const uint64_t first = db->first[i];
    fprintf (stdout, "%s\t%u", db->names + db->name[i], nk);
    if (o->total) {
      unsigned long long total = 0;
      for (unsigned int j = 0; j < nk; j++) total += count_at (c, first + j);
      fprintf (stdout, "\t%llu", total);
    }
    if (o->unique) {
      unsigned int uniq = 0;
      for (unsigned int j = 0; j < nk; j++)
        if (c->k16[first + j]) uniq += 1; /* (with -32 as well: the reference reads the 32-bit counters as 16-bit ones) */
      fprintf (stdout, "\t%u", uniq);
    }
    if (o->kmers)
      for (unsigned int j = 0; j < nk; j++) fprintf (stdout, "\t%u", count_at (c, first + j));
    if (o->distro) {
      if (sorted_len < nk) {
        sorted_len = nk;
        sorted = (unsigned int *) realloc (sorted, (size_t) sorted_len * 4);
      }
      for (unsigned int j = 0; j < nk; j++) sorted[j] = count_at (c, first + j);
      qsort (sorted, nk, 4, compare_counts);
      unsigned int j = 0;
      for (unsigned int current = 0; current <= o->distro; current++) {
        unsigned int count = 0;
        while (j < nk && sorted[j] == current) count++, j++;
        fprintf (stdout, "\t%u", count);
      }
    }
    fprintf (stdout, "\n");
  }
  free (sorted);
}

int main (int argc, const char *argv[])
{
  static Options o;
  read_environment (&o);
  parse_argv (argc, argv, &o);
  validate (&o);
  /* the database, on the host */
  uint64_t db_size = 0;
  unsigned char *db_text = read_db_file (o.db_name, &db_size);
  if (!db_text) {
    fprintf (stderr, "Cannot mmap database file %s\n", o.db_name);
    return 1;
  }
  static Db db;
  if (parse_db (o.db_name, db_text, db_size, o.max_kmers_per_node, &db)) {
    fprintf (stderr, "Cannot read text database (null)\n"); /* (the reference prints its unset -dbb name here, :305) */
    return 1;
  }
  free (db_text);
  uint64_t last = db.n_nodes;
  while (last && !db.nkmers[last - 1]) last--;
  if (o.dm && last && (db.nkmers[last - 1] & 1)) {
    fprintf (stderr, "Error: --double_median: the last node holds an odd number of k-mers (the reference pairs the last one with what lies behind its counters)\n");
    return 1;
  }
  static Text texts[MAX_FILES];
  for (unsigned int i = 0; i < o.nseqs; i++) text_open (&o, o.seqnames[i], &texts[i]);
  /* the device */
  gt4hip_context *ctx = NULL;
  if (gt4hip_create (o.device, &ctx)) {
    fprintf (stderr, "Error: no usable GPU: %s\n", gt4hip_last_error (NULL));
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
  if (o.env_verbose) fprintf (stderr, "Device: %s; pieces of %llu bytes; %llu nodes, %llu k-mers of %u\n", gt4hip_device_info (ctx), (unsigned long long) chunk,
                              (unsigned long long) db.n_nodes, (unsigned long long) db.n_kmers, db.wordsize);
  gt4hip_gmer_db *gdb = NULL;
  if (gt4hip_gmer_db_create (ctx, db.words, db.n_kmers, db.wordsize, &gdb)) {
    fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
    return 1;
  }
  gt4hip_gmer_stats sum;
  memset (&sum, 0, sizeof sum);
  for (unsigned int i = 0; i < o.nseqs; i++) {
    count_file (&o, ctx, gdb, &texts[i], chunk, &sum);
    if (texts[i].size) munmap ((void *) texts[i].data, texts[i].size);
  }
  /* download and clamp */
  Counts c;
  c.count_bits = o.big ? 32 : 16;
  c.n = db.n_kmers;
  c.k32 = (unsigned int *) calloc (db.n_kmers + 1, 4);
  c.k16 = (unsigned short *) c.k32;
  uint64_t *raw = (uint64_t *) malloc ((db.n_kmers + 1) * 8);
  if (!c.k32 || !raw) {
    fprintf (stderr, "Error: out of memory (%llu counters)\n", (unsigned long long) db.n_kmers);
    return 1;
  }
  CHK (ctx, gt4hip_gmer_counts_download (ctx, gdb, 0, db.n_kmers, raw));
  for (uint64_t i = 0; i < db.n_kmers; i++) {
    if (o.big) c.k32[i] = raw[i] < 0xffffffffull ? (unsigned int) raw[i] : 0xffffffffu;
    else c.k16[i] = raw[i] < 65535 ? (unsigned short) raw[i] : 65535;
  }
  free (raw);
  gt4hip_gmer_db_free (gdb);
  gt4hip_destroy (ctx);
  if (!o.silent) {
    fprintf (stdout, "#gmer_counter version %u.%u.%u (%s)\n", GT4_VERSION_MAJOR, GT4_VERSION_MINOR, GT4_VERSION_MICRO, GT4_VERSION_QUALIFIER);
    fprintf (stdout, "#TextDatabase\t%s\n", o.db_name);
    if (o.dm) fprintf (stdout, "#PairMedian\t%u\n", get_pair_median (&db, &c));
    if (o.stats) {
      const unsigned long long n_kmers = sum.n_hits;
      fprintf (stdout, "#LENGTH\t%llu\n", (unsigned long long) (sum.n_nucl + sum.n_n));
      fprintf (stdout, "#LENGTH_ACGT\t%llu\n", (unsigned long long) sum.n_nucl);
      fprintf (stdout, "#GC\t%.3f\n", (double) sum.n_gc / sum.n_nucl);
      fprintf (stdout, "#TOTAL_KMERS\t%llu\n", (unsigned long long) sum.n_words);
      fprintf (stdout, "#LIST_KMERS\t%llu\n", n_kmers);
      fprintf (stdout, "#LIST_KMER_GC\t%.3f\n", (double) sum.n_kmer_gc / (n_kmers * db.wordsize));
    }
    print_counts (&o, &db, &c);
  }
  return 0;
}
