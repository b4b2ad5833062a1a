/*
 * gt4_glistcompare_cli.c -- `glistcompare`, the drop-in command line of the GPU set-operation
 * path.  Host C; every merge runs in the HIP kernels behind include/gt4hip.h.
 *
 * Same argv grammar, defaults, validation order, messages, output names (`<out>_<k>_union.list`
 * ...), tmp + rename discipline, stdout of --count_only / --print_operation / -v and exit codes
 * as the reference's main() (reference src/glistcompare.c:84-429, naming :814-834, :907-953).
 * Deliberate differences, all loud:
 *   - a file that cannot be opened is an error message + exit 1 (the reference dereferences NULL);
 *   - --subset METHOD SIZE (gt4hip_list_subset: the reference's serial selection solved as a fixed point on the GPU, the
 *     same list for the same --seed) runs on one GPU with the list resident, like -mm: --gpus N > 1 or GT4HIP_HBM_LIMIT
 *     are an error + exit 1.  Where fewer than SIZE items are selected behind the last one (rand with SIZE above the sum
 *     of the counts, a rand_weighted_unique walk that falls short) the reference does not terminate: here that is
 *     "Error: ..." with the method, SIZE and the number reached, exit 1 and no output file.  A rename that fails is
 *     exit 1 (the reference reports it and exits 0).  GT4I index inputs are read as the sorted k-mer lists they
 *     contain, as in the reference;
 *   - -mm N (difference up to N mismatches, gt4hip_compare_mismatch) runs on one GPU with both lists
 *     resident: with --gpus N > 1 or GT4HIP_HBM_LIMIT it is an error + exit 1, and inputs that do not fit
 *     the device memory are an out-of-memory error, not a chunked run.  An empty lookup list holds no
 *     neighbour (the reference crashes there); -dd -du computes diff2 as the reference does, without its
 *     assertion message per lookup; -D prints the reference's level-1 lines, not the per-word and
 *     per-probe traces of -D -D and more;
 *   - --stream and --disable_scouts are accepted and ignored (the whole list is uploaded to HBM;
 *     results are identical for well-formed files);
 *   - --gpus N shards the job by key range over N GPUs (one worker process each, forked before any HIP
 *     call; every worker writes its own extents of the output files).  Inputs of 4 GiB and more, or that
 *     do not fit the device memory, stream through the GPU in key-range chunks.  Outputs are
 *     byte-identical to the single-pass run;
 *   - -u --min_lists M [--max_lists X] (not in the reference; gt4hip_select_multi) writes the records of the union -- same
 *     -r rule, same -c cutoff -- whose word lies in at least M and at most X of the N input files, to
 *     <out>_<k>_select_<M>_<X>.list; either option alone is enough (M = 1, X = N otherwise), two files take the N-way path
 *     too.  --count_only prints the two lines of -u --count_only for the selected list; -D adds nothing; --gpus and
 *     GT4HIP_HBM_LIMIT work as for -u.  Before any device is opened, one "Error: ..." line and exit 1 for: the options without
 *     -u or together with -i, -d, -dd, -du, -mm or --subset; M or X that is no integer; M < 1, X < M or X > N;
 *   - L1 .. LN --pairwise (not in the reference; gt4hip_pairwise_multi) takes two or more lists, writes no list file and
 *     prints to stdout the line "#I\tJ\tLIST_I\tLIST_J\tSHARED\tMIN_TOTAL\tUNION\tJACCARD" and one tab-separated line for every
 *     i <= j, in order of i, then j: the two indices from 0, the two file names as given, the words both lists hold with a count
 *     other than 0, the sum over the words of the smaller of the two counts (for i != j the NUnique and NTotal of
 *     `Li Lj -i --count_only`), the size of the union of the two, and shared / union with %.6f (0 where the union is empty).
 *     The lines with i = j give a list's words and the sum of its counts.  A stored record with count 0 is the same as
 *     absence, as for --min_lists: the count table cannot tell the two apart.  All lists and their count table are resident
 *     on one GPU: a job that does not fit, GT4HIP_HBM_LIMIT and GT4HIP_GPUS above 1 are refused with a message and exit 1 (the
 *     matrices are additive over key ranges: chunks and --gpus can follow); -D adds nothing.  Before any device is opened, one
 *     "Error: ..." line and exit 1 for: fewer than two lists; the option together with -u, -i, -d, -dd, -du, -mm, --subset,
 *     --min_lists, --max_lists, -r, -c / --count_cutoff, --count_only or --gpus;
 *   - without a usable GPU the program fails: there is no CPU fallback.
 * Environment, all of it read in read_environment():
 *   GT4HIP_GPUS=N            as --gpus N (which overrides it);
 *   GT4HIP_HBM_LIMIT=<bytes> ([K|M|G]) device bytes a worker holds in flight: key-range chunks (gt4_shard.c);
 *   GT4HIP_PIPELINE=0        inputs of 4 GiB and more stay in one piece as long as they fit the device;
 *   GT4HIP_GATHER=rccl       the shards of several GPUs are gathered on worker 0 over RCCL;
 *   GT4HIP_CHECK_SORTED=1    rejects an input that is not strictly ascending (the reference trusts it);
 *   GT4HIP_DEVICE=N          the device of a one-GPU run (default 0);
 *   GT4HIP_VERBOSE=1         prints the device, kernel times and the chunk plan on stderr (-D prints exactly
 *                            what the reference prints).
 */
#define _GNU_SOURCE
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <time.h>
#include <unistd.h>

#include "gt4_cli.h"
#include "gt4_listfile.h"
#include "gt4_shard.h"
#include "gt4hip.h"

#define MAX_FILES 1024

/* Weak: the product links libgt4hip.so, which defines them; the host-only sanitizer build of this file
 * (tests/harness, a CPU stand-in for the device layer) has no -mm, no --subset, no --min_lists and no --pairwise path and leaves
 * them NULL. */
#pragma weak gt4hip_compare_mismatch
#pragma weak gt4hip_mismatch_stats_get
#pragma weak gt4hip_list_subset
#pragma weak gt4hip_select_multi
#pragma weak gt4hip_pairwise_multi

enum { OPT_PLAIN, OPT_VERSION, OPT_HELP, OPT_OUT, OPT_CUTOFF, OPT_MM, OPT_UNION, OPT_INTRSEC, OPT_DIFF, OPT_DDIFF, OPT_DU,
       OPT_COUNT_ONLY, OPT_RULE, OPT_SUBSET, OPT_SEED, OPT_PRINT_OP, OPT_NOSCOUTS, OPT_STREAM, OPT_DEBUG, OPT_GPUS,
       OPT_MIN_LISTS, OPT_MAX_LISTS, OPT_PAIRWISE };

static const GT4CliOption OPTIONS[] = {
  { "-v", OPT_VERSION }, { "--version", OPT_VERSION }, { "-h", OPT_HELP }, { "--help", OPT_HELP }, { "-?", OPT_HELP },
  { "-o", OPT_OUT }, { "--outputname", OPT_OUT }, { "-c", OPT_CUTOFF }, { "--cutoff", OPT_CUTOFF },
  { "--count_cutoff", OPT_CUTOFF }, /* alias used by the benchmark description; not in the reference */
  { "--gpus", OPT_GPUS },           /* not in the reference: key-range shards over several GPUs */
  { "--min_lists", OPT_MIN_LISTS }, { "--max_lists", OPT_MAX_LISTS }, /* not in the reference: -u restricted to the words of M to X lists */
  { "--pairwise", OPT_PAIRWISE },   /* not in the reference: what every list shares with every other one, to stdout */
  { "-mm", OPT_MM }, { "--mismatch", OPT_MM }, { "-u", OPT_UNION }, { "--union", OPT_UNION },
  { "-i", OPT_INTRSEC }, { "--intersection", OPT_INTRSEC }, { "-d", OPT_DIFF }, { "--difference", OPT_DIFF },
  { "-dd", OPT_DDIFF }, { "--double_difference", OPT_DDIFF }, { "-du", OPT_DU }, { "--diff_union", OPT_DU },
  { "--count_only", OPT_COUNT_ONLY }, { "-r", OPT_RULE }, { "--rule", OPT_RULE }, { "-ss", OPT_SUBSET }, { "--subset", OPT_SUBSET },
  { "--seed", OPT_SEED }, { "--print_operation", OPT_PRINT_OP }, { "--disable_scouts", OPT_NOSCOUTS }, { "--stream", OPT_STREAM },
  { "-D", OPT_DEBUG },
};

static const char *const HELP_LINES[] = {
  "Usage: glistcompare INPUTLIST1 [INPUTLIST2...] METHOD [OPTIONS]",
  "Options:",
  "    -v, --version            - print version information and exit",
  "    -h, --help               - print this usage screen and exit",
  "    -u, --union              - union of input lists",
  "    -i, --intersection       - intersection of input lists",
  "    -d, --difference         - difference of input lists",
  "    -dd, --double_difference - double difference of input lists",
  "    -du, --diff_union        - subtract first list from the second and finds difference",
  "    -mm, --mismatch   NUMBER - specify number of mismatches (default 0, can be used with -diff and -ddiff)",
  "    -c, --cutoff NUMBER      - specify frequency cut-off (default 1)",
  "    -o, --outputname STRING  - specify output name (default \"out\")",
  "    -r, --rule STRING        - specify rule how final frequencies are calculated (default, add, subtract, min, max, first, second, 1, 2)",
  "                               NOTE: rules min, subtract, first and second can only be used with finding the intersection.",
  "    -ss, --subset METHOD SIZE - make subset with given method (rand, rand_unique, rand_weighted_unique)",
  "    --seed INTEGER           - Set seed of random number generator (default uses start time)",
  "    --count_only             - output count of k-mers instead of k-mers themself",
  "    --disable_scouts         - disable list read-ahead in background thread",
  "    --stream                 - read input as stream (do not memory map files)",
  "    -D                       - increase debug level",
};

static void print_help (int exit_value)
{
  gt4_cli_print_help (stdout, "glistcompare", HELP_LINES, sizeof HELP_LINES / sizeof HELP_LINES[0]);
  exit (exit_value);
}

static double now_seconds (void)
{
  struct timeval tv;
  gettimeofday (&tv, NULL);
  return tv.tv_sec + tv.tv_usec * 1e-6;
}

/* What argv and the environment decide.  read_environment and parse_argv fill it, validate settles
 * find_diff; the run_* stages only read it. */
typedef struct {
  const char *fnames[MAX_FILES];
  unsigned int nfiles;
  int rule;
  unsigned int cutoff, nmm, count_override;
  int find_union, find_intrsec, find_diff, find_ddiff, find_subset, subtraction, countonly, print_operation, debug;
  const char *subset_method_name;
  uint32_t subset_method;         /* GT4HIP_SUBSET_* */
  unsigned long long subset_size; /* as the reference holds it: strtoll into an unsigned long long */
  long seed;                      /* --seed; -1 (also when given): the start time */
  int pairwise;                   /* --pairwise */
  int have_rule, have_cutoff, have_gpus; /* -r, -c and --gpus were given (check_pairwise) */
  int select;                     /* --min_lists and / or --max_lists */
  int have_min, have_max;
  long long min_lists, max_lists; /* as given; check_select settles the defaults (1, the number of files) */
  const char *outputname;
  /* environment */
  int n_gpus;         /* GT4HIP_GPUS, or --gpus N */
  int verbose;        /* lines of this implementation's own (device, kernel times, chunk plan): -D stays the reference's transcript */
  uint64_t hbm_limit; /* bytes; 0: none given */
  int pipeline_off, gather_rccl, check_sorted;
  int device;
} Options;

/* every environment variable of the program, once */
static void read_environment (Options *o)
{
  const char *e;
  gt4_cli_read_environment (&o->device, &o->verbose);
  o->n_gpus = (e = getenv ("GT4HIP_GPUS")) ? atoi (e) : 0;
  o->hbm_limit = gt4_cli_parse_bytes (getenv ("GT4HIP_HBM_LIMIT"));
  o->pipeline_off = (e = getenv ("GT4HIP_PIPELINE")) && !atoi (e);
  o->gather_rccl = (e = getenv ("GT4HIP_GATHER")) && !strcmp (e, "rccl");
  o->check_sorted = (e = getenv ("GT4HIP_CHECK_SORTED")) && atoi (e);
}

/* argv (reference :107-230; every quirk of its hand-rolled loop is kept) */
static void parse_argv (int argc, const char *argv[], Options *o)
{
  int stream = 0;
  char *end;
  o->rule = GT4HIP_RULE_DEFAULT;
  o->cutoff = 1;
  o->count_override = 1;
  o->outputname = "out";
  o->seed = -1;
  for (int i = 1; i < argc; i++) {
    const char *arg = argv[i];
    if (arg[0] != '-') {
      if (o->nfiles >= MAX_FILES) {
        fprintf (stderr, "Too many file arguments (max %d)\n", MAX_FILES);
        print_help (1);
      }
      o->fnames[o->nfiles++] = arg;
      continue;
    }
    switch (gt4_cli_find_option (OPTIONS, sizeof OPTIONS / sizeof OPTIONS[0], arg)) {
      case OPT_VERSION:
        gt4_cli_print_version (stdout, "glistcompare");
        exit (0);
      case OPT_HELP:
        print_help (0);
        break;
      case OPT_OUT:
        if (!argv[i + 1] || argv[i + 1][0] == '-') {
          fprintf (stderr, "Warning: No output name specified!\n");
          i += 1; /* the reference skips the next argument here as well */
          break;
        }
        o->outputname = argv[++i];
        break;
      case OPT_CUTOFF:
        o->have_cutoff = 1;
        if (!argv[i + 1]) {
          fprintf (stderr, "Warning: No frequency cut-off specified! Using the default value: %d.\n", o->cutoff);
          break;
        }
        o->cutoff = (unsigned int) strtol (argv[i + 1], &end, 10);
        if (*end != 0) {
          fprintf (stderr, "Error: Invalid frequency cut-off: %s! Must be an integer.\n", argv[i + 1]);
          print_help (1);
        }
        i += 1;
        break;
      case OPT_MM:
        if (!argv[i + 1]) {
          fprintf (stderr, "Warning: No number of mismatches specified!");
          break;
        }
        o->nmm = (unsigned int) strtol (argv[i + 1], &end, 10);
        if (*end != 0) {
          fprintf (stderr, "Error: Invalid number of mismatches: %s! Must be an integer.\n", argv[i + 1]);
          print_help (1);
        }
        i += 1;
        break;
      case OPT_UNION: o->find_union = 1; break;
      case OPT_INTRSEC: o->find_intrsec = 1; break;
      case OPT_DIFF: o->find_diff = 1; break;
      case OPT_DDIFF: o->find_ddiff = 1; break;
      case OPT_DU:
        o->find_diff = 1;
        o->subtraction = 1;
        break;
      case OPT_COUNT_ONLY: o->countonly = 1; break;
      case OPT_RULE: {
        static const struct { const char *name; int rule; } RULES[] = {
          { "default", GT4HIP_RULE_DEFAULT }, { "add", GT4HIP_RULE_ADD }, { "sum", GT4HIP_RULE_ADD }, { "subtract", GT4HIP_RULE_SUBTRACT },
          { "min", GT4HIP_RULE_MIN }, { "max", GT4HIP_RULE_MAX }, { "first", GT4HIP_RULE_FIRST }, { "second", GT4HIP_RULE_SECOND },
        };
        o->have_rule = 1;
        i += 1;
        if (i >= argc) print_help (1);
        if (argv[i][0] >= '1' && argv[i][0] <= '9') {
          o->rule = GT4HIP_RULE_NUMBER;
          o->count_override = (unsigned int) strtol (argv[i], &end, 10);
        } else {
          for (size_t r = 0; r < sizeof RULES / sizeof RULES[0]; r++)
            if (!strcmp (argv[i], RULES[r].name)) o->rule = RULES[r].rule;
          /* an unknown rule name is silently ignored, as in the reference */
        }
        break;
      }
      case OPT_SUBSET:
        o->find_subset = 1;
        i += 1;
        if (i >= argc) print_help (1);
        if (!strcmp (argv[i], "rand")) o->subset_method = GT4HIP_SUBSET_RAND;
        else if (!strcmp (argv[i], "rand_unique")) o->subset_method = GT4HIP_SUBSET_RAND_UNIQUE;
        else if (!strcmp (argv[i], "rand_weighted_unique")) o->subset_method = GT4HIP_SUBSET_RAND_WEIGHTED_UNIQUE;
        else print_help (1);
        o->subset_method_name = argv[i];
        i += 1;
        if (i >= argc) print_help (1);
        o->subset_size = (unsigned long long) strtoll (argv[i], &end, 10);
        if (*end != 0) {
          fprintf (stderr, "Error: Invalid subset size: %s! Must be an integer.\n", argv[i]);
          print_help (1);
        }
        break;
      case OPT_SEED:
        i += 1;
        if (i >= argc) print_help (1);
        o->seed = (long) strtoll (argv[i], &end, 10); /* only --subset draws random numbers */
        break;
      case OPT_PRINT_OP: o->print_operation = 1; break;
      case OPT_NOSCOUTS: break;
      case OPT_STREAM: stream = 1; break;
      case OPT_DEBUG: o->debug += 1; break;
      case OPT_PAIRWISE: o->pairwise = 1; break;
      case OPT_GPUS:
        o->have_gpus = 1;
        i += 1;
        if (i >= argc) print_help (1);
        o->n_gpus = atoi (argv[i]);
        if (o->n_gpus < 1) {
          fprintf (stderr, "Error: Invalid number of GPUs: %s!\n", argv[i]);
          print_help (1);
        }
        break;
      case OPT_MIN_LISTS:
      case OPT_MAX_LISTS: {
        const int is_min = !strcmp (arg, "--min_lists");
        if (!argv[i + 1]) {
          fprintf (stderr, "Error: %s needs a number of lists\n", arg);
          exit (1);
        }
        errno = 0;
        const long long v = strtoll (argv[i + 1], &end, 10);
        if (*end != 0 || end == argv[i + 1] || errno) {
          fprintf (stderr, "Error: Invalid %s: %s! Must be an integer.\n", arg, argv[i + 1]);
          exit (1);
        }
        o->select = 1;
        *(is_min ? &o->have_min : &o->have_max) = 1;
        *(is_min ? &o->min_lists : &o->max_lists) = v;
        i += 1;
        break;
      }
      default:
        fprintf (stderr, "Unknown argument: %s!\n", arg);
        print_help (1);
    }
  }
  if (o->debug) fprintf (stderr, "Rule: %d\n", o->rule);
  if (o->debug) fprintf (stderr, "Num files: %d\n", o->nfiles);
  if ((o->nmm || o->find_subset) && stream) fprintf (stderr, "Warning: Subset and mismatches are incompatible with streaming, using mapping\n");
}

/* Maps the inputs (reference :250-290) and returns their word length; any bad file ends the program */
static unsigned int open_inputs (const Options *o, GT4ListFile *files)
{
  unsigned int wlen = 0, err = 0;
  for (unsigned int f = 0; f < o->nfiles; f++) {
    uint32_t code;
    files[f].file_map = NULL;
    if (gt4_listfile_sniff (o->fnames[f], &code)) {
      fprintf (stderr, "Error: Cannot open %s\n", o->fnames[f]);
      err = 1;
      continue;
    }
    if (code != GT4_LIST_CODE_VALUE && code != GT4_INDEX_CODE_VALUE) {
      /* the reference reports both: no object was made, so the interface lookup fails as well (:272-279) */
      fprintf (stderr, "Error: File %s has unknown format\n", o->fnames[f]);
      fprintf (stderr, "Error: File %s is invalid or corrupted\n", o->fnames[f]);
      err = 1;
      continue;
    }
    /* a GT4I index is read as the sorted (k-mer, number of locations) list it contains (:269-270) */
    if (code == GT4_INDEX_CODE_VALUE ? gt4_indexfile_open (o->fnames[f], GT4_VERSION_MAJOR, &files[f])
                                     : gt4_listfile_open (o->fnames[f], GT4_VERSION_MAJOR, &files[f])) {
      fprintf (stderr, "Error: File %s is invalid or corrupted\n", o->fnames[f]);
      err = 1;
      continue;
    }
    if (!wlen) {
      wlen = files[f].header.word_length;
    } else if (files[f].header.word_length != wlen) {
      fprintf (stderr, "Error: File %s has different word length (%u != %u)\n", o->fnames[f], files[f].header.word_length, wlen);
      err = 1;
    }
  }
  if (err) {
    fprintf (stderr, "Stopping...\n");
    exit (1);
  }
  return wlen;
}

/* validity checks, in the reference's order (:317-352) */
static void validate (Options *o)
{
  if (o->nfiles < 2) {
    fprintf (stderr, "Error: At least 2 list/index files are needed\n");
    exit (1);
  }
  if (o->nfiles > 2) {
    if (!(o->find_union || o->find_intrsec) || o->find_diff || o->find_ddiff) {
      fprintf (stderr, "Error: Algorithm incompatible with multiple files!\n");
      print_help (1);
    }
    if (o->nmm) {
      fprintf (stderr, "Error: Multiple files are not compatible with mismatches!\n");
      print_help (1);
    }
  }
  if (o->find_ddiff) o->find_diff = 1;
  if (!o->find_diff && o->nmm) fprintf (stderr, "Warning: Number of mismatches are not used!\n");
  if (!o->find_diff && o->subtraction) fprintf (stderr, "Warning: Subtraction is not used!\n");
  if (strlen (o->outputname) > 200) {
    fprintf (stderr, "Error: Output name exceeds the 200 character limit.\n");
    exit (1);
  }
  if (!o->find_intrsec && (o->rule == GT4HIP_RULE_MIN || o->rule == GT4HIP_RULE_FIRST || o->rule == GT4HIP_RULE_SECOND)) {
    fprintf (stderr, "Error: Rules min, fist and second can only be used with finding the intersection.\n");
    exit (1);
  }
  if ((!o->find_intrsec && !o->find_diff) && (o->rule == GT4HIP_RULE_SUBTRACT)) {
    fprintf (stderr, "Error: Rule subtract can only be used with intersection and difference.\n");
    exit (1);
  }
  if (o->print_operation) {
    fprintf (stdout, "Operation\t%s%s%s%s\trule\t%u\nFiles\t%u\n", o->find_union ? "U" : "", o->find_intrsec ? "I" : "", o->find_diff ? "D" : "",
             o->find_ddiff ? "X" : "", o->rule, o->nfiles);
    for (unsigned int f = 0; f < o->nfiles; f++) fprintf (stdout, "%u\t%s\n", f, o->fnames[f]);
  }
}

/* --min_lists / --max_lists: what argv alone decides, before a file or a device is opened; settles the defaults */
static void check_select (Options *o)
{
  if (!o->select) return;
  const char *with = o->find_subset ? "--subset" : o->nmm ? "-mm" : o->find_intrsec ? "-i" : o->subtraction ? "-du" : o->find_ddiff ? "-dd" : o->find_diff ? "-d" : NULL;
  if (with) {
    fprintf (stderr, "Error: --min_lists / --max_lists select from the union of the lists: they cannot be combined with %s\n", with);
    exit (1);
  }
  if (!o->find_union) {
    fprintf (stderr, "Error: --min_lists / --max_lists select from the union of the lists: -u is needed\n");
    exit (1);
  }
  if (o->nfiles < 2) {
    fprintf (stderr, "Error: At least 2 list/index files are needed\n");
    exit (1);
  }
  if (!o->have_min) o->min_lists = 1;
  if (!o->have_max) o->max_lists = o->nfiles;
  if (o->min_lists < 1 || o->max_lists < o->min_lists || o->max_lists > (long long) o->nfiles) {
    fprintf (stderr, "Error: --min_lists %lld, --max_lists %lld: 1 <= min_lists <= max_lists <= %u (the number of files) is needed\n", o->min_lists,
             o->max_lists, o->nfiles);
    exit (1);
  }
  if (!gt4hip_select_multi) {
    fprintf (stderr, "Error: this build has no --min_lists / --max_lists path\n");
    exit (1);
  }
}

/* --pairwise: what argv alone decides, before a file or a device is opened */
static void check_pairwise (const Options *o)
{
  if (!o->pairwise) return;
  const char *with = o->find_subset ? "--subset" : o->nmm ? "-mm" : o->select ? "--min_lists / --max_lists" : o->find_union ? "-u" : o->find_intrsec ? "-i"
                     : o->subtraction ? "-du" : o->find_ddiff ? "-dd" : o->find_diff ? "-d" : o->have_rule ? "-r" : o->have_cutoff ? "-c" : o->countonly ? "--count_only"
                     : o->have_gpus ? "--gpus" : NULL;
  if (with) {
    fprintf (stderr, "Error: --pairwise compares every list with every other one by itself: it cannot be combined with %s\n", with);
    exit (1);
  }
  if (o->nfiles < 2) {
    fprintf (stderr, "Error: At least 2 list/index files are needed\n");
    exit (1);
  }
  if (!gt4hip_pairwise_multi) {
    fprintf (stderr, "Error: this build has no --pairwise path\n");
    exit (1);
  }
}

/* ---- what the three execution paths share */

static gt4hip_context *create_context (const Options *o)
{
  gt4hip_context *ctx = NULL;
  if (gt4hip_create (o->device, &ctx)) {
    fprintf (stderr, "Error: %s\n", gt4hip_last_error (NULL));
    exit (1);
  }
  if (o->verbose) fprintf (stderr, "Device: %s\n", gt4hip_device_info (ctx));
  return ctx;
}

static void upload_inputs (const Options *o, gt4hip_context *ctx, const GT4ListFile *files, unsigned int wlen, gt4hip_list **lists)
{
  for (unsigned int f = 0; f < o->nfiles; f++) {
    if (files[f].index_kmers ? gt4hip_list_upload_index (ctx, files[f].index_kmers, files[f].header.n_words, files[f].index_locations, wlen, &lists[f])
                             : gt4hip_list_upload (ctx, files[f].records, files[f].header.n_words, wlen, &lists[f])) {
      fprintf (stderr, "Error: uploading %s to the GPU failed: %s\n", o->fnames[f], gt4hip_last_error (ctx));
      exit (1);
    }
    /* the reference trusts its inputs to be strictly ascending (results are undefined otherwise);
     * GT4HIP_CHECK_SORTED=1 verifies that on the device before merging */
    if (o->check_sorted) {
      int sorted = 0;
      if (gt4hip_list_is_sorted (ctx, lists[f], &sorted) || !sorted) {
        fprintf (stderr, "Error: File %s is not sorted by k-mer (strictly ascending, unique)\n", o->fnames[f]);
        exit (1);
      }
    }
  }
}

static uint32_t ops_mask (const Options *o)
{
  return (o->find_union ? GT4HIP_OP_UNION : 0) | (o->find_intrsec ? GT4HIP_OP_INTRSEC : 0) | (o->find_diff ? GT4HIP_OP_DIFF1 : 0) |
         (o->find_ddiff ? GT4HIP_OP_DIFF2 : 0);
}

static gt4hip_compare_params compare_params (const Options *o)
{
  return (gt4hip_compare_params) { .ops = ops_mask (o), .rule = o->rule, .cutoff = o->cutoff, .subtract = o->subtraction,
                                   .count_override = o->count_override, .count_only = o->countonly };
}

/* the -D lines at the head of compare_wordmaps (reference :789-955) and of compare_wordmaps_mm (:958-1093) */
static void print_lists_debug (const Options *o, const GT4ListFile *files)
{
  if (!o->debug) return;
  if (!o->nmm) fprintf (stderr, "compare_wordmaps: methods %u/%u/%u/%u\n", o->find_union, o->find_intrsec, o->find_diff, o->find_ddiff);
  fprintf (stderr, "compare_wordmaps: List 1: %llu entries\n", (unsigned long long) files[0].header.n_words);
  fprintf (stderr, "compare_wordmaps; List 2: %llu entries\n", (unsigned long long) files[1].header.n_words);
  if (!o->nmm) return;
  fprintf (stderr, "Table 1: %llu entries\n", (unsigned long long) files[0].header.n_words);
  fprintf (stderr, "Table 2: %llu entries\n", (unsigned long long) files[1].header.n_words);
}

/* the end of every path: the device lists and the mappings, file by file, then the context (NULL: none was made) */
static void release (const Options *o, GT4ListFile *files, gt4hip_list *const *lists, gt4hip_context *ctx)
{
  for (unsigned int f = 0; f < o->nfiles; f++) {
    if (lists) gt4hip_list_free (lists[f]);
    gt4_listfile_close (&files[f]);
  }
  gt4hip_destroy (ctx);
}

static void print_totals (uint64_t n_words, uint64_t total_count)
{
  fprintf (stdout, "NUnique\t%llu\nNTotal\t%llu\n", (unsigned long long) n_words, (unsigned long long) total_count);
}

/* "<out>_<k>_union.list", "_intrsec.list", "<out>_<k>_<mismatches>_diff1.list", "_diff2.list" (reference :814-834, -mm :1072-1091);
 * under --min_lists / --max_lists the union's place is "<out>_<k>_select_<M>_<X>.list": no file with the reference's name
 * for the union holds anything else */
static void output_name (const Options *o, unsigned int wlen, int s, char name[2048])
{
  if (s == 0 && o->select) snprintf (name, 2048, "%s_%u_select_%lld_%lld.list", o->outputname, wlen, o->min_lists, o->max_lists);
  else if (s < 2) snprintf (name, 2048, "%s_%u_%s.list", o->outputname, wlen, s ? "intrsec" : "union");
  else snprintf (name, 2048, "%s_%u_%u_%s.list", o->outputname, wlen, o->nmm, s == 2 ? "diff1" : "diff2");
}

/* The streams `ops` of a pair result: under --count_only their totals; else each to its own "<name>.tmp" at once (the copy
 * threads are dealt to the files), then header back-patch and rename in the reference's order (:907-953, -mm :1072-1091).
 * Frees the result lists.  Returns 1 after a message, with no temporary left behind. */
static int write_outputs (const Options *o, gt4hip_context *ctx, unsigned int wlen, uint32_t ops, gt4hip_compare_result *res)
{
  if (o->countonly) {
    for (int s = 0; s < 4; s++)
      if ((ops >> s) & 1u) print_totals (res->n_words[s], res->total_count[s]);
    return 0;
  }
  char name[4][2048], tmp_name[4][2100];
  GT4ListWriter w[4];
  const gt4hip_list *wl[4];
  uint64_t wfirst[4], wcount[4], woff[4];
  int wfd[4], ws[4];
  uint32_t nw = 0;
  int bad = 0;
  for (int s = 0; s < 4; s++) {
    if (!((ops >> s) & 1u)) continue;
    output_name (o, wlen, s, name[s]);
    snprintf (tmp_name[s], sizeof tmp_name[s], "%s.tmp", name[s]);
    /* fopen (.., "w") in the reference: mode 0666 minus umask */
    if (gt4_listwriter_begin (&w[s], tmp_name[s], wlen, 0666)) {
      fprintf (stderr, "Error: Cannot create output file %s\n", tmp_name[s]);
      bad = 1;
      break;
    }
    wl[nw] = res->out[s];
    wfirst[nw] = 0;
    wcount[nw] = res->n_words[s];
    wfd[nw] = w[s].fd;
    woff[nw] = 48;
    ws[nw] = s;
    nw++;
  }
  if (!bad && nw && gt4hip_lists_write_fd (ctx, nw, wl, wfirst, wcount, wfd, woff)) {
    fprintf (stderr, "Error: writing the results failed: %s\n", gt4hip_last_error (ctx));
    bad = 1;
  }
  for (uint32_t q = 0; q < nw; q++) {
    const int s = ws[q];
    if (bad) {
      gt4_listwriter_abort (&w[s]);
      unlink (tmp_name[s]);
      continue;
    }
    /* compare_wordmaps announces the renames of the differences under -D, compare_wordmaps_mm does not */
    if (o->debug && s >= 2 && !o->nmm) fprintf (stderr, "Renaming %s to %s\n", tmp_name[s], name[s]);
    if (gt4_listwriter_finish (&w[s], res->n_words[s], res->total_count[s])) {
      fprintf (stderr, "Error: writing %s failed: %s\n", tmp_name[s], strerror (errno));
      unlink (tmp_name[s]);
      bad = 1;
    } else if (rename (tmp_name[s], name[s])) {
      fprintf (stderr, "Error: Cannot rename %s to %s\n", tmp_name[s], name[s]);
      bad = 1;
    }
  }
  for (int s = 0; s < 4; s++) gt4hip_list_free (res->out[s]);
  return bad;
}

/* union_multi / intersect_multi (reference :366-422): the union pass, then the intersection pass.  With `job` every pass
 * is a gt4_shard_run, which writes the output itself; without it the lists are resident in `ctx`.  Returns the exit code. */
static int run_multi (const Options *o, const GT4ListFile *files, unsigned int wlen, GT4ShardJob *job, gt4hip_context *ctx, gt4hip_list *const *lists)
{
  int v = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int is_union = pass == 0;
    if (is_union ? !o->find_union : !o->find_intrsec) continue;
    char name[2048];
    output_name (o, wlen, pass, name);
    int rc;
    GT4ShardResult sres;
    gt4hip_multi_result mres;
    memset (&mres, 0, sizeof mres);
    const int is_select = is_union && o->select; /* the union restricted to the words of min_lists .. max_lists files */
    if (job) {
      job->mode = is_select ? GT4_SHARD_SELECT_MULTI : is_union ? GT4_SHARD_UNION_MULTI : GT4_SHARD_INTERSECT_MULTI;
      job->min_lists = (unsigned int) o->min_lists;
      job->max_lists = (unsigned int) o->max_lists;
      job->out_mode = 0644;
      job->out_name[0] = o->countonly ? NULL : name;
    }
    const double t_s = now_seconds ();
    if (job) rc = gt4_shard_run (job, &sres);
    else if (is_select)
      rc = gt4hip_select_multi (ctx, (const gt4hip_list *const *) lists, o->nfiles, (uint32_t) o->min_lists, (uint32_t) o->max_lists, o->cutoff, o->rule,
                                o->count_override, o->countonly, &mres);
    else rc = (is_union ? gt4hip_union_multi : gt4hip_intersect_multi) (ctx, (const gt4hip_list *const *) lists, o->nfiles, o->cutoff, o->rule,
                                                                        o->count_override, o->countonly, &mres);
    const double t_e = now_seconds ();
    const int rule_rejected = job ? sres.rule_rejected : rc == GT4HIP_ERULE;
    const char *message = job ? sres.message : rc ? gt4hip_last_error (ctx) : "";
    const uint64_t n_words = job ? sres.n_words[0] : mres.n_words, total_count = job ? sres.total_count[0] : mres.total_count;
    if (rc && rule_rejected) {
      fprintf (stderr, "%s\n", message);
      v = 1; /* the reference returns 1 from the merge and exits 1 without an output file */
      continue;
    }
    if (rc) {
      if (!job) fprintf (stderr, "Error: %s\n", message); /* gt4_shard_run has said why */
      exit (1);
    }
    v = 0;
    if (is_select && o->verbose && !job) fprintf (stderr, "GPU select kernels: %.3f ms, %llu of %llu distinct words kept\n", mres.device_ms,
                                                  (unsigned long long) mres.n_words, (unsigned long long) mres.records_read);
    if (o->debug && !is_select) { /* (the selection is no operation of the reference: -D adds nothing to it) */
      unsigned long long total = 0;
      for (unsigned int f = 0; f < o->nfiles; f++) total += files[f].header.n_words;
      fprintf (stderr, "Combined %u maps: input %llu (%.3f Mwords/s) output %llu (%.3f Mwords/s)\n", o->nfiles, is_union ? total : 0ull,
               (is_union ? total : 0ull) / (1000000 * (t_e - t_s)), (unsigned long long) n_words, n_words / (1000000 * (t_e - t_s)));
    }
    if (!job && !o->countonly) {
      /* creat (.., 0644) in the reference; a failed rename is fatal here */
      if (gt4_cli_write_list_file (ctx, mres.out, wlen, n_words, total_count, name, 0644, "Error: ")) exit (1);
      gt4hip_list_free (mres.out);
    }
    if (o->countonly || (o->debug && !is_select)) print_totals (n_words, total_count);
  }
  return v;
}

/* ---- the execution paths */

/* X0 of drand48's generator behind the reference's srand48 (reference :237-241; glibc: the low 32 bits of the seed above
 * 0x330E); no --seed, or --seed -1: the start time */
static uint64_t subset_state48 (long seed)
{
  const uint32_t low = seed == -1 ? (uint32_t) (unsigned int) time (NULL) : (uint32_t) (unsigned long) seed;
  return ((uint64_t) low << 16) | 0x330Eull;
}

/* subset (reference :292-315, :719-787): one list, SIZE of its records or occurrences selected at random */
static int run_subset (const Options *o, GT4ListFile *files, unsigned int wlen)
{
  if (o->nfiles != 1) {
    fprintf (stderr, "Error: Subsetting multiple files is not supported\n");
    exit (1);
  }
  const unsigned long long num_words = files[0].header.n_words;
  if (o->subset_method != GT4HIP_SUBSET_RAND && o->subset_size > num_words) {
    fprintf (stderr, "Error: Unique subset size (%llu) is bigger than number of unique kmers (%llu)\n", o->subset_size, num_words);
    exit (1);
  }
  if (o->n_gpus > 1 || o->hbm_limit) {
    fprintf (stderr, "Error: --subset needs the list resident on one GPU: it cannot be combined with %s\n",
             o->n_gpus > 1 ? "--gpus N > 1 (GT4HIP_GPUS)" : "GT4HIP_HBM_LIMIT");
    return 1;
  }
  if (!gt4hip_list_subset) {
    fprintf (stderr, "Error: this build has no --subset path\n");
    return 1;
  }
  gt4hip_context *ctx = create_context (o);
  gt4hip_list *lists[1];
  upload_inputs (o, ctx, files, wlen, lists);
  const gt4hip_subset_params prm = { .method = o->subset_method, .size = o->subset_size, .state48 = subset_state48 (o->seed) };
  gt4hip_list *result = NULL;
  uint64_t n_words = 0, total_count = 0;
  if (gt4hip_list_subset (ctx, lists[0], &prm, &result, &n_words, &total_count)) {
    fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
    release (o, files, lists, ctx);
    return 1;
  }
  char name[2048];
  snprintf (name, sizeof name, "%s_subset_%u.list", o->outputname, wlen);
  /* fopen (.., "w") in the reference: mode 0666 minus umask */
  const int bad = gt4_cli_write_list_file (ctx, result, wlen, n_words, total_count, name, 0666, "Error: ");
  gt4hip_list_free (result);
  release (o, files, lists, ctx);
  return bad ? 1 : 0;
}

/* compare_wordmaps_mm (reference :958-1093): two lists, diff1 and / or diff2 up to nmm mismatches */
static int run_mismatch (const Options *o, GT4ListFile *files, unsigned int wlen)
{
  print_lists_debug (o, files);
  /* without -d / -dd / -du the reference takes this path all the same and writes nothing */
  if (!o->find_diff) {
    release (o, files, NULL, NULL);
    return 0;
  }
  if (o->n_gpus > 1 || o->hbm_limit) {
    fprintf (stderr, "Error: -mm needs both lists resident on one GPU: it cannot be combined with %s\n",
             o->n_gpus > 1 ? "--gpus N > 1 (GT4HIP_GPUS)" : "GT4HIP_HBM_LIMIT");
    return 1;
  }
  if (!gt4hip_compare_mismatch || !gt4hip_mismatch_stats_get) {
    fprintf (stderr, "Error: this build has no -mm (mismatch difference) path\n");
    return 1;
  }
  gt4hip_context *ctx = create_context (o);
  /* inputs, outputs and the lookup tables (~48 bytes per record of each side) must fit: there is no chunked -mm */
  uint64_t free_b = 0, total_b = 0;
  gt4hip_device_memory (ctx, &free_b, &total_b);
  const uint64_t na = files[0].header.n_words, nb = files[1].header.n_words;
  const uint64_t need = 12 * (na + nb) + 60 * na + (o->find_ddiff ? 60 * nb : 0);
  if (free_b && need > free_b / 100 * 90) {
    fprintf (stderr, "Error: %s: -mm needs about %llu bytes of device memory, %llu are free (both lists stay resident on one GPU)\n",
             gt4hip_strerror (GT4HIP_ENOMEM), (unsigned long long) need, (unsigned long long) free_b);
    gt4hip_destroy (ctx);
    return 1;
  }
  gt4hip_list *lists[2];
  upload_inputs (o, ctx, files, wlen, lists);
  gt4hip_mismatch_params prm;
  memset (&prm, 0, sizeof prm);
  prm.ops = ops_mask (o) & (GT4HIP_OP_DIFF1 | GT4HIP_OP_DIFF2);
  prm.cutoff = o->cutoff;
  prm.subtract = o->subtraction;
  prm.n_mismatch = o->nmm;
  prm.count_only = o->countonly;
  gt4hip_compare_result res;
  memset (&res, 0, sizeof res);
  if (gt4hip_compare_mismatch (ctx, lists[0], lists[1], &prm, &res)) {
    fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
    exit (1);
  }
  gt4hip_mismatch_stats st;
  gt4hip_mismatch_stats_get (ctx, &st);
  if (o->debug) fprintf (stderr, "Finding diff with mismatches (%llu entries)\n", (unsigned long long) st.prepass_words[0]);
  if (o->verbose) {
    fprintf (stderr, "GPU mismatch pre-pass: %.3f ms, device total %.3f ms, %llu probes\n", res.merge_kernel_ms, res.device_ms,
             (unsigned long long) st.probes);
    for (uint32_t l = 0; l < st.n_levels; l++)
      fprintf (stderr, "  level %u: %llu words, %llu probes, %.3f ms\n", l + 1, (unsigned long long) st.level_words[l],
               (unsigned long long) st.level_probes[l], st.level_ms[l]);
  }
  if (write_outputs (o, ctx, wlen, prm.ops, &res)) exit (1);
  release (o, files, lists, ctx);
  return 0;
}

static uint64_t input_records (const Options *o, const GT4ListFile *files)
{
  uint64_t n = 0;
  for (unsigned int f = 0; f < o->nfiles; f++) n += files[f].header.n_words;
  return n;
}

/* --pairwise: every list against every other one from one count table (gt4hip_pairwise_multi); all of it resident */
static int run_pairwise (const Options *o, GT4ListFile *files, unsigned int wlen)
{
  if (o->hbm_limit || o->n_gpus > 1) {
    fprintf (stderr, "Error: --pairwise needs all lists resident on one GPU: it cannot be combined with %s\n",
             o->hbm_limit ? "GT4HIP_HBM_LIMIT" : "GT4HIP_GPUS");
    return 1;
  }
  gt4hip_context *ctx = create_context (o);
  /* the lists; the count table, a key and a count per file for every input record at worst, beside what builds it (the union's
   * keys, a merge's output); the workgroups' partial matrices (32 x 32 x 2 numbers each) and the two matrices */
  uint64_t free_b = 0, total_b = 0;
  gt4hip_device_memory (ctx, &free_b, &total_b);
  const uint64_t need = input_records (o, files) * (12 * 4 + 8 + 4ull * o->nfiles) + (64ull << 20) + 16ull * o->nfiles * o->nfiles;
  if (free_b && need > free_b / 100 * 85) {
    fprintf (stderr, "Error: %s: --pairwise needs about %llu bytes of device memory, %llu are free (the lists and their count table stay resident on one GPU)\n",
             gt4hip_strerror (GT4HIP_ENOMEM), (unsigned long long) need, (unsigned long long) free_b);
    gt4hip_destroy (ctx);
    return 1;
  }
  static gt4hip_list *lists[MAX_FILES];
  upload_inputs (o, ctx, files, wlen, lists);
  const size_t n = o->nfiles;
  uint64_t *shared = (uint64_t *) malloc (n * n * sizeof (uint64_t)), *min_total = (uint64_t *) malloc (n * n * sizeof (uint64_t));
  if (!shared || !min_total) {
    fprintf (stderr, "Error: out of memory for the matrices of %u lists\n", o->nfiles);
    exit (1);
  }
  float ms = 0;
  if (gt4hip_pairwise_multi (ctx, (const gt4hip_list *const *) lists, o->nfiles, shared, min_total, &ms)) {
    fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
    exit (1);
  }
  if (o->verbose) fprintf (stderr, "GPU pairwise kernels: %.3f ms, %u lists\n", ms, o->nfiles);
  fprintf (stdout, "#I\tJ\tLIST_I\tLIST_J\tSHARED\tMIN_TOTAL\tUNION\tJACCARD\n");
  for (size_t i = 0; i < n; i++)
    for (size_t j = i; j < n; j++) {
      const uint64_t s = shared[i * n + j], u = shared[i * n + i] + shared[j * n + j] - s;
      fprintf (stdout, "%u\t%u\t%s\t%s\t%llu\t%llu\t%llu\t%.6f\n", (unsigned int) i, (unsigned int) j, o->fnames[i], o->fnames[j], (unsigned long long) s,
               (unsigned long long) min_total[i * n + j], (unsigned long long) u, u ? (double) s / (double) u : 0.0);
    }
  free (shared);
  free (min_total);
  release (o, files, lists, ctx);
  return 0;
}

/* Big inputs with no plan given: key-range chunks through the loader / merger / writer pipeline, so that reading the next
 * chunk and writing the previous one overlap the merge (GT4HIP_PIPELINE=0 keeps everything in one piece).  The worker that
 * runs the job (in this process) measures the device's free memory and chooses the chunk budget itself. */
static int wants_pipeline (const Options *o, const GT4ListFile *files)
{
  return o->n_gpus < 1 && !o->hbm_limit && !o->pipeline_off && 12 * input_records (o, files) >= (4ull << 30);
}

/* The context of a resident run, or NULL: the job goes through the key-range shards, and no context may exist in this
 * process -- the workers are forked before any HIP call, and the HIP runtime starts once per process. */
static gt4hip_context *resident_context (const Options *o, const GT4ListFile *files)
{
  if (o->n_gpus >= 1 || o->hbm_limit || wants_pipeline (o, files)) return NULL;
  gt4hip_context *ctx = create_context (o);
  /* inputs + worst-case outputs (+ the N-way tree's intermediates) must fit, else stream in chunks */
  uint64_t free_b = 0, total_b = 0;
  gt4hip_device_memory (ctx, &free_b, &total_b);
  /* (the selection also holds the count table, a key and a count per file for every input record at worst, and 5 bytes per row) */
  const uint64_t need = o->select ? input_records (o, files) * (12 * 4 + 13 + 4ull * o->nfiles)
                                  : 12 * input_records (o, files) * (o->nfiles == 2 ? 1 + (uint64_t) (o->find_union + o->find_intrsec + o->find_diff + o->find_ddiff) : 4);
  if (free_b && need > free_b / 100 * 85) {
    if (o->verbose) fprintf (stderr, "Inputs and outputs need %llu bytes, %llu are free: streaming in key-range chunks\n", (unsigned long long) need, (unsigned long long) free_b);
    gt4hip_destroy (ctx);
    return NULL;
  }
  return ctx;
}

/* key-range shards: several GPUs and / or chunks streamed through the device memory (gt4_shard.c) */
static int run_sharded (const Options *o, GT4ListFile *files, unsigned int wlen)
{
  GT4ShardJob job;
  memset (&job, 0, sizeof job);
  job.n_files = o->nfiles;
  job.files = files;
  job.word_length = wlen;
  job.n_ranks = o->n_gpus >= 1 ? o->n_gpus : 1;
  job.hbm_limit = o->hbm_limit;
  job.auto_budget = wants_pipeline (o, files);
  job.gather_rccl = o->gather_rccl;
  job.debug = o->verbose;
  job.prm = compare_params (o); /* gt4_shard.c reads prm.ops in pair mode only */
  const int multi = o->nfiles > 2 || o->select; /* (two files with --min_lists / --max_lists take the N-way path) */
  const int v = multi ? run_multi (o, files, wlen, &job, NULL, NULL) : 0;
  if (!multi) print_lists_debug (o, files);
  if (!multi && job.prm.ops) {
    job.mode = GT4_SHARD_PAIR;
    job.out_mode = 0666;
    char names[4][2048];
    for (int s = 0; s < 4; s++) {
      if (!((job.prm.ops >> s) & 1u) || o->countonly) continue;
      output_name (o, wlen, s, names[s]);
      job.out_name[s] = names[s];
    }
    GT4ShardResult res;
    if (gt4_shard_run (&job, &res)) exit (1);
    if (o->verbose) fprintf (stderr, "Sharded run: %u chunks over %d GPU(s)\n", res.n_chunks, job.n_ranks);
    for (int s = 0; s < 4; s++) {
      if (!((job.prm.ops >> s) & 1u)) continue;
      if (o->countonly) print_totals (res.n_words[s], res.total_count[s]);
      else if (o->debug && s >= 2) fprintf (stderr, "Renaming %s.tmp to %s\n", names[s], names[s]);
    }
  }
  release (o, files, NULL, NULL);
  return v;
}

/* everything in device memory at once: compare_wordmaps (reference :789-955) or the N-way passes */
static int run_resident (const Options *o, GT4ListFile *files, unsigned int wlen, gt4hip_context *ctx)
{
  static gt4hip_list *lists[MAX_FILES];
  int v = 0;
  upload_inputs (o, ctx, files, wlen, lists);
  if (o->nfiles > 2 || o->select) {
    v = run_multi (o, files, wlen, NULL, ctx, lists);
  } else {
    print_lists_debug (o, files);
    const gt4hip_compare_params prm = compare_params (o);
    gt4hip_compare_result res;
    memset (&res, 0, sizeof res);
    if (prm.ops) {
      if (gt4hip_compare (ctx, lists[0], lists[1], &prm, &res)) {
        fprintf (stderr, "Error: %s\n", gt4hip_last_error (ctx));
        exit (1);
      }
      if (o->verbose) fprintf (stderr, "GPU merge kernel: %.3f ms (%llu tiles), device total %.3f ms\n", res.merge_kernel_ms,
                               (unsigned long long) res.merge_tiles, res.device_ms);
    }
    if (write_outputs (o, ctx, wlen, prm.ops, &res)) exit (1);
  }
  release (o, files, lists, ctx);
  return v;
}

int main (int argc, const char *argv[])
{
  static Options o;
  static GT4ListFile files[MAX_FILES];
  if (argc <= 1) print_help (1);
  read_environment (&o);
  parse_argv (argc, argv, &o); /* --gpus N overrides GT4HIP_GPUS */
  check_pairwise (&o);
  check_select (&o);
  const unsigned int wlen = open_inputs (&o, files);
  if (o.pairwise) return run_pairwise (&o, files, wlen);
  if (o.find_subset) return run_subset (&o, files, wlen); /* before the two-file checks, as in the reference (:292-315) */
  validate (&o);
  if (o.nmm) return run_mismatch (&o, files, wlen);
  gt4hip_context *ctx = resident_context (&o, files); /* run_resident owns it from here and destroys it */
  return ctx ? run_resident (&o, files, wlen, ctx) : run_sharded (&o, files, wlen);
}
