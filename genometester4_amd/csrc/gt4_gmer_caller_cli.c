/*
 * gt4_gmer_caller_cli.c -- `gmer_caller`, the drop-in command line that calls genotypes from the counts gmer_counter
 * prints (the calling half of FastGT; reference src/gmer_caller.c, src/simplex.c, src/binomial.c:161-174,
 * src/utils.c:209-248).  Host C; every likelihood -- the objective of each training step and the probabilities of every
 * marker printed -- is computed by the HIP kernels behind include/gt4hip.h (gt4hip_caller.hip).
 *
 * Stages: parse argv; read the text and build its line table; split the lines into autosomes, X and Y; pair medians and
 * the Poisson sex test; pick every marker's count pair; train the autosome model (and, for a male, the X model) by the
 * reference's downhill simplex, whose objective is one device call per evaluation on a set of markers that stays in
 * HBM; print.  The host part keeps the reference's types and order of operations -- `float` where it has float, libc's
 * rand () sequence after srand (1) in its order (ref_rand), the per-chunk `float` penalty of the coverage (a chunk is max (2000, ceil (training
 * markers / --num_threads)) markers: the only thing --num_threads still means), the `float` cast of the objective -- so
 * that a training takes the reference's path unless two objectives differ in the last bits a float keeps.
 * Same argv grammar, messages, output and exit codes as the reference's main ().  -D, -D -D print its debug lines on
 * stderr, the "Iteration N delta %.6f" line of every objective evaluation among them.
 * Deliberate differences, all one "Error: ..." line + exit 1, before any device is touched:
 *   - a line of a group that is used (autosomes, X, Y under --model full; every line otherwise) with fewer than 4 tokens:
 *     the reference reads counts it never set (and crashes on some such lines);
 *   - a text whose last byte is no newline: the reference reads behind its mapping;
 *   - --num_threads outside 1..32: the reference prints its message and usage and goes on: with 0 it divides by zero sizing
 *     the training chunks and, without training, never leaves its printing loop; above 32 it writes behind its 32 chunk
 *     records once a training has more chunks than that.
 * A NaN likelihood prints as the NaN this host's own arithmetic makes ("-nan" on x86-64), whatever sign the device's has.
 * The reference's assert () aborts (a NaN likelihood or parameter during training) are not reproduced.
 * Without a usable GPU the program fails where it first needs one: there is no CPU path.  A run that computes no
 * likelihood (-v, --runs 0 with --no_genotypes, every error above) needs none.
 * Environment: GT4HIP_DEVICE=N, GT4HIP_VERBOSE=1 as in the other tools.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <fcntl.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "gt4_cli.h"
#include "gt4_listfile.h"
#include "gt4hip.h"

#define MAX_THREADS 32
#define N_GT GT4HIP_CALLER_GENOTYPES
#define MIN_P (1.0f / 8192)
#define MAX_E 0.25f
#define PRINT_PIECE (1u << 20) /* markers per device call while printing */

enum { L_VIGA, P_0, P_1, P_2, LAMBDA, SIZE, SIZE2, N_PARAMS };
enum { MODEL_FULL, MODEL_DIPLOID, MODEL_HAPLOID };
enum { GT_A = 1, GT_B = 2, GT_AA = 3, GT_AB = 4, GT_BB = 5 };

static const char *const GT_NAMES[N_GT] = { "-", "A", "B", "AA", "AB", "BB", "AAA", "AAB", "BBA", "BBB", "AAAA", "AAAB", "BBBA", "AABB", "BBBB" };

static const char *const HELP_LINES[] = {
  "Usage:",
  "  gmer_caller ARGUMENTS COUNTS_FILE",
  "Arguments:",
  "    -v | --version      - Print version information and exit",
  "    --training_size NUM - Use NUM markers for training (default 100000)",
  "    --runs NUMBER       - Perfom NUMBER runs of model training (use 0 for no training)",
  "    --num_threads NUM   - Use NUM threads (min 1, max 32, default 16)",
  "    --header            - Print table header",
  "    --non_canonical     - Output non-canonical genotypes",
  "    --prob_cutoff       - probability cutoff for calling genotype (default 0)",
  "    --alternatives      - Print probabilities of all alternative genotypes",
  "    --info              - Print information about individual",
  "    --no_genotypes      - Print only summary information, not actual genotypes",
  "    --model TYPE        - Model type (full, diploid, haploid)",
  "    --params PARAMS     - Model parameters (error, p0, p1, p2, coverage, size, size2)",
  "    --coverage NUM      - Average coverage of reads",
  "    -D                  - increase debug level",
};

typedef struct {
  const char *call_fn;
  unsigned int nruns, max_training, nthreads, header, non_canonical, alternatives, info, print_gt, model, params_specified;
  float prob_cutoff;
  float params[N_PARAMS];
  unsigned int debug;
  int device, env_verbose;
} Options;

typedef struct {
  unsigned int line;
  unsigned short counts[2];
} Call;

/* the text: `size` bytes and a NUL behind them; line i is [start[i], start[i + 1]) */
typedef struct {
  const unsigned char *data;
  uint64_t size;
  uint64_t *start;
  unsigned int nlines;
} Text;

static unsigned int debug;
static gt4hip_context *ctx;
static int device_id;

/* rand () of the reference after its srand (1): the same generator of libc, on a state of our own (random_r).  The global
 * state of rand () belongs to the whole process, and whatever else draws from it -- a runtime library between two of our
 * calls -- would shift the sequence the training set and the simplex's starting points are made from. */
static struct random_data rand_state;
static char rand_buffer[128];
static void ref_srand (unsigned int seed) { initstate_r (seed, rand_buffer, sizeof rand_buffer, &rand_state); }
static int ref_rand (void)
{
  int32_t v = 0;
  random_r (&rand_state, &v);
  return (int) v;
}

static void print_usage (FILE *to) { gt4_cli_print_help (to, "gmer_caller", HELP_LINES, sizeof HELP_LINES / sizeof HELP_LINES[0]); }

static const char *value_arg (int argc, const char *argv[], int *i, int needed)
{
  *i += 1;
  if (*i + needed > argc) {
    print_usage (stderr);
    exit (1);
  }
  return argv[*i];
}

/* argv (reference :540-629) */
static void parse_argv (int argc, const char *argv[], Options *o)
{
  static const float initial[N_PARAMS] = { 0.0547219f, 4.2603e-05f, 0.014934f, 0.985023f, 0, 65.48f, -0.6792684f };
  memcpy (o->params, initial, sizeof initial);
  o->nruns = 5;
  o->max_training = 100000;
  o->nthreads = MAX_THREADS / 2;
  o->print_gt = 1;
  o->model = MODEL_FULL;
  for (int i = 1; i < argc; i++) {
    const char *a = argv[i];
    if (!strcmp (a, "-v") || !strcmp (a, "--version")) {
      gt4_cli_print_version (stdout, "gmer_caller");
      exit (0);
    } else if (!strcmp (a, "-D")) {
      o->debug += 1;
    } else if (!strcmp (a, "--runs")) {
      o->nruns = (unsigned int) strtol (value_arg (argc, argv, &i, 1), NULL, 10);
    } else if (!strcmp (a, "--training_size")) {
      o->max_training = (unsigned int) strtol (value_arg (argc, argv, &i, 1), NULL, 10);
    } else if (!strcmp (a, "--num_threads")) {
      o->nthreads = (unsigned int) strtol (value_arg (argc, argv, &i, 1), NULL, 10);
    } else if (!strcmp (a, "--header")) {
      o->header = 1;
    } else if (!strcmp (a, "--non_canonical")) {
      o->non_canonical = 1;
    } else if (!strcmp (a, "--prob_cutoff")) {
      o->prob_cutoff = (float) atof (value_arg (argc, argv, &i, 1));
    } else if (!strcmp (a, "--model")) {
      const char *m = value_arg (argc, argv, &i, 1);
      if (!strcmp (m, "full")) o->model = MODEL_FULL;
      else if (!strcmp (m, "diploid")) o->model = MODEL_DIPLOID;
      else if (!strcmp (m, "haploid")) o->model = MODEL_HAPLOID;
      else {
        print_usage (stderr);
        exit (1);
      }
    } else if (!strcmp (a, "--params")) {
      (void) value_arg (argc, argv, &i, N_PARAMS);
      for (int j = 0; j < N_PARAMS; j++) o->params[j] = (float) atof (argv[i + j]);
      o->params_specified = 1;
      i += N_PARAMS - 1;
    } else if (!strcmp (a, "--coverage")) {
      o->params[LAMBDA] = (float) atof (value_arg (argc, argv, &i, 1));
    } else if (!strcmp (a, "--alternatives")) {
      o->alternatives = 1;
    } else if (!strcmp (a, "--info")) {
      o->info = 1;
    } else if (!strcmp (a, "--no_genotypes")) {
      o->print_gt = 0;
    } else {
      if (o->call_fn) {
        print_usage (stderr);
        exit (1);
      }
      o->call_fn = a;
    }
  }
}

/* the file with a NUL behind it; a file that cannot be mapped gets gt4_mmap's message (reference src/utils.c:36-64) and NULL */
static unsigned char *read_text (const char *name, uint64_t *size)
{
  struct stat st;
  if (!name || stat (name, &st) < 0) {
    fprintf (stderr, "gt4_mmap (stat): %s\n", strerror (name ? errno : EFAULT));
    return NULL;
  }
  const int fd = open (name, O_RDONLY);
  if (fd < 0) {
    fprintf (stderr, "gt4_mmap (open): %s\n", strerror (errno));
    return NULL;
  }
  unsigned char *b = st.st_size ? (unsigned char *) malloc ((size_t) st.st_size + 1) : NULL;
  size_t got = 0;
  while (b && got < (size_t) st.st_size) {
    const ssize_t r = read (fd, b + got, (size_t) st.st_size - got);
    if (r <= 0) break;
    got += (size_t) r;
  }
  close (fd);
  if (!b || got != (size_t) st.st_size) {
    fprintf (stderr, "gt4_mmap (mmap): %s\n", strerror (!st.st_size ? EINVAL : b ? EIO : ENOMEM));
    free (b);
    return NULL;
  }
  b[got] = 0;
  *size = got;
  return b;
}

/* split_line (reference src/utils.c:233-248) of the line at `line`, `len` bytes with its '\n': up to `max` tokens parted by any byte < ' ' */
static unsigned int split_line (const unsigned char *line, uint64_t len, const unsigned char *tok[], unsigned int max)
{
  unsigned int i = 0;
  uint64_t s = 0;
  while (i < max && line[s] != '\n') {
    uint64_t e = s;
    tok[i++] = line + s;
    while (e < len && line[e] >= ' ') e++;
    s = e;
    if (line[s] != '\n') s++;
  }
  return i;
}

static unsigned int line_tokens (const Text *t, unsigned int line, const unsigned char *tok[])
{
  return split_line (t->data + t->start[line], t->start[line + 1] - t->start[line], tok, 8);
}

/* get_pair_median (reference :966-1025): the median of 6 x the mean pair sum of every line, by bisection, over 6 */
static unsigned int get_pair_median (const Text *t, const unsigned int idx[], unsigned int n)
{
  const unsigned char *tok[16];
  unsigned int *m6 = (unsigned int *) malloc ((n ? n : 1) * sizeof (unsigned int));
  unsigned int max = 0, min = 0xffffffff, med;
  for (unsigned int i = 0; i < n; i++) {
    const unsigned int npairs = (line_tokens (t, idx[i], tok) - 2) / 2; /* (at least 4 tokens: checked) */
    unsigned int sum = 0;
    for (unsigned int j = 0; j < npairs; j++) {
      sum += strtol ((const char *) tok[2 + 2 * j], NULL, 10);
      sum += strtol ((const char *) tok[2 + 2 * j + 1], NULL, 10);
    }
    m6[i] = sum * 6 / npairs;
    if (m6[i] > max) max = m6[i];
    if (m6[i] < min) min = m6[i];
  }
  med = (min + max) / 2;
  while (max > min) {
    unsigned int above = 0, below = 0, equal;
    for (unsigned int i = 0; i < n; i++) {
      above += m6[i] > med;
      below += m6[i] < med;
    }
    equal = n - above - below;
    if (debug > 1) fprintf (stderr, "Trying median %u (%u) - equal %u, below %u, above %u\n", med / 6, med, equal, below, above);
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
  free (m6);
  return med / 6;
}

/* poisson (reference src/binomial.c:161-174).  A group without lines has a "median" of 357,913,941 (get_pair_median of
 * nothing), and the reference walks that many steps; a product that has reached 0 stays 0, so the walk ends there. */
static double poisson (unsigned int k, double lambda)
{
  double dk = k, p = exp (-lambda);
  for (; k > 0 && p != 0; k--) {
    p *= lambda;
    p /= dk;
    dk -= 1;
  }
  return p;
}

/* parse_calls (reference :144-175): of every line the pair whose sum lies nearest the median, the first of equals; 16-bit counts */
static Call *parse_calls (const Text *t, const unsigned int idx[], unsigned int n, unsigned int pair_median)
{
  const unsigned char *tok[16];
  Call *calls = (Call *) malloc ((n ? n : 1) * sizeof (Call));
  for (unsigned int i = 0; i < n; i++) {
    const unsigned int npairs = (line_tokens (t, idx[i], tok) - 2) / 2;
    int best_a = 0, best_b = 0, best_delta = 0x7fffffff;
    for (unsigned int j = 0; j < npairs; j++) {
      const int a = (int) strtol ((const char *) tok[2 + 2 * j], NULL, 10), b = (int) strtol ((const char *) tok[2 + 2 * j + 1], NULL, 10);
      int delta = (int) ((unsigned int) a + (unsigned int) b - pair_median);
      if (delta < 0) delta = -delta;
      if (delta < best_delta) best_a = a, best_b = b, best_delta = delta;
    }
    calls[i].line = idx[i];
    calls[i].counts[0] = (unsigned short) best_a;
    calls[i].counts[1] = (unsigned short) best_b;
  }
  return calls;
}

/* calculate_allele_freq (reference :197-223): the mean of b / (a + b) over the markers with a count, each quotient in float */
static float allele_freq (const Call *calls, const unsigned int set[], unsigned int n)
{
  double ppB = 0, npB = 0;
  for (unsigned int i = 0; i < n; i++) {
    const Call *c = &calls[set ? set[i] : i];
    const unsigned int c0 = c->counts[0], c1 = c->counts[1];
    if (c0 + c1) {
      ppB += (1.0f * c1) / (c0 + c1);
      npB += 1;
    }
  }
  return npB ? (float) (ppB / npB) : 0;
}

/* build_training_set (reference :179-195) with rand_long_long (src/utils.c:209-214): the first `subset` entries of a partial shuffle */
static unsigned int *build_training_set (unsigned int set_size, unsigned int subset)
{
  unsigned int *train = (unsigned int *) malloc ((set_size ? set_size : 1) * sizeof (unsigned int));
  for (unsigned int i = 0; i < set_size; i++) train[i] = i;
  for (unsigned int i = 0; i < subset; i++) {
    const unsigned long long delta = (unsigned long long) (set_size - 1) - 0 + 1;
    const unsigned int p = (unsigned int) (0 + (unsigned long long) (delta * (ref_rand () / (RAND_MAX + 1.0))));
    const unsigned int v = train[i];
    train[i] = train[p];
    train[p] = v;
  }
  return train;
}

/* ------------------------------------------------------------------ the parameters as the simplex sees them */

static float logit (float p) { return logf (p / (1 - p)); }
static float logit_1 (float a) { return 1 / (1 + expf (-a)); }

static float logit_clamped (float p, float min, float max)
{
  if (p <= min) p = min;
  else if (p >= max) p = max;
  else p = (p - min) / (max - min);
  return logit (p);
}

static float logit_1_clamped (float a, float min, float max)
{
  a = logit_1 (a);
  return min + (max - min) * a;
}

/* the simplex's coordinates -> the model's parameters (reference :849-856, :875-886) */
static void unpack_params (const float x[N_PARAMS], float v[N_PARAMS])
{
  v[L_VIGA] = logit_1_clamped (x[0], MIN_P, MAX_E);
  v[P_0] = logit_1_clamped (x[1], MIN_P, 1 - MIN_P);
  v[P_1] = logit_1_clamped (x[2], MIN_P, 1 - MIN_P);
  v[P_2] = logit_1_clamped (x[3], MIN_P, 1 - MIN_P);
  v[LAMBDA] = expf (x[4]);
  v[SIZE] = x[5];
  v[SIZE2] = -expf (x[6]);
}

static void print_params (const float x[N_PARAMS], const char *prefix)
{
  float v[N_PARAMS];
  unpack_params (x, v);
  fprintf (stderr, "%s %g %g %g %g %g %g %g\n", prefix, v[0], v[1], v[2], v[3], v[4], v[5], v[6]);
}

/* ------------------------------------------------------------------ the device */

static void need_device (void)
{
  if (ctx) return;
  if (gt4hip_create (device_id, &ctx)) {
    fprintf (stderr, "Error: no usable GPU: %s\n", gt4hip_last_error (NULL));
    exit (1);
  }
}

static gt4hip_caller_set *upload_calls (const Call *calls, const unsigned int order[], unsigned int n)
{
  uint32_t *a = (uint32_t *) malloc ((n ? n : 1) * sizeof (uint32_t)), *b = (uint32_t *) malloc ((n ? n : 1) * sizeof (uint32_t));
  if (!a || !b) {
    fprintf (stderr, "Error: out of memory (%u markers)\n", n);
    exit (1);
  }
  for (unsigned int i = 0; i < n; i++) {
    const Call *c = &calls[order ? order[i] : i];
    a[i] = c->counts[0];
    b[i] = c->counts[1];
  }
  gt4hip_caller_set *set = NULL;
  need_device ();
  CHK (ctx, gt4hip_caller_set_create (ctx, a, b, n, &set));
  free (a);
  free (b);
  return set;
}

static gt4hip_caller_model make_model (const float v[N_PARAMS], float pB)
{
  gt4hip_caller_model m;
  m.l_viga = v[L_VIGA], m.p_0 = v[P_0], m.p_1 = v[P_1], m.p_2 = v[P_2], m.lambda = v[LAMBDA], m.size = v[SIZE], m.size2 = v[SIZE2], m.pB = pB;
  return m;
}

/* ------------------------------------------------------------------ training */

typedef struct {
  gt4hip_caller_set *set;
  unsigned int n_calls;        /* training markers */
  unsigned int n_chunks;       /* the reference's thread chunks ...                */
  unsigned int chunk_size;     /* ... of this many markers (the last one: the rest) */
  float pB, lambda_est, lambda_sigma;
} Training;

/* distanceL3 (reference :862-914) with optim_run (:845-860): the likelihood sum is one device call; the coverage penalty
 * is added once per chunk, in float, as every thread of the reference adds it to its own sum */
static float distance (const float x[N_PARAMS], Training *tr)
{
  static int iter = 1;
  float v[N_PARAMS];
  if (debug > 1) print_params (x, "Params");
  unpack_params (x, v);
  const float l_viga = v[L_VIGA], p_0 = v[P_0], p_1 = v[P_1], p_2 = v[P_2], lambda = v[LAMBDA], size = v[SIZE], size2 = v[SIZE2];
  const gt4hip_caller_model m = make_model (v, tr->pB);
  double result = 0;
  CHK (ctx, gt4hip_caller_mlogl (ctx, tr->set, 0, tr->n_calls, &m, &result));
  for (unsigned int i = 0; i < tr->n_chunks; i++) {
    unsigned int n = tr->chunk_size;
    if (i * tr->chunk_size + n > tr->n_calls) n = tr->n_calls - i * tr->chunk_size;
    result += n * (tr->lambda_est - lambda) * (tr->lambda_est - lambda) / (tr->lambda_sigma * tr->lambda_sigma);
  }
  if (p_0 + p_1 + p_2 > 1) result = result + 10000 - 100000 * (1 - p_0 - p_1 - p_2);
  const double delta0 = size + size2 * lambda / 2;
  if (delta0 < 0) result = result + 10000 + 100 * delta0;
  const double delta1 = size + size2 * l_viga;
  if (delta1 < 0) result = result + 10000 + 100 * delta1;
  if (debug > 1) fprintf (stderr, "Iteration %d delta %.6f\n", iter++, result);
  return (float) result;
}

#define NDIM N_PARAMS
#define MPTS (N_PARAMS + 1)

/* the objective at a point given in float: the point goes to x (the caller's parameters) first, as the reference's does */
static float eval_at (const float p[NDIM], float x[NDIM], Training *tr)
{
  for (int j = 0; j < NDIM; j++) x[j] = p[j];
  return distance (x, tr);
}

/* downhill_simplex (reference src/simplex.c:14-210) for 7 dimensions and 100 steps a run: `nruns` restarts around x with
 * edges dx x (0.9 .. 1.1, from rand ()) / (5 run + 1); a step reflects the worst vertex through the centre of the others,
 * expands a reflection that beats the best, and otherwise contracts, halves towards the best, mirrors at the best or
 * takes the minimum of a parabola through the last three trials, in that order.  Float and double are mixed as there. */
static void downhill_simplex (float x[NDIM], const float dx[NDIM], int nruns, Training *tr)
{
  const float al = 1.0, bt = 0.5, gm = 2.0;
  float mp[MPTS][NDIM], y[MPTS], pb[NDIM], pr[NDIM], prr[NDIM];
  y[0] = distance (x, tr);
  for (int run = 0; run < nruns; run++) {
    for (int i = 0; i < NDIM; i++) {
      for (int j = 0; j < MPTS; j++) mp[j][i] = x[i];
      mp[i][i] += dx[i] * (0.9 + 0.2 * ref_rand () / RAND_MAX) / (5 * run + 1);
    }
    for (int j = 0; j < MPTS; j++) y[j] = eval_at (mp[j], x, tr);
    for (int step = 0; step < 100; step++) {
      int lo = 0, hi, nhi;
      if (y[0] > y[1]) hi = 0, nhi = 1;
      else hi = 1, nhi = 0;
      for (int i = 0; i < MPTS; i++) {
        if (y[i] < y[lo]) lo = i;
        if (y[i] > y[hi]) nhi = hi, hi = i;
        else if (y[i] > y[nhi] && i != hi) nhi = i;
      }
      for (int j = 0; j < NDIM; j++) pb[j] = 0.0;
      for (int i = 0; i < MPTS; i++)
        if (i != hi)
          for (int j = 0; j < NDIM; j++) pb[j] += mp[i][j];
      for (int j = 0; j < NDIM; j++) {
        pb[j] /= NDIM;
        pr[j] = (1.0 + al) * pb[j] - al * mp[hi][j];
      }
      float ypr = eval_at (pr, x, tr), yprr;
      const float *take = NULL; /* the point that replaces the worst vertex, with its value */
      float ytake = 0;
      if (ypr <= y[lo]) {
        for (int j = 0; j < NDIM; j++) prr[j] = gm * pr[j] + (1.0 - gm) * pb[j];
        yprr = eval_at (prr, x, tr);
        if (ypr > yprr) take = prr, ytake = yprr;
        else take = pr, ytake = ypr;
      } else if (ypr >= y[nhi]) {
        if (ypr < y[hi]) {
          for (int j = 0; j < NDIM; j++) mp[hi][j] = pr[j];
          y[hi] = ypr;
        }
        for (int j = 0; j < NDIM; j++) prr[j] = bt * mp[hi][j] + (1.0 - bt) * pb[j];
        yprr = eval_at (prr, x, tr);
        if (yprr < y[hi]) {
          take = prr, ytake = yprr;
        } else {
          for (int j = 0; j < NDIM; j++) pr[j] = 0.5 * (mp[hi][j] + mp[lo][j]);
          ypr = eval_at (pr, x, tr);
          if (ypr < y[hi]) {
            take = pr, ytake = ypr;
          } else {
            for (int j = 0; j < NDIM; j++) prr[j] = -mp[hi][j] + 2.0 * mp[lo][j];
            yprr = eval_at (prr, x, tr);
            if (yprr < y[hi]) {
              take = prr, ytake = yprr;
            } else {
              const float xa = 3 * y[hi] - 8 * ypr + 6 * y[lo] - yprr;
              const float xb = y[hi] - 2 * y[lo] + yprr;
              const float xc = -0.5 * y[hi] + 8 * ypr / 3 - 2 * y[lo] + yprr / 6;
              const float xd = xb * xb - 4 * xa * xc;
              if (xd > 0) {
                const float lmin = 0.5 * (-xb - sqrt (xd)) / xa;
                if (isfinite (lmin))
                  for (int j = 0; j < NDIM; j++) pr[j] = lmin * mp[hi][j] + (1 - lmin) * mp[lo][j];
                else
                  for (int j = 0; j < NDIM; j++) pr[j] = 0.5f * mp[hi][j] + 0.5f * mp[lo][j];
                ypr = eval_at (pr, x, tr);
              }
              if (ypr < y[hi]) take = pr, ytake = ypr;
              else take = mp[lo], ytake = y[lo];
            }
          }
        }
      } else {
        take = pr, ytake = ypr;
      }
      for (int j = 0; j < NDIM; j++) mp[hi][j] = take[j];
      y[hi] = ytake;
    }
    int lo = 0;
    for (int i = 1; i < MPTS; i++)
      if (y[i] < y[lo]) lo = i;
    for (int i = 0; i < NDIM; i++) x[i] = mp[lo][i];
  }
}

/* train_model (reference :225-347): v in, v out; *pB is set from the training markers */
static void train_model (const Call *calls, unsigned int ncalls, unsigned int max_training, unsigned int nruns, float v[N_PARAMS], float *pB, unsigned int mul,
                         unsigned int nthreads)
{
  const unsigned int ntrain = ncalls < max_training ? ncalls : max_training;
  if (debug) fprintf (stderr, "Building training set...");
  unsigned int *train = build_training_set (ncalls, ntrain);
  if (debug) fprintf (stderr, "done\nCalculating mean...");
  double s0 = 0, s1 = 0;
  unsigned int max_c = 0;
  for (unsigned int i = 0; i < ntrain; i++) {
    const unsigned int c0 = calls[train[i]].counts[0], c1 = calls[train[i]].counts[1];
    if (c0 > max_c) max_c = c0;
    if (c1 > max_c) max_c = c0; /* (sic; debug output only) */
    s0 += c0;
    s1 += c1;
  }
  *pB = allele_freq (calls, train, ntrain);
  const double mean = (s0 + s1) / ntrain;
  if (debug) {
    fprintf (stderr, "done\nA %g B %g\nTraining size %u mean %.1f\npB %.3f\nMax count %u\n", s0, s1, ntrain, mean, *pB, max_c);
  }
  if (mean == 0) {
    fprintf (stderr, "No calls in training sample, aborting model optimization\n");
    return;
  }
  if (v[LAMBDA] == 0) v[LAMBDA] = mul * mean;
  float x[N_PARAMS], dx[N_PARAMS];
  x[0] = logit_clamped (v[0], MIN_P, MAX_E);
  x[1] = logit_clamped (v[1], MIN_P, 1 - MIN_P);
  x[2] = logit_clamped (v[2], MIN_P, 1 - MIN_P);
  x[3] = logit_clamped (v[3], MIN_P, 1 - MIN_P);
  x[LAMBDA] = logf (v[LAMBDA]);
  x[5] = v[5];
  x[6] = logf (-v[6]);
  for (int i = 0; i < N_PARAMS; i++) dx[i] = x[i] / 10;
  Training tr;
  tr.n_calls = ntrain;
  tr.pB = *pB;
  tr.lambda_est = v[LAMBDA];
  tr.lambda_sigma = tr.lambda_est / 4;
  tr.chunk_size = (ntrain + nthreads - 1) / nthreads;
  if (tr.chunk_size < 2000) tr.chunk_size = 2000;
  tr.n_chunks = (ntrain + tr.chunk_size - 1) / tr.chunk_size;
  tr.set = upload_calls (calls, train, ntrain); /* the training markers, in training order, resident for every evaluation */
  downhill_simplex (x, dx, (int) nruns, &tr);
  if (debug) {
    const float dist = distance (x, &tr);
    print_params (x, "Best");
    fprintf (stderr, "Best distance %.6f\n", dist);
  }
  gt4hip_caller_set_free (tr.set);
  unpack_params (x, v);
  free (train);
}

/* ------------------------------------------------------------------ output */

/* print_genotypes (reference :390-468) */
static void print_genotypes (const Text *t, const Call *calls, unsigned int ncalls, const float params[N_PARAMS], float pB, unsigned int nalleles, float pc,
                             unsigned int alt)
{
  if (!ncalls) return;
  gt4hip_caller_set *set = upload_calls (calls, NULL, ncalls);
  const gt4hip_caller_model m = make_model (params, pB);
  const unsigned int piece = ncalls < PRINT_PIECE ? ncalls : PRINT_PIECE;
  uint8_t *best = (uint8_t *) malloc (piece);
  double *a_best = (double *) malloc ((size_t) piece * 8), *a_sum = (double *) malloc ((size_t) piece * 8);
  double *a_all = alt ? (double *) malloc ((size_t) piece * 8 * N_GT) : NULL;
  if (!best || !a_best || !a_sum || (alt && !a_all)) {
    fprintf (stderr, "Error: out of memory (%u markers)\n", piece);
    exit (1);
  }
  /* a NaN as this host's arithmetic makes it: the sign printf shows is the reference's then, not the device's */
  volatile double zero = 0.0;
  const double host_nan = zero / zero;
  unsigned int iter = 0;
  for (unsigned int pos = 0; pos < ncalls; pos += piece) {
    const unsigned int n = ncalls - pos < piece ? ncalls - pos : piece;
    if (debug > 1) fprintf (stderr, "Printing iteration %u\n", iter++);
    CHK (ctx, gt4hip_caller_probabilities (ctx, set, pos, n, &m, best, a_best, a_sum, a_all));
    for (unsigned int k = 0; k < n; k++) {
      const Call *call = &calls[pos + k];
      const unsigned int best_gt = best[k];
      const double top = isnan (a_best[k]) ? host_nan : a_best[k], summa = isnan (a_sum[k]) ? host_nan : a_sum[k];
      const unsigned char *p = t->data + t->start[call->line];
      char c[256];
      unsigned int j = 0;
      while (p[j] != '\t' && j < 255 && p + j < t->data + t->size) j++;
      memcpy (c, p, j);
      c[j] = 0;
      fprintf (stdout, "%s", c);
      unsigned int cancall = 0;
      if (nalleles == 0) cancall = 1;
      else if (nalleles == 1) cancall = best_gt == GT_A || best_gt == GT_B;
      else if (nalleles == 2) cancall = best_gt == GT_AA || best_gt == GT_AB || best_gt == GT_BB;
      if (top < pc) cancall = 0;
      if (!call->counts[0] && !call->counts[1]) cancall = 0;
      if (cancall) fprintf (stdout, "\t%s\t%.2f", GT_NAMES[best_gt], top / summa);
      else fprintf (stdout, "\tNC\t");
      fprintf (stdout, "\t%u\t%u", call->counts[0], call->counts[1]);
      if (alt)
        for (j = 0; j < N_GT; j++) {
          const double a = a_all[(size_t) k * N_GT + j];
          fprintf (stdout, "\t%.2f", (isnan (a) ? host_nan : a) / summa);
        }
      fprintf (stdout, "\n");
    }
    if (debug > 1) fprintf (stderr, "Writing, pos %u\n", pos + n);
  }
  free (best), free (a_best), free (a_sum), free (a_all);
  gt4hip_caller_set_free (set);
}

/* what this program refuses in the text, before anything is computed */
static void check_text (const Options *o, const Text *t, const unsigned int *groups[3], const unsigned int n[3])
{
  const unsigned char *tok[16];
  for (int g = 0; g < 3; g++)
    for (unsigned int i = 0; i < n[g]; i++) {
      const unsigned int ntok = line_tokens (t, groups[g][i], tok);
      if (ntok < 4) {
        fprintf (stderr, "Error: %s: line %u has %u tokens: a marker line is ID, N_KMERS and at least one pair of counts\n", o->call_fn, groups[g][i] + 1, ntok);
        exit (1);
      }
    }
}

int main (int argc, const char *argv[])
{
  static Options o;
  gt4_cli_read_environment (&o.device, &o.env_verbose);
  ref_srand (1);
  parse_argv (argc, argv, &o);
  debug = o.debug;
  device_id = o.device;
  float *params = o.params, x_params[N_PARAMS], pB;
  if (!o.call_fn) {
    fprintf (stderr, "No input file specified\n");
    print_usage (stderr);
  }
  if (o.nthreads < 1 || o.nthreads > MAX_THREADS) {
    fprintf (stderr, "Invalid number of threads %u - should be 1-%u\n", o.nthreads, MAX_THREADS);
    print_usage (stderr);
    fprintf (stderr, "Error: --num_threads %u is not accepted (the reference goes on with a pool of that many threads)\n", o.nthreads);
    return 1;
  }
  if (o.model == MODEL_HAPLOID && !o.params_specified) {
    params[P_1] = 0.985023f;
    params[P_2] = 0.014934f;
  }
  /* the text and its lines (reference :648-665) */
  if (debug) fprintf (stderr, "Reading %s...", o.call_fn ? o.call_fn : "(null)");
  Text t;
  memset (&t, 0, sizeof t);
  t.data = read_text (o.call_fn, &t.size);
  if (!t.data) {
    fprintf (stderr, "Cannot read %s\n", o.call_fn ? o.call_fn : "(null)");
    return 1;
  }
  for (uint64_t i = 0; i < t.size; i++) t.nlines += t.data[i] == '\n';
  if (t.nlines < 1) {
    fprintf (stderr, "File contains no lines\n");
    return 1;
  }
  if (t.data[t.size - 1] != '\n') {
    fprintf (stderr, "Error: %s does not end with a newline (byte %llu of %llu): the last line is not complete\n", o.call_fn, (unsigned long long) t.size - 1,
             (unsigned long long) t.size);
    return 1;
  }
  if (debug) fprintf (stderr, "done (%u lines)\nBuilding line table...", t.nlines);
  t.start = (uint64_t *) malloc (((size_t) t.nlines + 1) * sizeof (uint64_t));
  if (!t.start) {
    fprintf (stderr, "Error: out of memory (%u lines)\n", t.nlines);
    return 1;
  }
  t.start[0] = 0;
  for (uint64_t i = 0, l = 0; i < t.size; i++)
    if (t.data[i] == '\n') t.start[++l] = i + 1;
  if (debug) fprintf (stderr, "done\nCounting chromosomes...");
  /* autosomes (or every line), X, Y by the first byte (:667-694) */
  unsigned int n[3] = { 0, 0, 0 }, *idx[3];
  for (int g = 0; g < 3; g++) idx[g] = (unsigned int *) malloc ((size_t) t.nlines * sizeof (unsigned int));
  if (!idx[0] || !idx[1] || !idx[2]) {
    fprintf (stderr, "Error: out of memory (%u lines)\n", t.nlines);
    return 1;
  }
  for (unsigned int i = 0; i < t.nlines; i++) {
    const unsigned char c = t.data[t.start[i]];
    if (o.model != MODEL_FULL || (c > '0' && c <= '9')) idx[0][n[0]++] = i;
    else if (c == 'X') idx[1][n[1]++] = i;
    else if (c == 'Y') idx[2][n[2]++] = i;
  }
  const unsigned int na = n[0], nx = n[1], ny = n[2], *a = idx[0], *x = idx[1], *y = idx[2];
  if (debug) fprintf (stderr, "done\nAutosomes %u X %u Y %u\n", na, nx, ny);
  {
    const unsigned int *groups[3] = { a, x, y };
    check_text (&o, &t, groups, n);
  }
  /* pair medians and sex (:696-732) */
  unsigned int a_med, x_med = 0, y_med = 0;
  if (debug) fprintf (stderr, "Calculating medians...");
  a_med = get_pair_median (&t, a, na);
  if (o.model == MODEL_FULL) {
    x_med = get_pair_median (&t, x, nx);
    y_med = get_pair_median (&t, y, ny);
  }
  if (debug) fprintf (stderr, "done\nAutosomes/unspecified %u X %u Y %u\n", a_med, x_med, y_med);
  double p_XX = 0, p_X = 0, p_Y = 0, p_1 = 0;
  if (o.model == MODEL_FULL) {
    p_XX = poisson (x_med, a_med);
    p_X = poisson (x_med, a_med / 2);
    p_Y = poisson (y_med, a_med / 2);
    p_1 = poisson (y_med, 1);
    if (debug) fprintf (stderr, "XX %g X %g Y %g 0 %g\nProbably %s\n", p_XX, p_X, p_Y, p_1, p_XX > p_X ? "female" : "male");
    if (p_XX > p_X ? p_Y > p_1 : p_Y < p_1) fprintf (stderr, "Y inconsistency: p_1 %g p_Y %g p_X %g p_XX %g\n", p_1, p_Y, p_X, p_XX);
  }
  const int female = p_XX > p_X;
  /* the autosome model (:734-762) */
  if (debug) fprintf (stderr, "Reading autosome/unspecified calls...");
  Call *calls_a = parse_calls (&t, a, na, a_med), *calls_x = NULL;
  if (debug) fprintf (stderr, "done\n");
  if (o.nruns && na > 0) {
    if (debug) fprintf (stderr, "Training autosome/unspecified model\n");
    train_model (calls_a, na, o.max_training, o.nruns, params, &pB, o.model == MODEL_HAPLOID ? 2 : 1, o.nthreads);
  } else {
    pB = allele_freq (calls_a, NULL, na);
  }
  static char out_buffer[1 << 20];
  setvbuf (stdout, out_buffer, _IOFBF, sizeof out_buffer);
  if (o.info) {
    fprintf (stdout, "#gmer_counter version %u.%u.%u (%s)\n", GT4_VERSION_MAJOR, GT4_VERSION_MINOR, GT4_VERSION_MICRO, GT4_VERSION_QUALIFIER); /* (sic) */
    if (o.model == MODEL_FULL) fprintf (stdout, "#Sex\t%s\n", female ? "F" : "M");
    fprintf (stdout, "#EstimatedCoverage\t%g\n", params[LAMBDA]);
    fprintf (stdout, "#AverageMAF\t%g\n", pB);
    fprintf (stdout, "#AutosomeModel\t%g %g %g %g %g %g %g\n", params[L_VIGA], params[P_0], params[P_1], params[P_2], params[LAMBDA], params[SIZE], params[SIZE2]);
  }
  /* the X model: the autosomes' unless a male's X is trained (:764-782) */
  memcpy (x_params, params, sizeof x_params);
  if (o.model == MODEL_FULL) {
    if (debug) fprintf (stderr, "Reading X calls...");
    calls_x = parse_calls (&t, x, nx, x_med);
    if (debug) fprintf (stderr, "done\n");
    if (nx > 0 && o.nruns && !female) {
      x_params[P_1] = 0.98f;
      x_params[P_2] = 0.01f;
      if (debug) fprintf (stderr, "Training X model\n");
      train_model (calls_x, nx, o.max_training, o.nruns, x_params, &pB, 2, o.nthreads);
      if (o.info)
        fprintf (stdout, "#XModel\t%g %g %g %g %g %g %g\n", x_params[L_VIGA], x_params[P_0], x_params[P_1], x_params[P_2], x_params[LAMBDA], x_params[SIZE],
                 x_params[SIZE2]);
    }
  }
  /* genotypes (:784-814) */
  if (o.print_gt) {
    if (o.header) {
      fprintf (stdout, "#ID\tGT\tPROB\tA_KMERS\tB_KMERS");
      for (unsigned int j = 0; j < N_GT; j++) fprintf (stdout, "\t%s", GT_NAMES[j]);
      fprintf (stdout, "\n");
    }
    const unsigned int any = o.non_canonical ? 0 : 2, one = o.non_canonical ? 0 : 1;
    print_genotypes (&t, calls_a, na, params, pB, o.model != MODEL_HAPLOID ? any : one, o.prob_cutoff, o.alternatives);
    if (o.model == MODEL_FULL) {
      if (female) {
        print_genotypes (&t, calls_x, nx, params, pB, any, o.prob_cutoff, o.alternatives);
      } else {
        print_genotypes (&t, calls_x, nx, x_params, pB, one, o.prob_cutoff, o.alternatives);
        if (debug) fprintf (stderr, "Reading Y calls...");
        Call *calls_y = parse_calls (&t, y, ny, y_med);
        if (debug) fprintf (stderr, "done\n");
        print_genotypes (&t, calls_y, ny, x_params, pB, one, o.prob_cutoff, o.alternatives);
        free (calls_y);
      }
    }
  }
  fflush (stdout);
  if (ctx) gt4hip_destroy (ctx);
  return 0;
}
