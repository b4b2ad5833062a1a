/* gt4hip_caller.hip -- gmer_caller on the device, gfx950, wave64: the 15 genotype likelihoods of a marker's two k-mer
 * counts (reference src/genotypes.c:9-124, src/binomial.c:67-80, :207-244) and what gmer_caller makes of them: the
 * objective of its training, mlogL3 (src/gmer_caller.c:821-843), and the best genotype of every marker, calc_run (:365-388).
 *
 * A likelihood is q0 * q1 * p[j]: two negative-binomial densities, one per count, and the genotype's prior.  Only five
 * means occur -- l_viga, lambda / 2, lambda, 1.5 lambda, 2 lambda -- so a marker needs ten densities, not the thirty the
 * reference evaluates.  Everything that depends on the model alone is computed per call on the HOST with libm, in the
 * reference's types and order (model_args), and reaches the kernels as arguments: it is bit-identical to the reference.
 * Per density the device is left with
 *     exp ((lgamma (k + r) - lgamma (r) - log k!) + log (p) k + log (1 - p) r)        (k = 0: the first term is 0)
 * in double, added in that order, without contraction into fused multiply-adds (the reference's host has none).  log k!
 * is the reference's table of 16,384 running sums of log (i), built on the host and uploaded once per context; counts at
 * and above 16,384 take its loop of log () on the device.  The products are formed as the reference forms them.
 *
 *   k_caller_mlogl   a thread takes markers gtid, gtid + threads, ... and adds log (max (sum of a[], 1e-30)) in that
 *                    order; the workgroup adds its 256 threads by a tree in LDS; the sum is published, a ticket drawn, and
 *                    the workgroup that draws the last one adds all the sums in index order by the same tree and
 *                    writes the negated total.  The grid is a function of n alone.  No floating-point atomics, no waiting.
 *   k_caller_probs   a thread per marker: best index (strict >, from 0), its likelihood, the sum, on request all 15.
 */
#pragma clang fp contract(off)
#define GT4_RESOLVE_LOOKBACK 0 /* (no chained scan of tile totals here) */
#include "gt4hip_device.h"
#include "gt4hip_host.h"

#include <math.h>
#include <string.h>

namespace gt4 {
namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_MAX_GRID = 1024;      /* workgroups of k_caller_mlogl at most: their sums are added by one workgroup */
static_assert (CL_THREADS == GT4HIP_CALLER_THREADS && CL_MAX_GRID == GT4HIP_CALLER_MAX_GRID, "counters \"caller_threads\" and \"caller_max_grid\" (gt4hip_host.h)");
constexpr u32 CL_MAX_PROD = 16384;     /* entries of the log-factorial table (MAX_PROD, src/binomial.c:11) */
constexpr int CL_MEANS = 5;
constexpr int CL_GENOTYPES = (int) GT4HIP_CALLER_GENOTYPES;
/* ctx->caller_tab: the table, the workgroups' sums, the result, the ticket */
constexpr size_t CL_TAB_BYTES = (size_t) CL_MAX_PROD * 8 + (size_t) CL_MAX_GRID * 8 + 64;

/* what a call computes of its model on the host */
struct CallerArgs {
  double prior[CL_GENOTYPES];
  double r[CL_MEANS];     /* size + size2 x mean                      */
  double lg_r[CL_MEANS];  /* lgamma (r)                               */
  double logp[CL_MEANS];  /* log (p), p = mean / (r + mean)           */
  double c1[CL_MEANS];    /* log (1 - p) * r                          */
  u32 zero;               /* bit m: r <= 0 or mean <= 0: the density is 0 (dnbinom_mu, src/binomial.c:240-241) */
};

/* genotype j is (count A under mean MEAN_A[j]) x (count B under mean MEAN_B[j]) x prior[j] (src/genotypes.c:50-123);
 * means: 0 l_viga, 1 lambda / 2, 2 lambda, 3 1.5 lambda, 4 2 lambda */
#define CL_FOR_GENOTYPES(F) F (0, 0, 0) F (1, 1, 0) F (2, 0, 1) F (3, 2, 0) F (4, 1, 1) F (5, 0, 2) F (6, 3, 0) F (7, 2, 1) F (8, 1, 2) F (9, 0, 3) \
  F (10, 4, 0) F (11, 3, 1) F (12, 1, 3) F (13, 2, 2) F (14, 0, 4)

/* log_factorial (src/binomial.c:67-80) */
__device__ __forceinline__ double log_factorial (u32 v, const double *__restrict__ lfact)
{
  double dv = (double) v, val = 0;
  while (v >= CL_MAX_PROD) {
    val += log (dv);
    dv -= 1;
    v -= 1;
  }
  return val + lfact[v];
}

/* dnbinom (x = k) (src/binomial.c:223-234) with the model's part of it precomputed */
__device__ __forceinline__ double density_term (u32 k, double r, double lg_r, double logp, double c1, const double *__restrict__ lfact)
{
  double c = 0;
  if (k) c = lgamma ((double) k + r) - lg_r - log_factorial (k, lfact);
  const double p0 = logp * (double) k;
  return exp (c + p0 + c1);
}

/* a[0..14] of one marker as 15 named values (no array a thread would index at run time) */
struct Likelihoods {
#define CL_FIELD(j, ma, mb) double a##j;
  CL_FOR_GENOTYPES (CL_FIELD)
#undef CL_FIELD
};

/* The ten densities, dnbinom_mu (:236-244) of either count under every mean, by a loop that is NOT unrolled: one copy of
 * lgamma's code.  (The file is built without machine LICM, csrc/Makefile: hoisted out of this loop, lgamma's constants alone
 * take every scalar register and 220 vector registers.)  The model's terms are read from the kernel's
 * arguments by the loop's index; the results go to named values by selects. */
__device__ __forceinline__ Likelihoods likelihoods (u32 ka, u32 kb, const CallerArgs &g, const double *__restrict__ lfact)
{
  double qa0 = 0, qa1 = 0, qa2 = 0, qa3 = 0, qa4 = 0, qb0 = 0, qb1 = 0, qb2 = 0, qb3 = 0, qb4 = 0;
#pragma unroll 1
  for (int t = 0; t < 2 * CL_MEANS; t++) { /* t = 2 m: count A under mean m; 2 m + 1: count B */
    const int m = t >> 1;
    if (g.zero >> m & 1u) continue; /* (uniform) */
    const double v = density_term (t & 1 ? kb : ka, g.r[m], g.lg_r[m], g.logp[m], g.c1[m], lfact);
    if (t == 0) qa0 = v;
    if (t == 1) qb0 = v;
    if (t == 2) qa1 = v;
    if (t == 3) qb1 = v;
    if (t == 4) qa2 = v;
    if (t == 5) qb2 = v;
    if (t == 6) qa3 = v;
    if (t == 7) qb3 = v;
    if (t == 8) qa4 = v;
    if (t == 9) qb4 = v;
  }
  Likelihoods l;
#define CL_PRODUCT(j, ma, mb) l.a##j = qa##ma * qb##mb * g.prior[j];
  CL_FOR_GENOTYPES (CL_PRODUCT)
#undef CL_PRODUCT
  return l;
}

/* a[0] + a[1] + ... + a[14], in that order */
__device__ __forceinline__ double likelihood_sum (const Likelihoods &l)
{
  double s = l.a0;
#define CL_ADD(j, ma, mb) if (j) s += l.a##j;
  CL_FOR_GENOTYPES (CL_ADD)
#undef CL_ADD
  return s;
}

/* v of the workgroup's 256 threads added by a fixed tree; the total is returned to thread 0 (others: a partial one) */
__device__ __forceinline__ double block_tree_sum (double v, double *s)
{
  s[threadIdx.x] = v;
  __syncthreads ();
#pragma unroll
  for (int w = CL_THREADS / 2; w > 0; w >>= 1) {
    if ((int) threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads ();
  }
  const double total = s[0];
  __syncthreads ();
  return total;
}

/* tab: the context's block -- the log-factorial table, then the workgroups' sums, the result and the ticket.  Every set of
 * the context shares it, which holds because a context has ONE stream and one host thread (include/gt4hip.h): launches of
 * this kernel never overlap, and gt4hip_caller_mlogl reads the result back before it returns.  The ticket is 0 between
 * launches because the workgroup that draws the last one resets it; a launch that does not finish (a failed device)
 * leaves the context unusable for this call as for every other. */
__global__ __launch_bounds__ (CL_THREADS) void k_caller_mlogl (CallerArgs g, const u32 *__restrict__ ca, const u32 *__restrict__ cb, u64 n, u64 *tab)
{
  const double *lfact = (const double *) tab;
  u64 *partial = tab + CL_MAX_PROD;
  double *out = (double *) (tab + CL_MAX_PROD + CL_MAX_GRID);
  u32 *ticket = (u32 *) (tab + CL_MAX_PROD + CL_MAX_GRID + 1);
  __shared__ double s_sum[CL_THREADS];
  __shared__ u32 s_last;
  double sum = 0;
  for (u64 i = (u64) blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * CL_THREADS) {
    const Likelihoods l = likelihoods (ca[i], cb[i], g, lfact);
    double call_sum = likelihood_sum (l);
    if (call_sum < 1e-30) call_sum = 1e-30;
    sum += log (call_sum);
  }
  const double total = block_tree_sum (sum, s_sum);
  if (threadIdx.x == 0) {
    publish_u64 (&partial[blockIdx.x], (u64) __double_as_longlong (total));
    __threadfence ();
    s_last = atomicAdd (ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads ();
  if (!s_last) return;
  __threadfence ();
  double v = 0;
  for (u32 b = threadIdx.x; b < gridDim.x; b += CL_THREADS) v += __longlong_as_double ((long long) peek_u64 (&partial[b]));
  const double all = block_tree_sum (v, s_sum);
  if (threadIdx.x == 0) {
    *out = -all;
    *ticket = 0; /* for the next launch on the stream */
  }
}

template <bool ALL>
__global__ __launch_bounds__ (CL_THREADS) void k_caller_probs (CallerArgs g, const u32 *__restrict__ ca, const u32 *__restrict__ cb, u64 n,
                                                               const double *__restrict__ lfact, unsigned char *__restrict__ best, double *__restrict__ a_best,
                                                               double *__restrict__ a_sum, double *__restrict__ a_all)
{
  for (u64 i = (u64) blockIdx.x * CL_THREADS + threadIdx.x; i < n; i += (u64) gridDim.x * CL_THREADS) {
    const Likelihoods l = likelihoods (ca[i], cb[i], g, lfact);
    double top = l.a0;
    u32 at = 0;
#define CL_BEST(j, ma, mb) if (j && l.a##j > top) top = l.a##j, at = j;
    CL_FOR_GENOTYPES (CL_BEST)
#undef CL_BEST
    best[i] = (unsigned char) at;
    a_best[i] = top;
    a_sum[i] = likelihood_sum (l);
    if (ALL) {
#define CL_STORE(j, ma, mb) a_all[i * CL_GENOTYPES + j] = l.a##j;
      CL_FOR_GENOTYPES (CL_STORE)
#undef CL_STORE
    }
  }
}

/* combinations_d (n, k) for n in {3, 4} (src/binomial.c:97-123): exp of sums of log (i) added in the order of t_log_sums_d */
double combinations (unsigned n, unsigned k)
{
  if (!k || k == n) return exp (0.0);
  if (k == 1) return exp (log ((double) n));
  double sums[5] = { 0, 0, 0, 0, 0 };
  for (unsigned i = 1; i <= 4; i++) {
    sums[i] = log ((double) i);
    for (unsigned j = 2; j < i; j++) sums[i] += log ((double) j);
  }
  return exp (sums[n] - sums[n - k] - sums[k]);
}

/* dbinom (src/binomial.c:176-185) */
double dbinom (unsigned x, unsigned n, double p)
{
  if (x == 0 && p == 0) return 1;
  if (x == n && p == 1) return 1;
  const double c = combinations (n, x), p0 = pow (p, (double) x), p1 = pow (1 - p, (double) (n - x));
  return c * p0 * p1;
}

/* the head of genotype_probabilities (src/genotypes.c:17-48) and the arguments of its 30 dnbinom_mu calls (:50-123) */
void model_args (const gt4hip_caller_model *m, CallerArgs *g)
{
  const double l_viga = m->l_viga, p_0 = m->p_0, p_1 = m->p_1, p_2 = m->p_2, lambda = m->lambda, size = m->size, size2 = m->size2;
  const double pb = m->pB, pa = 1 - pb;
  double *p = g->prior;
  p[0] = p_0;
  p[1] = pa * p_1;
  p[2] = pb * p_1;
  p[3] = pa * pa * p_2;
  p[4] = 2 * pa * pb * p_2;
  p[5] = pb * pb * p_2;
  const double p_lisa = 1 - p_0 - p_1 - p_2;
  double p_lisa1 = 0, p_lisa2 = 0;
  if (p_lisa >= 0) {
    p_lisa1 = (-1 + sqrtf ((float) (1 + 4 * p_lisa))) / 2;
    p_lisa2 = p_lisa1 * p_lisa1;
  }
  p[6] = dbinom (3, 3, pa) * p_lisa1;   /* AAA  */
  p[9] = dbinom (0, 3, pa) * p_lisa1;   /* BBB  */
  p[7] = dbinom (2, 3, pa) * p_lisa1;   /* AAB  */
  p[8] = dbinom (1, 3, pa) * p_lisa1;   /* BBA  */
  p[10] = dbinom (4, 4, pa) * p_lisa2;  /* AAAA */
  p[14] = dbinom (0, 4, pa) * p_lisa2;  /* BBBB */
  p[11] = dbinom (3, 4, pa) * p_lisa2;  /* AAAB */
  p[13] = dbinom (2, 4, pa) * p_lisa2;  /* AABB */
  p[12] = dbinom (1, 4, pa) * p_lisa2;  /* BBBA */
  const double mu[CL_MEANS] = { l_viga, lambda / 2, lambda, lambda * 1.5, lambda * 2 };
  const double r[CL_MEANS] = { size + size2 * l_viga, size + size2 * lambda / 2, size + size2 * lambda, size + size2 * lambda * 1.5, size + size2 * lambda * 2 };
  g->zero = 0;
  for (int i = 0; i < CL_MEANS; i++) {
    if (r[i] <= 0 || mu[i] <= 0) { /* (a NaN compares false, as in the reference, and goes on to NaN densities) */
      g->zero |= 1u << i;
      g->r[i] = g->lg_r[i] = g->logp[i] = g->c1[i] = 0; /* never read */
      continue;
    }
    const double pr = mu[i] / (r[i] + mu[i]);
    g->r[i] = r[i];
    g->logp[i] = log (pr);
    g->c1[i] = log (1 - pr) * r[i];
    g->lg_r[i] = lgamma (r[i]);
  }
}

/* the context's table block, made and filled by the first set */
int caller_tab (gt4hip_context *ctx)
{
  if (ctx->caller_tab) return GT4HIP_OK;
  void *d = NULL;
  const hipError_t e = gt4hip_dev_alloc (ctx, &d, CL_TAB_BYTES);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "gt4hip_caller_set_create: %zu bytes for the log-factorial table: %s", CL_TAB_BYTES, hipGetErrorString (e));
  std::vector<double> t (CL_MAX_PROD);
  t[0] = 0;
  for (u32 i = 1; i < CL_MAX_PROD; i++) t[i] = t[i - 1] + log ((double) i); /* init_combination_tables, src/binomial.c:22-29 */
  hipError_t e2 = hipMemsetAsync (d, 0, CL_TAB_BYTES, ctx->stream);
  if (e2 == hipSuccess) e2 = hipMemcpyAsync (d, t.data (), (size_t) CL_MAX_PROD * 8, hipMemcpyHostToDevice, ctx->stream);
  if (e2 == hipSuccess) e2 = hipStreamSynchronize (ctx->stream);
  if (e2 != hipSuccess) {
    hipFree (d);
    return gt4hip_fail (ctx, GT4HIP_EHIP, "gt4hip_caller_set_create: uploading the log-factorial table failed: %s", hipGetErrorString (e2));
  }
  ctx->caller_tab = d;
  return GT4HIP_OK;
}

inline const double *tab_lfact (const gt4hip_context *ctx) { return (const double *) ctx->caller_tab; }
inline const double *tab_result (const gt4hip_context *ctx) { return (const double *) ctx->caller_tab + CL_MAX_PROD + CL_MAX_GRID; }

/* workgroups of k_caller_mlogl for n markers: a function of n alone, so that a sum does not depend on the device */
inline int mlogl_grid (u64 n)
{
  const u64 b = (n + CL_THREADS - 1) / CL_THREADS;
  return (int) (b < 1 ? 1 : b < (u64) CL_MAX_GRID ? b : (u64) CL_MAX_GRID);
}

}  // namespace
}  // namespace gt4

using namespace gt4;

struct gt4hip_caller_set {
  gt4hip_context *ctx;
  u32 *a, *b;
  void *a_owner, *b_owner;
  u64 n;
  double last_ms;
};

extern "C" void gt4hip_caller_set_free (gt4hip_caller_set *set)
{
  if (!set) return;
  gt4hip_block_free (set->a_owner);
  gt4hip_block_free (set->b_owner);
  delete set;
}

extern "C" uint64_t gt4hip_caller_set_n (const gt4hip_caller_set *set) { return set ? set->n : 0; }
extern "C" double gt4hip_caller_set_last_ms (const gt4hip_caller_set *set) { return set ? set->last_ms : 0.0; }

extern "C" int gt4hip_caller_set_create (gt4hip_context *ctx, const uint32_t *a_counts, const uint32_t *b_counts, uint64_t n, gt4hip_caller_set **out)
{
  if (!ctx || !out || (n && (!a_counts || !b_counts))) return GT4HIP_EINVAL;
  *out = NULL;
  if (n >= (1ull << 40)) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_caller_set_create: %llu markers", (unsigned long long) n);
  HIPCHK (ctx, hipSetDevice (ctx->device));
  int rc = caller_tab (ctx);
  if (rc) return rc;
  gt4hip_caller_set *set = new (std::nothrow) gt4hip_caller_set ();
  if (!set) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  set->ctx = ctx;
  set->n = n;
  set->last_ms = 0;
  set->a_owner = set->b_owner = NULL;
  rc = gt4hip_block_alloc (ctx, n ? n * 4 : 16, (void **) &set->a, &set->a_owner);
  if (!rc) rc = gt4hip_block_alloc (ctx, n ? n * 4 : 16, (void **) &set->b, &set->b_owner);
  if (!rc && n) rc = gt4hip_io_upload (ctx, a_counts, set->a, n * 4);
  if (!rc && n) rc = gt4hip_io_upload (ctx, b_counts, set->b, n * 4);
  if (rc) {
    gt4hip_caller_set_free (set);
    return rc;
  }
  *out = set;
  return GT4HIP_OK;
}

namespace {

int check_range (gt4hip_context *ctx, const gt4hip_caller_set *set, u64 first, u64 n, const char *who)
{
  if (first > set->n || n > set->n - first)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "%s: [%llu, +%llu) of %llu markers", who, (unsigned long long) first, (unsigned long long) n, (unsigned long long) set->n);
  return GT4HIP_OK;
}

}  // namespace

extern "C" int gt4hip_caller_mlogl (gt4hip_context *ctx, gt4hip_caller_set *set, uint64_t first, uint64_t n, const gt4hip_caller_model *m, double *sum)
{
  if (!ctx || !set || set->ctx != ctx || !m || !sum) return GT4HIP_EINVAL;
  int rc = check_range (ctx, set, first, n, "gt4hip_caller_mlogl");
  if (rc) return rc;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  CallerArgs g;
  model_args (m, &g);
  HIPCHK (ctx, hipEventRecord (ctx->ev[0], ctx->stream));
  hipLaunchKernelGGL (k_caller_mlogl, dim3 (mlogl_grid (n)), dim3 (CL_THREADS), 0, ctx->stream, g, (const u32 *) set->a + first, (const u32 *) set->b + first, (u64) n,
                      (u64 *) ctx->caller_tab);
  HIPCHK (ctx, hipGetLastError ());
  HIPCHK (ctx, hipEventRecord (ctx->ev[1], ctx->stream));
  rc = gt4hip_read_back (ctx, ctx->scratch_host, tab_result (ctx), 8, "gt4hip_caller_mlogl: reading the sum back failed");
  if (rc) return rc;
  float ms = 0;
  set->last_ms = hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess ? ms : 0.0;
  memcpy (sum, &ctx->scratch_host[0], 8);
  return GT4HIP_OK;
}

extern "C" int gt4hip_caller_probabilities (gt4hip_context *ctx, gt4hip_caller_set *set, uint64_t first, uint64_t n, const gt4hip_caller_model *m,
                                            uint8_t *best, double *a_best, double *a_sum, double *a_all)
{
  if (!ctx || !set || set->ctx != ctx || !m || (n && (!best || !a_best || !a_sum))) return GT4HIP_EINVAL;
  int rc = check_range (ctx, set, first, n, "gt4hip_caller_probabilities");
  if (rc) return rc;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  set->last_ms = 0;
  if (!n) return GT4HIP_OK;
  CallerArgs g;
  model_args (m, &g);
  /* a piece: its results in one block -- sums, best likelihoods, on request all 15, the indices last */
  const size_t per = 8 + 8 + (a_all ? 8 * (size_t) CL_GENOTYPES : 0) + 1;
  const u64 piece_max = ctx->caller_piece ? ctx->caller_piece : a_all ? 1ull << 20 : 1ull << 22;
  u64 piece = n < piece_max ? n : piece_max;
  TempBlocks blk;
  char *d = NULL;
  for (;;) {
    rc = blk.get (ctx, (size_t) piece * per + 64, (void **) &d);
    if (rc != GT4HIP_ENOMEM || piece <= 4096) break;
    piece /= 2; /* what the pool and the driver still give */
  }
  if (rc) return rc;
  double *d_sum = (double *) d, *d_best = d_sum + piece, *d_all = a_all ? d_best + piece : NULL;
  unsigned char *d_idx = (unsigned char *) (d_best + piece + (a_all ? piece * CL_GENOTYPES : 0));
  for (u64 at = 0; at < n; at += piece) {
    const u64 len = n - at < piece ? n - at : piece;
    const u32 *ca = set->a + first + at, *cb = set->b + first + at;
    const int grid = gt4hip_grid (ctx, len, CL_THREADS);
    HIPCHK (ctx, hipEventRecord (ctx->ev[0], ctx->stream));
    if (a_all) hipLaunchKernelGGL (k_caller_probs<true>, dim3 (grid), dim3 (CL_THREADS), 0, ctx->stream, g, ca, cb, len, tab_lfact (ctx), d_idx, d_best, d_sum, d_all);
    else hipLaunchKernelGGL (k_caller_probs<false>, dim3 (grid), dim3 (CL_THREADS), 0, ctx->stream, g, ca, cb, len, tab_lfact (ctx), d_idx, d_best, d_sum, d_all);
    HIPCHK (ctx, hipGetLastError ());
    HIPCHK (ctx, hipEventRecord (ctx->ev[1], ctx->stream));
    HIPCHK (ctx, hipMemcpyAsync (a_sum + at, d_sum, (size_t) len * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK (ctx, hipMemcpyAsync (a_best + at, d_best, (size_t) len * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (a_all) HIPCHK (ctx, hipMemcpyAsync (a_all + at * CL_GENOTYPES, d_all, (size_t) len * 8 * CL_GENOTYPES, hipMemcpyDeviceToHost, ctx->stream));
    rc = gt4hip_read_back (ctx, best + at, d_idx, (size_t) len, "gt4hip_caller_probabilities: reading the results back failed");
    if (rc) return rc;
    float ms = 0;
    if (hipEventElapsedTime (&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) set->last_ms += ms;
  }
  return GT4HIP_OK;
}
