/*
 * gt4hip_multi.hip -- operations on N lists: gt4hip_union_multi (levels of launches of the N-way tile kernel of
 * gt4hip_nway.hip, or the pairwise tree of pair merges), gt4hip_intersect_multi (a chain of pair merges), and the key
 * ranges that shard them across GPUs (gt4hip_shard_cuts, gt4hip_shard_first_key).
 * Two kernels live here: k_share_probe (in how many of the lists a key lies: decides between one pass over up to 32
 * lists and levels of eight) and k_sample_stride (every stride-th key of a list, for the shard cuts).
 */
#include "gt4hip_host.h"

#include <string.h>
#include <algorithm>
#include <vector>

using namespace gt4;

PairParams gt4hip_nway_params (uint32_t op_bit, uint32_t rule, uint32_t cutoff, uint32_t ovr, uint32_t filter)
{
  PairParams p;
  memset (&p, 0, sizeof p);
  p.ops = op_bit;
  for (int s = 0; s < 4; s++) p.rule[s] = rule;
  p.cutoff = cutoff;
  p.count_override = ovr;
  p.filter = filter;
  return p;
}

/* Final step shared by both N-way ops: merge (a, b) into the caller-visible result. */
static int nway_final (gt4hip_context *ctx, const gt4hip_list *a, const gt4hip_list *b, const PairParams &p, int stream_idx,
                       bool count_only, gt4hip_multi_result *res)
{
  gt4hip_list *out[4] = { NULL, NULL, NULL, NULL };
  out[stream_idx] = count_only ? NULL : res->out;
  PairRun run;
  int rc = gt4hip_pair_with_outputs (ctx, a, b, p, count_only, out, &run);
  if (rc) return rc;
  res->n_words = run.n_words[stream_idx];
  res->total_count = run.total_count[stream_idx];
  res->out = count_only ? NULL : out[stream_idx];
  res->device_ms += run.device_ms;
  res->records_read += a->n_words + b->n_words;
  if (!count_only) res->records_written += run.n_words[stream_idx];
  return GT4HIP_OK;
}

static int empty_result (gt4hip_context *ctx, uint32_t word_length, bool count_only, gt4hip_multi_result *res)
{
  res->n_words = 0;
  res->total_count = 0;
  if (count_only) {
    res->out = NULL;
    return GT4HIP_OK;
  }
  if (res->out) {
    res->out->n_words = 0;
    return GT4HIP_OK;
  }
  return gt4hip_list_new (ctx, 0, word_length, &res->out);
}

/* N-way union by the one-pass tile kernel (gt4hip_nway.hip): groups of up to eight lists per launch;
 * more than eight lists take levels of eight-way merges that keep every key (ADD / MAX are
 * associative, NUMBER ignores the counts), the cutoff is applied once, at the last level (:574).
 * *done = 0: nothing was produced, the caller takes the pairwise tree. */
/* In how many of the lists does a key of the lists lie?  256 keys of each of four probe lists, looked up in every list
 * (binary searches): matches[0] += lists holding the key.  One pass over 9 .. 32 lists ranks a key among everything in its
 * bucket, and a key that sixteen lists share puts sixteen records there: measured (32 x 1.25e8 records, profiles/round5):
 * one pass 47.9 ms against 67.7 for levels of eight-way merges where few keys are shared, 64.6 against 54.1 where sixteen
 * of the lists are the same. */
struct ShareProbe {
  const uint32_t *list[32];
  uint64_t n[32];
  uint32_t k;
  uint32_t probe[4];
};

__global__ __launch_bounds__ (256) void k_share_probe (ShareProbe sp, unsigned long long *matches)
{
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = id % sp.k, j = (id / sp.k) % 256u, a = sp.probe[(id / sp.k) / 256u];
  if (id >= 4u * 256u * sp.k || !sp.n[a] || !sp.n[b]) return;
  const uint32_t *pa = sp.list[a] + 3 * (uint64_t) (((unsigned __int128) sp.n[a] * j) / 256u);
  const uint64_t key = (uint64_t) pa[0] | ((uint64_t) pa[1] << 32);
  uint64_t lo = 0, hi = sp.n[b];
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    const uint32_t *q = sp.list[b] + 3 * mid;
    if (((uint64_t) q[0] | ((uint64_t) q[1] << 32)) < key) lo = mid + 1;
    else hi = mid;
  }
  bool hit = false;
  if (lo < sp.n[b]) {
    const uint32_t *q = sp.list[b] + 3 * lo;
    hit = ((uint64_t) q[0] | ((uint64_t) q[1] << 32)) == key;
  }
  const unsigned long long m = __builtin_amdgcn_ballot_w64 (hit);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd (matches, (unsigned long long) __popcll (m));
}

/* the mean number of lists a probed key lies in (1: the lists share nothing) */
static int shared_key_multiplicity (gt4hip_context *ctx, const std::vector<const gt4hip_list *> &lists, double *mean)
{
  ShareProbe sp;
  memset (&sp, 0, sizeof sp);
  sp.k = (uint32_t) (lists.size () < 32 ? lists.size () : 32);
  for (uint32_t i = 0; i < sp.k; i++) {
    sp.list[i] = (const uint32_t *) lists[i]->dev;
    sp.n[i] = lists[i]->n_words;
  }
  sp.probe[0] = 0;
  sp.probe[1] = (sp.k / 4 + 1) % sp.k;
  sp.probe[2] = sp.k / 2;
  sp.probe[3] = (3 * sp.k / 4 + 1) % sp.k;
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 8, ctx->stream));
  hipLaunchKernelGGL (k_share_probe, dim3 ((4 * 256 * sp.k + 255) / 256), dim3 (256), 0, ctx->stream, sp, ctx->scratch);
  const int rc = gt4hip_read_scratch (ctx, 1);
  if (rc) return rc;
  uint32_t probed = 0;
  for (int q = 0; q < 4; q++) probed += sp.n[sp.probe[q]] ? 256u : 0u;
  *mean = probed ? (double) ctx->scratch_host[0] / probed : 1.0;
  return GT4HIP_OK;
}

static int union_multi_kway (gt4hip_context *ctx, const std::vector<const gt4hip_list *> &work, uint32_t rule, uint32_t cutoff, uint32_t ovr,
                             bool count_only, gt4hip_multi_result *res, int *done)
{
  *done = 0;
  std::vector<const gt4hip_list *> cur = work;
  TempLists owned; /* the results of the level below the one in the making */
  const uint32_t wl = work[0]->word_length;
  int rc = GT4HIP_OK;
  uint64_t rd = 0, wr = 0;
  double ms_total = 0;
  /* lists per launch of the tile kernel: up to 32 in ONE pass (round 5; glistmaker's collation width, reference
   * src/glistmaker.c:787-835), option "kway_max" = 8 restores the levels of eight-way merges */
  size_t W = ctx->kway_max == 8 ? 8 : 32;
  if (W == 32 && cur.size () > 8 && ctx->kway_max != 33) { /* ("kway_max" = 33: one pass whatever the keys; tests) */
    double m = 1.0;
    if ((rc = shared_key_multiplicity (ctx, cur, &m))) return rc;
    ctx->kway_shared_x100 = (uint64_t) (100.0 * m);
    if (m > 5.0) W = 8; /* keys that many lists share: levels of eight-way merges fold them step by step */
  }
  ctx->kway_width = cur.size () <= 8 ? 8u : (uint64_t) W; /* (up to eight lists take the eight-list instance of the kernel) */
  while (cur.size () > W) {
    std::vector<const gt4hip_list *> next;
    TempLists level;
    for (size_t i = 0; i < cur.size (); i += W) {
      const size_t g = cur.size () - i < W ? cur.size () - i : W;
      if (g < 3) { /* one or two left over: carried to the next level as they are */
        for (size_t j = 0; j < g; j++) next.push_back (cur[i + j]);
        continue;
      }
      uint64_t cap = 0;
      for (size_t j = 0; j < g; j++) cap += cur[i + j]->n_words;
      TempLists group; /* (goes back first when the group's launch declines) */
      gt4hip_list *o = NULL;
      if ((rc = gt4hip_list_new (ctx, cap, wl, &o))) return rc;
      group.adopt (o);
      uint64_t n = 0, t = 0;
      double ms = 0;
      int used = 0;
      rc = gt4hip_nway_union (ctx, &cur[i], (uint32_t) g, rule, cutoff, ovr, FILTER_RAW, false, o, &n, &t, &ms, &used);
      if (rc || !used) return rc;
      o->n_words = n;
      rd += cap;
      wr += n;
      ms_total += ms;
      next.push_back (o);
      group.release ();
      level.adopt (o);
    }
    owned.next_level (level, next);
    cur.swap (next);
  }
  if (cur.size () < (ctx->kway_enabled == 2 ? 2u : 3u)) {
    /* (possible only behind a level of eight-way merges) the last one or two go through the pair kernel */
    const gt4hip_list empty_b = gt4hip_empty_list (ctx, wl);
    const PairParams fin = gt4hip_nway_params (GT4HIP_OP_UNION, rule, cutoff, ovr, FILTER_RESULT);
    res->device_ms += ms_total;
    res->records_read += rd;
    res->records_written += wr;
    rc = nway_final (ctx, cur[0], cur.size () > 1 ? cur[1] : &empty_b, fin, 0, count_only, res);
    *done = rc == GT4HIP_OK;
    if (*done) ctx->kway_calls++;
    return rc;
  }
  uint64_t cap = 0;
  for (const gt4hip_list *l : cur) cap += l->n_words;
  TempLists made;
  gt4hip_list *o = NULL;
  if (!count_only && (rc = gt4hip_output_list (ctx, -1, res->out, cap, wl, made, &o))) return rc;
  uint64_t n = 0, t = 0;
  double ms = 0;
  int used = 0;
  rc = gt4hip_nway_union (ctx, cur.data (), (uint32_t) cur.size (), rule, cutoff, ovr, FILTER_RESULT, count_only, o, &n, &t, &ms, &used);
  owned.clear (); /* (the levels below are consumed; they go back before an output the launch declined) */
  if (rc || !used) return rc;
  made.release ();
  if (o) {
    o->n_words = n;
    o->word_length = wl;
  }
  res->n_words = n;
  res->total_count = t;
  res->out = count_only ? NULL : o;
  res->device_ms += ms_total + ms;
  res->records_read += rd + cap;
  res->records_written += wr + (count_only ? 0 : n);
  ctx->kway_calls++;
  *done = 1;
  return GT4HIP_OK;
}

extern "C" int gt4hip_union_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, uint32_t cutoff,
                                    int32_t rule, uint32_t ovr, int32_t count_only, gt4hip_multi_result *res)
{
  if (!ctx || !lists || !n_lists || !res) return GT4HIP_EINVAL;
  /* src/glistcompare.c:518-523 */
  if (rule == GT4HIP_RULE_DEFAULT) rule = GT4HIP_RULE_ADD;
  else if (rule != GT4HIP_RULE_ADD && rule != GT4HIP_RULE_MAX && rule != GT4HIP_RULE_NUMBER)
    return gt4hip_fail (ctx, GT4HIP_ERULE, "union_multi: Invalid rule %u (only ADD, MAX and NUMBER allowed)", (unsigned) rule);
  for (uint32_t j = 0; j < n_lists; j++) {
    if (!lists[j]) return GT4HIP_EINVAL;
    if (lists[j]->word_length != lists[0]->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ");
  }
  HIPCHK (ctx, hipSetDevice (ctx->device));
  res->device_ms = 0;
  res->records_read = res->records_written = 0;
  std::vector<const gt4hip_list *> work;
  for (uint32_t j = 0; j < n_lists; j++)
    if (lists[j]->n_words) work.push_back (lists[j]); /* :525-532 empty lists are dropped */
  const uint32_t wl = lists[0]->word_length;
  ctx->last_multi_one_pass = 0;
  if (work.empty ()) return empty_result (ctx, wl, count_only != 0, res);
  if (ctx->kway_enabled && work.size () >= (ctx->kway_enabled == 2 ? 2u : 3u)) {
    int done = 0;
    const int krc = union_multi_kway (ctx, work, (uint32_t) rule, cutoff, ovr, count_only != 0, res, &done);
    if (!krc && done) ctx->last_multi_one_pass = 1;
    if (krc || done) return krc;
    res->device_ms = 0;
    res->records_read = res->records_written = 0;
  }
  const gt4hip_list empty_b = gt4hip_empty_list (ctx, wl);
  int rc;
  TempLists owned; /* intermediate levels, freed as soon as consumed */
  /* pairwise tree in HBM: intermediate levels keep every key (count rules ADD/MAX are associative
   * and commutative), the cutoff is applied once, on the final count (:574) */
  const PairParams raw = gt4hip_nway_params (GT4HIP_OP_UNION, (uint32_t) rule, cutoff, ovr, FILTER_RAW);
  while (work.size () > 2) {
    std::vector<const gt4hip_list *> next;
    TempLists level;
    for (size_t i = 0; i + 1 < work.size (); i += 2) {
      gt4hip_list *out[4] = { NULL, NULL, NULL, NULL };
      PairRun run;
      if ((rc = gt4hip_pair_with_outputs (ctx, work[i], work[i + 1], raw, false, out, &run))) return rc;
      res->device_ms += run.device_ms;
      res->records_read += work[i]->n_words + work[i + 1]->n_words;
      res->records_written += run.n_words[0];
      next.push_back (level.adopt (out[0]));
    }
    if (work.size () & 1) next.push_back (work.back ()); /* an odd one is carried over */
    owned.next_level (level, next);
    work.swap (next);
  }
  const PairParams fin = gt4hip_nway_params (GT4HIP_OP_UNION, (uint32_t) rule, cutoff, ovr, FILTER_RESULT);
  return nway_final (ctx, work[0], work.size () > 1 ? work[1] : &empty_b, fin, 0, count_only != 0, res);
}

extern "C" int gt4hip_intersect_multi (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n_lists, uint32_t cutoff,
                                        int32_t rule, uint32_t ovr, int32_t count_only, gt4hip_multi_result *res)
{
  if (!ctx || !lists || !n_lists || !res) return GT4HIP_EINVAL;
  /* src/glistcompare.c:622-627 */
  if (rule == GT4HIP_RULE_DEFAULT) rule = GT4HIP_RULE_MIN;
  else if (rule != GT4HIP_RULE_ADD && rule != GT4HIP_RULE_MIN && rule != GT4HIP_RULE_MAX && rule != GT4HIP_RULE_NUMBER)
    return gt4hip_fail (ctx, GT4HIP_ERULE, "intersect_multi: Invalid rule %u (only ADD, MIN, MAX and NUMBER allowed)", (unsigned) rule);
  bool any_empty = false;
  for (uint32_t j = 0; j < n_lists; j++) {
    if (!lists[j]) return GT4HIP_EINVAL;
    if (lists[j]->word_length != lists[0]->word_length) return gt4hip_fail (ctx, GT4HIP_EWORDLEN, "word lengths differ");
    any_empty |= lists[j]->n_words == 0;
  }
  HIPCHK (ctx, hipSetDevice (ctx->device));
  res->device_ms = 0;
  res->records_read = res->records_written = 0;
  const uint32_t wl = lists[0]->word_length;
  if (any_empty) return empty_result (ctx, wl, count_only != 0, res); /* :633-636 */
  /* Left-to-right chain R_k = R_{k-1} n L_k, exactly the reference's fold order over the lists
   * (:655-678): the running MIN restarts at 0 (RULE_MINZ), which is not associative, so no tree. */
  const uint32_t krule = rule == GT4HIP_RULE_MIN ? RULE_MINZ : (uint32_t) rule;
  if (n_lists == 1) {
    const gt4hip_list empty_b = gt4hip_empty_list (ctx, wl);
    /* fold(0, c) of one list: c for MIN/MAX/ADD, the override for NUMBER */
    const PairParams fin = gt4hip_nway_params (GT4HIP_OP_UNION, rule == GT4HIP_RULE_NUMBER ? GT4HIP_RULE_NUMBER : GT4HIP_RULE_FIRST, cutoff, ovr, FILTER_RESULT);
    return nway_final (ctx, lists[0], &empty_b, fin, 0, count_only != 0, res);
  }
  const gt4hip_list *acc = lists[0];
  TempLists acc_owned; /* the running intersection, once it is not lists[0] */
  for (uint32_t k = 1; k + 1 < n_lists; k++) {
    gt4hip_list *out[4] = { NULL, NULL, NULL, NULL };
    PairRun run;
    const int rc = gt4hip_pair_with_outputs (ctx, acc, lists[k], gt4hip_nway_params (GT4HIP_OP_INTRSEC, krule, cutoff, ovr, FILTER_RAW), false, out, &run);
    if (rc) return rc;
    res->device_ms += run.device_ms;
    res->records_read += acc->n_words + lists[k]->n_words;
    res->records_written += run.n_words[1];
    acc_owned.clear ();
    acc = acc_owned.adopt (out[1]);
  }
  return nway_final (ctx, acc, lists[n_lists - 1], gt4hip_nway_params (GT4HIP_OP_INTRSEC, krule, cutoff, ovr, FILTER_RESULT), 1, count_only != 0, res);
}

/* every stride-th key of a list (the last key of every full block of `stride` records) -> out[0 .. n / stride) */
__global__ void k_sample_stride (const uint32_t *__restrict__ rec, uint64_t n, uint64_t stride, unsigned long long *__restrict__ out)
{
  const uint64_t m = n / stride;
  for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (uint64_t) gridDim.x * blockDim.x) {
    const uint32_t *q = rec + 3 * ((j + 1) * stride - 1);
    out[j] = (unsigned long long) q[0] | ((unsigned long long) q[1] << 32);
  }
}

/* SAMPLED splitters: equal-width key ranges balance the shards only for uniformly spread keys;
 * 2-bit packed k-mers of a real genome are not (src/sequence.c:116-130: the word IS the sequence, low-complexity and
 * GC-poor prefixes are crowded).  Every S-th key of every list (S = all records / 65536), merged on the host; the
 * first key of shard g is the merged sample at g / n_shards: the shards' INPUT records then differ by at most
 * n_lists * S.  Every rank that holds the same lists computes the same cuts.  first_keys[0] = 0. */
extern "C" int gt4hip_shard_cuts (gt4hip_context *ctx, const gt4hip_list *const lists[], uint32_t n, uint32_t n_shards, uint64_t *first_keys)
{
  if (!ctx || !lists || !n || !n_shards || !first_keys) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  uint64_t total = 0;
  uint32_t wl = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!lists[i]) return GT4HIP_EINVAL;
    total += lists[i]->n_words;
    wl = lists[i]->word_length > wl ? lists[i]->word_length : wl;
  }
  const uint64_t target = 65536;
  const uint64_t stride = total / target ? total / target : 1;
  uint64_t m_total = 0;
  for (uint32_t i = 0; i < n; i++) m_total += lists[i]->n_words / stride;
  first_keys[0] = 0;
  if (m_total < (uint64_t) n_shards) { /* (hardly any records: equal-width ranges) */
    for (uint32_t g = 1; g < n_shards; g++) first_keys[g] = gt4hip_shard_first_key (wl, n_shards, g);
    return GT4HIP_OK;
  }
  TempBlocks blk;
  void *dev = NULL;
  int rc = blk.get (ctx, (size_t) m_total * 8, &dev);
  if (rc) return rc;
  std::vector<unsigned long long> host ((size_t) m_total);
  uint64_t at = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t m = lists[i]->n_words / stride;
    if (!m) continue;
    const int grid = gt4hip_grid (ctx, m, GT4HIP_LIST_THREADS); /* (m < 2 * target: 512 blocks at most) */
    hipLaunchKernelGGL (k_sample_stride, dim3 (grid), dim3 (GT4HIP_LIST_THREADS), 0, ctx->stream, (const uint32_t *) lists[i]->dev, lists[i]->n_words, stride, (unsigned long long *) dev + at);
    at += m;
  }
  rc = gt4hip_read_back (ctx, host.data (), dev, (size_t) m_total * 8, "gt4hip_shard_cuts");
  blk.clear (); /* (before the host sort) */
  if (rc) return rc;
  std::sort (host.begin (), host.end ());
  for (uint32_t g = 1; g < n_shards; g++) {
    /* (the sample itself goes to the shard on its left: the cut is one above it) */
    const unsigned long long sk = host[(size_t) (((unsigned __int128) m_total * g) / n_shards) - 1];
    const uint64_t cut = sk == ~0ull ? sk : sk + 1;
    first_keys[g] = cut > first_keys[g - 1] ? cut : first_keys[g - 1];
  }
  return GT4HIP_OK;
}

extern "C" uint64_t gt4hip_shard_first_key (uint32_t word_length, uint32_t n_shards, uint32_t g)
{
  if (!n_shards || g >= n_shards) return 0;
  const unsigned __int128 space = word_length >= 32 ? ((unsigned __int128) 1 << 64) : ((unsigned __int128) 1 << (2 * word_length));
  return (uint64_t) (space * g / n_shards);
}
