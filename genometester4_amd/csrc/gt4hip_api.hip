/*
 * gt4hip_api.hip -- the base of the C ABI declared in include/gt4hip.h: errors, context create / destroy, options and
 * counters, the block pool and every device allocation, the workspace grow, list objects and the small list queries,
 * read-backs, gt4hip_generate*.  Host code only, no kernel (the queries launch kernels of gt4hip_kernels.hip); the
 * operations are in gt4hip_pair.hip, gt4hip_multi.hip and gt4hip_table.hip.  Nothing falls back to the CPU.
 */
#include "gt4hip_host.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>

using namespace gt4;

static thread_local char g_create_err[512] = ""; /* per thread: a worker's loader, merger and writer threads each create a context (found by ThreadSanitizer on the CPU harness) */

static void pool_flush (gt4hip_context *ctx);

int gt4hip_fail (gt4hip_context *ctx, int code, const char *fmt, ...)
{
  va_list ap;
  va_start (ap, fmt);
  vsnprintf (ctx ? ctx->err : g_create_err, 512, fmt, ap);
  va_end (ap);
  return code;
}

extern "C" const char *gt4hip_strerror (int code)
{
  switch (code) {
    case GT4HIP_OK: return "ok";
    case GT4HIP_EINVAL: return "invalid argument";
    case GT4HIP_ENODEVICE: return "no usable HIP device";
    case GT4HIP_ENOMEM: return "out of memory";
    case GT4HIP_ERULE: return "rule not allowed for this operation";
    case GT4HIP_EHIP: return "HIP runtime error";
    case GT4HIP_EWORDLEN: return "lists have different word lengths";
    case GT4HIP_EINTERNAL: return "internal consistency check failed";
    case GT4HIP_ECALLBACK: return "stopped by callback";
    case GT4HIP_EIO: return "file I/O failed";
    case GT4HIP_ECOMM: return "RCCL communication failed";
    case GT4HIP_EFORMAT: return "malformed sequence text";
    default: return "unknown error";
  }
}

extern "C" const char *gt4hip_last_error (const gt4hip_context *ctx)
{
  return ctx ? ctx->err : g_create_err;
}

extern "C" int gt4hip_device_count (void)
{
  int n = 0;
  if (hipGetDeviceCount (&n) != hipSuccess) return 0;
  return n;
}

extern "C" int gt4hip_create (int device, gt4hip_context **out)
{
  if (!out || device < 0) return gt4hip_fail (NULL, GT4HIP_EINVAL, "gt4hip_create: bad arguments");
  *out = NULL;
  int n = 0;
  hipError_t e = hipGetDeviceCount (&n);
  if (e != hipSuccess || n <= 0)
    return gt4hip_fail (NULL, GT4HIP_ENODEVICE, "gt4hip_create: no HIP device (%s)", e != hipSuccess ? hipGetErrorString (e) : "count 0");
  if (device >= n) return gt4hip_fail (NULL, GT4HIP_ENODEVICE, "gt4hip_create: device %d not present (%d visible)", device, n);
  if ((e = hipSetDevice (device)) != hipSuccess)
    return gt4hip_fail (NULL, GT4HIP_ENODEVICE, "gt4hip_create: hipSetDevice(%d): %s", device, hipGetErrorString (e));
  gt4hip_context *ctx = new (std::nothrow) gt4hip_context ();
  if (!ctx) return gt4hip_fail (NULL, GT4HIP_ENOMEM, "gt4hip_create: host allocation failed");
  memset (ctx, 0, sizeof *ctx);
  ctx->device = device;
  ctx->pool = new (std::nothrow) std::vector<std::pair<void *, size_t>> ();
  ctx->pool_enabled = ctx->pool != NULL;
  hipDeviceProp_t prop;
  if ((e = hipGetDeviceProperties (&prop, device)) != hipSuccess) {
    delete ctx->pool;
    delete ctx;
    return gt4hip_fail (NULL, GT4HIP_ENODEVICE, "gt4hip_create: hipGetDeviceProperties: %s", hipGetErrorString (e));
  }
  ctx->n_cus = prop.multiProcessorCount;
  ctx->pool_cap = prop.totalGlobalMem / 2;
  {
    const char *e = getenv ("GT4HIP_DYNAMIC"); /* diagnostic: the whole test-suite through the other dealing */
    ctx->dynamic = e ? atoi (e) : 0; /* 0: automatic */
  }
  ctx->kway_max = 32;
  ctx->kway_enabled = 1; /* N-way unions of three lists or more take the one-pass tile kernel (gt4hip_nway.hip); option "kway": 0 the pairwise tree, 2 also two lists */
  snprintf (ctx->info, sizeof ctx->info, "%s|%s|%d|%zu", prop.name, prop.gcnArchName, prop.multiProcessorCount, prop.totalGlobalMem);
  if ((e = hipStreamCreateWithFlags (&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
    delete ctx->pool;
    delete ctx;
    return gt4hip_fail (NULL, GT4HIP_ENODEVICE, "gt4hip_create: hipStreamCreate: %s", hipGetErrorString (e));
  }
  for (int i = 0; i < 4; i++) hipEventCreate (&ctx->ev[i]);
  if (hipMalloc ((void **) &ctx->ctl, sizeof (PairControl)) != hipSuccess ||
      hipHostMalloc ((void **) &ctx->ctl_host, sizeof (PairControl), hipHostMallocDefault) != hipSuccess ||
      hipMalloc ((void **) &ctx->scratch, 64) != hipSuccess ||
      hipHostMalloc ((void **) &ctx->scratch_host, 64, hipHostMallocDefault) != hipSuccess) {
    gt4hip_destroy (ctx);
    return gt4hip_fail (NULL, GT4HIP_ENOMEM, "gt4hip_create: control block allocation failed");
  }
  *out = ctx;
  return GT4HIP_OK;
}

extern "C" void gt4hip_destroy (gt4hip_context *ctx)
{
  if (!ctx) return;
  hipSetDevice (ctx->device);
  if (ctx->stream) hipStreamSynchronize (ctx->stream);
  gt4hip_io_destroy (ctx);
  gt4hip_words_free (ctx, NULL);
  gt4hip_index_free (ctx);
  gt4hip_pairs_release (ctx);
  gt4hip_locations_free (ctx);
  if (ctx->pool) {
    pool_flush (ctx);
    delete ctx->pool;
  }
  void *const dev[] = { ctx->part, ctx->kway_part, ctx->kway_cnt, ctx->kway_part2, ctx->kway_need, ctx->desc, ctx->block_sums, ctx->ctl, ctx->scratch, ctx->caller_tab };
  for (void *p : dev)
    if (p) hipFree (p);
  if (ctx->ctl_host) hipHostFree (ctx->ctl_host);
  if (ctx->scratch_host) hipHostFree (ctx->scratch_host);
  for (int i = 0; i < 4; i++) if (ctx->ev[i]) hipEventDestroy (ctx->ev[i]);
  if (ctx->stream) hipStreamDestroy (ctx->stream);
  delete ctx;
}

extern "C" const char *gt4hip_device_info (const gt4hip_context *ctx)
{
  return ctx ? ctx->info : "";
}

extern "C" int gt4hip_context_device (const gt4hip_context *ctx) { return ctx ? ctx->device : -1; }

extern "C" int gt4hip_trim (gt4hip_context *ctx)
{
  if (!ctx) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  pool_flush (ctx);
  return GT4HIP_OK;
}

extern "C" int gt4hip_device_memory (gt4hip_context *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
  if (!ctx) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  size_t f = 0, t = 0;
  HIPCHK (ctx, hipMemGetInfo (&f, &t));
  /* what the context's pool holds can be had back at once */
  if (free_bytes) *free_bytes = (uint64_t) f + ctx->pool_bytes;
  if (total_bytes) *total_bytes = (uint64_t) t;
  return GT4HIP_OK;
}

extern "C" int gt4hip_set_option (gt4hip_context *ctx, const char *name, int64_t value)
{
  if (!ctx || !name) return GT4HIP_EINVAL;
  if (!strcmp (name, "two_pass")) ctx->two_pass = value != 0;
  else if (!strcmp (name, "pool")) {
    ctx->pool_enabled = value != 0 && ctx->pool;
    if (!ctx->pool_enabled) pool_flush (ctx);
  }
  else if (!strcmp (name, "pool_cap_mb")) {
    ctx->pool_cap = value > 0 ? (size_t) value << 20 : 0;
    if (ctx->pool_bytes > ctx->pool_cap) pool_flush (ctx);
  }
  else if (!strcmp (name, "grid")) ctx->grid_override = value;
  else if (!strcmp (name, "scan_group")) ctx->scan_group = (int) value;
  else if (!strcmp (name, "dynamic")) ctx->dynamic = (int) value;
  else if (!strcmp (name, "a_rows")) ctx->a_rows = (int) value;
  else if (!strcmp (name, "part_guided")) ctx->part_guided = (int) value;
  else if (!strcmp (name, "select_vec")) ctx->select_vec = (int) value;
  else if (!strcmp (name, "grid_cap")) ctx->grid_limit.cap = value > 0 ? value : 0;
  else if (!strcmp (name, "poison")) ctx->poison = value != 0;
  else if (!strcmp (name, "caller_piece")) ctx->caller_piece = value > 0 ? (uint64_t) value : 0;
  else if (!strcmp (name, "kway")) ctx->kway_enabled = (int) value;
  else if (!strcmp (name, "kway_max")) ctx->kway_max = value == 8 ? 8 : (value == 33 ? 33 : 32);
  else if (!strcmp (name, "kway_g")) ctx->kway_g = value;
  else if (!strcmp (name, "kway_vt")) ctx->kway_vt = value;
  else if (!strcmp (name, "spin_limit")) ctx->spin_limit = value > 0 ? (uint32_t) value : 0u;
  else if (!strcmp (name, "geom1")) ctx->force_geom = value != 0 ? 1 : 0;
  else if (!strcmp (name, "geom0")) ctx->force_geom = value != 0 ? -1 : 0;
  else return gt4hip_fail (ctx, GT4HIP_EINVAL, "unknown option %s", name);
  return GT4HIP_OK;
}

extern "C" int gt4hip_get_counter (gt4hip_context *ctx, const char *name, uint64_t *value)
{
  if (!ctx || !name || !value) return GT4HIP_EINVAL;
  if (!strcmp (name, "single_pass_fallbacks")) *value = ctx->single_pass_fallbacks;
  else if (!strcmp (name, "partition_us")) *value = (uint64_t) (ctx->partition_ms * 1000.0);
  else if (!strcmp (name, "kway_calls")) *value = ctx->kway_calls;
  else if (!strcmp (name, "kway_overflows")) *value = ctx->kway_overflows;
  else if (!strcmp (name, "kway_declined")) *value = ctx->kway_declined;
  else if (!strcmp (name, "kway_splits")) *value = ctx->kway_splits;
  else if (!strcmp (name, "kway_shared_x100")) *value = ctx->kway_shared_x100;
  else if (!strcmp (name, "kway_width")) *value = ctx->kway_width;
  else if (!strcmp (name, "nway_kernel_us")) *value = (uint64_t) (ctx->nway_kernel_ms * 1000.0);
  else if (!strcmp (name, "nway_tiles")) *value = ctx->nway_tiles;
  else if (!strcmp (name, "nway_sample_tiles")) *value = ctx->nway_sample_tiles;
  else if (!strcmp (name, "nway_one_pass")) *value = (uint64_t) ctx->last_multi_one_pass;
  else if (!strcmp (name, "sort_us")) *value = (uint64_t) (ctx->sort_ms * 1000.0);
  else if (!strcmp (name, "fold_us")) *value = (uint64_t) (ctx->fold_ms * 1000.0);
  else if (!strcmp (name, "extract_us")) *value = (uint64_t) (ctx->extract_ms * 1000.0);
  else if (!strcmp (name, "maker_text_tile") || !strcmp (name, "maker_code_tile")) *value = GT4HIP_MAKER_TILE;
  else if (!strcmp (name, "table_us")) *value = (uint64_t) (ctx->table_ms * 1000.0);
  else if (!strcmp (name, "query_wide")) *value = ctx->query_wide;
  else if (!strcmp (name, "mm_wide_levels")) *value = ctx->mm_wide_levels;
  else if (!strcmp (name, "mm_unskipped_levels")) *value = ctx->mm_unskipped_levels;
  else if (!strcmp (name, "subset_passes")) *value = ctx->subset_passes;
  else if (!strcmp (name, "subset_tile")) *value = GT4HIP_SUBSET_TILE;
  else if (!strcmp (name, "subset_scan_tile")) *value = 256u * GT4HIP_SUBSET_SCAN_V;
  else if (!strcmp (name, "pack_threads")) *value = GT4HIP_PACK_THREADS;
  else if (!strcmp (name, "subset_us")) *value = (uint64_t) (ctx->subset_ms * 1000.0);
  else if (!strcmp (name, "mask_ends_us")) *value = (uint64_t) (ctx->mask_ends_ms * 1000.0);
  else if (!strcmp (name, "mask_apply_us")) *value = (uint64_t) (ctx->mask_apply_ms * 1000.0);
  else if (!strcmp (name, "select_wide")) *value = ctx->select_wide;
  else if (!strcmp (name, "select_segment")) *value = GT4HIP_SELECT_SEGMENT;
  else if (!strcmp (name, "grid_capped")) *value = ctx->grid_limit.capped;
  else if (!strcmp (name, "mm_threads")) *value = GT4HIP_MM_THREADS;
  else if (!strcmp (name, "mm_tile")) *value = (uint64_t) GT4HIP_MM_THREADS * GT4HIP_MM_ROUNDS;
  else if (!strcmp (name, "gather_tile")) *value = (uint64_t) GT4HIP_MM_THREADS * GT4HIP_GATHER_ROUNDS;
  else if (!strcmp (name, "profile_tile")) *value = (uint64_t) GT4HIP_MM_THREADS * GT4HIP_PROFILE_ROUNDS;
  else if (!strcmp (name, "hist_lds_bins")) *value = GT4HIP_HIST_LDS_BINS;
  else if (!strcmp (name, "list_threads")) *value = GT4HIP_LIST_THREADS;
  else if (!strcmp (name, "caller_threads")) *value = GT4HIP_CALLER_THREADS;
  else if (!strcmp (name, "caller_max_grid")) *value = GT4HIP_CALLER_MAX_GRID;
  else if (!strcmp (name, "sort_hist_chunk")) *value = (uint64_t) GT4HIP_SORT_HIST_THREADS * GT4HIP_SORT_HIST_ITEMS;
  else return gt4hip_fail (ctx, GT4HIP_EINVAL, "unknown counter %s", name);
  return GT4HIP_OK;
}

extern "C" int gt4hip_synchronize (gt4hip_context *ctx)
{
  if (!ctx) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

/* ------------------------------------------------------------------ device memory */

static void pool_flush (gt4hip_context *ctx)
{
  if (!ctx->pool) return;
  for (auto &b : *ctx->pool) hipFree (b.first);
  ctx->pool->clear ();
  ctx->pool_bytes = 0;
}

/* Option "poison" (tests): a block as it is handed out holds 0xA5 bytes, not what the call before left there -- as likely as
 * not the results this call is to compute, which would then pass for them where a kernel skips an item.  Waited for: the
 * staging threads of gt4hip_io.hip copy on streams of their own. */
static void poison (gt4hip_context *ctx, void *p, size_t bytes)
{
  if (!ctx->poison || !bytes) return;
  if (hipMemsetAsync (p, 0xA5, bytes, ctx->stream) != hipSuccess || hipStreamSynchronize (ctx->stream) != hipSuccess) (void) hipGetLastError ();
}

/* Every device allocation of the library goes through here: when the driver is out of memory the
 * pooled blocks (freed list storage kept for reuse) are given back and the allocation is retried. */
hipError_t gt4hip_dev_alloc (gt4hip_context *ctx, void **p, size_t bytes)
{
  hipError_t e = hipMalloc (p, bytes);
  if (e != hipSuccess && ctx->pool && !ctx->pool->empty ()) {
    (void) hipGetLastError ();
    pool_flush (ctx);
    e = hipMalloc (p, bytes);
  }
  if (e != hipSuccess) (void) hipGetLastError ();
  else poison (ctx, *p, bytes);
  return e;
}

/* ------------------------------------------------------------------ lists */

int gt4hip_list_new (gt4hip_context *ctx, uint64_t capacity, uint32_t word_length, gt4hip_list **out)
{
  gt4hip_list *l = new (std::nothrow) gt4hip_list ();
  if (!l) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  l->ctx = ctx;
  l->dev = NULL;
  l->n_words = capacity;
  l->capacity = capacity;
  l->word_length = word_length;
  l->owns = 1;
  /* 16 bytes of slack so that 16-byte vector loads that straddle the end stay inside the allocation */
  const size_t bytes = (((size_t) capacity * GT4HIP_RECORD_BYTES + 16) + 255) & ~(size_t) 255;
  /* reuse a pooled block that fits without wasting more than half of it */
  if (ctx->pool_enabled) {
    size_t best = (size_t) -1, best_i = 0;
    for (size_t i = 0; i < ctx->pool->size (); i++) {
      const size_t b = (*ctx->pool)[i].second;
      if (b >= bytes && b / 2 <= bytes && b < best) {
        best = b;
        best_i = i;
      }
    }
    if (best != (size_t) -1) {
      l->dev = (*ctx->pool)[best_i].first;
      l->bytes = best;
      ctx->pool_bytes -= best;
      ctx->pool->erase (ctx->pool->begin () + (long) best_i);
      poison (ctx, l->dev, l->bytes);
    }
  }
  if (!l->dev) {
    const hipError_t e = gt4hip_dev_alloc (ctx, &l->dev, bytes);
    if (e != hipSuccess) {
      delete l;
      return gt4hip_fail (ctx, GT4HIP_ENOMEM, "hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString (e));
    }
    l->bytes = bytes;
  }
  *out = l;
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_alloc (gt4hip_context *ctx, uint64_t capacity, uint32_t word_length, gt4hip_list **out)
{
  if (!ctx || !out) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  return gt4hip_list_new (ctx, capacity, word_length, out);
}

extern "C" int gt4hip_list_upload (gt4hip_context *ctx, const void *host_records, uint64_t n_words, uint32_t word_length,
                                    gt4hip_list **out)
{
  if (!ctx || !out || (n_words && !host_records)) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_list *l = NULL;
  int rc = gt4hip_list_new (ctx, n_words, word_length, &l);
  if (rc) return rc;
  if (n_words) {
    rc = gt4hip_list_load (ctx, l, host_records, n_words); /* large buffers: pinned staging on the copy threads */
    if (rc) {
      gt4hip_list_free (l);
      return rc;
    }
  }
  *out = l;
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_upload_index (gt4hip_context *ctx, const void *host_kmers, uint64_t n_words, uint64_t num_locations,
                                          uint32_t word_length, gt4hip_list **out)
{
  if (!ctx || !out || (n_words && !host_kmers)) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  gt4hip_list *l = NULL;
  int rc = gt4hip_list_new (ctx, n_words, word_length, &l);
  if (rc) return rc;
  if (n_words) {
    void *tmp = NULL;
    hipError_t e = gt4hip_dev_alloc (ctx, &tmp, (size_t) n_words * 16);
    if (e != hipSuccess) {
      gt4hip_list_free (l);
      return gt4hip_fail (ctx, GT4HIP_ENOMEM, "hipMalloc of %llu bytes for the index table failed", (unsigned long long) n_words * 16);
    }
    e = hipMemcpyAsync (tmp, host_kmers, (size_t) n_words * 16, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = launch_decode_index (ctx->stream, ctx->grid_limit, (const unsigned long long *) tmp, n_words, num_locations, (uint32_t *) l->dev);
    if (e == hipSuccess) e = hipStreamSynchronize (ctx->stream);
    hipFree (tmp);
    if (e != hipSuccess) {
      gt4hip_list_free (l);
      return gt4hip_fail (ctx, GT4HIP_EHIP, "index upload failed: %s", hipGetErrorString (e));
    }
  }
  *out = l;
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_wrap (gt4hip_context *ctx, void *device_records, uint64_t n_words, uint32_t word_length, gt4hip_list **out)
{
  if (!ctx || !out || (n_words && !device_records)) return GT4HIP_EINVAL;
  if (((uintptr_t) device_records) & 3) return gt4hip_fail (ctx, GT4HIP_EINVAL, "device records must be 4-byte aligned");
  gt4hip_list *l = new (std::nothrow) gt4hip_list (gt4hip_empty_list (ctx, word_length));
  if (!l) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "host allocation failed");
  l->dev = device_records;
  l->n_words = l->capacity = n_words;
  *out = l;
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_slice (gt4hip_context *ctx, const gt4hip_list *list, uint64_t first, uint64_t count, gt4hip_list **out)
{
  if (!ctx || !list || !out || first > list->n_words || count > list->n_words - first) return GT4HIP_EINVAL;
  return gt4hip_list_wrap (ctx, (char *) list->dev + first * GT4HIP_RECORD_BYTES, count, list->word_length, out);
}

extern "C" int gt4hip_list_download_range (gt4hip_context *ctx, const gt4hip_list *list, uint64_t first, uint64_t count, void *host)
{
  if (!ctx || !list || first > list->n_words || count > list->n_words - first || (count && !host)) return GT4HIP_EINVAL;
  if (!count) return GT4HIP_OK;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if ((size_t) count * GT4HIP_RECORD_BYTES >= ((size_t) 32 << 20))
    return gt4hip_io_download (ctx, (const char *) list->dev + first * GT4HIP_RECORD_BYTES, host, (size_t) count * GT4HIP_RECORD_BYTES);
  HIPCHK (ctx, hipMemcpyAsync (host, (const char *) list->dev + first * GT4HIP_RECORD_BYTES, (size_t) count * GT4HIP_RECORD_BYTES,
                               hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_download (gt4hip_context *ctx, const gt4hip_list *list, void *host)
{
  if (!list) return GT4HIP_EINVAL;
  return gt4hip_list_download_range (ctx, list, 0, list->n_words, host);
}

extern "C" void gt4hip_list_free (gt4hip_list *l)
{
  if (!l) return;
  if (l->owns && l->dev) {
    gt4hip_context *const ctx = l->ctx;
    if (ctx->pool_enabled && l->bytes <= ctx->pool_cap) {
      /* the pool never holds more than its cap: the oldest blocks go back to the driver first */
      while (ctx->pool_bytes + l->bytes > ctx->pool_cap && !ctx->pool->empty ()) {
        hipSetDevice (ctx->device);
        hipFree (ctx->pool->front ().first);
        ctx->pool_bytes -= ctx->pool->front ().second;
        ctx->pool->erase (ctx->pool->begin ());
      }
      ctx->pool->push_back (std::make_pair (l->dev, l->bytes));
      ctx->pool_bytes += l->bytes;
    } else {
      hipSetDevice (l->ctx->device);
      hipFree (l->dev);
    }
  }
  delete l;
}

extern "C" uint64_t gt4hip_list_n_words (const gt4hip_list *l) { return l ? l->n_words : 0; }
extern "C" uint32_t gt4hip_list_word_length (const gt4hip_list *l) { return l ? l->word_length : 0; }
extern "C" void *gt4hip_list_device_ptr (const gt4hip_list *l) { return l ? l->dev : NULL; }

extern "C" int gt4hip_list_set_n_words (gt4hip_list *l, uint64_t n)
{
  if (!l || n > l->capacity) return GT4HIP_EINVAL;
  l->n_words = n;
  return GT4HIP_OK;
}

gt4hip_list gt4hip_empty_list (gt4hip_context *ctx, uint32_t word_length)
{
  return { ctx, NULL, 0, 0, 0, word_length, 0 };
}

int gt4hip_output_list (gt4hip_context *ctx, int s, gt4hip_list *given, uint64_t need, uint32_t word_length, TempLists &made, gt4hip_list **out)
{
  char stream[16] = "";
  if (s >= 0) snprintf (stream, sizeof stream, " %d", s);
  if (given && given->capacity < need)
    return gt4hip_fail (ctx, GT4HIP_EINVAL, "output%s: capacity %llu < worst case %llu", stream, (unsigned long long) given->capacity, (unsigned long long) need);
  *out = given;
  const int rc = given ? GT4HIP_OK : gt4hip_list_new (ctx, need, word_length, out);
  if (!given && !rc) made.adopt (*out);
  return rc;
}

int gt4hip_read_back (gt4hip_context *ctx, void *host, const void *dev, size_t bytes, const char *what)
{
  hipError_t e = hipMemcpyAsync (host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize (ctx->stream);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_EHIP, "%s: %s", what, hipGetErrorString (e));
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_sum_counts (gt4hip_context *ctx, const gt4hip_list *l, uint64_t *sum)
{
  if (!ctx || !l || !sum) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 64, ctx->stream));
  if (l->n_words) HIPCHK (ctx, launch_sum_counts (ctx->stream, ctx->grid_limit, (const uint32_t *) l->dev, l->n_words, ctx->scratch));
  int rc = gt4hip_read_scratch (ctx, 1);
  if (rc) return rc;
  *sum = ctx->scratch_host[0];
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_is_sorted (gt4hip_context *ctx, const gt4hip_list *l, int *sorted)
{
  if (!ctx || !l || !sorted) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  HIPCHK (ctx, hipMemsetAsync (ctx->scratch, 0, 64, ctx->stream));
  if (l->n_words > 1) HIPCHK (ctx, launch_check_sorted (ctx->stream, ctx->grid_limit, (const uint32_t *) l->dev, l->n_words, (unsigned int *) ctx->scratch));
  int rc = gt4hip_read_scratch (ctx, 1);
  if (rc) return rc;
  *sorted = (ctx->scratch_host[0] & 0xffffffffu) == 0;
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_lower_bound (gt4hip_context *ctx, const gt4hip_list *l, uint64_t key, uint64_t *index)
{
  if (!ctx || !l || !index) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  if (!l->n_words) {
    *index = 0;
    return GT4HIP_OK;
  }
  HIPCHK (ctx, launch_lower_bound (ctx->stream, (const uint32_t *) l->dev, l->n_words, key, ctx->scratch));
  int rc = gt4hip_read_scratch (ctx, 1);
  if (rc) return rc;
  *index = ctx->scratch_host[0];
  return GT4HIP_OK;
}

extern "C" int gt4hip_list_get_word (gt4hip_context *ctx, const gt4hip_list *l, uint64_t idx, uint64_t *word, uint32_t *count)
{
  if (!ctx || !l || idx >= l->n_words) return GT4HIP_EINVAL;
  unsigned char rec[12];
  int rc = gt4hip_list_download_range (ctx, l, idx, 1, rec);
  if (rc) return rc;
  if (word) memcpy (word, rec, 8);
  if (count) memcpy (count, rec + 8, 4);
  return GT4HIP_OK;
}

extern "C" int gt4hip_generate_ex (gt4hip_context *ctx, gt4hip_list *l, uint64_t n, uint64_t key_seed, uint64_t count_seed,
                                   uint32_t max_count, uint64_t mult, uint64_t add)
{
  if (!ctx || !l || n > l->capacity || !max_count || !l->word_length || l->word_length > 32 || !mult || add >= mult) return GT4HIP_EINVAL;
  HIPCHK (ctx, hipSetDevice (ctx->device));
  l->n_words = n;
  if (!n) return GT4HIP_OK;
  /* keyspace 4^k (2^64 for k = 32), thinned by `mult`; stride = floor(keyspace / mult / n) */
  unsigned __int128 space = l->word_length == 32 ? ((unsigned __int128) 1 << 64) : ((unsigned __int128) 1 << (2 * l->word_length));
  space /= mult;
  unsigned __int128 st = space / n;
  if (st > 0xffffffffffffffffull) st = 0xffffffffffffffffull;
  const uint64_t stride = (uint64_t) st;
  if (!stride) return gt4hip_fail (ctx, GT4HIP_EINVAL, "gt4hip_generate: %llu keys do not fit k=%u", (unsigned long long) n, l->word_length);
  HIPCHK (ctx, launch_generate (ctx->stream, ctx->grid_limit, (uint32_t *) l->dev, n, stride, key_seed, count_seed, max_count, mult, add));
  HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
  return GT4HIP_OK;
}

extern "C" int gt4hip_generate (gt4hip_context *ctx, gt4hip_list *l, uint64_t n, uint64_t seed, uint32_t max_count)
{
  return gt4hip_generate_ex (ctx, l, n, seed, seed + 1, max_count, 1, 0);
}

/* ------------------------------------------------------------------ workspace */

int gt4hip_grow (gt4hip_context *ctx, void **p, size_t *have, size_t need)
{
  if (*have >= need) return GT4HIP_OK;
  if (*p) {
    HIPCHK (ctx, hipStreamSynchronize (ctx->stream));
    HIPCHK (ctx, hipFree (*p));
    *p = NULL;
    *have = 0;
  }
  need += need / 8; /* slack so that slightly larger follow-up calls do not reallocate */
  hipError_t e = gt4hip_dev_alloc (ctx, p, need);
  if (e != hipSuccess) return gt4hip_fail (ctx, GT4HIP_ENOMEM, "workspace hipMalloc of %zu bytes failed: %s", need, hipGetErrorString (e));
  *have = need;
  return GT4HIP_OK;
}
