/* gt4_cli.c -- the helpers of gt4_cli.h.  Of the device layer only gt4hip_list_download_range and gt4hip_last_error are called. */
#define _GNU_SOURCE
#include "gt4_cli.h"
#include "gt4_listfile.h"
#include "gt4hip.h"

#include <errno.h>
#include <string.h>
#include <unistd.h>

int gt4_cli_find_option (const GT4CliOption *options, size_t n_options, const char *arg)
{
  for (size_t i = 0; i < n_options; i++)
    if (!strcmp (arg, options[i].name)) return options[i].opt;
  return -1;
}

void gt4_cli_print_version (FILE *to, const char *tool)
{
  fprintf (to, "%s version %u.%u.%u (%s)\n", tool, GT4_VERSION_MAJOR, GT4_VERSION_MINOR, GT4_VERSION_MICRO, GT4_VERSION_QUALIFIER);
}

void gt4_cli_print_help (FILE *to, const char *tool, const char *const *lines, size_t n_lines)
{
  gt4_cli_print_version (to, tool);
  for (size_t i = 0; i < n_lines; i++) fprintf (to, "%s\n", lines[i]);
}

uint64_t gt4_cli_parse_bytes (const char *s)
{
  if (!s || !*s) return 0;
  char *end;
  double v = strtod (s, &end);
  if (*end == 'K' || *end == 'k') v *= 1024.0;
  else if (*end == 'M' || *end == 'm') v *= 1024.0 * 1024.0;
  else if (*end == 'G' || *end == 'g') v *= 1024.0 * 1024.0 * 1024.0;
  return v > 0 ? (uint64_t) v : 0;
}

void gt4_cli_read_environment (int *device, int *verbose)
{
  const char *e;
  *device = (e = getenv ("GT4HIP_DEVICE")) ? atoi (e) : 0;
  *verbose = (e = getenv ("GT4HIP_VERBOSE")) && atoi (e);
}

int gt4_cli_refuse_gzip (const char *name, int c0, int c1)
{
  if (c0 != 0x1f || c1 != 0x8b) return 0;
  fprintf (stderr, "Error: %s is gzip-compressed: decompress it first (compressed sequence files are not read)\n", name);
  return 1;
}

uint64_t gt4_cli_name_length (const unsigned char *data, uint64_t size, uint64_t name_pos)
{
  uint64_t len = 0;
  if (!data || name_pos >= size) return 0;
  while (name_pos + len < size && data[name_pos + len] > ' ') len++;
  return len;
}

void gt4_mask_tail_init (GT4MaskTail *t, int soft, unsigned char mask_byte, GT4MaskWrite write, void *arg)
{
  memset (t, 0, sizeof *t);
  t->soft = soft, t->mask_byte = mask_byte, t->write = write, t->arg = arg;
}

/* where the tail to hold begins in b[0 .. n): at the (k - 1)-th last byte >= ' '; n when k is 1; (size_t) -1 when b holds
 * fewer (*seen: how many it holds) */
static size_t mask_hold_point (const unsigned char *b, size_t n, unsigned int want, unsigned int *seen)
{
  size_t i = n;
  *seen = 0;
  if (!want) return n;
  while (i) {
    i--;
    if (b[i] >= ' ' && ++*seen == want) return i;
  }
  return (size_t) -1;
}

static int mask_tail_keep (GT4MaskTail *t, const unsigned char *bytes, size_t n, int append)
{
  const size_t at = append ? t->n : 0;
  if (n > (size_t) -1 - at) return 1;
  if (at + n > t->cap) {
    const size_t cap = at + n + (at + n) / 2 + 64;
    unsigned char *h = (unsigned char *) realloc (t->held, cap > at + n ? cap : at + n);
    if (!h) return 1;
    t->held = h, t->cap = cap > at + n ? cap : at + n;
  }
  if (n) memmove (t->held + at, bytes, n); /* (bytes may lie in t->held) */
  t->n = at + n;
  return 0;
}

int gt4_mask_tail_push (GT4MaskTail *t, const unsigned char *masked, size_t len, unsigned int back, unsigned int k)
{
  size_t i = t->n;
  while (back) {
    if (!i) return 1;
    i--;
    if (t->held[i] >= ' ') {
      t->held[i] = t->soft ? (unsigned char) (t->held[i] | 0x20) : t->mask_byte;
      back--;
    }
  }
  const unsigned int want = k ? k - 1 : 0;
  unsigned int in_piece = 0, in_tail = 0;
  size_t hold = mask_hold_point (masked, len, want, &in_piece);
  if (hold != (size_t) -1) { /* the piece alone holds the new tail: the old one and the piece's front go out */
    if (t->n && t->write (t->held, t->n, t->arg)) return 1;
    if (hold && t->write (masked, hold, t->arg)) return 1;
    return mask_tail_keep (t, masked + hold, len - hold, 0);
  }
  hold = mask_hold_point (t->held, t->n, want - in_piece, &in_tail);
  if (hold != (size_t) -1 && hold) {
    if (t->write (t->held, hold, t->arg)) return 1;
    if (mask_tail_keep (t, t->held + hold, t->n - hold, 0)) return 1;
  }
  return mask_tail_keep (t, masked, len, 1);
}

int gt4_mask_tail_finish (GT4MaskTail *t)
{
  const int failed = t->n && t->write (t->held, t->n, t->arg);
  free (t->held);
  t->held = NULL, t->n = t->cap = 0;
  return failed;
}

int gt4_cli_write_list_file (gt4hip_context *ctx, const gt4hip_list *list, unsigned int word_length, uint64_t n_words, uint64_t total_count,
                             const char *final_name, unsigned int mode, const char *prefix)
{
  char tmp_name[2100];
  snprintf (tmp_name, sizeof tmp_name, "%.2048s.tmp", final_name);
  GT4ListWriter w;
  if (gt4_listwriter_begin (&w, tmp_name, word_length, mode)) {
    fprintf (stderr, "%sCannot create output file %s\n", prefix, tmp_name);
    return 1;
  }
  int bad = 0;
  void *buf = n_words ? malloc ((size_t) (n_words < DOWNLOAD_CHUNK ? n_words : DOWNLOAD_CHUNK) * 12u) : NULL;
  if (n_words && !buf) bad = 1;
  for (uint64_t first = 0; first < n_words && !bad; first += DOWNLOAD_CHUNK) {
    const uint64_t cnt = n_words - first < DOWNLOAD_CHUNK ? n_words - first : DOWNLOAD_CHUNK;
    if (gt4hip_list_download_range (ctx, list, first, cnt, buf)) {
      fprintf (stderr, "Error: reading results back from the GPU failed: %s\n", gt4hip_last_error (ctx));
      bad = 1;
    } else if (gt4_listwriter_append (&w, buf, cnt)) {
      fprintf (stderr, "Error: writing %s failed: %s\n", tmp_name, strerror (errno));
      bad = 1;
    }
  }
  free (buf);
  if (bad) {
    gt4_listwriter_abort (&w);
    unlink (tmp_name);
    return 1;
  }
  if (gt4_listwriter_finish (&w, n_words, total_count)) {
    fprintf (stderr, "Error: writing %s failed: %s\n", tmp_name, strerror (errno));
    unlink (tmp_name);
    return 1;
  }
  if (rename (tmp_name, final_name)) {
    fprintf (stderr, "%sCannot rename %s to %s\n", prefix, tmp_name, final_name);
    return 2;
  }
  return 0;
}
