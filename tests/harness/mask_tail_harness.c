/* mask_tail_harness.c -- the hold-back unit of glistquery --mask (GT4MaskTail, csrc/gt4_cli.c) as a stand-alone program,
 * for the sanitizer run of tests/test_gqmask_host_sanitizers.py.
 *
 *   mask_tail_harness FILE K SOFT PIECE BACK...
 *
 * FILE holds a text as gt4hip_query_mask_text gives it piece by piece (each piece's own covered bases replaced); it is pushed
 * in pieces of PIECE bytes with the BACK of each piece, then finished; what the unit writes goes to stdout.  Behind every
 * push the unit may hold at most K - 1 bytes >= ' ', beginning with one unless it holds everything it was ever given and
 * has written nothing: exit status 3 when it holds more, 2 for a failed call or bad arguments. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../genometester4_amd/csrc/gt4_cli.h"

static size_t written;

static int to_stdout (const void *bytes, size_t n, void *arg)
{
  (void) arg;
  written += n;
  return fwrite (bytes, 1, n, stdout) != n;
}

int main (int argc, char **argv)
{
  if (argc < 5) return 2;
  FILE *f = fopen (argv[1], "rb");
  if (!f) return 2;
  fseek (f, 0, SEEK_END);
  const long size = ftell (f);
  rewind (f);
  unsigned char *text = (unsigned char *) malloc (size > 0 ? (size_t) size : 1);
  if (!text || (size > 0 && fread (text, 1, (size_t) size, f) != (size_t) size)) return 2;
  fclose (f);
  const unsigned int k = (unsigned int) strtoul (argv[2], NULL, 10);
  const int soft = atoi (argv[3]);
  const size_t piece = (size_t) strtoull (argv[4], NULL, 10);
  if (!piece || !k) return 2;
  GT4MaskTail t;
  gt4_mask_tail_init (&t, soft, 'N', to_stdout, NULL);
  size_t pos = 0;
  int arg = 5;
  while (pos < (size_t) size) {
    const size_t len = (size_t) size - pos < piece ? (size_t) size - pos : piece;
    const unsigned int back = arg < argc ? (unsigned int) strtoul (argv[arg], NULL, 10) : 0;
    arg++;
    /* the piece from a block of exactly its size: an access behind it is one the sanitizer sees */
    unsigned char *copy = (unsigned char *) malloc (len);
    if (!copy) return 2;
    memcpy (copy, text + pos, len);
    const int failed = gt4_mask_tail_push (&t, copy, len, back, k);
    free (copy);
    if (failed) return 2;
    pos += len;
    unsigned int kept = 0;
    for (size_t i = 0; i < t.n; i++) kept += t.held[i] >= ' ';
    if (kept > k - 1 || written + t.n != pos) return 3;
    if (t.n && t.held[0] < ' ' && written) return 3;
  }
  if (gt4_mask_tail_finish (&t) || written != (size_t) size) return 2;
  free (text);
  return fflush (stdout) != 0;
}
