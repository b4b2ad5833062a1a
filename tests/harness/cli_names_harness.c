/* tests/harness/cli_names_harness.c -- TEST INFRASTRUCTURE ONLY: a stand-alone caller of the host-only helpers that
 * glistquery --per_sequence added to csrc/gt4_cli.c, built with AddressSanitizer and UndefinedBehaviorSanitizer by
 * tests/test_gqseq_host_sanitizers.py.  The file is read into a heap block of exactly its size, so that one byte read
 * behind it is a report.
 *
 *   cli_names_harness FILE POS...      prints "<pos>\t<length>\t<name>\n" for every position
 *   cli_names_harness --bytes TEXT...  prints gt4_cli_parse_bytes of every text */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../genometester4_amd/csrc/gt4_cli.h"

int main (int argc, char **argv)
{
  if (argc >= 2 && !strcmp (argv[1], "--bytes")) {
    for (int i = 2; i < argc; i++) printf ("%llu\n", (unsigned long long) gt4_cli_parse_bytes (argv[i]));
    printf ("%llu\n", (unsigned long long) gt4_cli_parse_bytes (NULL));
    return 0;
  }
  if (argc < 2) return 2;
  FILE *f = fopen (argv[1], "rb");
  if (!f) return 2;
  fseek (f, 0, SEEK_END);
  const long size = ftell (f);
  rewind (f);
  unsigned char *data = size ? (unsigned char *) malloc ((size_t) size) : NULL;
  if (size && (!data || fread (data, 1, (size_t) size, f) != (size_t) size)) return 2;
  fclose (f);
  for (int i = 2; i < argc; i++) {
    const uint64_t pos = strtoull (argv[i], NULL, 10);
    const uint64_t len = gt4_cli_name_length (data, (uint64_t) size, pos);
    printf ("%llu\t%llu\t", (unsigned long long) pos, (unsigned long long) len);
    if (len) fwrite (data + pos, 1, (size_t) len, stdout);
    printf ("\n");
  }
  free (data);
  return 0;
}
