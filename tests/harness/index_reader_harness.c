/*
 * index_reader_harness.c -- TEST INFRASTRUCTURE ONLY: opens a GT4I index with gt4_indexfile_open and reads everything
 * the reader exposes (every k-mer entry, every location, every file and sequence of the file block), so that
 * AddressSanitizer / UndefinedBehaviorSanitizer see any access a hostile header could lead out of the mapping.
 * Prints "rc=<code>" and, for a file that opens, "ok files=<n> sequences=<n> sum=<checksum>".  Built by
 * tests/test_hostile_index.py with gt4_listfile.c; no device code.
 */
#include <stdio.h>
#include <string.h>

#include "gt4_listfile.h"

int main (int argc, char **argv)
{
  GT4ListFile lf;
  if (argc != 2) return 2;
  const int rc = gt4_indexfile_open (argv[1], GT4_VERSION_MAJOR, &lf);
  printf ("rc=%d\n", rc);
  if (rc) return 0;
  uint64_t sum = 0, n_seqs = 0, v;
  for (uint64_t i = 0; i < 2 * lf.header.n_words; i++) {
    memcpy (&v, lf.index_kmers + 8 * i, 8);
    sum += v;
  }
  for (uint64_t i = 0; i < lf.index_locations; i++) {
    memcpy (&v, lf.index_location_words + 8 * i, 8);
    sum += v;
  }
  for (uint32_t i = 0; i < lf.index_n_files; i++) {
    GT4IndexFile f;
    if (gt4_indexfile_file (&lf, i, &f)) return 3;
    sum += f.size + strlen (f.name);
    for (uint64_t j = 0; j < f.n_sequences; j++) {
      GT4IndexSequence s;
      if (gt4_indexfile_sequence (&f, j, &s)) return 3;
      sum += s.name_pos + s.name_len + s.seq_pos + s.seq_len;
      n_seqs++;
    }
    GT4IndexSequence s;
    if (gt4_indexfile_sequence (&f, f.n_sequences, &s) != GT4_LISTFILE_ESIZE) return 4; /* one past the end is refused */
  }
  GT4IndexFile f;
  if (gt4_indexfile_file (&lf, lf.index_n_files, &f) != GT4_LISTFILE_ESIZE) return 4;
  printf ("ok files=%u sequences=%llu sum=%llu\n", lf.index_n_files, (unsigned long long) n_seqs, (unsigned long long) sum);
  gt4_listfile_close (&lf);
  return 0;
}
