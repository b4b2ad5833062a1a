/* tests/harness/corank_model.cc -- TEST INFRASTRUCTURE ONLY: the pair partition's co-rank search
 * (genometester4_amd/csrc/gt4hip_corank.h, nothing else of the product) on two key arrays in host memory, with its probes
 * counted.  The two levels run as the kernels run them: the coarse boundaries over the whole of A, every tile boundary
 * between its two coarse neighbours.
 * usage:  corank_model KEYS_A KEYS_B TILE_RECORDS      (the key files: ascending little-endian u64, nothing else)
 * stdout: `k <PART_COARSE> <CORANK_GUIDED_MAX> <CORANK_NARROW>` (the header's constants), then one line per coarse boundary, `c <c> <co-rank guided> <probes guided> <co-rank bisected> <probes bisected> <width>`,
 *         then one per tile boundary, `t <t> <a guided> <b guided> <probes guided> <a bisected> <b bisected> <probes bisected> <width>`
 *         (width: the bracket the search started from after its clamp to the diagonal; a, b: the part[] words).
 * tests/test_corank_model.py builds it with g++ -fsanitize=address,undefined and holds it against numpy. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "gt4hip_corank.h"

struct KeyOf {
  const std::vector<uint64_t> *v;
  uint64_t operator() (uint64_t i) const { return v->at (i); } /* (range-checked: a probe outside the list aborts) */
};

static bool read_keys (const char *path, std::vector<uint64_t> &out)
{
  FILE *f = fopen (path, "rb");
  if (!f) return false;
  uint64_t buf[4096];
  size_t n;
  while ((n = fread (buf, 8, 4096, f)) > 0) out.insert (out.end (), buf, buf + n);
  fclose (f);
  return true;
}

/* the bracket a search starts from, as corank_search clamps it */
static uint64_t width (uint64_t nA, uint64_t nB, uint64_t diag, uint64_t lo, uint64_t hi)
{
  const uint64_t lo0 = diag > nB ? diag - nB : 0, hi0 = diag < nA ? diag : nA;
  if (lo < lo0) lo = lo0;
  if (hi > hi0) hi = hi0;
  return hi > lo ? hi - lo : 0;
}

int main (int argc, char **argv)
{
  std::vector<uint64_t> A, B;
  if (argc != 4 || !read_keys (argv[1], A) || !read_keys (argv[2], B)) return 2;
  const uint64_t T = strtoull (argv[3], NULL, 10);
  if (!T) return 2;
  const uint64_t nA = A.size (), nB = B.size (), total = nA + nB, tiles = (total + T - 1) / T;
  const uint64_t n_coarse = (tiles + gt4::PART_COARSE - 1) / gt4::PART_COARSE;
  const KeyOf ka = { &A }, kb = { &B };
  printf ("k %llu %d %llu\n", (unsigned long long) gt4::PART_COARSE, gt4::CORANK_GUIDED_MAX, (unsigned long long) gt4::CORANK_NARROW);
  std::vector<uint64_t> coarse[2];
  for (uint64_t c = 0; c <= n_coarse; c++) {
    uint32_t pr[2];
    for (int g = 0; g < 2; g++) coarse[g].push_back (gt4::corank_coarse_boundary (ka, nA, kb, nB, T, c, g == 0, &pr[g]));
    uint64_t diag = c * gt4::PART_COARSE * T;
    if (diag > total) diag = total;
    printf ("c %llu %llu %u %llu %u %llu\n", (unsigned long long) c, (unsigned long long) coarse[0][c], pr[0], (unsigned long long) coarse[1][c], pr[1],
            (unsigned long long) width (nA, nB, diag, 0, nA));
  }
  for (uint64_t t = 0; t <= tiles; t++) {
    const uint64_t c = t / gt4::PART_COARSE;
    uint64_t a[2], b[2];
    uint32_t pr[2];
    for (int g = 0; g < 2; g++) gt4::corank_tile_boundary (ka, nA, kb, nB, T, t, coarse[g][c], coarse[g][c + 1], g == 0, &a[g], &b[g], &pr[g]);
    uint64_t diag = t * T;
    if (diag > total) diag = total;
    const uint64_t w = (t % gt4::PART_COARSE) ? width (nA, nB, diag, coarse[1][c], coarse[1][c + 1]) : 0;
    printf ("t %llu %llu %llu %u %llu %llu %u %llu\n", (unsigned long long) t, (unsigned long long) a[0], (unsigned long long) b[0], pr[0], (unsigned long long) a[1],
            (unsigned long long) b[1], pr[1], (unsigned long long) w);
  }
  return 0;
}
