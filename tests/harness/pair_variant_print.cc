/* tests/harness/pair_variant_print.cc -- TEST INFRASTRUCTURE ONLY: the product's own selection of a k_pair_merge
 * instantiation (genometester4_amd/csrc/gt4hip_pair_variant.h, nothing else of the product) as a filter.
 * stdin:  lines of `geom mode ops rule0 rule1 rule2 rule3 cutoff subtract filter`
 * stdout: per line the instantiation's name as the compiler prints it, and the records per tile.
 * tests/test_pair_variant_map.py builds it with g++ and holds tests/pair_variants.py against it. */
#include <stdio.h>

#include "gt4hip_pair_variant.h"

int main ()
{
  int geom, mode;
  gt4::PairParams p = {};
  while (scanf ("%d %d %u %u %u %u %u %u %u %u", &geom, &mode, &p.ops, &p.rule[0], &p.rule[1], &p.rule[2], &p.rule[3], &p.cutoff, &p.subtract, &p.filter) == 10) {
    const gt4::PairVariant v = gt4::pair_variant (geom, mode, p);
    if (!gt4::pair_variant_exists (v)) return 2;
    printf ("k_pair_merge<%d, %d, %d, %d, %d, %d> %llu\n", v.nt, v.ipt, v.mode, v.cls, v.fast, v.opset, (unsigned long long) gt4::merge_tile_records (v));
  }
  return feof (stdin) ? 0 : 1;
}
