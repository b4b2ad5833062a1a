/* gt4hip_pair_variant.h -- which k_pair_merge<NT, IPT, MODE, OPS, FAST, OPSET> instantiation a pair call takes: the
 * call's parameters, the kernel's geometry constants and the one selection function (pair_variant).  Plain C++17, no HIP
 * header: tests/harness/pair_variant_print.cc compiles it with g++ and ties tests/pair_variants.py to it. */
#ifndef GT4HIP_PAIR_VARIANT_H
#define GT4HIP_PAIR_VARIANT_H

#include <stdint.h>

namespace gt4 {

/* Internal rule code on top of the reference's enum Rules (src/glistcompare.c:45-54):
 * the running minimum of intersect_multi, which restarts whenever it is 0
 * (`if (!freq || c < freq) freq = c`, src/glistcompare.c:669). */
constexpr uint32_t RULE_MINZ = 8;

/* How an output stream decides to keep a key once its count is computed. */
enum Filter : uint32_t {
  FILTER_REFERENCE = 0, /* include_in_{union,intersection,complement}, src/glistcompare.c:459-489   */
  FILTER_RAW = 1,       /* keep every key of the stream's domain (intermediate N-way levels)        */
  FILTER_RESULT = 2     /* keep iff count >= cutoff (union_multi/intersect_multi, :574, :682)       */
};

struct PairParams {
  uint32_t ops;            /* bit s: stream s is produced (0 union, 1 intrsec, 2 diff1, 3 diff2) */
  uint32_t rule[4];        /* resolved rule per stream (never DEFAULT)                           */
  uint32_t cutoff;
  uint32_t subtract;       /* diff1 only                                                         */
  uint32_t count_override;
  uint32_t filter;
  uint32_t spin_limit;     /* bound of every inter-workgroup wait (0: the default, ~seconds); tests set it low */
  uint32_t scan_group;     /* 0: one scanner wavefront per stream; 1: summers + chainer (launches with many rows) */
  uint32_t dynamic;        /* 0: tiles dealt round-robin; 1: by a ticket counter (ctl->ticket), three tiles ahead */
  uint32_t a_rows_off;     /* A-only kernels: 0: a tile whose A records fit half the position rows takes the A-rows body; 1: never */
};

enum MergeMode : int {
  MODE_COUNT = 0,     /* totals only (--count_only), also pass 1 of the two-pass path: writes tile counts */
  MODE_LOOKBACK = 1,  /* single pass: a scanner wavefront chains tile totals into output offsets          */
  MODE_OFFSETS = 2    /* pass 2 of the two-pass path: tile offsets already scanned                       */
};

/* Geometry of the merge kernel: workgroups of 512 threads (geom 0: count-only
 * calls) or 1024 threads (geom 1: calls that materialise records), MERGE_VT positions per thread --
 * 6 for the single-output intersection (merge_ipt).  A tile holds
 * threads x positions - 64 records (the pair fix-up makes it +-1): in the workgroup's position
 * space the B records start at the next multiple of 64 after the A records, so that no 64-position
 * chunk mixes the two lists, and both record ranges fit in 16-byte chunks. */
/* Two workgroup geometries (measured): count-only calls run fastest with 512 threads
 * and 2048-record tiles (two workgroups per CU overlap their phases); calls that materialise
 * records run fastest with 1024 threads and 4096-record tiles (half as many tiles on the scan
 * chain, whose hop latency is fixed, and room for the staging slots in one workgroup per CU). */
constexpr int MERGE_VT = 4;
constexpr int MERGE_TILE_SLACK = 64;

constexpr int GT4_IPT_UNION = 4; /* 6 (one staging slot written out late) measured 3 % slower than 4 with two slots */
constexpr int GT4_IPT_INTERSECT = 6;
constexpr int GT4_IPT_INTERSECT_SMALL = 4; /* positions per thread of the 512-thread intersection (experiments: 6) */

/* launch bound (waves per SIMD): count-only kernels of the small geometry fit 85 VGPRs and 26 KB of
 * LDS -> three workgroups per CU; everything else runs at 4 waves per SIMD */
constexpr int merge_waves_per_simd (int nt, int mode, int ops = 0, int fast = 0)
{
  /* the small geometry's folded intersection fits 80 registers and 50 KB too: three workgroups per CU */
  return (nt == 512 && (mode == MODE_COUNT || (ops == 2 && fast == 1 && GT4_IPT_INTERSECT_SMALL <= 4))) ? 6 : 4;
}

/* records per thread: an intersection does per-record work on the A half of a tile only and
 * stages at most half a tile, so its tiles are 1.5x as long (6 positions per thread, 6080 records:
 * the per-tile costs -- barriers, ring, scan, fetch set-up -- are paid two thirds as often) */
constexpr int merge_ipt (int nt, int ops_class)
{
  return (nt == 1024 && ops_class == 2) ? GT4_IPT_INTERSECT
         : ((nt == 1024 && ops_class == 1) ? GT4_IPT_UNION : ((nt == 512 && ops_class == 2) ? GT4_IPT_INTERSECT_SMALL : MERGE_VT)); /* 0 (any) and 4 (complement): MERGE_VT */
}

/* One instantiation of k_pair_merge, as values: cls is the template's OPS (the kernel specialisation of a set of
 * outputs: one of {union, intersection, first complement} alone, else 0). */
struct PairVariant {
  int nt, ipt, mode, cls, fast, opset;
};

/* the fixed output sets (OPSET) are built for the geometry that runs them by default: 512 threads count, 1024 write */
constexpr bool opset_geometry (int nt, int mode) { return mode == MODE_COUNT ? nt == 512 : nt == 1024; }

/* the instantiations that exist: exactly what pair_variant can return (k_pair_merge asserts it, the dispatch in
 * gt4hip_kernels.hip instantiates nothing else) */
constexpr bool pair_variant_exists (const PairVariant &v)
{
  return (v.nt == 512 || v.nt == 1024) && (v.mode == MODE_COUNT || v.mode == MODE_LOOKBACK || v.mode == MODE_OFFSETS) &&
         (v.cls == 0 || v.cls == 1 || v.cls == 2 || v.cls == 4) && v.ipt == merge_ipt (v.nt, v.cls) &&
         (v.fast == 0 || v.fast == 1 || ((v.fast == 2 || v.fast == 3) && (v.cls == 1 || v.cls == 2))) &&
         (v.opset == 0 || ((v.opset == 3 || v.opset == 5 || v.opset == 15) && v.cls == 0 && v.fast == 1 && opset_geometry (v.nt, v.mode)));
}

/* THE selection: the instantiation a launch of `mode` takes in geometry `geom` (0: 512 threads, 1: 1024) for the
 * call's parameters.  Single-output calls (glistcompare -u / -i, every N-way level) take a specialised kernel. */
constexpr PairVariant pair_variant (int geom, int mode, const PairParams &p)
{
  const int nt = geom ? 1024 : 512;
  const int cls = (p.ops == 1u || p.ops == 2u || p.ops == 4u) ? (int) p.ops : 0;
  /* the rule-folded variant a call takes (see FAST in k_pair_merge); 0: the general coefficient form.  2 and 3 arise
   * for the union and the intersection only: the other classes have no such kernels */
  int fast = 0;
  if (p.filter == FILTER_REFERENCE) {
    if (cls == 1 && p.rule[0] == 1u) fast = 1;
    if (cls == 2 && p.rule[1] == 3u) fast = 1;
    if (cls == 4 && p.rule[2] == 2u && !p.subtract) fast = 1;
  } else if (cls == 1 && p.rule[0] == 1u) {
    fast = p.filter == FILTER_RAW ? 2 : 3; /* N-way union levels: keep every key / keep sums >= cutoff (union_multi, :574) */
  } else if (cls == 2 && p.rule[1] == RULE_MINZ) {
    fast = p.filter == FILTER_RAW ? 2 : 3; /* the steps of intersect_multi's chain under its default rule (:655-683) */
  }
  /* any combination of outputs with every requested stream on its default rule, any cutoff, no -du */
  if (cls == 0 && p.filter == FILTER_REFERENCE && !p.subtract && (!(p.ops & 1u) || p.rule[0] == 1u) && (!(p.ops & 2u) || p.rule[1] == 3u) &&
      (!(p.ops & 4u) || p.rule[2] == 2u) && (!(p.ops & 8u) || p.rule[3] == 2u))
    fast = 1;
  /* the commonest output sets with the default rules (-u -i, -u -d, all four): the stream set is a
   * compile-time constant */
  const bool set = cls == 0 && fast == 1 && (p.ops == 3u || p.ops == 5u || p.ops == 15u) && opset_geometry (nt, mode);
  return PairVariant{ nt, merge_ipt (nt, cls), mode, cls, fast, set ? (int) p.ops : 0 };
}

constexpr uint64_t merge_tile_records (const PairVariant &v) { return (uint64_t) v.nt * v.ipt - MERGE_TILE_SLACK; }

}  // namespace gt4

#endif
