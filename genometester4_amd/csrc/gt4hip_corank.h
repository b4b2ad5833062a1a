/* gt4hip_corank.h -- the merge-path co-rank search of the pair partition (k_partition_coarse, k_partition in
 * gt4hip_kernels.hip) as a function template over two key-load functors.  Plain C++17, no HIP header: the kernels
 * instantiate it on device loads, tests/harness/corank_model.cc compiles it with g++ on arrays and counts its probes.
 *
 * The co-rank of a diagonal is the number of A records among the first `diag` records of merge (A, B), A first on ties:
 * the least a in [lo, hi] for which A[a] <= B[diag - 1 - a] does not hold.  The predicate is monotone in a, so ANY probe
 * position in [lo, hi) keeps the invariant "the bracket holds the answer" and the result is bisection's, whatever the
 * keys are; only the number of probes depends on where they are placed.  A probe is one key of A and one of B at
 * addresses no neighbouring thread shares; the partition's time follows their number, less than in proportion (measured:
 * profiles/round8/README.md).
 *
 * Guided search (a CorankGuide is given): the bracket comes from two coarse neighbours, whose diagonals and co-ranks
 * are known.
 *   probe 1      rank space: the co-rank is close to linear in the diagonal between the neighbours wherever the two
 *                lists' local densities keep their ratio, whatever the key values do;
 *   probes 2..4  key space (at most CORANK_KEY_PROBES): the two keys of the previous probe differ by delta, the bracket
 *                of the neighbours spans `slope` key units per step of a (both lists' key span per record, added: one
 *                step of a moves A's key up and B's down); the next probe goes delta / slope further, plus an overshoot
 *                of three times the square root of that step (the position noise of independent keys) and two, so that
 *                it lands on the other side of the answer and the bracket closes from both ends;
 *   the rest     plain midpoints.
 * Guards: every guided probe is clamped into [lo, hi); a key-placed probe that leaves more than 1 / CORANK_SHRINK of the
 * bracket ends guiding, a bracket of CORANK_NARROW records or fewer (three 128-byte lines of 12-byte records) ends it,
 * and a bracket whose end keys give no positive slope (one record, equal keys) never starts it.  Nor does a bracket whose
 * keys lie in stretches between wide gaps: there the mean slope says nothing about the keys next to a probe, the placed
 * probes are wasted and, unlike bisection's first midpoints, no two threads of the bracket share them (the
 * bench's clustered lists without this guard: 470 us per partition against bisection's 421, profiles/round8/README.md;
 * tests/test_corank_model.py holds the guard on its `stretches` input).  Such a bracket is known by its own ends, at no further
 * cache line: the first and the last gap of each list in it are all below 1 / CORANK_STRETCH of that list's mean gap
 * (independent keys: a gap is that small with probability 0.12, all four with 2e-4); it is bisected from the start.
 * WORST CASE: a search from a bracket of W = hi - lo records (after the clamp to the diagonal) makes at most
 * corank_bisect_bound (W) + CORANK_GUIDED_MAX probes: at most CORANK_GUIDED_MAX = 1 + CORANK_KEY_PROBES placed probes,
 * each of which takes at least one record off the bracket, then bisection of what is left, which needs
 * ceil (log2 (W' + 1)) probes at most for W' <= W.  Bisection alone makes at most corank_bisect_bound (W).
 * Arithmetic: key differences are taken larger minus smaller in 64 bits, steps in doubles that are compared with the
 * bracket's width before they are converted; nothing divides by zero and nothing signed can overflow (k = 32: keys 0
 * and 2^64 - 1 in one bracket, spans above 2^63).
 * No waits and nothing shared between threads: every thread's loop is its own. */
#ifndef GT4HIP_CORANK_H
#define GT4HIP_CORANK_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GT4_HD __host__ __device__ __attribute__ ((always_inline))
#else
#define GT4_HD __attribute__ ((always_inline))
#endif

namespace gt4 {

constexpr uint64_t PART_COARSE = 64; /* tiles per coarse partition interval: the 64 boundaries of a wavefront share one bracket */

constexpr int CORANK_KEY_PROBES = 3;                     /* K: key-placed probes after the rank-placed one */
constexpr int CORANK_GUIDED_MAX = 1 + CORANK_KEY_PROBES; /* the constant of the worst case */
constexpr uint64_t CORANK_NARROW = 32;                   /* records: guiding ends at this width */
constexpr uint64_t CORANK_SHRINK = 4;                    /* a key-placed probe must leave at most 1 / 4 of the bracket */
constexpr double CORANK_STRETCH = 8.0;                   /* first and last gap of both lists below 1 / 8 of the mean gap: keys in stretches */

/* The bracket's two coarse neighbours: co-rank a0 at diagonal d0, a1 at d1 (d0 <= diag <= d1, a0 <= a1, a1 - a0 <= d1 - d0). */
struct CorankGuide {
  uint64_t d0, a0, d1, a1;
};

/* most probes of a bisection over a bracket of w records (w + 1 candidates): ceil (log2 (w + 1)) */
GT4_HD inline uint32_t corank_bisect_bound (uint64_t w)
{
  uint32_t n = 0;
  while (w) {
    n++;
    w >>= 1;
  }
  return n;
}

/* The co-rank of `diag`, searched inside [lo, hi] (the caller's bracket must contain the answer).  key_a (i) / key_b (i):
 * the key of record i.  guided false: plain bisection (option "part_guided" = -1, `guide` is not looked at), else see above.  *probes, if
 * given, receives the number of probes (loop iterations; the four end keys of the guide's bracket, which all searches of
 * one bracket share, are not counted). */
template <class KeyA, class KeyB>
GT4_HD inline uint64_t corank_search (KeyA key_a, uint64_t nA, KeyB key_b, uint64_t nB, uint64_t diag, uint64_t lo, uint64_t hi,
                                      bool guided, const CorankGuide &guide, uint32_t *probes = nullptr)
{
  const uint64_t lo0 = diag > nB ? diag - nB : 0, hi0 = diag < nA ? diag : nA;
  if (lo < lo0) lo = lo0;
  if (hi > hi0) hi = hi0;
  /* phase 0: the rank-placed probe is next; 1: a key-placed probe at `next`; 2: midpoints */
  int phase = 2, left = 0;
  uint64_t next = 0;
  double slope = 0.0;
  if (guided && lo < hi && hi - lo > CORANK_NARROW && guide.d1 > guide.d0 && guide.a1 >= guide.a0) {
    const uint64_t dd = guide.d1 - guide.d0, da = guide.a1 - guide.a0, db = dd >= da ? dd - da : 0;
    const uint64_t off = diag > guide.d0 ? (diag < guide.d1 ? diag - guide.d0 : dd) : 0;
    const double r = (double) da * ((double) off / (double) dd); /* 0 <= r <= da */
    next = guide.a0 + (r < (double) da ? (uint64_t) r : da);
    phase = 0;
    /* key units per step of a over the neighbours' bracket */
    const uint64_t b0 = guide.d0 - guide.a0;
    bool stretches = true; /* every gap looked at is far below its list's mean gap */
    if (da > 1 && guide.a1 <= nA) {
      const uint64_t k0 = key_a (guide.a0), k1 = key_a (guide.a1 - 1);
      const double s = (double) (k1 - k0) / (double) (da - 1);
      slope += s;
      stretches = stretches && (double) (key_a (guide.a0 + 1) - k0) * CORANK_STRETCH < s && (double) (k1 - key_a (guide.a1 - 2)) * CORANK_STRETCH < s;
    }
    if (db > 1 && b0 + db <= nB) {
      const uint64_t k0 = key_b (b0), k1 = key_b (b0 + db - 1);
      const double s = (double) (k1 - k0) / (double) (db - 1);
      slope += s;
      stretches = stretches && (double) (key_b (b0 + 1) - k0) * CORANK_STRETCH < s && (double) (k1 - key_b (b0 + db - 2)) * CORANK_STRETCH < s;
    }
    left = slope > 0.0 ? CORANK_KEY_PROBES : 0;
    if (slope > 0.0 && stretches) phase = 2;
  }
  uint32_t n = 0;
  while (lo < hi) {
    uint64_t mid = lo + ((hi - lo) >> 1);
    if (phase < 2) mid = next < lo ? lo : (next >= hi ? hi - 1 : next);
    const uint64_t ka = key_a (mid), kb = key_b (diag - 1 - mid);
    n++;
    const uint64_t w0 = hi - lo;
    const bool up = ka <= kb;
    if (up) lo = mid + 1;
    else hi = mid;
    if (phase == 2) continue;
    const uint64_t w = hi - lo;
    if ((phase == 1 && w > w0 / CORANK_SHRINK) || left == 0 || w <= CORANK_NARROW) {
      phase = 2;
      continue;
    }
    left--;
    phase = 1;
    double step = (double) (up ? kb - ka : ka - kb) / slope;
    step += 3.0 * __builtin_sqrt (step) + 2.0;
    const uint64_t su = step < (double) (w - 1) ? (uint64_t) step : w - 1; /* w > CORANK_NARROW: never 0 */
    next = up ? lo + su : hi - 1 - su;
  }
  if (probes) *probes = n;
  return lo;
}

/* Boundary t of a partition into tiles of tile_records merged records: part[2 t], part[2 t + 1] = the records of A and of B
 * before the tile.  c_lo / c_hi: the co-ranks of the coarse boundaries t / PART_COARSE and the next (the boundary itself
 * when t is a multiple of PART_COARSE).  Keys are unique inside a list, so a key present in both lists sits as an adjacent
 * (A, B) pair in the merged order; if the diagonal falls between them the B record is pulled back into the earlier tile
 * so that one tile owns the pair. */
template <class KeyA, class KeyB>
GT4_HD inline void corank_tile_boundary (KeyA key_a, uint64_t nA, KeyB key_b, uint64_t nB, uint64_t tile_records, uint64_t t, uint64_t c_lo,
                                         uint64_t c_hi, bool guided, uint64_t *a_out, uint64_t *b_out, uint32_t *probes = nullptr)
{
  const uint64_t total = nA + nB, span = PART_COARSE * tile_records, c = t / PART_COARSE;
  uint64_t diag = t * tile_records;
  if (diag > total) diag = total;
  uint64_t a = c_lo;
  if (probes) *probes = 0;
  if (t % PART_COARSE) {
    CorankGuide g;
    g.d0 = c * span < total ? c * span : total;
    g.d1 = (c + 1) * span < total ? (c + 1) * span : total;
    g.a0 = c_lo;
    g.a1 = c_hi;
    a = corank_search (key_a, nA, key_b, nB, diag, c_lo, c_hi, guided, g, probes);
  }
  uint64_t b = diag - a;
  if (a > 0 && b < nB && key_a (a - 1) == key_b (b)) b += 1;
  *a_out = a;
  *b_out = b;
}

/* Coarse boundary c (every PART_COARSE-th tile boundary): searched over the whole of A, guided by the lists' ends. */
template <class KeyA, class KeyB>
GT4_HD inline uint64_t corank_coarse_boundary (KeyA key_a, uint64_t nA, KeyB key_b, uint64_t nB, uint64_t tile_records, uint64_t c, bool guided,
                                               uint32_t *probes = nullptr)
{
  const uint64_t total = nA + nB;
  uint64_t diag = c * PART_COARSE * tile_records;
  if (diag > total) diag = total;
  const CorankGuide g = { 0, 0, total, nA };
  return corank_search (key_a, nA, key_b, nB, diag, 0, nA, guided, g, probes);
}

}  // namespace gt4

#endif
