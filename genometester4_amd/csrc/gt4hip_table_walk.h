/* gt4hip_table_walk.h -- how a kernel walks a gt4hip_count_table as gt4hip_union_table leaves it, ragged or contiguous
 * (DESIGN.md 4.11): in SEGMENTS of consecutive rows -- the rows of one tile of the N-way tile kernel in a ragged table (they
 * lie together where the tile's records start, so no row is searched for), GT4HIP_SELECT_SEGMENT rows in a contiguous one.
 * Shared by gt4hip_select.hip and gt4hip_pairwise.hip; include behind gt4hip_device.h and gt4hip_host.h. */
#ifndef GT4HIP_TABLE_WALK_H
#define GT4HIP_TABLE_WALK_H

namespace gt4 {
namespace {

struct SelTable {
  const u64 *keys;
  const u32 *counts;
  u32 n_lists;
  u64 n_keys;
  const u64 *compact, *padded; /* ragged: rows before every tile, where the tile's rows lie (segments + 1 entries); else NULL */
  u64 segments;
};

/* segment s: its first row in the compact numbering, where that row lies in the arrays, and its rows.  All wave-uniform.
 * Whatever the index says, no row beyond n_keys is touched in the per-row arrays or the output. */
__device__ __forceinline__ void segment_of (const SelTable &t, u64 s, u64 &row_base, u64 &src_base, u32 &rows)
{
  u64 end;
  if (t.compact) {
    row_base = t.compact[s];
    end = t.compact[s + 1];
    src_base = t.padded[s];
  } else {
    row_base = s * (u64) GT4HIP_SELECT_SEGMENT;
    end = row_base + GT4HIP_SELECT_SEGMENT;
    src_base = row_base;
  }
  if (end > t.n_keys) end = t.n_keys;
  if (row_base > end) row_base = end;
  const u64 n = end - row_base;
  rows = n < 0x40000000ull ? (u32) n : 0x40000000u;
}

/* the walk of a table on the host's side: its arrays and its segments (0: nothing to walk) */
inline SelTable table_walk (const gt4hip_count_table *table)
{
  SelTable t;
  t.keys = (const u64 *) table->device_keys;
  t.counts = (const u32 *) table->device_counts;
  t.n_lists = table->n_lists;
  t.n_keys = table->n_keys;
  t.compact = (const u64 *) gt4hip_table_compact_bases (const_cast<gt4hip_count_table *> (table));
  t.padded = (const u64 *) gt4hip_table_padded_bases (const_cast<gt4hip_count_table *> (table));
  t.segments = t.compact ? gt4hip_table_ragged_tiles (table) : (t.n_keys + GT4HIP_SELECT_SEGMENT - 1) / GT4HIP_SELECT_SEGMENT;
  return t;
}

}  // namespace
}  // namespace gt4

#endif
