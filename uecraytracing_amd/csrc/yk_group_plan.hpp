// yk_group_plan.hpp — the band and exchange plan of a group film's filter (include/ykgpu.h "group
// films").  A pure host function, no HIP in here, so the CPU tests reach it
// (yk_host.cpp yk_group_film_plan).
//
// The render deals tile row t to entry t mod k, where it is row t / k of that entry's sub-tile.
// The filter deals consecutive rows: entry e owns the band [begin, begin + count), the first
// rows % k bands one row taller than the rest, and holds the rows [lo, hi) = band grown by `halo`
// and clipped at the tile.  An entry without a band has lo == hi and holds nothing.  The rows of
// one source inside one band+halo are consecutive in the source and land every k-th row in the
// destination: one pitched copy per (source, destination) pair and plane.
#ifndef YK_GROUP_PLAN_HPP
#define YK_GROUP_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ykplan {

struct Band {
  uint32_t begin, count;  // the tile rows whose outputs the entry keeps
  uint32_t lo, hi;        // the tile rows it holds: [max(0, begin - halo), min(rows, begin + count + halo))
};

struct Copy {
  uint32_t src, src_row;  // the entry that rendered the rows and the first one, in its sub-tile
  uint32_t rows;          // consecutive source rows
  uint32_t dst, dst_row;  // the entry that holds them and the first one's row in its [lo, hi)
  uint32_t dst_pitch;     // rows between two of them in the destination (k)
};

inline void group_film_plan(uint32_t rows, uint32_t k, uint32_t halo, std::vector<Band>& bands,
                            std::vector<Copy>& copies) {
  bands.assign(k, Band{0, 0, 0, 0});
  copies.clear();
  if (!k) return;
  uint32_t at = 0;
  for (uint32_t e = 0; e < k; ++e) {
    Band& b = bands[e];
    b.begin = at;
    b.count = rows / k + (e < rows % k ? 1u : 0u);
    at += b.count;
    if (!b.count) {
      b.lo = b.hi = b.begin;
      continue;
    }
    b.lo = b.begin > halo ? b.begin - halo : 0;
    b.hi = (uint32_t)std::min<uint64_t>(rows, (uint64_t)b.begin + b.count + halo);
    for (uint32_t s = 0; s < k; ++s) {
      // the first tile row >= lo that entry s rendered
      const uint32_t t0 = b.lo + (s + k - b.lo % k) % k;
      if (t0 >= b.hi) continue;
      copies.push_back(Copy{s, t0 / k, (b.hi - t0 + k - 1) / k, e, t0 - b.lo, k});
    }
  }
}

}  // namespace ykplan

#endif
