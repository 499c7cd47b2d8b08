// yk_seed_table.hpp — the seed table's key and index (host and device; DESIGN.md §3 "Seed table").
//
// The counter seed of sample s of image pixel (x, y) is seed0 + (y*W + x)*spp + s in uint32
// arithmetic (ykd::sample_seed): a function of seed0, the image width, the call's spp and the pixel
// alone, not of the scene, the camera, max_depth or t_min.  x_397 of the mt19937 seeding sequence
// (ykd::mt_walk397xn) is a pure function of the seed, so a context that renders one tile at one spp
// again and again (a camera move, a scene edit, an animation) walks the same seeds every frame.  The
// table keeps x_397 of every sample of the tile, one uint32_t each, filled by the second
// consecutive eligible call of a key (which walks as ever and also stores; the first only walks)
// and read by the sky kernel in the calls after it.
//
// Index: tab[s * T + q], s the sample in [0, spp), q the TILE PIXEL (tile row * tile width + tile
// column: the value the processing orders hold) and T the tile's pixel count.  It depends on
// neither the launch plan (which samples a launch takes) nor on which order lists the pixel (the
// sky split moves pixels between the path order and the sky list with the camera) nor on the wrap
// of the seed.  The 64 lanes of a warm-up wave are one 8 x 8 block of one sample: eight runs of
// 32 bytes.
#ifndef YK_SEED_TABLE_HPP
#define YK_SEED_TABLE_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define YKSEED_HD __host__ __device__
#else
#define YKSEED_HD
#endif

namespace ykseed {

// What the seeds of a tile depend on: seed0, the image width, spp and the tile's row and column set
// (yk_render_params' fields; a tile of every column is normalised to 0, W, 1, 0).
struct Key {
  uint32_t seed0, W, spp;
  uint32_t row_begin, row_count, row_stride, row_band_log2;
  uint32_t col_begin, col_count, col_stride, col_band_log2;
};
inline Key make_key(uint32_t seed0, uint32_t W, uint32_t spp, uint32_t row_begin, uint32_t row_count,
                    uint32_t row_stride, uint32_t row_band_log2, uint32_t col_begin, uint32_t col_count,
                    uint32_t col_stride, uint32_t col_band_log2) {
  if (!col_count) return Key{seed0, W, spp, row_begin, row_count, row_stride, row_band_log2, 0u, W, 1u, 0u};
  return Key{seed0,      W,         spp,        row_begin,    row_count, row_stride, row_band_log2,
             col_begin,  col_count, col_stride, col_band_log2};
}
inline bool same_key(const Key& a, const Key& b) {
  return a.seed0 == b.seed0 && a.W == b.W && a.spp == b.spp && a.row_begin == b.row_begin &&
         a.row_count == b.row_count && a.row_stride == b.row_stride && a.row_band_log2 == b.row_band_log2 &&
         a.col_begin == b.col_begin && a.col_count == b.col_count && a.col_stride == b.col_stride &&
         a.col_band_log2 == b.col_band_log2;
}

// tile pixels T (check_params keeps it below 2^31) and the table's words, T * spp
YKSEED_HD inline uint32_t tile_pixels(const Key& k) { return k.row_count * k.col_count; }
YKSEED_HD inline uint64_t table_words(const Key& k) { return (uint64_t)tile_pixels(k) * k.spp; }

// the word of sample s of tile pixel q in a table of T tile pixels (64 bits: the headline frame's
// table has 1.06e9 words, config 5's 8.5e9)
YKSEED_HD inline uint64_t table_index(uint32_t s, uint32_t q, uint32_t T) { return (uint64_t)s * T + q; }

// image row of tile row t and image column of tile column j (bands of 2^band_log2, every stride-th)
YKSEED_HD inline uint32_t tile_y(const Key& k, uint32_t t) {
  return k.row_begin + (((t >> k.row_band_log2) * k.row_stride) << k.row_band_log2) +
         (t & ((1u << k.row_band_log2) - 1u));
}
YKSEED_HD inline uint32_t tile_x(const Key& k, uint32_t j) {
  return k.col_begin + (((j >> k.col_band_log2) * k.col_stride) << k.col_band_log2) +
         (j & ((1u << k.col_band_log2) - 1u));
}
// the counter seed whose x_397 the word table_index(s, q, T) holds
YKSEED_HD inline uint32_t seed_at(const Key& k, uint32_t s, uint32_t q) {
  const uint32_t t = q / k.col_count, j = q - t * k.col_count;
  return k.seed0 + (tile_y(k, t) * k.W + tile_x(k, j)) * k.spp + s;
}

}  // namespace ykseed

#endif
