// yk_sky.hpp — the sky-block classifier (host; implemented in yk_bvh.cpp beside the BVH build, the
// other culling structure made from the scene and the camera; DESIGN.md §3 "Sky blocks").
//
// A processing block (yk_pipeline.hip build_order: tw x th tile pixels) is a SKY BLOCK when no
// camera ray of any sample of any of its pixels can hit any sphere: every such sample is the
// reference's sky expression on its camera ray and needs no traversal, so those blocks leave the
// path kernel (yk_pipeline.hip yk_sky_samples renders them).
//
// The ray family of a block is everything camera_ray (yk_render_device.hpp) can produce for it:
// jitter canonicals in [0, 1]^2 over the bounding rectangle of its pixels in the image, so
// u in [x_min / W, (x_max + 1) / W], v in [(H - 1 - y_max) / H, (H - y_min) / H], focus point
// F = llc + u hor + v ver, and a lens offset off = lens_radius (px lens_u + py lens_v) with
// px^2 + py^2 < 1, so |off| <= L = lens_radius sqrt(|lens_u|^2 + |lens_v|^2).  A ray point is
//   P(t) = O + off + t d,   d = F - O - off,   t >= 0.
// Take a unit normal n with n.(F - O) >= L for every F of the block's rectangle (linear in F: the
// four corners decide).  Then n.d >= 0 for every direction of the family and n.off >= -L, so every
// ray point has n.(P - O) >= -L, and a sphere (C, r) with n.(C - O) < -(|r| + L) cannot be hit.
// Five such normals are tested: the axis of the block's pyramid (apex O, through the rectangle;
// this is the behind-the-camera test, and it needs the focus plane farther than the lens is wide)
// and the inward normals of four side planes through O, tilted outward from the pinhole pyramid's
// sides by the lens (planes through the edges of the rectangle widened by a few L).  (Planes of
// the pinhole pyramid itself with the lens in the distance instead, |r| + (1 + t_max) L, are weaker
// by the factor t_max, ~200 for the ground sphere of the book scenes: their horizon is then never
// excluded.)  A sixth test covers what planes miss beside a sphere that is large on the screen
// (the corners of its bounding rectangle): every direction of the family lies within the cone
// angle beta of the axis (the corners' angles, plus asin(L / f_min) for the lens), and from a lens
// point A the sphere lies within asin(|r| / |C - A|) of C - A, itself within asin(L / |C - O|) of
// C - O; an axis farther from C - O than the three angles together excludes the sphere.  rho = |r| + L also carries an explicit
// margin for the rounding of the camera's and the sphere test's arithmetic (yk_bvh.cpp; the only
// part that grows with t <= t_max = (|C - O| + |r| + L) / (f_min - L)).  t_min is ignored (that
// only flags fewer blocks).
//
// The test is conservative in one direction only: a flagged block has no hit, an unflagged block
// may have none either.  Nothing is flagged when a plane normal is not finite, when the pyramid
// is degenerate (a camera without extent, a focus plane closer than the lens is wide), or when
// the test cannot decide; a camera origin inside a sphere fails every plane test by itself.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/ykgpu.h"

namespace yksky {

// The image and the tile (yk_render_params' row and column sets; a tile of every column has
// col_begin 0, col_count W, col_stride 1, col_band_log2 0).
struct Tile {
  uint32_t W, H;
  uint32_t row_begin, row_count, row_stride, row_band_log2;
  uint32_t col_begin, col_count, col_stride, col_band_log2;
};

// flag[j * bx + i] != 0: block column i, block row j of the tile's grid of tw x th tile pixels
// (bx = ceil(col_count / tw), by = ceil(row_count / th)) is a sky block.  Blocks are tested under
// super-blocks of 8 x 8 blocks first, each block then only against the spheres its super-block
// could not exclude.
std::vector<uint8_t> sky_blocks(const yk_camera& cam, const double* centers, const double* radii, uint32_t n,
                                const Tile& t, uint32_t tw, uint32_t th);

}  // namespace yksky
