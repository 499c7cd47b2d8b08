// Host-only driver of tests/test_sky_blocks.py: runs the sky-block classifier (yk_sky.hpp,
// implemented in yk_bvh.cpp) on a scene file and one tile geometry and prints the block grid as JSON.
//   driver <scene.txt> <W> <H> <row_begin> <row_count> <row_stride> <row_band_log2>
//          <col_begin> <col_count> <col_stride> <col_band_log2> <order_stride> [<repeat>]
// scene.txt: one line "camera" + 19 doubles (origin, lower_left_corner, horizontal, vertical, lens_u,
// lens_v, lens_radius), then "cx cy cz radius" per sphere.  order_stride picks the block shape as
// the library does (yk_schedule.hpp order_block).  repeat > 1 classifies that many times and
// reports the mean time of one (milliseconds) — the cost the first call of a context pays.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../uecraytracing_amd/csrc/yk_schedule.hpp"
#include "../uecraytracing_amd/csrc/yk_sky.hpp"

int main(int argc, char** argv) {
  if (argc != 13 && argc != 14) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 3;
  yk_camera cam;
  std::memset(&cam, 0, sizeof cam);
  double c[19];
  char word[16];
  if (std::fscanf(f, "%15s", word) != 1 || std::strcmp(word, "camera") != 0) return 4;
  for (int k = 0; k < 19; ++k)
    if (std::fscanf(f, "%lf", &c[k]) != 1) return 4;
  std::memcpy(cam.origin, c, 3 * sizeof(double));
  std::memcpy(cam.lower_left_corner, c + 3, 3 * sizeof(double));
  std::memcpy(cam.horizontal, c + 6, 3 * sizeof(double));
  std::memcpy(cam.vertical, c + 9, 3 * sizeof(double));
  std::memcpy(cam.lens_u, c + 12, 3 * sizeof(double));
  std::memcpy(cam.lens_v, c + 15, 3 * sizeof(double));
  cam.lens_radius = c[18];
  std::vector<double> centers, radii;
  double v[4];
  while (std::fscanf(f, "%lf %lf %lf %lf", &v[0], &v[1], &v[2], &v[3]) == 4) {
    centers.insert(centers.end(), v, v + 3);
    radii.push_back(v[3]);
  }
  std::fclose(f);
  uint32_t a[11];
  for (int k = 0; k < 11; ++k) a[k] = (uint32_t)std::strtoul(argv[2 + k], nullptr, 10);
  const yksky::Tile t{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]};
  uint32_t tw = 0, th = 0;
  order_block(a[10], tw, th);
  const int repeat = argc == 14 ? std::atoi(argv[13]) : 1;
  std::vector<uint8_t> flag;
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < (repeat > 0 ? repeat : 1); ++r)
    flag = yksky::sky_blocks(cam, centers.data(), radii.data(), (uint32_t)radii.size(), t, tw, th);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() /
                    (repeat > 0 ? repeat : 1);
  const uint32_t bx = (t.col_count + tw - 1) / tw, by = (t.row_count + th - 1) / th;
  std::printf("{\"tw\": %u, \"th\": %u, \"bx\": %u, \"by\": %u, \"ms\": %.4f, \"flags\": [", tw, th, bx, by, ms);
  for (size_t i = 0; i < flag.size(); ++i) std::printf("%s%u", i ? ", " : "", (unsigned)flag[i]);
  std::printf("]}\n");
  return flag.size() == (size_t)bx * by ? 0 : 5;
}
