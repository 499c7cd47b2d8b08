// yk_host.cpp — host-side scene helpers of the C-ABI (no device code): the reference camera,
// the positionable camera extension and the named scenes of the BASELINE configs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ykgpu.h"
#include "yk_group_plan.hpp"
#include "yk_schedule.hpp"

namespace {

struct d3 {
  double x, y, z;
};
d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
d3 operator*(d3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
d3 operator/(d3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
d3 unit(d3 a) { return a / std::sqrt(dot(a, a)); }
void put(double* dst, d3 v) {
  dst[0] = v.x;
  dst[1] = v.y;
  dst[2] = v.z;
}

// Scene generator RNG: mt19937 + generate_canonical<double> (two words per double), the same
// engine the renderer draws from, so a scene is a pure function of its seed.
struct scene_rng {
  uint32_t x[624];
  uint32_t p = 624;
  explicit scene_rng(uint32_t sd) {
    x[0] = sd;
    for (uint32_t i = 1; i < 624; ++i) x[i] = 1812433253u * (x[i - 1] ^ (x[i - 1] >> 30)) + i;
  }
  uint32_t next() {
    if (p >= 624) {
      for (uint32_t k = 0; k < 624; ++k) {
        uint32_t y = (x[k] & 0x80000000u) | (x[(k + 1) % 624] & 0x7fffffffu);
        x[k] = x[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      p = 0;
    }
    uint32_t z = x[p++];
    z ^= z >> 11;
    z ^= (z << 7) & 0x9d2c5680u;
    z ^= (z << 15) & 0xefc60000u;
    z ^= z >> 18;
    return z;
  }
  double canonical() {
    double s = (double)next();
    s = s + (double)next() * 4294967296.0;
    double r = s / 18446744073709551616.0;
    return r >= 1.0 ? 1.0 - 0x1p-53 : r;
  }
  double uniform(double a, double b) { return canonical() * (b - a) + a; }
};

yk_sphere lam(d3 c, double r, d3 alb) {
  yk_sphere s{};
  put(s.center, c);
  s.radius = r;
  put(s.albedo, alb);
  s.material = YK_MATERIAL_LAMBERTIAN;
  return s;
}
yk_sphere met(d3 c, double r, d3 alb, double fuzz) {
  yk_sphere s = lam(c, r, alb);
  s.material = YK_MATERIAL_METAL;
  s.fuzz = fuzz;
  return s;
}
yk_sphere die(d3 c, double r, double ior) {
  yk_sphere s = lam(c, r, {1.0, 1.0, 1.0});
  s.material = YK_MATERIAL_DIELECTRIC;
  s.ior = ior;
  return s;
}

// RTIOW book 1 final scene (configs 3/4), or its dielectric-heavy variant (config 5).
std::vector<yk_sphere> random_scene(uint32_t seed, bool glass_heavy) {
  scene_rng rng(seed);
  std::vector<yk_sphere> w;
  w.push_back(lam({0, -1000, 0}, 1000, {0.5, 0.5, 0.5}));
  const double p_lam = glass_heavy ? 0.3 : 0.8, p_met = glass_heavy ? 0.5 : 0.95;
  for (int a = -11; a < 11; ++a) {
    for (int b = -11; b < 11; ++b) {
      const double choose = rng.canonical();
      const double cx = a + 0.9 * rng.canonical();
      const double cz = b + 0.9 * rng.canonical();
      const d3 center{cx, 0.2, cz};
      const d3 dd = center - d3{4, 0.2, 0};
      if (std::sqrt(dot(dd, dd)) <= 0.9) continue;
      if (choose < p_lam) {
        d3 a1{rng.canonical(), rng.canonical(), rng.canonical()};
        d3 a2{rng.canonical(), rng.canonical(), rng.canonical()};
        w.push_back(lam(center, 0.2, {a1.x * a2.x, a1.y * a2.y, a1.z * a2.z}));
      } else if (choose < p_met) {
        d3 alb{rng.uniform(0.5, 1), rng.uniform(0.5, 1), rng.uniform(0.5, 1)};
        const double fuzz = rng.uniform(0, 0.5);
        w.push_back(met(center, 0.2, alb, fuzz));
      } else {
        w.push_back(die(center, 0.2, 1.5));
      }
    }
  }
  w.push_back(die({0, 1, 0}, 1.0, 1.5));
  if (glass_heavy) {
    w.push_back(die({-4, 1, 0}, 1.0, 1.5));
    w.push_back(die({-4, 1, 0}, -0.9, 1.5));
  } else {
    w.push_back(lam({-4, 1, 0}, 1.0, {0.4, 0.2, 0.1}));
  }
  w.push_back(met({4, 1, 0}, 1.0, {0.7, 0.6, 0.5}, 0.0));
  return w;
}

}  // namespace

extern "C" {

uint32_t yk_image_height_for(uint32_t width) {
  return static_cast<uint32_t>(width / (16.0 / 9.0));  // source.cpp:59-62
}

int yk_camera_reference(yk_camera* out) {
  if (!out) return YK_ERR_INVALID;
  // camera.hpp:16-27, same operations in the same order
  const double aspect_ratio = 16.0 / 9.0;
  const double viewport_height = 2.0;
  const double viewport_width = aspect_ratio * viewport_height;
  const double focal_length = 1.0;
  const d3 h{viewport_width, 0.0, 0.0}, v{0.0, viewport_height, 0.0};
  std::memset(out, 0, sizeof(*out));
  put(out->origin, {0, 0, 0});
  put(out->horizontal, h);
  put(out->vertical, v);
  put(out->lower_left_corner, d3{0, 0, 0} - h / 2 - v / 2 - d3{0, 0, focal_length});
  out->lens_radius = 0.0;
  return YK_OK;
}

int yk_camera_look(yk_camera* out, const double lookfrom[3], const double lookat[3],
                   const double vup[3], double vfov_deg, double aspect, double aperture,
                   double focus_dist) {
  if (!out || !lookfrom || !lookat || !vup || !(vfov_deg > 0) || !(aspect > 0) ||
      !(focus_dist > 0) || !(aperture >= 0))
    return YK_ERR_INVALID;
  const double theta = vfov_deg * M_PI / 180.0;
  const double hh = std::tan(theta / 2);
  const double vh = 2.0 * hh, vw = aspect * vh;
  const d3 from{lookfrom[0], lookfrom[1], lookfrom[2]}, at{lookat[0], lookat[1], lookat[2]};
  const d3 w = unit(from - at);
  const d3 u = unit(cross({vup[0], vup[1], vup[2]}, w));
  const d3 v = cross(w, u);
  const d3 horizontal = u * (focus_dist * vw), vertical = v * (focus_dist * vh);
  std::memset(out, 0, sizeof(*out));
  put(out->origin, from);
  put(out->horizontal, horizontal);
  put(out->vertical, vertical);
  put(out->lower_left_corner, from - horizontal / 2 - vertical / 2 - w * focus_dist);
  put(out->lens_u, u);
  put(out->lens_v, v);
  out->lens_radius = aperture / 2;
  return YK_OK;
}

int yk_scene_build(const char* name, uint32_t seed, yk_sphere* spheres, uint32_t capacity,
                   uint32_t* count, yk_camera* camera) {
  if (!name) return YK_ERR_INVALID;
  const std::string n = name;
  std::vector<yk_sphere> w;
  yk_camera cam{};
  yk_camera_reference(&cam);
  if (n == "ref4") {  // source.cpp:103-112
    w = {lam({0, 0, -1}, 0.5, {0.7, 0.3, 0.3}), lam({0, -100.5, -1}, 100.0, {0.8, 0.8, 0.0}),
         met({-1.0, 0.0, -1.0}, 0.5, {0.8, 0.8, 0.8}, 0), met({1.0, 0.0, -1.0}, 0.5, {0.8, 0.6, 0.2}, 0)};
  } else if (n == "lambert3") {
    w = {lam({0, 0, -1}, 0.5, {0.7, 0.3, 0.3}), lam({0, -100.5, -1}, 100.0, {0.8, 0.8, 0.0}),
         lam({-1.0, 0.0, -1.0}, 0.5, {0.8, 0.8, 0.8})};
  } else if (n == "mixed12") {
    w = {lam({0, -100.5, -1}, 100.0, {0.8, 0.8, 0.0}),  lam({0, 0, -1}, 0.5, {0.1, 0.2, 0.5}),
         met({-1.0, 0.0, -1.0}, 0.5, {0.8, 0.8, 0.8}, 0), met({1.0, 0.0, -1.0}, 0.5, {0.8, 0.6, 0.2}, 0),
         met({0, 0, -1}, 0.5, {0.9, 0.9, 0.9}, 0),       lam({-0.5, 0.6, -1.5}, 0.3, {0.9, 0.1, 0.1}),
         met({0.5, 0.6, -1.5}, 0.3, {0.2, 0.9, 0.2}, 0), lam({0, -0.3, -0.6}, 0.15, {0.2, 0.2, 0.9}),
         met({0.3, 0.1, -0.45}, 0.1, {0.95, 0.95, 0.95}, 0), lam({-0.35, -0.35, -0.7}, 0.12, {0.5, 0.9, 0.5}),
         lam({0, 1.2, -2.5}, 0.6, {0.7, 0.7, 0.7}),      lam({1.0, 0.0, -1.0}, 0.25, {0.3, 0.3, 0.3})};
  } else if (n == "walls2") {
    w = {lam({0, -300.5, -1}, 300.0, {0.9, 0.85, 0.8}), lam({0, 300.5, -1}, 300.0, {0.8, 0.9, 0.95})};
  } else if (n == "rtiow5") {  // config 2: RTIOW three spheres + hollow glass
    w = {lam({0, -100.5, -1}, 100.0, {0.8, 0.8, 0.0}), lam({0, 0, -1}, 0.5, {0.1, 0.2, 0.5}),
         die({-1, 0, -1}, 0.5, 1.5), die({-1, 0, -1}, -0.4, 1.5),
         met({1, 0, -1}, 0.5, {0.8, 0.6, 0.2}, 0.0)};
    const double f[3] = {-2, 2, 1}, a[3] = {0, 0, -1}, up[3] = {0, 1, 0};
    yk_camera_look(&cam, f, a, up, 20.0, 16.0 / 9.0, 0.0, 1.0);
  } else if (n == "final" || n == "glass") {  // configs 3/4 and 5
    w = random_scene(seed, n == "glass");
    const double f[3] = {13, 2, 3}, a[3] = {0, 0, 0}, up[3] = {0, 1, 0};
    yk_camera_look(&cam, f, a, up, 20.0, 16.0 / 9.0, 0.1, 10.0);
  } else {
    return YK_ERR_INVALID;
  }
  if (count) *count = (uint32_t)w.size();
  if (camera) *camera = cam;
  if (spheres) {
    if (capacity < w.size()) return YK_ERR_INVALID;
    std::memcpy(spheres, w.data(), w.size() * sizeof(yk_sphere));
  }
  return YK_OK;
}

// The launch schedule of a render call (yk_schedule.hpp), for the CPU tests: not part of the C-ABI
// (include/ykgpu.h does not declare it).  A call of spp samples per pixel from s_begin over nps
// processing slots on a persistent grid of `lanes` threads, synced or in flight; kmax: the launch
// buffers' samples per pixel (0: the ideal, no memory pressure).  sizes[3] receives kideal, ksynced,
// kfloor; s0[i], take[i] the launches (the first `cap` of them).  Returns the number of launches.
uint32_t yk_schedule_plan(uint32_t nps, uint32_t spp, uint32_t s_begin, uint64_t lanes, int inflight, uint32_t kmax,
                          uint32_t* sizes, uint32_t* s0, uint32_t* take, uint32_t cap) {
  if (!nps || !spp) return 0;
  const yksched::LaunchSizes z = yksched::launch_sizes(nps, spp, lanes);
  if (sizes) sizes[0] = z.kideal, sizes[1] = z.ksynced, sizes[2] = z.kfloor;
  std::vector<std::pair<uint32_t, uint32_t>> sched;
  yksched::launch_schedule(sched, spp, s_begin, kmax ? kmax : z.kideal, z.ksynced, inflight != 0);
  for (uint32_t i = 0; i < sched.size() && i < cap; ++i) {
    if (s0) s0[i] = sched[i].first;
    if (take) take[i] = sched[i].second;
  }
  return (uint32_t)sched.size();
}

// The band and exchange plan of a group film's filter (yk_group_plan.hpp), for the CPU tests: not
// part of the C-ABI.  bands (may be null) receives k records of 4 words (begin, count, lo, hi),
// copies (may be null) the first `cap` records of 6 words (source entry, first source row, rows,
// destination entry, first destination row, destination pitch in rows).  Returns the number of copies.
uint32_t yk_group_film_plan(uint32_t rows, uint32_t k, uint32_t halo, uint32_t* bands, uint32_t* copies, uint32_t cap) {
  std::vector<ykplan::Band> b;
  std::vector<ykplan::Copy> c;
  ykplan::group_film_plan(rows, k, halo, b, c);
  for (uint32_t e = 0; bands && e < b.size(); ++e)
    bands[4 * e] = b[e].begin, bands[4 * e + 1] = b[e].count, bands[4 * e + 2] = b[e].lo, bands[4 * e + 3] = b[e].hi;
  for (uint32_t i = 0; copies && i < c.size() && i < cap; ++i) {
    uint32_t* o = copies + 6 * i;
    o[0] = c[i].src, o[1] = c[i].src_row, o[2] = c[i].rows, o[3] = c[i].dst, o[4] = c[i].dst_row, o[5] = c[i].dst_pitch;
  }
  return (uint32_t)c.size();
}

}  // extern "C"

// ---- the start of a camera sample (include/ykgpu.h "radiance queries") --------------------
namespace {
// a sample's engine on the host, counting its words: mt19937 (scene_rng is one) or yk::xor128
// (random.hpp:18-41: x, y, z at their defaults, w = 88675123 ^ seed)
struct sample_rng {
  scene_rng mt;
  uint32_t xs[4];
  bool x128;
  uint32_t words = 0;
  sample_rng(uint32_t seed, bool xor128) : mt(xor128 ? 0u : seed), xs{123456789u, 362436069u, 521288629u, 88675123u ^ seed}, x128(xor128) {}
  uint32_t next() {
    ++words;
    if (!x128) return mt.next();
    const uint32_t t = xs[0] ^ (xs[0] << 11);
    xs[0] = xs[1], xs[1] = xs[2], xs[2] = xs[3];
    return xs[3] = (xs[3] ^ (xs[3] >> 19)) ^ (t ^ (t >> 8));
  }
  // generate_canonical<double, 53> (random.hpp:161-183) and uniform_real_distribution (:273-278)
  double canonical() {
    double s = (double)next();
    s = s + (double)next() * 4294967296.0;
    const double r = s / 18446744073709551616.0;
    return r >= 1.0 ? 1.0 - 0x1p-53 : r;
  }
  double uniform(double a, double b) { return (canonical() * (b - a)) + a; }
};
d3 operator+(d3 a, d3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
d3 of(const double* p) { return {p[0], p[1], p[2]}; }
}  // namespace

extern "C" int yk_camera_sample_ray(const yk_camera* cam, const yk_render_params* p, uint32_t y, uint32_t x, uint32_t s,
                                    yk_path_ray* out) {
  if (!cam || !p || !out) return YK_ERR_INVALID;
  if (y >= p->image_height || x >= p->image_width || s >= p->samples_per_pixel) return YK_ERR_INVALID;
  if (p->precision != YK_PRECISION_FP64) return YK_ERR_UNSUPPORTED;
  if (p->rng != YK_RNG_MT19937 && p->rng != YK_RNG_XOR128) return YK_ERR_UNSUPPORTED;
  if (p->seed_mode != YK_SEED_COUNTER && p->seed_mode != YK_SEED_RANDOM_DEVICE) return YK_ERR_INVALID;
  // the sample's seed: source.cpp:154-158 in uint32 arithmetic, or the call's key hashed with the
  // sample's 64-bit linear index (YK_SEED_RANDOM_DEVICE: splitmix64's finaliser, high word)
  uint32_t seed = p->seed0 + (y * p->image_width + x) * p->samples_per_pixel + s;
  if (p->seed_mode == YK_SEED_RANDOM_DEVICE) {
    uint64_t z = p->seed_key + ((((uint64_t)y * p->image_width + x) * p->samples_per_pixel + s) + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    seed = (uint32_t)(z >> 32);
  }
  sample_rng g(seed, p->rng == YK_RNG_XOR128);
  // jitter (source.cpp:160-164) and camera::get_ray (camera.hpp:29-32), then the thin lens' point by
  // rejection (extension)
  const double u = (x + g.uniform(0, 1)) / p->image_width;
  const double v = (p->image_height - y - 1 + g.uniform(0, 1)) / p->image_height;
  d3 org = of(cam->origin);
  d3 dir = ((of(cam->lower_left_corner) + of(cam->horizontal) * u) + of(cam->vertical) * v) - org;
  if (cam->lens_radius > 0) {
    double px, py;
    for (;;) {
      px = g.uniform(-1, 1);
      py = g.uniform(-1, 1);
      if (px * px + py * py < 1.0) break;
    }
    const double rx = px * cam->lens_radius, ry = py * cam->lens_radius;
    const d3 off = of(cam->lens_u) * rx + of(cam->lens_v) * ry;
    org = org + off;
    dir = dir - off;
  }
  std::memset(out, 0, sizeof(*out));
  put(out->origin, org);
  put(out->direction, dir);
  out->seed = seed;
  out->skip = g.words;
  return YK_OK;
}

// ---- the path rays of a gather point (include/ykgpu.h "gather queries") --------------------
namespace {
// math::sqrt (math.hpp:10-19) as DESIGN.md §3 describes it: x = s/2, then x <- (x + s/x)/2 until
// two iterates are equal.  (The bound only matters for NaN and infinity, where the loop has no end.)
double newton_sqrt(double s) {
  double x = s / 2.0, prev = 0.0;
  for (int guard = 0; x != prev && guard < 4096; ++guard) {
    prev = x;
    x = (x + s / x) / 2.0;
  }
  return x;
}
constexpr uint32_t kGatherMaxSkip = 221;  // the scatter's six words lie inside mt19937's 227 lazy words
}  // namespace

extern "C" int yk_gather_sample_ray(const yk_gather_point* pt, uint32_t rng, uint32_t s, yk_path_ray* out) {
  if (!pt || !out) return YK_ERR_INVALID;
  if (rng != YK_RNG_MT19937 && rng != YK_RNG_XOR128) return YK_ERR_UNSUPPORTED;
  const uint32_t seed = pt->seed + s;
  const d3 n = of(pt->n);
  d3 d{0.0, 0.0, 0.0};
  // (a point past the skip limit or with a zero normal does no arithmetic: a zero direction)
  if (pt->skip <= kGatherMaxSkip && !(n.x == 0.0 && n.y == 0.0 && n.z == 0.0)) {
    sample_rng g(seed, rng == YK_RNG_XOR128);
    for (uint32_t k = 0; k < pt->skip; ++k) (void)g.next();
    // lambertian::scatter (material.hpp:50-59) with random_unit_vector (:33-36)
    d3 ru;
    ru.x = g.uniform(-1, 1);
    ru.y = g.uniform(-1, 1);
    ru.z = g.uniform(-1, 1);
    ru = ru / newton_sqrt(dot(ru, ru));
    d = n + ru;
    if (std::fabs(d.x) < 1e-8 && std::fabs(d.y) < 1e-8) d = n;  // near_zero (vec3.hpp:76-80): x and y only
  }
  std::memset(out, 0, sizeof(*out));
  put(out->origin, of(pt->p));
  put(out->direction, d);
  out->seed = seed;
  out->skip = pt->skip + 6u;
  return YK_OK;
}

// ... for every sample of n_points points -> out[i * n_samples + s]; large batches are split over a
// few host threads
extern "C" int yk_gather_sample_rays(const yk_gather_point* points, uint64_t n_points, uint32_t rng, uint32_t n_samples,
                                     yk_path_ray* out) {
  if (n_points && n_samples && (!points || !out)) return YK_ERR_INVALID;
  if (rng != YK_RNG_MT19937 && rng != YK_RNG_XOR128) return YK_ERR_UNSUPPORTED;
  const uint64_t n = n_points * n_samples;
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t nt = n < 65536 ? 1 : std::min<uint64_t>(16, hw ? hw : 1);
  auto work = [&](uint64_t t) {
    for (uint64_t j = n * t / nt; j < n * (t + 1) / nt; ++j)
      (void)yk_gather_sample_ray(&points[j / n_samples], rng, (uint32_t)(j % n_samples), &out[j]);
  };
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (std::thread& t : th) t.join();
  return YK_OK;
}

// ---- scene files -------------------------------------------------------------------------
// Text, one record per line, numbers as %.17g (every double round-trips exactly):
//   yk-scene 1
//   camera <origin 3> <lower_left_corner 3> <horizontal 3> <vertical 3> <lens_u 3> <lens_v 3> <lens_radius>
//   sphere <lambertian|metal|dielectric> <cx cy cz> <radius> <albedo r g b> <fuzz> <ior>
// '#' starts a comment line.  The spheres keep file order = tuple order (it defines rec.id).
namespace {
const char* kind_name(uint32_t k) {
  return k == YK_MATERIAL_LAMBERTIAN ? "lambertian" : k == YK_MATERIAL_METAL ? "metal" : "dielectric";
}
}  // namespace

int yk_scene_write(const char* path, const yk_sphere* spheres, uint32_t count, const yk_camera* camera) {
  if (!path || !camera || (count && !spheres)) return YK_ERR_INVALID;
  FILE* f = std::fopen(path, "w");
  if (!f) return YK_ERR_INVALID;
  std::fprintf(f, "yk-scene 1\n# %u spheres; tuple order\ncamera", count);
  const double* cv[6] = {camera->origin, camera->lower_left_corner, camera->horizontal,
                         camera->vertical, camera->lens_u, camera->lens_v};
  for (const double* v : cv) std::fprintf(f, " %.17g %.17g %.17g", v[0], v[1], v[2]);
  std::fprintf(f, " %.17g\n", camera->lens_radius);
  for (uint32_t i = 0; i < count; ++i) {
    const yk_sphere& s = spheres[i];
    std::fprintf(f, "sphere %s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", kind_name(s.material),
                 s.center[0], s.center[1], s.center[2], s.radius, s.albedo[0], s.albedo[1], s.albedo[2],
                 s.fuzz, s.ior);
  }
  const bool ok = std::ferror(f) == 0;
  return (std::fclose(f) == 0 && ok) ? YK_OK : YK_ERR_INVALID;
}

int yk_scene_read(const char* path, yk_sphere* spheres, uint32_t capacity, uint32_t* count, yk_camera* camera) {
  if (!path) return YK_ERR_INVALID;
  FILE* f = std::fopen(path, "r");
  if (!f) return YK_ERR_INVALID;
  std::vector<yk_sphere> w;
  yk_camera cam{};
  bool have_header = false, have_camera = false, bad = false;
  char line[1024];
  while (!bad && std::fgets(line, sizeof line, f)) {
    char word[32] = {0};
    if (line[0] == '#' || std::sscanf(line, "%31s", word) != 1) continue;
    const std::string wd = word;
    if (wd == "yk-scene") {
      int v = 0;
      bad = std::sscanf(line, "%*s %d", &v) != 1 || v != 1;
      have_header = true;
    } else if (wd == "camera") {
      double* cv[6] = {cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical, cam.lens_u, cam.lens_v};
      const char* p = line + 6;
      int used = 0;
      for (double* v : cv)
        for (int k = 0; k < 3 && !bad; ++k) {
          bad = std::sscanf(p, "%lf%n", &v[k], &used) != 1;
          p += used;
        }
      bad = bad || std::sscanf(p, "%lf", &cam.lens_radius) != 1;
      have_camera = true;
    } else if (wd == "sphere") {
      yk_sphere s;
      std::memset(&s, 0, sizeof s);
      char kind[32] = {0};
      bad = std::sscanf(line, "%*s %31s %lf %lf %lf %lf %lf %lf %lf %lf %lf", kind, &s.center[0], &s.center[1],
                        &s.center[2], &s.radius, &s.albedo[0], &s.albedo[1], &s.albedo[2], &s.fuzz, &s.ior) != 10;
      const std::string k = kind;
      if (k == "lambertian") s.material = YK_MATERIAL_LAMBERTIAN;
      else if (k == "metal") s.material = YK_MATERIAL_METAL;
      else if (k == "dielectric") s.material = YK_MATERIAL_DIELECTRIC;
      else bad = true;
      w.push_back(s);
    } else {
      bad = true;
    }
  }
  std::fclose(f);
  if (bad || !have_header || !have_camera) return YK_ERR_INVALID;
  if (count) *count = (uint32_t)w.size();
  if (camera) *camera = cam;
  if (spheres) {
    if (capacity < w.size()) return YK_ERR_INVALID;
    if (!w.empty()) std::memcpy(spheres, w.data(), w.size() * sizeof(yk_sphere));
  }
  return YK_OK;
}


// ---- film files (include/ykgpu.h "progressive film") -----------------------------------------
// Binary, little-endian (the only byte order the library is built for): FilmHeader, the
// yk_render_params record, pixels * 3 sums, pixels * 3 second moments.  The doubles are written
// as they lie in memory, so every bit pattern round-trips.
namespace {
struct FilmHeader {  // 32 bytes
  char magic[8];     // "ykfilm1\0"
  uint32_t params_bytes, done;
  uint64_t pixels, scene_hash;
};
static_assert(sizeof(FilmHeader) == 32, "film header layout");
const char kFilmMagic[8] = {'y', 'k', 'f', 'i', 'l', 'm', '1', '\0'};

uint64_t film_pixels(const yk_render_params* p) {
  return (uint64_t)p->row_count * (p->col_count ? p->col_count : p->image_width);
}

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
  const unsigned char* b = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}
}  // namespace

uint64_t yk_scene_hash(const yk_sphere* spheres, uint32_t count, const yk_camera* camera) {
  uint64_t h = 0xcbf29ce484222325ull;
  h = fnv1a(h, &count, sizeof count);
  for (uint32_t i = 0; spheres && i < count; ++i) {
    const yk_sphere& s = spheres[i];
    h = fnv1a(h, s.center, sizeof s.center);
    h = fnv1a(h, &s.radius, sizeof s.radius);
    h = fnv1a(h, s.albedo, sizeof s.albedo);
    h = fnv1a(h, &s.fuzz, sizeof s.fuzz);
    h = fnv1a(h, &s.ior, sizeof s.ior);
    h = fnv1a(h, &s.material, sizeof s.material);
  }
  if (camera) {
    const double* cv[6] = {camera->origin, camera->lower_left_corner, camera->horizontal,
                           camera->vertical, camera->lens_u, camera->lens_v};
    for (const double* v : cv) h = fnv1a(h, v, 3 * sizeof(double));
    h = fnv1a(h, &camera->lens_radius, sizeof(double));
  }
  return h;
}

int yk_film_save(const char* path, const yk_render_params* params, uint64_t scene_hash, uint32_t done,
                 const double* sums, const double* sumsq) {
  if (!path || !params || !sums || !sumsq) return YK_ERR_INVALID;
  const uint64_t pixels = film_pixels(params);
  if (!pixels || done > params->samples_per_pixel) return YK_ERR_INVALID;
  // written beside the target and renamed over it: an interrupted save leaves the previous
  // checkpoint whole
  const std::string tmp = std::string(path) + ".part";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return YK_ERR_INVALID;
  FilmHeader h;
  std::memcpy(h.magic, kFilmMagic, sizeof h.magic);
  h.params_bytes = (uint32_t)sizeof(yk_render_params);
  h.done = done;
  h.pixels = pixels;
  h.scene_hash = scene_hash;
  const size_t n = (size_t)pixels * 3;
  bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite(params, sizeof *params, 1, f) == 1 &&
            std::fwrite(sums, sizeof(double), n, f) == n && std::fwrite(sumsq, sizeof(double), n, f) == n;
  ok = std::fclose(f) == 0 && ok;
  if (ok) ok = std::rename(tmp.c_str(), path) == 0;
  if (!ok) std::remove(tmp.c_str());
  return ok ? YK_OK : YK_ERR_INVALID;
}

int yk_film_load(const char* path, yk_render_params* params, uint64_t* scene_hash, uint32_t* done,
                 double* sums, double* sumsq, uint64_t capacity_pixels) {
  if (!path) return YK_ERR_INVALID;
  FILE* f = std::fopen(path, "rb");
  if (!f) return YK_ERR_INVALID;
  FilmHeader h;
  yk_render_params p;
  bool ok = std::fread(&h, sizeof h, 1, f) == 1 && std::memcmp(h.magic, kFilmMagic, sizeof h.magic) == 0 &&
            h.params_bytes == sizeof(yk_render_params) && std::fread(&p, sizeof p, 1, f) == 1;
  ok = ok && h.pixels != 0 && h.pixels == film_pixels(&p) && h.pixels < (1ull << 31) &&
       h.done <= p.samples_per_pixel;
  // the whole payload must be there, and nothing after it, whether or not it is read
  if (ok) {
    const long at = std::ftell(f);
    ok = at >= 0 && std::fseek(f, 0, SEEK_END) == 0 &&
         (uint64_t)std::ftell(f) == (uint64_t)at + h.pixels * 6 * sizeof(double) && std::fseek(f, at, SEEK_SET) == 0;
  }
  if (ok && (sums || sumsq)) {
    const size_t n = (size_t)h.pixels * 3;
    ok = capacity_pixels >= h.pixels;
    std::vector<double> skip;
    if (ok && !(sums && sumsq)) skip.resize(n);
    ok = ok && std::fread(sums ? sums : skip.data(), sizeof(double), n, f) == n &&
         std::fread(sumsq ? sumsq : skip.data(), sizeof(double), n, f) == n;
  }
  std::fclose(f);
  if (!ok) return YK_ERR_INVALID;
  if (params) *params = p;
  if (scene_hash) *scene_hash = h.scene_hash;
  if (done) *done = h.done;
  return YK_OK;
}

// ---- film files with per-pixel counts (include/ykgpu.h "adaptive passes") ----------------------
// "ykfilm2\0": the v1 header (its `done` holds the smallest count) and params record, then
// pixels counts (uint32), pixels * 3 sums, pixels * 3 second moments.  yk_film_load keeps to v1.
namespace {
const char kFilmMagic2[8] = {'y', 'k', 'f', 'i', 'l', 'm', '2', '\0'};
}

int yk_film_save_counts(const char* path, const yk_render_params* params, uint64_t scene_hash, const uint32_t* counts,
                        const double* sums, const double* sumsq) {
  if (!path || !params || !counts || !sums || !sumsq) return YK_ERR_INVALID;
  const uint64_t pixels = film_pixels(params);
  if (!pixels) return YK_ERR_INVALID;
  uint32_t lo = counts[0];
  for (uint64_t i = 0; i < pixels; ++i) {
    if (counts[i] > params->samples_per_pixel) return YK_ERR_INVALID;
    lo = counts[i] < lo ? counts[i] : lo;
  }
  const std::string tmp = std::string(path) + ".part";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) return YK_ERR_INVALID;
  FilmHeader h;
  std::memcpy(h.magic, kFilmMagic2, sizeof h.magic);
  h.params_bytes = (uint32_t)sizeof(yk_render_params);
  h.done = lo;
  h.pixels = pixels;
  h.scene_hash = scene_hash;
  const size_t n = (size_t)pixels * 3;
  bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite(params, sizeof *params, 1, f) == 1 &&
            std::fwrite(counts, sizeof(uint32_t), (size_t)pixels, f) == (size_t)pixels &&
            std::fwrite(sums, sizeof(double), n, f) == n && std::fwrite(sumsq, sizeof(double), n, f) == n;
  ok = std::fclose(f) == 0 && ok;
  if (ok) ok = std::rename(tmp.c_str(), path) == 0;
  if (!ok) std::remove(tmp.c_str());
  return ok ? YK_OK : YK_ERR_INVALID;
}

int yk_film_load_counts(const char* path, yk_render_params* params, uint64_t* scene_hash, uint32_t* counts,
                        double* sums, double* sumsq, uint64_t capacity_pixels) {
  if (!path) return YK_ERR_INVALID;
  FILE* f = std::fopen(path, "rb");
  if (!f) return YK_ERR_INVALID;
  FilmHeader h;
  yk_render_params p;
  bool ok = std::fread(&h, sizeof h, 1, f) == 1;
  const bool v2 = ok && std::memcmp(h.magic, kFilmMagic2, sizeof h.magic) == 0;
  ok = ok && (v2 || std::memcmp(h.magic, kFilmMagic, sizeof h.magic) == 0) &&
       h.params_bytes == sizeof(yk_render_params) && std::fread(&p, sizeof p, 1, f) == 1;
  ok = ok && h.pixels != 0 && h.pixels == film_pixels(&p) && h.pixels < (1ull << 31) &&
       h.done <= p.samples_per_pixel;
  // the whole payload must be there, and nothing after it, whether or not it is read
  if (ok) {
    const long at = std::ftell(f);
    const uint64_t payload = h.pixels * 6 * sizeof(double) + (v2 ? h.pixels * sizeof(uint32_t) : 0);
    ok = at >= 0 && std::fseek(f, 0, SEEK_END) == 0 && (uint64_t)std::ftell(f) == (uint64_t)at + payload &&
         std::fseek(f, at, SEEK_SET) == 0;
  }
  if (ok && (counts || sums || sumsq)) ok = capacity_pixels >= h.pixels;
  if (ok) {
    // the counts are always read: one above the target makes the file foreign
    std::vector<uint32_t> cn((size_t)h.pixels, h.done);
    if (v2) ok = std::fread(cn.data(), sizeof(uint32_t), cn.size(), f) == cn.size();
    for (size_t i = 0; ok && i < cn.size(); ++i) ok = cn[i] <= p.samples_per_pixel && cn[i] >= h.done;
    if (ok && counts) std::memcpy(counts, cn.data(), cn.size() * sizeof(uint32_t));
  }
  if (ok && (sums || sumsq)) {
    const size_t n = (size_t)h.pixels * 3;
    std::vector<double> skip;
    if (!(sums && sumsq)) skip.resize(n);
    ok = std::fread(sums ? sums : skip.data(), sizeof(double), n, f) == n &&
         std::fread(sumsq ? sumsq : skip.data(), sizeof(double), n, f) == n;
  }
  std::fclose(f);
  if (!ok) return YK_ERR_INVALID;
  if (params) *params = p;
  if (scene_hash) *scene_hash = h.scene_hash;
  return YK_OK;
}

// The same for n samples (ys[i], xs[i], ss[i]) -> out[i]; large batches are split over a few host
// threads (every record depends on its own sample alone).  The first error of any sample is returned.
extern "C" int yk_camera_sample_rays(const yk_camera* cam, const yk_render_params* p, const uint32_t* ys,
                                     const uint32_t* xs, const uint32_t* ss, uint64_t n, yk_path_ray* out) {
  if (!cam || !p || (n && (!ys || !xs || !ss || !out))) return YK_ERR_INVALID;
  const unsigned hw = std::thread::hardware_concurrency();
  const uint64_t nt = n < 65536 ? 1 : std::min<uint64_t>(16, hw ? hw : 1);
  std::vector<int> rc(nt, YK_OK);
  auto work = [&](uint64_t t) {
    for (uint64_t i = n * t / nt; i < n * (t + 1) / nt && rc[t] == YK_OK; ++i)
      rc[t] = yk_camera_sample_ray(cam, p, ys[i], xs[i], ss[i], &out[i]);
  };
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; ++t) th.emplace_back(work, t);
  work(0);
  for (std::thread& t : th) t.join();
  for (int r : rc)
    if (r != YK_OK) return r;
  return YK_OK;
}
