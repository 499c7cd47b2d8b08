// yk_bvh.cpp — binned-SAH BVH builder (host).  See yk_bvh.hpp for the culling contract.  Below it,
// the other culling structure built from the scene and the camera: the sky-block classifier
// (yk_sky.hpp).
#include "yk_bvh.hpp"

#include "yk_sky.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace ykbvh {
namespace {

struct Box {
  double lo[3] = {INFINITY, INFINITY, INFINITY};
  double hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  void grow(const Box& b) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], b.lo[k]);
      hi[k] = std::max(hi[k], b.hi[k]);
    }
  }
  void grow(const double* p) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], p[k]);
      hi[k] = std::max(hi[k], p[k]);
    }
  }
  double area() const {
    if (!(hi[0] >= lo[0])) return 0;
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return 2 * (dx * dy + dy * dz + dz * dx);
  }
};

struct Builder {
  const double* c;
  std::vector<Box> sbox;     // per sphere, grown by delta
  std::vector<double> cent;  // centroids
  std::vector<uint32_t> idx;
  std::vector<Node> nodes;
  bool median_only = false;
  uint32_t max_depth = 0;
  Options opt;

  Box bounds(uint32_t b, uint32_t e) const {
    Box r;
    for (uint32_t i = b; i < e; ++i) r.grow(sbox[idx[i]]);
    return r;
  }

  // returns a child code for the subtree over idx[b, e)
  int32_t rec(uint32_t b, uint32_t e, uint32_t depth) {
    const uint32_t n = e - b;
    if (n <= opt.max_leaf) {
      max_depth = std::max(max_depth, depth);
      return ~int32_t((b << 4) | n);
    }
    Box cb;
    for (uint32_t i = b; i < e; ++i) cb.grow(&cent[3 * idx[i]]);
    int axis = 0;
    for (int k = 1; k < 3; ++k)
      if (cb.hi[k] - cb.lo[k] > cb.hi[axis] - cb.lo[axis]) axis = k;
    uint32_t mid = b + n / 2;
    double ext = cb.hi[axis] - cb.lo[axis];
    if (!median_only && ext > 0) {
      const int kBins = std::min(std::max(opt.bins, 2), 256);
      // binned SAH over the longest centroid axis, or (opt.all_axes) the cheapest of the three
      double best = INFINITY;
      int best_q = -1, best_axis = axis;
      for (int ax = 0; ax < 3; ++ax) {
        if (!opt.all_axes && ax != axis) continue;
        const double ex = cb.hi[ax] - cb.lo[ax];
        if (!(ex > 0)) continue;
        std::vector<Box> bb(kBins);
        std::vector<uint32_t> cnt(kBins, 0);
        for (uint32_t i = b; i < e; ++i) {
          const uint32_t sp = idx[i];
          const int q = std::min(std::max(int((cent[3 * sp + ax] - cb.lo[ax]) / ex * kBins), 0), kBins - 1);
          bb[q].grow(sbox[sp]);
          ++cnt[q];
        }
        for (int q = 1; q < kBins; ++q) {
          Box l, r;
          uint32_t nl = 0, nr = 0;
          for (int t = 0; t < q; ++t) { l.grow(bb[t]); nl += cnt[t]; }
          for (int t = q; t < kBins; ++t) { r.grow(bb[t]); nr += cnt[t]; }
          if (!nl || !nr) continue;
          const double cost = l.area() * nl + r.area() * nr;
          if (cost < best) { best = cost; best_q = q; best_axis = ax; }
        }
      }
      axis = best_axis;
      ext = cb.hi[axis] - cb.lo[axis];
      auto bin_of = [&](uint32_t sp) {
        int q = int((cent[3 * sp + axis] - cb.lo[axis]) / ext * kBins);
        return std::min(std::max(q, 0), kBins - 1);
      };
      if (best_q > 0) {
        auto it = std::partition(idx.begin() + b, idx.begin() + e,
                                 [&](uint32_t sp) { return bin_of(sp) < best_q; });
        mid = uint32_t(it - idx.begin());
      }
    }
    if (mid == b || mid == e || median_only || ext == 0) {
      mid = b + n / 2;
      std::nth_element(idx.begin() + b, idx.begin() + mid, idx.begin() + e,
                       [&](uint32_t x, uint32_t y) { return cent[3 * x + axis] < cent[3 * y + axis]; });
    }
    const int32_t me = int32_t(nodes.size());
    nodes.emplace_back();
    const int32_t l = rec(b, mid, depth + 1);
    const int32_t r = rec(mid, e, depth + 1);
    const Box bl = bounds(b, mid), br = bounds(mid, e);
    Node& nd = nodes[me];
    const Box* kids[2] = {&bl, &br};
    for (int k = 0; k < 2; ++k) {
      // outward rounding to float: nextafter past the double bound
      auto dn = [](double v) { float f = (float)v; return (double)f > v ? std::nextafter(f, -INFINITY) : f; };
      auto up = [](double v) { float f = (float)v; return (double)f < v ? std::nextafter(f, INFINITY) : f; };
      nd.lo_x[k] = dn(kids[k]->lo[0]);
      nd.lo_y[k] = dn(kids[k]->lo[1]);
      nd.lo_z[k] = dn(kids[k]->lo[2]);
      nd.hi_x[k] = up(kids[k]->hi[0]);
      nd.hi_y[k] = up(kids[k]->hi[1]);
      nd.hi_z[k] = up(kids[k]->hi[2]);
    }
    nd.child[0] = l;
    nd.child[1] = r;
    nd.pad[0] = nd.pad[1] = 0;
    return me;
  }
};

}  // namespace

Built build(const double* centers, const double* radii, uint32_t n, double camera_extent,
            const Options& opt) {
  Built out;
  double ext = camera_extent;
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) ext = std::max(ext, std::fabs(centers[3 * i + k]) + std::fabs(radii[i]));
  // origins of secondary rays lie on sphere surfaces (|o| <= ext); allow 4x headroom
  out.origin_bound = 4.0 * ext;
  out.delta = (float)std::ldexp(out.origin_bound, -21);
  for (int attempt = 0; attempt < 2; ++attempt) {
    Builder bd;
    bd.c = centers;
    bd.median_only = attempt == 1;
    bd.opt = opt;
    bd.sbox.resize(n);
    bd.cent.assign(centers, centers + 3 * size_t(n));
    bd.idx.resize(n);
    std::iota(bd.idx.begin(), bd.idx.end(), 0u);
    for (uint32_t i = 0; i < n; ++i) {
      const double ar = std::fabs(radii[i]);
      double g = ar * opt.radius_grow;
      if (opt.f32_big) {
        const double* c = centers + 3 * i;
        const double reach = std::sqrt(3.0) * out.origin_bound + std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + ar;
        if (kF32BigReach * ar >= reach * (1.0 + 0x1p-20)) g = std::min(g, ar * kF32BigGrow);
      }
      const double r = ar + g + out.delta;
      for (int k = 0; k < 3; ++k) {
        bd.sbox[i].lo[k] = centers[3 * i + k] - r;
        bd.sbox[i].hi[k] = centers[3 * i + k] + r;
      }
    }
    out.root = bd.rec(0, n, 0);
    out.depth = bd.max_depth;
    if (out.depth <= kMaxDepth || attempt == 1) {
      out.nodes = std::move(bd.nodes);
      out.order = std::move(bd.idx);
      break;
    }
  }
  return out;
}


namespace {
struct Slot {
  float lo[3], hi[3];
  int32_t code;  // binary-tree code: >= 0 inner node index, < 0 leaf
};

float slot_area(const Slot& e) {
  const float dx = e.hi[0] - e.lo[0], dy = e.hi[1] - e.lo[1], dz = e.hi[2] - e.lo[2];
  return dx * dy + dy * dz + dz * dx;
}

Slot child_slot(const Node& n, int k) {
  return Slot{{n.lo_x[k], n.lo_y[k], n.lo_z[k]}, {n.hi_x[k], n.hi_y[k], n.hi_z[k]}, n.child[k]};
}

double box_area(const float* lo, const float* hi) {
  const double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
  return dx * dy + dy * dz + dz * dx;
}

double box_dist2(const float* lo, const float* hi, const double* p) {
  double d2 = 0;
  for (int a = 0; a < 3; ++a) {
    const double d = p[a] < lo[a] ? lo[a] - p[a] : (p[a] > hi[a] ? p[a] - hi[a] : 0.0);
    d2 += d * d;
  }
  return d2;
}

bool box_spans(const float* lo, const float* hi, const float* node_lo, const float* node_hi) {
  return box_area(lo, hi) >= kSpanArea * box_area(node_lo, node_hi);
}

struct Collapser {
  const Built& b;
  const WideOptions& opt;
  std::vector<WideNode>& out;
  std::vector<uint32_t> leaves;  // leaves under each binary node (opt.expand 1, 2)
  uint32_t max_depth = 0;

  uint32_t count_leaves(int32_t code) {
    if (code < 0) return 1;
    if (leaves.empty()) leaves.assign(b.nodes.size(), 0);
    if (leaves[code]) return leaves[code];
    return leaves[code] = count_leaves(b.nodes[code].child[0]) + count_leaves(b.nodes[code].child[1]);
  }
  double score(const Slot& e) {
    const double a = slot_area(e);
    if (opt.expand == 0) return a;
    const double nl = count_leaves(e.code);
    return opt.expand == 1 ? a * nl : a * std::sqrt(nl);
  }

  // The used slots in visit order reversed (see SlotOrder): a stable sort, so equal keys keep the
  // binary tree's order.
  void order_slots(std::vector<Slot>& slots) const {
    if (!opt.view || opt.order == SlotOrder::kTree) return;
    float nlo[3] = {3e38f, 3e38f, 3e38f}, nhi[3] = {-3e38f, -3e38f, -3e38f};
    for (const Slot& e : slots)
      for (int a = 0; a < 3; ++a) {
        nlo[a] = std::min(nlo[a], e.lo[a]);
        nhi[a] = std::max(nhi[a], e.hi[a]);
      }
    struct Key {
      int low;  // 1: moved to the lowest indices
      double d2;
      Slot slot;
    };
    auto before = [](const Key& x, const Key& y) { return x.low != y.low ? x.low > y.low : x.d2 > y.d2; };
    Key keys[4];  // an insertion sort (stable) of at most 4 keys: no allocation per node
    size_t n = 0;
    for (const Slot& e : slots) {
      const bool leaf = e.code < 0;
      const bool low = opt.order == SlotOrder::kNearLeavesLow
                           ? leaf
                           : (opt.order == SlotOrder::kNearSpanLow && leaf && box_spans(e.lo, e.hi, nlo, nhi));
      const Key key{low ? 1 : 0, box_dist2(e.lo, e.hi, opt.view), e};
      size_t at = n++;
      for (; at > 0 && before(key, keys[at - 1]); --at) keys[at] = keys[at - 1];
      keys[at] = key;
    }
    for (size_t k = 0; k < n; ++k) slots[k] = keys[k].slot;
  }

  // Emits the wide node for binary inner node `idx` (and its subtree) into out; returns its index.
  uint32_t collapse(int32_t idx, uint32_t depth) {
    std::vector<Slot> slots = {child_slot(b.nodes[idx], 0), child_slot(b.nodes[idx], 1)};
    while (slots.size() < 4) {
      int best = -1;
      for (size_t i = 0; i < slots.size(); ++i)
        if (slots[i].code >= 0 && (best < 0 || score(slots[i]) > score(slots[best]))) best = (int)i;
      if (best < 0) break;
      const Node& c = b.nodes[slots[best].code];
      slots[best] = child_slot(c, 0);
      slots.insert(slots.begin() + best + 1, child_slot(c, 1));  // siblings stay adjacent
    }
    order_slots(slots);
    max_depth = std::max(max_depth, depth + 1);
    const uint32_t me = (uint32_t)out.size();
    out.emplace_back();
    int32_t codes[4];
    for (int k = 0; k < 4; ++k) {
      if (k >= (int)slots.size()) {
        codes[k] = kEmptyLeaf;
      } else if (slots[k].code >= 0) {
        codes[k] = (int32_t)(collapse(slots[k].code, depth + 1) * sizeof(WideNode));
      } else {
        codes[k] = slots[k].code;
      }
    }
    WideNode& w = out[me];
    float* ax[3] = {w.x, w.y, w.z};
    for (int k = 0; k < 4; ++k) {
      const bool used = k < (int)slots.size();
      for (int a = 0; a < 3; ++a) {
        const float lo = used ? slots[k].lo[a] : 3e38f, hi = used ? slots[k].hi[a] : -3e38f;
        ax[a][k] = lo;
        ax[a][4 + k] = hi;
        ax[a][8 + k] = lo;
      }
      w.child[k] = codes[k];
    }
    return me;
  }
};

void slot_box(const WideNode& w, int k, float* lo, float* hi) {
  const float* ax[3] = {w.x, w.y, w.z};
  for (int a = 0; a < 3; ++a) {
    lo[a] = ax[a][k];
    hi[a] = ax[a][4 + k];
  }
}
}  // namespace

bool slot_spans(const WideNode& w, int k) {
  float nlo[3] = {3e38f, 3e38f, 3e38f}, nhi[3] = {-3e38f, -3e38f, -3e38f}, lo[3], hi[3];
  for (int j = 0; j < 4; ++j) {
    slot_box(w, j, lo, hi);
    if (!(lo[0] <= hi[0])) continue;  // unused
    for (int a = 0; a < 3; ++a) {
      nlo[a] = std::min(nlo[a], lo[a]);
      nhi[a] = std::max(nhi[a], hi[a]);
    }
  }
  slot_box(w, k, lo, hi);
  return lo[0] <= hi[0] && box_spans(lo, hi, nlo, nhi);
}

double slot_dist2(const WideNode& w, int k, const double* p) {
  float lo[3], hi[3];
  slot_box(w, k, lo, hi);
  return box_dist2(lo, hi, p);
}

std::vector<WideNode> wide_nodes(const Built& b, int32_t* root_code, uint32_t* wide_depth,
                                 const WideOptions& wopt) {
  std::vector<WideNode> out;
  uint32_t depth = 0;
  if (b.root >= 0) {
    Collapser c{b, wopt, out, {}, 0};
    c.collapse(b.root, 0);
    depth = c.max_depth;
    *root_code = 0;
  } else {
    *root_code = b.root;  // a single leaf
  }
  *wide_depth = depth;
  return out;
}

}  // namespace ykbvh

// =========================================================================================
// The sky-block classifier (yk_sky.hpp has the ray family, the bound and what is never flagged)
// =========================================================================================
namespace yksky {
namespace {

struct V {
  double x, y, z;
};
inline V vsub(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V vadd(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V vmul(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline double vdot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V vcross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double vlen(V a) { return std::sqrt(vdot(a, a)); }
inline V v3(const double* p) { return {p[0], p[1], p[2]}; }

// The margins.  kRel widens the block's rectangle (in u, v: 1e-9 of the image, against roundings of
// 1e-16) and every length the bound is made of; the camera's arithmetic moves a ray point by a few
// ulps of the camera's own magnitudes times (1 + t), and the reference's discriminant
// hb^2 - a c, evaluated in double, can accept a ray that misses the sphere by up to about
// 4 eps |oc|^2 / |r|: both are covered a thousandfold and more (cam_scale, kDisc).
constexpr double kRel = 1e-9;
constexpr double kDisc = 0x1p-40;  // >= 4096 eps

// The plane set of a rectangle of the focus plane: unit inward normals of the four sides, the unit
// axis, and f_min; ok == false: nothing may be excluded with it
struct Pyramid {
  V n[5];
  double fmin = 0;
  double cone = 0;  // every direction of the family is within this angle of the axis n[4]
  V corner[4];      // the rectangle's own corner directions F - O
  bool ok = false;
};

struct Cam {
  V o, llc, hor, ver;
  double L = 0;      // bound of the lens offset's length
  double scale = 0;  // |O| + |llc| + |hor| + |ver|: what the camera's roundings are relative to
};

Cam make_cam(const yk_camera& c) {
  Cam k;
  k.o = v3(c.origin), k.llc = v3(c.lower_left_corner), k.hor = v3(c.horizontal), k.ver = v3(c.vertical);
  if (c.lens_radius > 0) {  // (the kernels' own test for "has a lens")
    const V lu = v3(c.lens_u), lv = v3(c.lens_v);
    k.L = c.lens_radius * std::sqrt(vdot(lu, lu) + vdot(lv, lv)) * (1 + kRel);
  }
  k.scale = vlen(k.o) + vlen(k.llc) + vlen(k.hor) + vlen(k.ver);
  return k;
}

// the four corner directions F - O of the rectangle [u0, u1] x [v0, v1] of the focus plane
void corners(const Cam& c, double u0, double u1, double v0, double v1, V (&e)[4]) {
  const double us[4] = {u0, u1, u1, u0}, vs[4] = {v0, v0, v1, v1};
  for (int k = 0; k < 4; ++k) e[k] = vsub(vadd(vadd(c.llc, vmul(c.hor, us[k])), vmul(c.ver, vs[k])), c.o);
}

Pyramid make_pyramid(const Cam& c, double u0, double u1, double v0, double v1) {
  Pyramid p;
  // the block's own corner directions (the rectangle widened against the roundings of u and v)
  V in[4];
  corners(c, u0 - kRel / 2, u1 + kRel / 2, v0 - kRel / 2, v1 + kRel / 2, in);
  const double need = c.L * (1 + kRel);
  // the axis: every focus point in front of the camera by more than the lens is wide
  V w = vadd(vadd(in[0], in[1]), vadd(in[2], in[3]));
  const double wl = vlen(w);
  if (!(wl > 0) || !std::isfinite(wl)) return p;
  w = vmul(w, 1.0 / wl);
  double fmin = INFINITY;
  for (int k = 0; k < 4; ++k) fmin = std::min(fmin, vdot(w, in[k]));
  if (!(fmin * (1 - kRel) > need) || !std::isfinite(fmin)) return p;
  // the cone of the directions: the corners' angles from the axis bound the rectangle's (a
  // circular cone is convex), and the lens turns a direction F - O by at most asin(L / |F - O|)
  double cmin = 1.0;
  for (int k = 0; k < 4; ++k) cmin = std::min(cmin, vdot(w, in[k]) / vlen(in[k]));
  p.cone = std::acos(std::max(-1.0, std::min(1.0, cmin))) + std::asin(need / (fmin * (1 - kRel))) + kRel;
  if (!std::isfinite(p.cone)) return p;
  // the sides: planes through O and the edges of the rectangle widened by g L in the focus plane,
  // g raised until every one of the block's own corners is `need` inside every plane (the
  // condition itself is what the bound rests on; the widening is only a way to meet it, and the
  // least g that does excludes the most: a plane's tilt is about L / |F - O| over the pinhole's)
  const double hl = vlen(c.hor), vl = vlen(c.ver);
  for (double g = 1.0 + 0x1p-20; g <= 32.0; g *= (need > 0 ? 1.0625 : 64.0)) {
    const double du = kRel + g * c.L / hl, dv = kRel + g * c.L / vl;
    if (!std::isfinite(du) || !std::isfinite(dv)) return p;
    V e[4];
    corners(c, u0 - du, u1 + du, v0 - dv, v1 + dv, e);
    bool good = true;
    for (int k = 0; k < 4 && good; ++k) {
      V n = vcross(e[k], e[(k + 1) & 3]);
      const double len = vlen(n);
      if (!(len > 0) || !std::isfinite(len)) return p;
      n = vmul(n, 1.0 / len);
      if (vdot(n, w) < 0) n = vmul(n, -1.0);  // inward
      for (int j = 0; j < 4 && good; ++j) good = vdot(n, in[j]) >= need && vdot(n, in[j]) > 0;
      p.n[k] = n;
    }
    if (!good) continue;
    p.n[4] = w;
    p.fmin = fmin * (1 - kRel);
    for (int k = 0; k < 4; ++k) p.corner[k] = in[k];
    p.ok = true;
    return p;
  }
  return p;
}

// true: no ray of the pyramid's family can hit the sphere (C, r)
bool excluded(const Cam& c, const Pyramid& p, V C, double r) {
  if (!p.ok) return false;
  const V oc = vsub(C, c.o);
  const double D = vlen(oc), ar = std::fabs(r);
  const double reach = D + ar + c.L;
  const double tmax = reach / (p.fmin - c.L);  // (only the roundings grow with t)
  const double rho = (ar + c.L) * (1 + kRel) + kRel * (reach + (1 + tmax) * c.scale) + kDisc * reach * reach / ar;
  if (!(rho >= 0) || !std::isfinite(rho)) return false;
  for (int k = 0; k < 5; ++k)
    if (vdot(p.n[k], oc) < -rho) return true;
  // the cone test (what the planes miss beside a sphere that is large on the screen): from a lens
  // point A the sphere, grown to rho - L for the roundings, lies within asin((rho - L) / |C - A|)
  // of C - A, |C - A| >= D - L, and C - A within asin(L / D) of C - O; a direction farther from
  // C - O than both and the cone's own angle together cannot hit
  if (D - c.L > rho - c.L && D > c.L) {
    const double theta = std::acos(std::max(-1.0, std::min(1.0, vdot(p.n[4], oc) / D)));
    const double need = p.cone + std::asin(c.L / D) + std::asin((rho - c.L) / (D - c.L)) + kRel;
    if (theta > need) return true;
  }
  return false;
}

// true: the pinhole ray through every point of the pyramid's rectangle hits the sphere (C, r) in
// front of the camera, so no block inside the rectangle is a sky block (the lens point 0 belongs to
// every family).  The directions from O that hit a sphere form a convex cone, so the four corners
// decide; 1e-6 keeps the test clear of its own roundings.  Only saves work: such blocks would fail
// `excluded` one by one.
bool covered(const Cam& c, const Pyramid& p, V C, double r) {
  if (!p.ok) return false;
  const V oc = vsub(C, c.o);
  const double tan2 = vdot(oc, oc) - r * r;  // (distance to the tangent points)^2
  if (!(tan2 > 0)) return false;
  for (int k = 0; k < 4; ++k) {
    const double a = vdot(p.corner[k], oc);
    if (!(a > 0) || !(a * a > tan2 * vdot(p.corner[k], p.corner[k]) * (1 + 1e-6))) return false;
  }
  return true;
}

// image row of tile row t, image column of tile column j (yk_render_params' banded sets)
inline uint64_t banded(uint32_t begin, uint32_t stride, uint32_t L, uint32_t t) {
  return (uint64_t)begin + ((((uint64_t)(t >> L)) * stride) << L) + (t & ((1u << L) - 1u));
}

}  // namespace

std::vector<uint8_t> sky_blocks(const yk_camera& cam, const double* centers, const double* radii, uint32_t n,
                                const Tile& t, uint32_t tw, uint32_t th) {
  const uint32_t bx = (t.col_count + tw - 1) / tw, by = (t.row_count + th - 1) / th;
  std::vector<uint8_t> flag((size_t)bx * by, 0);
  if (!bx || !by || !t.W || !t.H) return flag;
  const Cam c = make_cam(cam);
  const double W = (double)t.W, H = (double)t.H;
  // the pyramid of tile columns [j0, j1) x tile rows [r0, r1): both maps increase, so the first
  // and last entries bound the pixels' rectangle in the image
  auto pyramid = [&](uint32_t j0, uint32_t j1, uint32_t r0, uint32_t r1) {
    const double x0 = (double)banded(t.col_begin, t.col_stride, t.col_band_log2, j0);
    const double x1 = (double)banded(t.col_begin, t.col_stride, t.col_band_log2, j1 - 1);
    const double y0 = (double)banded(t.row_begin, t.row_stride, t.row_band_log2, r0);
    const double y1 = (double)banded(t.row_begin, t.row_stride, t.row_band_log2, r1 - 1);
    return make_pyramid(c, x0 / W, (x1 + 1) / W, (H - 1 - y1) / H, (H - y0) / H);
  };
  constexpr uint32_t kSuper = 8;
  std::vector<uint32_t> left;
  for (uint32_t sj = 0; sj < by; sj += kSuper)
    for (uint32_t si = 0; si < bx; si += kSuper) {
      const uint32_t ei = std::min(bx, si + kSuper), ej = std::min(by, sj + kSuper);
      const Pyramid sp = pyramid(si * tw, std::min(t.col_count, ei * tw), sj * th, std::min(t.row_count, ej * th));
      left.clear();
      bool hidden = false;  // some sphere fills the whole super-block: its blocks stay unflagged
      for (uint32_t s = 0; s < n && !hidden; ++s) {
        if (excluded(c, sp, v3(centers + 3 * (size_t)s), radii[s])) continue;
        left.push_back(s);
        hidden = covered(c, sp, v3(centers + 3 * (size_t)s), radii[s]);
      }
      if (hidden) continue;
      for (uint32_t j = sj; j < ej; ++j)
        for (uint32_t i = si; i < ei; ++i) {
          bool sky = sp.ok;  // (an undecidable super-block: every sphere is in `left`)
          if (!left.empty()) {
            const Pyramid bp =
                pyramid(i * tw, std::min(t.col_count, (i + 1) * tw), j * th, std::min(t.row_count, (j + 1) * th));
            sky = bp.ok;
            for (size_t k = 0; sky && k < left.size(); ++k)
              sky = excluded(c, bp, v3(centers + 3 * (size_t)left[k]), radii[left[k]]);
          }
          flag[(size_t)j * bx + i] = sky ? 1 : 0;
        }
    }
  return flag;
}

}  // namespace yksky
