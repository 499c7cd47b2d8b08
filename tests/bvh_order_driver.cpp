// Host-only driver of tests/test_bvh_slot_order.py: builds the BVH over the spheres of a text file
// ("cx cy cz radius" per line) and prints the binary tree and the wide nodes as JSON, floats as their
// bit patterns.
//   driver <spheres.txt> <max_leaf> <all_axes> <order 0..3> [<ox> <oy> <oz>]
// Without a view origin the wide nodes come from wide_nodes() with its default arguments.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../uecraytracing_amd/csrc/yk_bvh.hpp"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 5 && argc != 8) return 2;
  std::vector<double> c, r;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 3;
  double v[4];
  while (std::fscanf(f, "%lf %lf %lf %lf", &v[0], &v[1], &v[2], &v[3]) == 4) {
    c.insert(c.end(), v, v + 3);
    r.push_back(v[3]);
  }
  std::fclose(f);
  ykbvh::Options opt;
  opt.max_leaf = (uint32_t)std::atoi(argv[2]);
  opt.all_axes = std::atoi(argv[3]) != 0;
  const ykbvh::Built b = ykbvh::build(c.data(), r.data(), (uint32_t)r.size(), 13.0, opt);
  int32_t root = 0;
  uint32_t depth = 0;
  std::vector<ykbvh::WideNode> wide;
  double view[3];
  if (argc == 8) {
    for (int k = 0; k < 3; ++k) view[k] = std::strtod(argv[5 + k], nullptr);
    ykbvh::WideOptions wopt;
    wopt.view = view;
    wopt.order = (ykbvh::SlotOrder)std::atoi(argv[4]);
    wide = ykbvh::wide_nodes(b, &root, &depth, wopt);
  } else {
    wide = ykbvh::wide_nodes(b, &root, &depth);
  }
  std::printf("{\"root\": %d, \"binary_root\": %d, \"wide_depth\": %u, \"span_area\": %.17g, \"order\": [", root, b.root,
              depth, ykbvh::kSpanArea);
  for (size_t i = 0; i < b.order.size(); ++i) std::printf("%s%u", i ? ", " : "", b.order[i]);
  std::printf("],\n\"binary\": [");
  for (size_t i = 0; i < b.nodes.size(); ++i) {
    const ykbvh::Node& n = b.nodes[i];
    std::printf("%s\n[", i ? "," : "");
    for (int k = 0; k < 2; ++k)
      std::printf("[%" PRIu32 ", %" PRIu32 ", %" PRIu32 ", %" PRIu32 ", %" PRIu32 ", %" PRIu32 ", %d]%s", bits(n.lo_x[k]),
                  bits(n.lo_y[k]), bits(n.lo_z[k]), bits(n.hi_x[k]), bits(n.hi_y[k]), bits(n.hi_z[k]), n.child[k],
                  k ? "" : ", ");
    std::printf("]");
  }
  std::printf("],\n\"wide\": [");
  for (size_t i = 0; i < wide.size(); ++i) {
    uint32_t w[sizeof(ykbvh::WideNode) / 4];
    std::memcpy(w, &wide[i], sizeof w);
    std::printf("%s\n[", i ? "," : "");
    for (size_t k = 0; k < sizeof w / 4; ++k) std::printf("%s%" PRIu32, k ? ", " : "", w[k]);
    std::printf("]");
  }
  // the library's own view of every slot: does it span its node, and how far is it from the origin
  std::printf("],\n\"spans\": [");
  for (size_t i = 0; i < wide.size(); ++i)
    std::printf("%s[%d, %d, %d, %d]", i ? ", " : "", (int)ykbvh::slot_spans(wide[i], 0), (int)ykbvh::slot_spans(wide[i], 1),
                (int)ykbvh::slot_spans(wide[i], 2), (int)ykbvh::slot_spans(wide[i], 3));
  std::printf("],\n\"dist2\": [");
  for (size_t i = 0; i < wide.size() && argc == 8; ++i)
    std::printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", ykbvh::slot_dist2(wide[i], 0, view),
                ykbvh::slot_dist2(wide[i], 1, view), ykbvh::slot_dist2(wide[i], 2, view),
                ykbvh::slot_dist2(wide[i], 3, view));
  std::printf("]}\n");
  return 0;
}
