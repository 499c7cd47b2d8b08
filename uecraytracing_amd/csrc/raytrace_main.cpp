// raytrace_main.cpp — the repository's `raytrace` program: the reference's main()
// (/root/reference/source.cpp:190-231) with render() (source.cpp:98-178) served by the GPU
// through include/ykgpu.h, plus the runtime render parameters BASELINE configs 2-5 need.
//
// This is NOT the reference's binary: its option parser and PNG writer are this file's own (the
// reference's are cxxopts and stb_image_write, which this repository does not vendor).  The
// reference's exact program — its cxxopts CLI, its stb PNG bytes — is the reference's own
// source.cpp with oracle/source_cpp_ykgpu.patch applied (tests/test_cli.py
// checks that build's PNG byte for byte against the reference's constexpr build).
//
// Kept from the reference: -h/--help, -v/--verbose, -o/--output, -l/--verbose-level and the
// positional output (source.cpp:197-216: help or no output → usage + exit 0; the last -l wins),
// the messages "rendering...", "rendering finished", "write to file : <f>", "success" / "error"
// with exit 1 (source.cpp:114,174-175,223-230), the default image (YK_IMAGE_WIDTH 400, YK_SPP 100,
// YK_MAX_DEPTH 50; source.cpp:43-53) and the reference scene (source.cpp:103-112), built with the
// same yk calls.  A bad argument is reported with a message and exit status 2 (the reference
// lets cxxopts' exception escape main and aborts).
//
// Added (render parameters are compile-time macros in the reference): --width, --spp,
// --depth, --scene, --scene-seed, --scene-file, --save-scene, --seed0, --precision, --rng,
// --device, --devices (a device list as the bridge's YKGPU_DEVICES takes it: the rows dealt over a
// group, films as group films, include/ykgpu.h "group films"), --stats, --pick, --probe and --gather (one ray query / one pixel's radiance queries /
// one gather at a pixel's first hit instead of a render), the progressive film's --progressive, --until, --checkpoint, --stop-after
// (include/ykgpu.h "progressive film": the image in chunks of samples, the same bytes as in one
// call), and --denoise with --denoise-radius, --denoise-patch, --denoise-k2 (include/ykgpu.h "film
// denoise": the final image and every preview through the film's variance-guided filter),
// --denoise-features, --feature-grid and --aov (include/ykgpu.h "film features": the filter guided
// by first-hit albedo, normal and depth, and those three as images).  --seed0 fixes the per-sample seed base (seed0 + (y*W+x)*spp + s, the constexpr
// build's formula, source.cpp:154-158); without it every sample gets its own seed from a
// per-call std::random_device key (YK_SEED_RANDOM_DEVICE), like the reference's runtime build
// (source.cpp:159).  --precision fp32 renders render<float> (T = float, source.cpp:98);
// --rng xor128 seeds the reference's yk::xor128 (random.hpp:18-41) per sample instead of
// yk::mt19937.
// Verbose output: the reference's per-pixel / per-sample lines (levels 1-2) and, at level 3, every
// ray ray_color is called with (raytracer.hpp:21-25, from ykgpu_render_trace), in the
// reference's order, after the GPU render.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <random>
#include <string>
#include <vector>

#include "png_write.hpp"
#include "yk/scene.hpp"
#include "yk/ykgpu_bridge.hpp"

#ifndef YK_IMAGE_WIDTH
#define YK_IMAGE_WIDTH 400
#endif
#ifndef YK_SPP
#define YK_SPP 100
#endif
#ifndef YK_MAX_DEPTH
#define YK_MAX_DEPTH 50
#endif

namespace {

struct option_error {
  std::string what;
};

const char* kHelp =
    "raytracing program\n"
    "Usage:\n"
    "  raytrace [OPTION...] positional parameters\n"
    "\n"
    "  -h, --help                print usage\n"
    "  -v, --verbose             verbose output\n"
    "  -o, --output arg          filename of output\n"
    "  -l, --verbose-level arg   set verbose level\n"
    "      --width arg           image width (default: " "400" ")\n"
    "      --spp arg             samples per pixel (default: 100)\n"
    "      --depth arg           max bounce depth (default: 50)\n"
    "      --scene arg           ref4|lambert3|mixed12|walls2|rtiow5|final|glass (default: ref4)\n"
    "      --scene-seed arg      generator seed of final/glass (default: 42)\n"
    "      --scene-file arg      load the scene from a yk-scene file (overrides --scene)\n"
    "      --save-scene arg      write the scene to a yk-scene file\n"
    "      --seed0 arg           per-sample seed base (default: random_device)\n"
    "      --precision arg       fp64|fp32: the T of render<T> (default: fp64)\n"
    "      --rng arg             mt19937|xor128: the per-sample engine (default: mt19937)\n"
    "      --device arg          GPU index (default: 0)\n"
    "      --devices arg         a device list instead: 0,1,2,3 or all (repeats allowed: 0,0,0 runs\n"
    "                            three contexts on device 0); the image's rows are dealt over the\n"
    "                            list, and every film option runs through a group film (the same\n"
    "                            bytes as on one device)\n"
    "      --stats               print kernel time and throughput\n"
    "      --progressive arg     render in chunks of arg samples per pixel, rewriting the image\n"
    "                            after each chunk (the same image as in one call)\n"
    "      --until arg           stop once no pixel's standard error exceeds arg; prints the\n"
    "                            samples used (chunks of --progressive, default 16)\n"
    "      --adaptive            with --until: every chunk samples only the pixels still over the\n"
    "                            bound; prints the samples used per pixel\n"
    "      --checkpoint arg      save the film to this file after every chunk; resume from it\n"
    "                            when it exists (same parameters and scene, else an error)\n"
    "      --stop-after arg      render at most arg chunks in this run (resume with --checkpoint)\n"
    "      --denoise             write the variance-guided non-local-means filter of the film's\n"
    "                            mean (the final image and every --progressive preview) instead\n"
    "                            of the raw mean; needs at least 2 samples per pixel\n"
    "      --denoise-radius arg  the filter's window radius, 0..10 (default: 5)\n"
    "      --denoise-patch arg   the filter's patch radius, 0..3 (default: 1)\n"
    "      --denoise-k2 arg      the filter's variance scale, > 0 (default: 0.5)\n"
    "      --denoise-features    --denoise with the filter's weight bounded by first-hit albedo,\n"
    "                            normal and depth (pinhole rays: sharp where a lens defocuses),\n"
    "                            at the pair of defaults tuned together (k2 2, grid 2); the\n"
    "                            --denoise-* options still set the colour side\n"
    "      --feature-grid arg    sub-rays per pixel side of the feature pass, 1..4 (default: 2)\n"
    "      --feature-samples arg the features of --denoise-features and --aov from the first hits of\n"
    "                            the render's own first arg samples, 1..256 and at most --spp (lens\n"
    "                            and jitter included: defocused where the image is) instead of\n"
    "                            pinhole sub-rays; --feature-grid is then unused\n"
    "      --aov arg             also write the feature means F as arg.albedo.png, arg.normal.png\n"
    "                            and arg.depth.png: trunc(clamp(x, 0, 0.999) * 256) of F0..F2, of\n"
    "                            0.5 * F + 0.5 for F3..F5, and of F6 / (1 + F6) (grey: r = g = b)\n"
    "      --matte arg           arg = a comma list of sphere ids and/or 'sky': after the render, the\n"
    "                            antialiased coverage of those ids, from the first hits of each\n"
    "                            pixel's own samples (lens and jitter included), written to\n"
    "                            --matte-out as grey trunc(clamp(cov, 0, 0.999) * 256); prints\n"
    "                            'matte: pixels <n> uncertain <n> samples <n> of <n>'\n"
    "      --matte-out arg       the matte's PNG file (needs --matte, and --matte needs it)\n"
    "      --matte-samples arg   the matte from the first arg samples of every pixel, at most --spp,\n"
    "                            instead of the samples each pixel got (default: 0, those)\n"
    "      --pick arg            arg = X,Y: cast the pixel-centre pinhole ray of image pixel (X, Y)\n"
    "                            (column, row from the top) at the render's t_min, print\n"
    "                            'pick X Y: id <n> t <t> p (<x>, <y>, <z>) normal (<x>, <y>, <z>)\n"
    "                            front <0|1>' (%.17g) or 'pick X Y: miss', and exit without\n"
    "                            rendering (no output file needed)\n"
    "      --probe arg           arg = X,Y: run the --spp samples of image pixel (X, Y) one by one\n"
    "                            through the radiance query instead of rendering; per sample\n"
    "                            'sample <s>: colour (<r>, <g>, <b>) words <n> segments <n> end <how>'\n"
    "                            (%.17g; how: sky|absorbed|depth|out-of-domain), then 'sum (...)',\n"
    "                            the samples added in order, and 'rgb <r> <g> <b>', the pixel of the\n"
    "                            image (fp64 only, needs --seed0; no output file needed)\n"
    "      --gather arg          arg = X,Y: cast the pixel-centre pinhole ray of --pick and run one\n"
    "                            gather query at the hit's p and normal: --spp lambertian scatters\n"
    "                            from seed --seed0, each followed to --depth; prints\n"
    "                            'gather X Y: id <n> samples <N> sum (<r>, <g>, <b>) mean (<r>, <g>,\n"
    "                            <b>) open <k>' (%.17g) or 'gather X Y: miss' (fp64 only, needs\n"
    "                            --seed0; no output file needed)\n";

struct args {
  bool help = false, verbose_flag = false, stats = false;
  std::vector<uint32_t> levels;
  std::string output;
  bool have_output = false;
  uint32_t width = YK_IMAGE_WIDTH, spp = YK_SPP, depth = YK_MAX_DEPTH, scene_seed = 42;
  int device = 0;
  bool have_device = false;
  std::string devices;  // --devices: the list as given (parsed once the library is there)
  bool have_devices = false;
  bool have_seed0 = false;
  uint32_t seed0 = 0;
  std::string precision = "fp64";
  std::string rng = "mt19937";
  std::string scene = "ref4";
  std::string scene_file, save_scene;
  // the progressive film
  bool have_progressive = false, have_until = false, have_stop_after = false;
  uint32_t progressive = 0, stop_after = 0;
  double until = 0;
  std::string checkpoint;
  bool adaptive = false;
  // the film's denoise filter (the options other than --denoise only set its parameters)
  bool denoise = false, have_denoise_params = false;
  yk_denoise_params dn{};
  // the guided filter and the feature images (--feature-grid alone sets the grid of either)
  bool denoise_features = false, have_feature_grid = false;
  uint32_t feature_samples = 0;  // --feature-samples: != 0, the sampled feature pass at that n
  yk_feature_params fp{};
  std::string aov;
  // --matte IDS --matte-out FILE [--matte-samples N]: the ids' coverage after the render
  std::vector<uint32_t> matte_ids;
  std::string matte_out;
  bool have_matte = false, have_matte_out = false, have_matte_samples = false;
  uint32_t matte_samples = 0;
  // --pick X,Y: one ray query instead of a render
  bool have_pick = false;
  uint32_t pick_x = 0, pick_y = 0;
  // --probe X,Y: the pixel's samples through the radiance query instead of a render
  bool have_probe = false;
  uint32_t probe_x = 0, probe_y = 0;
  // --gather X,Y: one gather query at the pixel's first hit instead of a render
  bool have_gather = false;
  uint32_t gather_x = 0, gather_y = 0;
  bool film() const { return denoise || !aov.empty() || have_matte || adaptive || have_progressive || have_until || have_stop_after || !checkpoint.empty(); }
};

uint32_t to_u32(const std::string& opt, const std::string& v) {
  char* end = nullptr;
  const unsigned long long x = std::strtoull(v.c_str(), &end, 10);
  if (v.empty() || *end || x > 0xffffffffull || v[0] == '-')
    throw option_error{"Argument '" + v + "' failed to parse (option " + opt + ")"};
  return (uint32_t)x;
}

double to_error_bound(const std::string& opt, const std::string& v) {
  char* end = nullptr;
  const double x = std::strtod(v.c_str(), &end);
  if (v.empty() || *end || !(x >= 0) || !std::isfinite(x))
    throw option_error{"Argument '" + v + "' failed to parse (option " + opt + ")"};
  return x;
}

double to_positive(const std::string& opt, const std::string& v) {
  const double x = to_error_bound(opt, v);
  if (!(x > 0)) throw option_error{"Argument '" + v + "' must be greater than 0 (option " + opt + ")"};
  return x;
}

uint32_t to_count(const std::string& opt, const std::string& v) {
  const uint32_t x = to_u32(opt, v);
  if (!x) throw option_error{"Argument '" + v + "' must be at least 1 (option " + opt + ")"};
  return x;
}

args parse(int argc, char** argv) {
  args a;
  yk_denoise_defaults(&a.dn);
  yk_guided_defaults(nullptr, &a.fp);
  bool have_k2 = false;
  int positional = 0;
  auto value = [&](int& i, const std::string& name, const std::string& inl) -> std::string {
    if (!inl.empty()) return inl;
    if (i + 1 >= argc) throw option_error{"Option '" + name + "' is missing an argument"};
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    std::string inl;
    if (s.rfind("--", 0) == 0 && s.size() > 2) {
      const size_t eq = s.find('=');
      if (eq != std::string::npos) {
        inl = s.substr(eq + 1);
        s = s.substr(0, eq);
      }
      const std::string n = s.substr(2);
      if (n == "help") a.help = true;
      else if (n == "verbose") a.verbose_flag = true;
      else if (n == "stats") a.stats = true;
      else if (n == "output") { a.output = value(i, n, inl); a.have_output = true; }
      else if (n == "verbose-level") {
        std::string v = value(i, n, inl);
        for (size_t p = 0; p <= v.size();) {  // cxxopts vector values: comma separated
          const size_t q = v.find(',', p);
          a.levels.push_back(to_u32(n, v.substr(p, q == std::string::npos ? std::string::npos : q - p)));
          if (q == std::string::npos) break;
          p = q + 1;
        }
      } else if (n == "width") a.width = to_u32(n, value(i, n, inl));
      else if (n == "spp") a.spp = to_u32(n, value(i, n, inl));
      else if (n == "depth") a.depth = to_u32(n, value(i, n, inl));
      else if (n == "scene-seed") a.scene_seed = to_u32(n, value(i, n, inl));
      else if (n == "device") { a.device = (int)to_u32(n, value(i, n, inl)); a.have_device = true; }
      else if (n == "devices") {
        a.devices = value(i, n, inl);
        a.have_devices = true;
        if (a.devices.empty()) throw option_error{"Option 'devices' needs a device list"};
      }
      else if (n == "scene") a.scene = value(i, n, inl);
      else if (n == "scene-file") a.scene_file = value(i, n, inl);
      else if (n == "save-scene") a.save_scene = value(i, n, inl);
      else if (n == "seed0") { a.seed0 = to_u32(n, value(i, n, inl)); a.have_seed0 = true; }
      else if (n == "precision") a.precision = value(i, n, inl);
      else if (n == "rng") a.rng = value(i, n, inl);
      else if (n == "progressive") { a.progressive = to_count(n, value(i, n, inl)); a.have_progressive = true; }
      else if (n == "until") { a.until = to_error_bound(n, value(i, n, inl)); a.have_until = true; }
      else if (n == "stop-after") { a.stop_after = to_count(n, value(i, n, inl)); a.have_stop_after = true; }
      else if (n == "adaptive") { a.adaptive = true; }
      else if (n == "denoise") { a.denoise = true; }
      else if (n == "denoise-radius") { a.dn.radius = to_u32(n, value(i, n, inl)); a.have_denoise_params = true; }
      else if (n == "denoise-patch") { a.dn.patch = to_u32(n, value(i, n, inl)); a.have_denoise_params = true; }
      else if (n == "denoise-k2") { a.dn.k2 = to_positive(n, value(i, n, inl)); a.have_denoise_params = true; have_k2 = true; }
      else if (n == "denoise-features") { a.denoise = a.denoise_features = true; }
      else if (n == "feature-grid") { a.fp.grid = to_u32(n, value(i, n, inl)); a.have_feature_grid = true; }
      else if (n == "feature-samples") {
        a.feature_samples = to_u32(n, value(i, n, inl));
        if (a.feature_samples < 1 || a.feature_samples > 256) throw option_error{"Option 'feature-samples' must be 1..256"};
      }
      else if (n == "aov") {
        a.aov = value(i, n, inl);
        if (a.aov.empty()) throw option_error{"Option 'aov' needs a file name prefix"};
      }
      else if (n == "matte") {
        const std::string v = value(i, n, inl);
        for (size_t p = 0; p <= v.size();) {
          const size_t q = v.find(',', p);
          const std::string id = v.substr(p, q == std::string::npos ? std::string::npos : q - p);
          a.matte_ids.push_back(id == "sky" ? (uint32_t)YK_MATTE_SKY : to_u32(n, id));
          if (q == std::string::npos) break;
          p = q + 1;
        }
        a.have_matte = true;
      }
      else if (n == "matte-out") {
        a.matte_out = value(i, n, inl);
        a.have_matte_out = true;
        if (a.matte_out.empty()) throw option_error{"Option 'matte-out' needs a file name"};
      }
      else if (n == "matte-samples") { a.matte_samples = to_u32(n, value(i, n, inl)); a.have_matte_samples = true; }
      else if (n == "pick") {
        const std::string v = value(i, n, inl);
        const size_t c = v.find(',');
        if (c == std::string::npos) throw option_error{"Option 'pick' needs X,Y"};
        a.pick_x = to_u32(n, v.substr(0, c));
        a.pick_y = to_u32(n, v.substr(c + 1));
        a.have_pick = true;
      }
      else if (n == "probe") {
        const std::string v = value(i, n, inl);
        const size_t c = v.find(',');
        if (c == std::string::npos) throw option_error{"Option 'probe' needs X,Y"};
        a.probe_x = to_u32(n, v.substr(0, c));
        a.probe_y = to_u32(n, v.substr(c + 1));
        a.have_probe = true;
      }
      else if (n == "gather") {
        const std::string v = value(i, n, inl);
        const size_t c = v.find(',');
        if (c == std::string::npos) throw option_error{"Option 'gather' needs X,Y"};
        a.gather_x = to_u32(n, v.substr(0, c));
        a.gather_y = to_u32(n, v.substr(c + 1));
        a.have_gather = true;
      }
      else if (n == "checkpoint") {
        a.checkpoint = value(i, n, inl);
        if (a.checkpoint.empty()) throw option_error{"Option 'checkpoint' needs a file name"};
      }
      else throw option_error{"Option '" + n + "' does not exist"};
    } else if (s.size() > 1 && s[0] == '-') {
      for (size_t k = 1; k < s.size(); ++k) {
        const char c = s[k];
        const std::string rest = s.substr(k + 1);
        if (c == 'h') a.help = true;
        else if (c == 'v') a.verbose_flag = true;
        else if (c == 'o') { a.output = value(i, "o", rest); a.have_output = true; break; }
        else if (c == 'l') { a.levels.push_back(to_u32("l", value(i, "l", rest))); break; }
        else throw option_error{std::string("Option '") + c + "' does not exist"};
      }
    } else {
      // one positional argument, the output file (source.cpp:206)
      if (positional++ == 0) {
        a.output = s;
        a.have_output = true;
      } else {
        throw option_error{"unexpected second positional argument '" + s + "'"};
      }
    }
  }
  if (a.have_device && a.have_devices) throw option_error{"Options 'device' and 'devices' exclude each other"};
  if (a.adaptive && !a.have_until) throw option_error{"Option 'adaptive' needs --until"};
  if (a.have_probe && a.have_pick) throw option_error{"Options 'probe' and 'pick' exclude each other"};
  if (a.have_probe && !a.have_seed0) throw option_error{"Option 'probe' needs --seed0 (the samples it repeats)"};
  if (a.have_probe && a.precision != "fp64") throw option_error{"Option 'probe' is fp64 only"};
  if (a.have_probe && !a.spp) throw option_error{"Option 'probe' needs --spp of at least 1"};
  if (a.have_gather && a.have_pick) throw option_error{"Options 'gather' and 'pick' exclude each other"};
  if (a.have_gather && a.have_probe) throw option_error{"Options 'gather' and 'probe' exclude each other"};
  if (a.have_gather && !a.have_seed0) throw option_error{"Option 'gather' needs --seed0 (the samples it draws)"};
  if (a.have_gather && a.precision != "fp64") throw option_error{"Option 'gather' is fp64 only"};
  if (a.have_gather && !a.spp) throw option_error{"Option 'gather' needs --spp of at least 1"};
  if (a.have_matte != a.have_matte_out) throw option_error{"Options 'matte' and 'matte-out' need each other"};
  if (a.have_matte_samples && !a.have_matte) throw option_error{"Option 'matte-samples' needs --matte"};
  if (a.matte_samples > a.spp) throw option_error{"Option 'matte-samples' must be at most --spp"};
  if (a.have_matte && (a.have_pick || a.have_probe || a.have_gather))
    throw option_error{"Option 'matte' needs a render: not with --pick, --probe or --gather"};
  if (a.have_denoise_params && !a.denoise) throw option_error{"The denoise parameters need --denoise"};
  if (a.have_feature_grid && !a.denoise_features && a.aov.empty())
    throw option_error{"Option 'feature-grid' needs --denoise-features or --aov"};
  if (a.fp.grid < 1 || a.fp.grid > 4) throw option_error{"Option 'feature-grid' must be 1..4"};
  if (a.feature_samples && !a.denoise_features && a.aov.empty())
    throw option_error{"Option 'feature-samples' needs --denoise-features or --aov"};
  if (a.feature_samples > a.spp) throw option_error{"Option 'feature-samples' must be at most --spp"};
  if (a.denoise_features) {  // the pair of the pass in use; the colour side unless the option set it
    yk_denoise_params pair;
    if (a.feature_samples)
      yk_guided_sampled_defaults(&pair, &a.fp, nullptr);
    else
      yk_guided_defaults(&pair, nullptr);
    if (!have_k2) a.dn.k2 = pair.k2;
  }
  if (a.dn.radius > 10) throw option_error{"Option 'denoise-radius' must be at most 10"};
  if (a.dn.patch > 3) throw option_error{"Option 'denoise-patch' must be at most 3"};
  return a;
}

}  // namespace

int main(int argc, char* argv[]) {
  std::ios::sync_with_stdio(false);
  std::cout.tie(nullptr);

  args a;
  try {
    a = parse(argc, argv);
  } catch (const option_error& e) {
    std::cerr << "raytrace: " << e.what << " (see --help)" << std::endl;
    return 2;
  }
  if (a.help || (!a.have_output && !a.have_pick && !a.have_probe && !a.have_gather)) {
    std::cout << kHelp << std::endl;
    std::exit(EXIT_SUCCESS);
  }
  uint32_t verbose = 0;
  if (a.verbose_flag && !verbose) ++verbose;
  if (!a.levels.empty()) verbose = a.levels.back();

  const uint32_t W = a.width, H = yk_image_height_for(W);
  if (a.have_pick && (a.pick_x >= W || a.pick_y >= H)) {
    std::cerr << "raytrace: Option 'pick' names a pixel outside the " << W << " x " << H << " image (see --help)"
              << std::endl;
    return 2;
  }
  if (a.have_probe && (a.probe_x >= W || a.probe_y >= H)) {
    std::cerr << "raytrace: Option 'probe' names a pixel outside the " << W << " x " << H << " image (see --help)"
              << std::endl;
    return 2;
  }
  if (a.have_gather && (a.gather_x >= W || a.gather_y >= H)) {
    std::cerr << "raytrace: Option 'gather' names a pixel outside the " << W << " x " << H << " image (see --help)"
              << std::endl;
    return 2;
  }
  const uint32_t seed0 = a.have_seed0 ? a.seed0 : 0u;
  ykgpu::render_options ro;
  ro.seed_mode = a.have_seed0 ? YK_SEED_COUNTER : YK_SEED_RANDOM_DEVICE;
  if (a.precision == "fp32") {
    ro.precision = YK_PRECISION_FP32;
  } else if (a.precision != "fp64") {
    std::cerr << "unknown precision " << a.precision << " (fp64|fp32)" << std::endl;
    return EXIT_FAILURE;
  }
  if (a.rng == "xor128") {
    ro.rng = YK_RNG_XOR128;
  } else if (a.rng != "mt19937") {
    std::cerr << "unknown rng " << a.rng << " (mt19937|xor128)" << std::endl;
    return EXIT_FAILURE;
  }
  std::vector<uint8_t> image;
  try {
    // one context, or with --devices a group (a list of one device is one context)
    ykgpu::renderer gpu(a.have_devices ? ykgpu::devices_from_list(a.devices, "--devices") : std::vector<int>{a.device});
    if (!a.scene_file.empty()) {
      uint32_t n = 0;
      yk_camera cam;
      if (yk_scene_read(a.scene_file.c_str(), nullptr, 0, &n, &cam) != YK_OK) {
        std::cerr << "cannot read scene file " << a.scene_file << std::endl;
        return EXIT_FAILURE;
      }
      std::vector<yk_sphere> s(n);
      yk_scene_read(a.scene_file.c_str(), s.data(), n, &n, nullptr);
      gpu.set_records(s, cam);
      if (!a.save_scene.empty()) yk_scene_write(a.save_scene.c_str(), s.data(), n, &cam);
    } else if (a.scene == "ref4") {
      // the reference's world, built with the reference's calls (source.cpp:100-112)
      using T = double;
      using yk::lambertian, yk::metal, yk::pos3, yk::sphere, yk::world_tag;
      const yk::camera<T> cam = {};
      const auto world =
          yk::hittable_list<T>{}
              .add(sphere(pos3<T, world_tag>(0, 0, -1), 0.5, lambertian<double>({0.7, 0.3, 0.3})))
              .add(sphere(pos3<T, world_tag>(0, -100.5, -1), 100.0, lambertian<double>({0.8, 0.8, 0.0})))
              .add(sphere(pos3<T, world_tag>(-1.0, 0.0, -1.0), 0.5, metal<double>({0.8, 0.8, 0.8})))
              .add(sphere(pos3<T, world_tag>(1.0, 0.0, -1.0), 0.5, metal<double>({0.8, 0.6, 0.2})));
      gpu.set_scene(world, cam);
      if (!a.save_scene.empty()) {
        const std::vector<yk_sphere> s = ykgpu::flatten(world);
        const yk_camera c = ykgpu::camera_record(cam);
        yk_scene_write(a.save_scene.c_str(), s.data(), (uint32_t)s.size(), &c);
      }
    } else {
      uint32_t n = 0;
      yk_camera cam;
      if (yk_scene_build(a.scene.c_str(), a.scene_seed, nullptr, 0, &n, &cam) != YK_OK) {
        std::cerr << "unknown scene " << a.scene << std::endl;
        return EXIT_FAILURE;
      }
      std::vector<yk_sphere> s(n);
      yk_scene_build(a.scene.c_str(), a.scene_seed, s.data(), n, &n, nullptr);
      gpu.set_records(s, cam);
      if (!a.save_scene.empty()) yk_scene_write(a.save_scene.c_str(), s.data(), n, &cam);
    }
    if (a.have_pick || a.have_gather) {
      // the feature pass's sub-ray with a = b = 0.5 (include/ykgpu.h "film features"), every step one
      // IEEE double operation, through the bridge's hit()
      const uint32_t px = a.have_pick ? a.pick_x : a.gather_x, py = a.have_pick ? a.pick_y : a.gather_y;
      const yk_camera& c = gpu.camera();
      const double u = ((double)px + 0.5) / (double)W;
      const double v = ((double)(H - py - 1) + 0.5) / (double)H;
      yk::ray<double> r{};
      r.origin = {c.origin[0], c.origin[1], c.origin[2]};
      r.direction = {((c.lower_left_corner[0] + c.horizontal[0] * u) + c.vertical[0] * v) - c.origin[0],
                     ((c.lower_left_corner[1] + c.horizontal[1] * u) + c.vertical[1] * v) - c.origin[1],
                     ((c.lower_left_corner[2] + c.horizontal[2] * u) + c.vertical[2] * v) - c.origin[2]};
      const auto rec = gpu.hit(std::vector<yk::ray<double>>{r}, ro.t_min, (double)INFINITY)[0];
      if (a.have_gather) {
        // one gather at the hit's (p, normal): N = --spp, seed = --seed0, skip = 0 (include/ykgpu.h
        // "gather queries")
        if (!rec) {
          std::printf("gather %u %u: miss\n", px, py);
          return EXIT_SUCCESS;
        }
        yk_gather_point pt{};
        pt.p[0] = rec->p.x, pt.p[1] = rec->p.y, pt.p[2] = rec->p.z;
        pt.n[0] = rec->normal.x, pt.n[1] = rec->normal.y, pt.n[2] = rec->normal.z;
        pt.seed = seed0;
        const yk_gather g = gpu.gather(std::vector<yk_gather_point>{pt}, a.spp, a.depth, ro)[0];
        std::printf("gather %u %u: id %zu samples %u sum (%.17g, %.17g, %.17g) mean (%.17g, %.17g, %.17g) open %u\n", px,
                    py, rec->id, g.samples, g.sum[0], g.sum[1], g.sum[2], g.sum[0] / (double)g.samples,
                    g.sum[1] / (double)g.samples, g.sum[2] / (double)g.samples, g.open);
        return EXIT_SUCCESS;
      }
      if (!rec) {
        std::printf("pick %u %u: miss\n", a.pick_x, a.pick_y);
      } else {
        std::printf("pick %u %u: id %zu t %.17g p (%.17g, %.17g, %.17g) normal (%.17g, %.17g, %.17g) front %d\n",
                    a.pick_x, a.pick_y, rec->id, rec->t, rec->p.x, rec->p.y, rec->p.z, rec->normal.x, rec->normal.y,
                    rec->normal.z, rec->front_face ? 1 : 0);
      }
      return EXIT_SUCCESS;
    }
    if (a.have_probe) {
      // every sample of the pixel as render() starts it (yk_camera_sample_ray), through ray_color
      const yk_render_params p = ykgpu::renderer::params(W, H, a.spp, a.depth, seed0, ro);
      std::vector<yk_path_ray> rays(a.spp);
      for (uint32_t s = 0; s < a.spp; ++s)
        if (yk_camera_sample_ray(&gpu.camera(), &p, a.probe_y, a.probe_x, s, &rays[s]) != YK_OK)
          throw ykgpu::error(YK_ERR_INVALID, "yk_camera_sample_ray");
      const std::vector<yk_radiance> recs = gpu.radiance(rays, a.depth, ro);
      double sum[3] = {0.0, 0.0, 0.0};
      for (uint32_t s = 0; s < a.spp; ++s) {
        const yk_radiance& r = recs[s];
        const char* how = (r.flags & YK_RAD_SKY) ? "sky" : (r.flags & YK_RAD_ABSORBED) ? "absorbed"
                          : (r.flags & YK_RAD_DEPTH) ? "depth" : "out-of-domain";
        std::printf("sample %u: colour (%.17g, %.17g, %.17g) words %u segments %u end %s\n", s, r.colour[0], r.colour[1],
                    r.colour[2], r.words, r.segments, how);
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + r.colour[c];  // transform_reduce's order (source.cpp:137-167)
      }
      // to_color3b (source.cpp:73-83): math::sqrt (math.hpp:10-19) of the mean, clamped, times 256
      uint32_t rgb[3];
      for (int c = 0; c < 3; ++c) {
        const double m = sum[c] / a.spp;
        double x = m / 2.0, prev = 0.0;
        for (int guard = 0; x != prev && guard < 4096; ++guard) {
          prev = x;
          x = (x + m / x) / 2.0;
        }
        x = (x < 0.0) ? 0.0 : (0.999 < x) ? 0.999 : x;
        rgb[c] = (uint8_t)(x * 256);
      }
      std::printf("sum (%.17g, %.17g, %.17g)\nrgb %u %u %u\n", sum[0], sum[1], sum[2], rgb[0], rgb[1], rgb[2]);
      return EXIT_SUCCESS;
    }
    std::cout << "rendering..." << std::endl;
    yk_render_stats st{};
    if (!a.film()) {
      image = gpu.render(W, H, a.spp, a.depth, seed0, ro);
      st = gpu.stats();
    } else {
      // The progressive film: the image in chunks of samples.  Sample s of the film is sample s of
      // the one-shot render, so every way through here ends in the bytes the branch above renders.
      if (!a.spp) throw ykgpu::error(YK_ERR_INVALID, "--spp must be at least 1");
      yk_render_params p = ykgpu::renderer::params(W, H, a.spp, a.depth, seed0, ro);
      const uint64_t scene = gpu.scene_hash();
      bool resume = false;
      if (!a.checkpoint.empty()) {
        yk_render_params fp;
        if (FILE* f = std::fopen(a.checkpoint.c_str(), "rb")) {
          std::fclose(f);
          resume = true;
          // a run seeded from random_device continues with the key its checkpoint holds
          if (yk_film_load_counts(a.checkpoint.c_str(), &fp, nullptr, nullptr, nullptr, nullptr, 0) == YK_OK &&
              p.seed_mode == YK_SEED_RANDOM_DEVICE && fp.seed_mode == YK_SEED_RANDOM_DEVICE)
            p.seed_key = fp.seed_key;
        }
      }
      // a film on the one context, a group film on a device list: the same bytes either way
      const std::unique_ptr<ykgpu::any_film> film_owner = gpu.film(p);
      ykgpu::any_film& film = *film_owner;
      if (resume) {
        try {
          film.load(a.checkpoint, scene);
        } catch (const ykgpu::error& e) {
          std::cerr << "raytrace: cannot resume: " << e.what() << std::endl;
          return EXIT_FAILURE;
        }
      }
      const uint32_t chunk = a.have_progressive ? a.progressive : a.have_until ? 16u : a.spp;
      const double threshold2 = a.until * a.until;
      auto converged = [&]() { return a.have_until && film.done() >= 2 && film.error_stats(threshold2).pixels_over == 0; };
      // the picture of the film's state: its mean, or with --denoise the filtered mean (a preview
      // of a film that still has a pixel below two samples stays the raw mean; the final image
      // does not: the filter's error is the run's)
      auto picture = [&](bool preview) {
        if (!a.denoise || (preview && film.count_range().first < 2)) return film.resolve();
        if (a.denoise_features && a.feature_samples) return film.denoise_guided_sampled(a.dn, a.fp, a.feature_samples);
        return a.denoise_features ? film.denoise_guided(a.dn, a.fp) : film.denoise(a.dn);
      };
      uint32_t chunks = 0;
      if (a.adaptive) {
        // every chunk is an adaptive pass at the bound: the first, on a fresh film, is uniform, the
        // later ones sample only the pixels still over it; the pass that selects nothing ends the run
        bool stop = false;
        while (!stop && !(a.have_stop_after && chunks >= a.stop_after)) {
          stop = film.accumulate_adaptive(threshold2, chunk).pixels_selected == 0;
          if (stop) break;
          ++chunks;
          const yk_render_stats cs = gpu.stats();
          st.kernel_ms += cs.kernel_ms;
          st.samples += cs.samples;
          if (!a.checkpoint.empty()) film.save(a.checkpoint, scene);
          ykpng::write_rgb(a.output.c_str(), W, H, picture(true).data());
        }
        const auto range = film.count_range();
        if (range.second == 0) throw ykgpu::error(YK_ERR_INVALID, "nothing rendered");
        uint64_t total = 0;
        for (uint32_t c : film.counts()) total += c;
        image = picture(false);
        std::cout << "samples used : " << range.first << ".." << range.second << " per pixel, " << total << " in all"
                  << std::endl;
        if (!stop) std::cout << "stopped after " << chunks << " passes" << std::endl;
      } else {
        bool stop = converged();
        while (!stop && film.done() < a.spp && !(a.have_stop_after && chunks >= a.stop_after)) {
          film.accumulate(std::min(chunk, a.spp - film.done()));
          ++chunks;
          const yk_render_stats cs = gpu.stats();
          st.kernel_ms += cs.kernel_ms;
          st.samples += cs.samples;
          st.seed_key = cs.seed_key;
          if (!a.checkpoint.empty()) film.save(a.checkpoint, scene);
          stop = converged();
          // the image so far, for whoever watches the file (the last chunk's is written below)
          if (!stop && film.done() < a.spp) ykpng::write_rgb(a.output.c_str(), W, H, picture(true).data());
        }
        if (film.done() == 0) throw ykgpu::error(YK_ERR_INVALID, "nothing rendered");
        image = picture(false);
        if (a.have_until) std::cout << "samples used : " << film.done() << std::endl;
        if (film.done() < a.spp && !stop)
          std::cout << "stopped at " << film.done() << " of " << a.spp << " samples" << std::endl;
      }
      st.seed_key = film.params().seed_key;
      if (!a.aov.empty()) {
        // the feature means as images (include/ykgpu.h "film features"): one operation per step
        const std::vector<double> F = a.feature_samples ? film.features_sampled(a.feature_samples) : film.features(a.fp.grid);
        const auto enc = [](double x) {
          x = (x < 0.0) ? 0.0 : (0.999 < x) ? 0.999 : x;
          return (uint8_t)(uint32_t)(x * 256);
        };
        std::vector<uint8_t> albedo((size_t)W * H * 3), normal(albedo.size()), depth(albedo.size());
        for (size_t px = 0; px < (size_t)W * H; ++px) {
          const double* f = &F[px * 7];
          for (int c = 0; c < 3; ++c) {
            albedo[px * 3 + c] = enc(f[c]);
            normal[px * 3 + c] = enc(0.5 * f[3 + c] + 0.5);
            depth[px * 3 + c] = enc(f[6] / (1.0 + f[6]));
          }
        }
        for (const auto& [name, img] : {std::pair<const char*, const std::vector<uint8_t>*>{"albedo", &albedo},
                                        {"normal", &normal}, {"depth", &depth}}) {
          const std::string path = a.aov + "." + name + ".png";
          if (!ykpng::write_rgb(path.c_str(), W, H, img->data())) throw ykgpu::error(YK_ERR_INVALID, "cannot write " + path);
        }
      }
      if (a.have_matte) {
        // the ids' coverage (include/ykgpu.h "film mattes") from the samples each pixel got, or from
        // every pixel's first --matte-samples; grey as the depth image is: r = g = b
        const yk_matte_stats ms = film.mattes(a.matte_samples);
        yk_matte_coverage_stats cs{};
        const std::vector<uint8_t> grey = film.matte_coverage(a.matte_ids, &cs);
        std::vector<uint8_t> rgb((size_t)W * H * 3);
        for (size_t px = 0; px < (size_t)W * H; ++px) rgb[px * 3] = rgb[px * 3 + 1] = rgb[px * 3 + 2] = grey[px];
        if (!ykpng::write_rgb(a.matte_out.c_str(), W, H, rgb.data()))
          throw ykgpu::error(YK_ERR_INVALID, "cannot write " + a.matte_out);
        std::cout << "matte: pixels " << cs.pixels_selected << " uncertain " << cs.pixels_uncertain << " samples "
                  << cs.samples_selected << " of " << ms.samples << std::endl;
      }
    }
    if (verbose) {
      ykgpu::render_options vo = ro;
      vo.seed_key = st.seed_key;  // level 3 traces the same samples the image summed
      gpu.print_verbose(std::cout, W, H, a.spp, a.depth, seed0, verbose, vo);
    }
    std::cout << "rendering finished" << std::endl;
    if (a.stats) {
      std::cerr << "kernels " << st.kernel_ms << " ms, " << (double)st.samples / st.kernel_ms / 1e3
                << " Msamples/s, ";
      if (a.have_seed0)
        std::cerr << "seed0 " << seed0 << std::endl;
      else
        std::cerr << "seed key 0x" << std::hex << st.seed_key << std::dec << std::endl;
    }
  } catch (const ykgpu::error& e) {
    std::cerr << e.what() << std::endl;
    return EXIT_FAILURE;
  }

  std::cout << "write to file : " << a.output << std::endl;
  if (!ykpng::write_rgb(a.output.c_str(), W, H, image.data())) {
    std::cout << "error" << std::endl;
    std::exit(EXIT_FAILURE);
  }
  std::cout << "success" << std::endl;
}
