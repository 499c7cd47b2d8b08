// yk_schedule.hpp — the host-side tuning block and the launch schedule of a render call as a pure
// rule: no HIP in here, so the CPU tests reach it (yk_host.cpp yk_schedule_plan).
#ifndef YK_SCHEDULE_HPP
#define YK_SCHEDULE_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <utility>
#include <vector>

// ---- Host-side tuning constants (each overridable with -DYK_...; the kernels' are at the top of
// yk_render_device.hpp) ----
#ifndef YK_LAUNCH_MB
#define YK_LAUNCH_MB 8192
#endif
// colour records of one launch at most: bounds a launch's slots for very large tiles (kmax in
// launch())
constexpr uint64_t kLaunchBytes = (uint64_t)YK_LAUNCH_MB << 20;
// samples per pixel per launch at most: many mid-sized launches beat a few big ones, because the
// launches alternate between two streams and each one's drain overlaps the next one's start
// (round 1, 1920x1080x512 259.5 -> 254.0 ms at 64 spp/launch; with the render
// streams at top priority, bench 205.5 ms at 64, 199.6 at 32, 199.8 at 24, 206.3 at 16)
#ifndef YK_LAUNCH_SPP
#define YK_LAUNCH_SPP 32
#endif
constexpr uint32_t kLaunchSpp = YK_LAUNCH_SPP;
// ... and for a call enqueued while the previous one still runs (launch() `inflight`): its launches
// need no ramp and overlap the calls around them, so the per-launch handover is what is left, and
// half as many launches pay it (frame: 8 of 64 instead of 16 of 32: bench -1.7%); a synced call
// keeps kLaunchSpp (64 there cost it 2%: the 64-spp warm-up under the ramp's 32-spp render and a
// longer last launch alone on the device, profiles/r06_ab/shade/).  The rings hold the larger
// launch in both, so a synced call and the in-flight calls after it share one ring geometry.
#ifndef YK_LAUNCH_SPP_OV
#define YK_LAUNCH_SPP_OV 64
#endif
constexpr uint32_t kLaunchSppOv = YK_LAUNCH_SPP_OV;
// ... or spp / kLaunchesPerCall when that is more (a long call: launch())
#ifndef YK_LAUNCHES_PER_CALL
#define YK_LAUNCHES_PER_CALL 32
#endif
constexpr uint32_t kLaunchesPerCall = YK_LAUNCHES_PER_CALL;
// ... and launches of about kLaunchSlots sample slots when the tile is small: a launch has a fixed
// cost (the handover of every CU from its render workgroup to the next launch's, filled by seed
// walks: ~0.2 ms per launch), so a call is split into round(slots / kLaunchSlots)
// launches — the frame's 32-spp launches are 66M slots, and a tile's launches are as large (the
// 8-way tile of 1920x1080x512: 2 launches of 256 spp; with 2^25-slot launches, 4 of 128, its
// back-to-back calls cost 2% more per sample than the frame's, profiles/r06_ab/tiles/)
#ifndef YK_LAUNCH_SLOTS
#define YK_LAUNCH_SLOTS (1u << 26)
#endif
constexpr uint64_t kLaunchSlots = YK_LAUNCH_SLOTS;
// ... and of about kLaunchSlotsOv for an in-flight call (as kLaunchSppOv for the frame), never
// fewer than two launches where a synced call has two: the 4-way tile 38.73 -> 38.59 ms, the 2-way
// 76.73 -> 76.18, config 4's 8-way 153.78 -> 153.10, the 8-way unchanged (profiles/r06_ab/tiles/r06ae_*)
#ifndef YK_LAUNCH_SLOTS_OV
#define YK_LAUNCH_SLOTS_OV (1u << 27)
#endif
constexpr uint64_t kLaunchSlotsOv = YK_LAUNCH_SLOTS_OV;
// global launch numbers whose dependency events (ykgpu_context::gev) are kept: more than any ring
// is deep
constexpr uint32_t kDepRing = 16;
// Under memory pressure (launch()): launches shrink down to this many sample slots before a call
// fails with YK_ERR_NOMEM, and the rings leave kMemReserve of the device free
constexpr uint64_t kMemFloorSlots = 1ull << 24;
constexpr size_t kMemReserve = (size_t)512 << 20;
// Start-record ring: the warm-ups run on ctx->aux, beside the render launches (their wave slots
// and VGPRs fit next to the render kernel's, and the render leaves most VALU issue slots idle),
// into a ring of min(launches, kWarmRingDepth) launch buffers (YKGPU_WARM_RING overrides); warm-up
// c waits for the render of launch c - ring.  Sized to the call: ring x slots x record (1920x1080
// at 32 spp per launch: 66M slots x 64 B = 4.2 GB per launch buffer).
#ifndef YK_WARM_RING
#define YK_WARM_RING 3
#endif
constexpr uint32_t kWarmRingDepth = YK_WARM_RING;
#ifndef YK_FIRST_LAUNCH
#define YK_FIRST_LAUNCH 4
#endif
constexpr uint32_t kFirstLaunch = YK_FIRST_LAUNCH;  // samples per pixel in the first launch
// ... and each next launch grows by this factor until kmax: 4, 8, 16, 32, 32, ... (1920x1080x512:
// 4 + 8 + 16 + 14 x 32 + 18 + 18 = 512 spp in 19 launches).  Before round 4: 8, 32, 32, ...; its second
// warm-up (32 spp of walks beside the first render) sometimes finished late and delayed every
// launch after it: 20 synced calls on one box spread 173.6-177.4 ms (max/min 1.022), against
// 173.6-174.6 (1.0059) with 4, 8, 16 (tools/variance_ab.py, profiles/r04_ab/variance/)
#ifndef YK_SCHED_GROW
#define YK_SCHED_GROW 2
#endif
constexpr uint32_t kSchedGrow = YK_SCHED_GROW;
// ... and for a call enqueued while the previous one still runs (launch(): `inflight`): every
// launch at kmax (YK_FIRST_LAUNCH_OV 0; else that many samples per pixel first, growing by
// YK_SCHED_GROW_OV)
#ifndef YK_FIRST_LAUNCH_OV
#define YK_FIRST_LAUNCH_OV 0
#endif
#ifndef YK_SCHED_GROW_OV
#define YK_SCHED_GROW_OV 4
#endif
constexpr uint32_t kFirstLaunchOv = YK_FIRST_LAUNCH_OV, kSchedGrowOv = YK_SCHED_GROW_OV;
static_assert(YK_FIRST_LAUNCH >= 1 && YK_LAUNCH_SPP >= 1, "launch sizes must be >= 1 sample per pixel");
#ifndef YK_TILE
#define YK_TILE 8
#endif
constexpr uint32_t kTile = YK_TILE;  // processing blocks of kTile x kTile pixels (0: row-major)
// the shape of a processing block, tw x th tile pixels (kTile x kTile of them), for a tile of every
// stride-th image row (build_order, yk_pipeline.hip; the sky-block classifier tests these blocks)
inline void order_block(uint32_t stride, uint32_t& tw, uint32_t& th) {
  th = stride <= 1 ? kTile : (stride <= 4 ? std::max(1u, kTile / 2) : std::max(1u, kTile / 4));
  tw = kTile * kTile / std::max(1u, th);
}
// colour buffers in flight (col_ring())
#ifndef YK_COL_RING
#define YK_COL_RING 2
#endif
// FP64 warm-up grid: blocks per CU (warm_per_cu(); each thread walks n / grid slots, at least kWarmSlots)
#ifndef YK_WARM_PER_CU
#define YK_WARM_PER_CU 32
#endif
#ifndef YK_WARM_SLOTS
#define YK_WARM_SLOTS 4
#endif
constexpr uint32_t kWarmSlots = YK_WARM_SLOTS;

// A/B knobs: environment overrides of the launch schedule, rings, grids and tree build that the
// A/B tools time (tools/abtime.py `lib@YKGPU_X=v`).  They exist only in variant builds
// (tools/build_variant.sh <name> -DYK_AB_KNOBS): in the product library ab_knob() is a
// constant nullptr, so nothing in a caller's environment changes the schedule or the tree.  The
// documented diagnostics YKGPU_TIMELINE and YKGPU_OVERLAP stay.
namespace {
#ifdef YK_AB_KNOBS
inline const char* ab_knob(const char* name) { return std::getenv(name); }
#else
constexpr const char* ab_knob(const char*) { return nullptr; }
#endif
}  // namespace

// ---- The launch schedule of a render call (launch(), yk_pipeline.hip) as a pure rule ----
namespace yksched {

// a sample slot's colour record (kColStride doubles, yk_render_device.hpp)
constexpr uint64_t kColourBytes = 32;

// samples per pixel of a call's largest launch: the rings' (an in-flight call's launches, and what a
// launch buffer holds), a synced call's own (<= kideal), and the floor memory pressure shrinks to
struct LaunchSizes {
  uint32_t kideal, ksynced, kfloor;
};

// nps: the call's processing slots (>= pixels); spp: its samples per pixel; lanes: the threads of the
// persistent grid
inline LaunchSizes launch_sizes(uint32_t nps, uint32_t spp, uint64_t lanes) {
  // (slots of a launch stay below 2^31: the kernels' fdiv takes 31-bit numerators)
  // A launch of few pixels still gets enough slots to fill the persistent grid (16 per lane):
  // a thin row tile at high spp would otherwise run dozens of launches that each pay a ramp and
  // a drain.  Neither floor nor cap exceeds the colour budget or 2^31 slots.
  const uint64_t fill_spp = (lanes * 16 + nps - 1) / nps;
  uint64_t launch_slots = kLaunchSlots;  // (A/B knob: YKGPU_LAUNCH_SLOTS)
  if (const char* e = ab_knob("YKGPU_LAUNCH_SLOTS")) launch_slots = (uint64_t)std::max(1ll, std::atoll(e));
  auto launches_for = [&](uint64_t lslots) {
    return std::max<uint64_t>(1, ((uint64_t)nps * spp + lslots / 2) / lslots);
  };
  // (in flight: never fewer than two launches where a synced call has two — a one-launch call has
  // rings of one buffer and overlaps nothing: the 8-way tile 19.6 -> 25.5 ms, r06ad; one launch
  // with the rings' full depth kept instead: +1.5%, profiles/r06_ab/tiles/r06al_*)
  const uint64_t call_launches = launches_for(launch_slots);
  const uint64_t call_launches_ov =
      std::max(std::min<uint64_t>(call_launches, 2), launches_for(std::max(launch_slots, kLaunchSlotsOv)));
  const uint64_t slot_spp = (spp + call_launches - 1) / call_launches;
  const uint64_t slot_spp_ov = (spp + call_launches_ov - 1) / call_launches_ov;
  // A long call takes longer launches: every launch pays a drain whose length is the longest path
  // of its last samples, and many launches per call buy nothing once there are ~32 (config 5,
  // 1920x1080x4096 at depth 200 on the glass scene: 32 spp per launch 1730 ms, 64 1631, 121 (the
  // colour budget then) 1589, with a warm ring of 2 1610; config 3's 512 spp stay at 32, where 64
  // costs 5%; profiles/r04_ab/launch_size/).  The rings grow with the launch: config 5's launches
  // are spp / kLaunchesPerCall = 128 spp, and it holds ~68 GB (3 x 2.07M x 128 x 64 B of start
  // records, 2 x 2.07M x 128 x 32 B of colours).
  uint64_t launch_spp = std::max<uint64_t>(kLaunchSpp, spp / kLaunchesPerCall);
  if (const char* e = ab_knob("YKGPU_LAUNCH_SPP")) launch_spp = (uint64_t)std::max(1, std::atoi(e));  // (A/B)
  const uint64_t launch_spp_ov = std::max<uint64_t>(std::max<uint64_t>(kLaunchSppOv, launch_spp), spp / kLaunchesPerCall);
  auto ideal_for = [&](uint64_t lspp, uint64_t sspp) {
    return (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>({spp, kLaunchBytes / (kColourBytes * nps),
                               std::max<uint64_t>({lspp, fill_spp, sspp}), ((1ull << 31) - 1) / nps}));
  };
  LaunchSizes z;
  z.kideal = ideal_for(launch_spp_ov, slot_spp_ov);
  z.ksynced = ideal_for(launch_spp, slot_spp);
  // (under memory pressure launches shrink down to kMemFloorSlots sample slots)
  z.kfloor = (uint32_t)std::min<uint64_t>(z.kideal, std::max<uint64_t>(1, (kMemFloorSlots + nps - 1) / nps));
  return z;
}

// The launches (first sample, samples per pixel) of a call of spp samples per pixel from s_begin,
// whose launch buffers hold kmax samples per pixel (kideal, or less under memory pressure).
// Synced: kFirstLaunch (4), growing by kSchedGrow (2) up to min(kmax, ksynced) — kLaunchSpp = 32 for
// the frame, more for a small tile — 1920x1080x512: 4, 8, 16, 14 x 32, 18, 18 = 19 launches.  The
// first render waits only for a 4-sample warm-up, and each next warm-up, twice the one before,
// finishes under the render before it (see kSchedGrow).
// A call enqueued while the previous one still runs (back-to-back steps, `inflight`) starts its first
// warm-ups under the previous call's last launches, so it needs no small first launch: every
// launch at kmax — the frame is 8 launches of 64, the 8-way tile of config 3 two of 256.  (Measured
// in round 4, when kmax was 32 for the frame and ~130 for that tile: bench 8 steps 172.4 ms per
// step with 4, 8, 16, 32; 170.8 with 8, 32; 168.4 with 32, 32, ...; profiles/r04_ab/schedule/; the
// tile 23.1 ms per call starting at 32, 21.8 at 128; the 4-way tile 44.3 -> 43.0 ms starting at 64;
// profiles/r04_ab/tiles/)
// (A/B knobs: YKGPU_FIRST_LAUNCH, YKGPU_SCHED_GROW and their _OV forms — the first launch's
// samples per pixel and the factor each next launch grows by until kmax)
inline void launch_schedule(std::vector<std::pair<uint32_t, uint32_t>>& sched, uint32_t spp, uint32_t s_begin,
                            uint32_t kmax, uint32_t ksynced, bool inflight) {
  // this call's largest launch: the rings' (kmax) in flight, a synced call's own below it
  const uint32_t kcap = inflight ? kmax : std::min(kmax, ksynced);
  uint32_t first_k = inflight ? (kFirstLaunchOv ? kFirstLaunchOv : kmax) : kFirstLaunch;
  uint32_t grow_k = inflight ? kSchedGrowOv : kSchedGrow;
  if (const char* e = ab_knob(inflight ? "YKGPU_FIRST_LAUNCH_OV" : "YKGPU_FIRST_LAUNCH"))
    first_k = (uint32_t)std::max(1, std::atoi(e));
  if (const char* e = ab_knob(inflight ? "YKGPU_SCHED_GROW_OV" : "YKGPU_SCHED_GROW"))
    grow_k = (uint32_t)std::max(2, std::atoi(e));
  sched.clear();
  // the ramp (first_k, growing by grow_k), then launches of kmax; a short tail launch, which would
  // pay its own drain, is folded into the launch before it, or that launch and the tail are split
  // into two equal launches when one would exceed kmax — so no launch exceeds kmax, and every call
  // of the same kmax places its launches in the rings alike (a back-to-back call overlaps the
  // call before it, synced or not).  Launches of exactly kmax also keep the warm-up's walks
  // aligned: at 32 spp its grid-stride is the pixel count, so a lane's four walks are four
  // samples of one pixel (their processing-order reads coincide; a 30- or 31-spp launch fetches
  // 1.7x the bytes per slot in the warm-up, profiles/r06_ab/pmc/)
  for (uint32_t s0 = 0, k = std::min(first_k, kcap); s0 < spp;) {
    uint32_t take = std::min(k, spp - s0);
    const uint32_t rest = spp - (s0 + take);
    if (rest > 0 && rest < std::max(1u, take / 4))
      take = spp - s0 <= kcap ? spp - s0 : (spp - s0 + 1) / 2;
    sched.emplace_back(s_begin + s0, take);
    s0 += take;
    // (a ramp growing by half past 32 or 16 spp did not recover the synced call of 64-spp
    // launches: profiles/r06_ab/shade/r06z_*, r06aa_*)
    k = std::min(grow_k * k, kcap);
  }
}

}  // namespace yksched

#endif
