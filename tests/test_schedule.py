"""The launch schedule of a render call as a pure function (csrc/yk_schedule.hpp), on the CPU.

launch() (csrc/yk_pipeline.hip) takes a call's launch sizes and its (first sample, samples) list
from yksched::launch_sizes / launch_schedule; the library exports them for this test as
yk_schedule_plan (yk_host.cpp; not in include/ykgpu.h).

Where the expected values come from: `parent_sizes` / `parent_schedule` below restate by hand, in
Python, the rule as the one-file launch() of commit a09cfe3 had it inline (its ideal_for lambda and
its ramp / tail-fold loop, with that commit's tuning constants).  The pinned lists were produced by
that restatement and agree with the schedules quoted in DESIGN.md §8 and the docstrings of
test_gpu_film.py and test_gpu_robust.py.  Config 5 (4,096 spp) is not pinned as a list: the
restatement gives ring launches of 128 spp (the comments that said 121 dated from a smaller colour
budget and were corrected); the cross-check below covers it.
"""
import ctypes

import pytest

import uecraytracing_amd as yk
from film_adaptive_ref import launches_of

LANES = 256 * 768  # the persistent grid of the mt19937 instances: one 768-thread workgroup per CU
FRAME = 2_073_600  # 1920 x 1080 in 8 x 8 blocks
TILE8 = 259_200  # the 8-way tile of config 3
SMALL = 144  # a 12 x 12 test tile

# the parent's host tuning block
LAUNCH_BYTES, COLOUR_BYTES = 8192 << 20, 32
LAUNCH_SPP, LAUNCH_SPP_OV, LAUNCHES_PER_CALL = 32, 64, 32
LAUNCH_SLOTS, LAUNCH_SLOTS_OV, MEM_FLOOR_SLOTS = 1 << 26, 1 << 27, 1 << 24
FIRST, GROW, FIRST_OV, GROW_OV = 4, 2, 0, 4


def parent_sizes(nps, spp, lanes):
    fill_spp = (lanes * 16 + nps - 1) // nps

    def launches_for(lslots):
        return max(1, (nps * spp + lslots // 2) // lslots)

    call = launches_for(LAUNCH_SLOTS)
    call_ov = max(min(call, 2), launches_for(max(LAUNCH_SLOTS, LAUNCH_SLOTS_OV)))
    slot_spp, slot_spp_ov = (spp + call - 1) // call, (spp + call_ov - 1) // call_ov
    launch_spp = max(LAUNCH_SPP, spp // LAUNCHES_PER_CALL)
    launch_spp_ov = max(LAUNCH_SPP_OV, launch_spp, spp // LAUNCHES_PER_CALL)

    def ideal_for(lspp, sspp):
        return max(1, min(spp, LAUNCH_BYTES // (COLOUR_BYTES * nps), max(lspp, fill_spp, sspp), ((1 << 31) - 1) // nps))

    kideal, ksynced = ideal_for(launch_spp_ov, slot_spp_ov), ideal_for(launch_spp, slot_spp)
    kfloor = min(kideal, max(1, (MEM_FLOOR_SLOTS + nps - 1) // nps))
    return kideal, ksynced, kfloor


def parent_schedule(spp, s_begin, kmax, ksynced, inflight):
    kcap = kmax if inflight else min(kmax, ksynced)
    first_k = (FIRST_OV or kmax) if inflight else FIRST
    grow_k = GROW_OV if inflight else GROW
    out, s0, k = [], 0, min(first_k, kcap)
    while s0 < spp:
        take = min(k, spp - s0)
        rest = spp - (s0 + take)
        if 0 < rest < max(1, take // 4):
            take = spp - s0 if spp - s0 <= kcap else (spp - s0 + 1) // 2
        out.append((s_begin + s0, take))
        s0 += take
        k = min(grow_k * k, kcap)
    return out


@pytest.fixture(scope="module")
def plan():
    lib = yk.load_library()
    f = lib.yk_schedule_plan
    u32, p32 = ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)
    f.argtypes = [u32, u32, u32, ctypes.c_uint64, ctypes.c_int, u32, p32, p32, p32, u32]
    f.restype = u32

    def call(nps, spp, inflight, s_begin=0, lanes=LANES, kmax=0):
        cap = 4096
        sizes, s0, take = (u32 * 3)(), (u32 * cap)(), (u32 * cap)()
        n = f(nps, spp, s_begin, lanes, int(inflight), kmax, sizes, s0, take, cap)
        assert n <= cap
        return tuple(sizes), [(s0[i], take[i]) for i in range(n)]

    return call


def takes(sched):
    return [t for _, t in sched]


PINNED = [
    (FRAME, 512, False, [4, 8, 16] + [32] * 14 + [18, 18]),
    (FRAME, 512, True, [64] * 8),
    (FRAME, 64, False, [4, 8, 16, 18, 18]),
    (FRAME, 64, True, [64]),
    (TILE8, 512, True, [256, 256]),
    (SMALL, 13, False, [4, 9]),
    (SMALL, 16, False, [4, 8, 4]),
    (SMALL, 40, False, [4, 8, 16, 12]),
    (SMALL, 4, False, [4]),
]


@pytest.mark.parametrize("nps,spp,inflight,want", PINNED)
def test_pinned_schedules(plan, nps, spp, inflight, want):
    # (the restatement produced the list ...)
    kideal, ksynced, _ = parent_sizes(nps, spp, LANES)
    assert takes(parent_schedule(spp, 0, kideal, ksynced, inflight)) == want
    # ... and the library's function gives it
    sizes, sched = plan(nps, spp, inflight)
    assert takes(sched) == want


def test_frame_ring_launch_size(plan):
    """The frame at 512 spp: 19 synced launches, launch buffers of 64 samples per pixel."""
    sizes, sched = plan(FRAME, 512, False)
    assert len(sched) == 19 and sizes[0] == 64 and sizes[1] == 32


CASES = [(SMALL, spp) for spp in range(1, 301)] + [
    (FRAME, 1), (FRAME, 31), (FRAME, 33), (FRAME, 64), (FRAME, 100), (FRAME, 512), (FRAME, 1000), (FRAME, 4096),
    (TILE8, 512), (TILE8, 64), (FRAME // 2, 512), (FRAME // 4, 512), (1920 * 8, 4096)]


def test_schedule_properties(plan):
    for nps, spp in CASES:
        for inflight in (False, True):
            for s_begin in (0, 7):
                sizes, sched = plan(nps, spp, inflight, s_begin)
                kideal, ksynced, kfloor = sizes
                assert sum(takes(sched)) == spp, (nps, spp, inflight)
                assert max(takes(sched)) <= kideal and min(takes(sched)) >= 1, (nps, spp, inflight, sched)
                assert 1 <= kfloor <= kideal and ksynced <= kideal
                at = s_begin
                for s0, t in sched:
                    assert s0 == at, (nps, spp, inflight, sched)
                    at += t
                if nps == SMALL and not inflight:
                    assert len(sched) == launches_of(spp), (spp, sched)


def test_matches_the_parents_rule(plan):
    """Every case above, and the launch sizes memory pressure shrinks to, against the restatement."""
    for nps, spp in CASES:
        want_sizes = parent_sizes(nps, spp, LANES)
        for inflight in (False, True):
            kmax = want_sizes[0]
            while True:
                sizes, sched = plan(nps, spp, inflight, 3, kmax=kmax)
                assert sizes == want_sizes, (nps, spp)
                assert sched == parent_schedule(spp, 3, kmax, want_sizes[1], inflight), (nps, spp, inflight, kmax)
                if kmax <= want_sizes[2]:
                    break
                kmax = max(want_sizes[2], kmax // 2)  # launch()'s shrink
