"""Chooses the sampled guided filter's default point (yk_guided_sampled_defaults) on the CPU (a tool,
not a test).

tools/features_tune.py with the guides of the sampled feature pass (tests/film_features_sampled_ref.py:
the first hits of the render's own first n samples, lens and jitter included) instead of the pinhole
sub-rays.  The same four cases, the oracle's samples and the MSE against the oracle's 1024-spp mean
(DESIGN.md §6.4), plus one control that takes no part in the choice: the final scene at 96x54 and
16 spp with the lens switched off (lens_radius = 0), where the sampled guides see jitter only.  The grid

  n in {4, 8, 16} (a case of fewer samples per pixel uses min(n, spp): a pass cannot sample past the
  film's target),  colour k2 in {0.5, 1, 2},  k2_f in {0.5, 1, 2},  tau_albedo, tau_normal in
  {1e-3, 1e-2, 1e-1},  tau_depth in {1e-2, 1e-1, 1, inf},  alpha_f = 1       (972 points per case)

The score of a point is §6.4's: the geometric mean over the four cases of guided MSE / colour-only
MSE.  The chosen point minimises it, unless the pinhole pass at yk_guided_defaults scores at least as
well: then yk_guided_sampled_defaults keeps that pair, with n = 16.  The figures of the chosen point
are recomputed through the yardstick itself (film_features_ref.guided_nlm) before they are written.

usage: python tools/features_sampled_tune.py [--out profiles/TAG_features_sampled_tune.json] [--jobs 5]
"""
import argparse
import itertools
import json
import math
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import features_tune as ft  # noqa: E402
import film_denoise_ref as fdr  # noqa: E402
import film_features_ref as ffr  # noqa: E402
import film_features_sampled_ref as fsr  # noqa: E402
import film_ref  # noqa: E402
from uecraytracing_amd.records import Camera, make_params  # noqa: E402

NS = (4, 8, 16)
CONTROL = "final_pinhole"
CASES = dict(ft.CASES, **{CONTROL: ft.CASES["final"]})
SCORED = tuple(ft.CASES)
NAMES = ("colour_k2", "k2_f", "tau_albedo", "tau_normal", "tau_depth", "n")
FALLBACK_N = 16


def scene_of(name):
    if name != CONTROL:
        return ft.scene_of(name)
    spheres, cam = ft.scene_of("final")
    return spheres, Camera(cam.origin, cam.lower_left_corner, cam.horizontal, cam.vertical, cam.lens_u, cam.lens_v, 0.0)


def existing_pair():
    c, f = ffr.COLOUR_DEFAULTS, ffr.FEATURE_DEFAULTS
    return (c["k2"], f["k2"], f["tau_albedo"], f["tau_normal"], f["tau_depth"])


def run_case(name):
    w, h, spp = CASES[name]
    spheres, cam = scene_of(name)
    p = make_params(w, h, spp, 50, 404)
    truth = fdr.truth(spheres, cam, w, h)
    S, Q = film_ref.prefixes(film_ref.colours(spheres, cam, p))
    m, v = fdr.moments(S[spp], Q[spp], spp)
    raw = fdr.mse(m, truth)
    base = fdr.mse(fdr.nlm(m, v, **fdr.DEFAULTS), truth)
    pinhole = fdr.mse(ffr.denoise_guided(S[spp], Q[spp], spp, spheres, cam, p), truth)
    mq = np.stack([m[cy][:, cx] for _, _, _, cy, cx in ft.offsets(h, w)])
    wcs = {k2: ft.colour_weights(m, v, np.float64(k2)) for k2 in ft.K2}
    res = {}
    with np.errstate(invalid="ignore"):
        for n in NS:
            F, U, _ = fsr.features(spheres, cam, p, min(n, spp))
            for k2_f in ft.K2F:
                num, den = ft.feature_phis(F, U, np.float64(k2_f))
                phi = [{t: num[..., k] / (np.float64(t) + den[..., k]) for t in taus}
                       for k, taus in enumerate((ft.TAU_A, ft.TAU_N, ft.TAU_Z))]
                for ta, tn, tz in itertools.product(ft.TAU_A, ft.TAU_N, ft.TAU_Z):
                    DF = np.zeros(num.shape[:3])
                    for x in (phi[0][ta], phi[1][tn], phi[2][tz]):
                        DF = np.where(DF > x, DF, x)
                    tf = 1.0 - 0.25 * DF
                    tf = np.where(tf > 0.0, tf, 0.0)
                    wf = (tf * tf) * (tf * tf)
                    for k2 in ft.K2:
                        wgt = np.where(wf < wcs[k2], wf, wcs[k2])
                        res[(k2, k2_f, ta, tn, tz, n)] = fdr.mse(ft.fold(wgt, mq), truth)
    return name, raw, base, pinhole, res


def yardstick_mse(name, point):
    k2, k2_f, ta, tn, tz, n = point
    w, h, spp = CASES[name]
    spheres, cam = scene_of(name)
    p = make_params(w, h, spp, 50, 404)
    S, Q = film_ref.prefixes(film_ref.colours(spheres, cam, p))
    out = fsr.denoise_guided(S[spp], Q[spp], spp, spheres, cam, p, min(n, spp), colour=dict(radius=ft.R, patch=ft.FP, k2=k2),
                             feat=dict(k2=k2_f, alpha=1.0, tau_albedo=ta, tau_normal=tn, tau_depth=tz))
    return fdr.mse(out, fdr.truth(spheres, cam, w, h))


def geomean(xs):
    return math.exp(sum(math.log(x) for x in xs) / len(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--jobs", type=int, default=5)
    a = ap.parse_args()
    with multiprocessing.Pool(max(1, min(a.jobs, len(CASES)))) as pool:
        results = {r[0]: r[1:] for r in pool.map(run_case, list(CASES))}
    points = list(results[SCORED[0]][3])
    score = {pt: geomean([results[c][3][pt] / results[c][1] for c in SCORED]) for pt in points}
    best = min(points, key=lambda pt: score[pt])
    pinhole_score = geomean([results[c][2] / results[c][1] for c in SCORED])
    same_pair = existing_pair() + (FALLBACK_N,)
    beats = score[best] < pinhole_score
    chosen = best if beats else same_pair
    out = {"tool": "tools/features_sampled_tune.py",
           "cases": {c: dict(zip(("width", "height", "spp"), CASES[c])) for c in CASES},
           "control": CONTROL,
           "measure": "MSE against the oracle's 1024-spp mean; score: geometric mean over the four scored cases of "
                      "guided / colour-only; a case uses min(n, spp) samples",
           "pinhole_pair_score": pinhole_score, "best_sampled": dict(zip(NAMES, best), score=score[best]),
           "sampled_at_the_pinhole_pair": dict(zip(NAMES, same_pair), score=score[same_pair]),
           "a_sampled_point_beats_the_pinhole_pair": beats,
           "chosen": dict(zip(NAMES, chosen)), "score": score[chosen], "best_per_n": {}, "table": {}}
    for n in NS:
        bn = min((pt for pt in points if pt[5] == n), key=lambda pt: score[pt])
        out["best_per_n"][str(n)] = dict(zip(NAMES, bn), score=score[bn])
    for c in CASES:
        raw, base, pinhole, res = results[c]
        sampled = yardstick_mse(c, chosen)
        assert abs(sampled - res[chosen]) <= 1e-9 * sampled, (c, sampled, res[chosen])
        out["table"][c] = {"raw": raw, "colour_only": base, "guided_pinhole_g2": pinhole, "guided_sampled": sampled,
                           "n_used": min(chosen[5], CASES[c][2]),
                           "sampled_over_colour_only": sampled / base, "pinhole_over_colour_only": pinhole / base,
                           "sampled_over_pinhole": sampled / pinhole,
                           "sampled_at_the_pinhole_pair_by_n": {str(n): res[same_pair[:5] + (n,)] for n in NS},
                           "best_sampled_point": res[best]}
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
