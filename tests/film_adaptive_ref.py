"""The yardstick of the adaptive-film tests (TEST INFRASTRUCTURE ONLY): the selection rule of
include/ykgpu.h "adaptive passes" simulated in numpy on film_ref's prefix folds — not the code
under test.  A pixel with count n holds S[n], Q[n] (film_ref.prefixes) by construction, so the
expected state of a film is fully described by its count map.

  selected  n < target and (n < 2 or e2(S[n], Q[n], n) > threshold2)      (strict)
  take      min(n_samples, target - n)
  groups    the distinct (n, take) among the selected pixels, ascending n

Thresholds come from the reference: np.quantile(e2 map after the uniform first pass, q,
method="lower"), so one pixel sits exactly on the threshold.  A pass is (q, n_samples); q None is
threshold2 = -1 (every unfinished pixel)."""
import numpy as np

import film_ref


def at_counts(stack, counts):
    """stack[counts[y, x], y, x, ...]"""
    a = np.stack(stack)
    idx = counts.astype(np.intp).reshape((1,) + counts.shape + (1,) * (a.ndim - 1 - counts.ndim))
    return np.ascontiguousarray(np.take_along_axis(a, idx, 0)[0])


def e2_at(S, Q, counts):
    """film_ref.e2_map at each pixel's own count; +inf below two samples."""
    e2 = np.full(counts.shape, np.inf, np.float64)
    for v in np.unique(counts):
        if v >= 2:
            m = counts == v
            e2[m] = film_ref.e2_map(S[v], Q[v], int(v))[m]
    return e2


def image_at(S, counts):
    """film_ref.to_color3b(S[n], n) per pixel; black at n = 0."""
    out = np.zeros(counts.shape + (3,), np.uint8)
    for v in np.unique(counts):
        if v >= 1:
            m = counts == v
            out[m] = film_ref.to_color3b(S[v], int(v))[m]
    return out


def launches_of(take):
    """Launches of a synced call of `take` samples per pixel on a small tile (the launch schedule
    of DESIGN.md §8: 4, doubling, a tail shorter than a quarter of a launch folded into it)."""
    n, s0, k = 0, 0, min(4, take)
    while s0 < take:
        t = min(k, take - s0)
        rest = take - (s0 + t)
        if 0 < rest < max(1, t // 4):
            t = take - s0
        s0 += t
        n += 1
        k = min(2 * k, take)
    return n


class Sim:
    def __init__(self, cols):
        self.S, self.Q = film_ref.prefixes(cols)
        self.target = cols.shape[2]
        self.counts = np.zeros(cols.shape[:2], np.uint32)
        self.first_e2 = None  # the e2 map after the first pass: the quantiles' source

    def threshold2(self, q):
        return -1.0 if q is None else float(np.quantile(self.first_e2, q, method="lower"))

    def step(self, threshold2, n_samples):
        """Applies one pass; returns what yk_film_pass must report (groups as a list of (n, take))."""
        c = self.counts
        sel = (c < self.target) & ((c < 2) | (e2_at(self.S, self.Q, c) > threshold2))
        take = np.minimum(np.uint32(n_samples), self.target - c).astype(np.uint32)
        groups = sorted({(int(n), int(t)) for n, t in zip(c[sel], take[sel])})
        self.counts = np.where(sel, c + take, c).astype(np.uint32)
        if self.first_e2 is None:
            self.first_e2 = e2_at(self.S, self.Q, self.counts)
        return dict(pixels_selected=int(sel.sum()), samples_added=int(take[sel].sum()), groups=groups,
                    launches=sum(launches_of(t) for _, t in groups), min_count=int(self.counts.min()),
                    max_count=int(self.counts.max()))

    def sums(self):
        return at_counts(self.S, self.counts)

    def sumsq(self):
        return at_counts(self.Q, self.counts)

    def e2(self):
        return e2_at(self.S, self.Q, self.counts)

    def image(self):
        return image_at(self.S, self.counts)


PASSES_A = [(None, 4), (0.75, 5), (0.25, 3), (0.5, 4), (None, 20)]
