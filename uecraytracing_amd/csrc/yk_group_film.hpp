// yk_group_film.hpp — group films (include/ykgpu.h "group films"): ykgpu_group_film_*.
// Part of yk_group.hip (included at its end, like yk_cast.hpp in yk_features.hip).
//
// A group film is, by definition, the single-context film of its params; entry e holds an ordinary
// film of the group render's sub-tile (tile row t → entry t mod k, row t / k there) and every call
// is that film's call per entry, with the rows dealt back into the whole tile's arrays on the host.
// The filters deal bands of consecutive rows instead (yk_group_plan.hpp): the moments run on the
// render-side films, pitched copies move the rows to the band buffers, the unchanged filter
// kernels run per band (yk_denoise.hip denoise_band_enqueue).
#ifndef YK_GROUP_FILM_HPP
#define YK_GROUP_FILM_HPP

namespace {

using GroupHist = std::map<uint32_t, uint64_t>;

// the whole tile's count histogram: the entries' merged
GroupHist gf_hist(const ykgpu_group_film* f) {
  GroupHist h;
  for (const ykgpu_film* film : f->film)
    if (film)
      for (const auto& kv : film->hist)
        if (kv.second) h[kv.first] += kv.second;
  return h;
}

int gf_ready(const ykgpu_group_film* f) {
  if (!f) return fail(YK_ERR_INVALID, "null group film");
  bool torn = f->torn;
  for (const ykgpu_film* film : f->film) torn = torn || (film && film->torn);
  if (torn)
    return fail(YK_ERR_INVALID, "the group film's last accumulate failed part-way: restore it with ykgpu_group_film_write");
  return YK_OK;
}

int gf_stale(const ykgpu_group_film* f) {
  for (uint32_t e = 0; e < f->k; ++e)
    if (f->film[e] && f->g->ctx[e]->scene_gen != f->gen[e])
      return fail(YK_ERR_INVALID, "the group's scene was set after the group film was created");
  return YK_OK;
}

// the calling thread's last error, with the entry's name in front
int entry_fail(uint32_t e, int rc, const std::string& msg) {
  return fail(rc, "group film entry " + std::to_string(e) + ": " + msg);
}
int entry_fail(uint32_t e, int rc) { return entry_fail(e, rc, std::string(last_error())); }

// entry e's sub-tile rows into their rows of the whole tile (per: values per pixel), and back
template <typename T>
void gf_scatter(const ykgpu_group_film* f, uint32_t e, const T* sub, T* whole, size_t per) {
  const size_t row = (size_t)f->wt * per;
  for (uint32_t r = 0; r < f->rows[e]; ++r)
    std::memcpy(whole + ((size_t)e + (size_t)r * f->k) * row, sub + (size_t)r * row, row * sizeof(T));
}
template <typename T>
void gf_gather(const ykgpu_group_film* f, uint32_t e, const T* whole, T* sub, size_t per) {
  const size_t row = (size_t)f->wt * per;
  for (uint32_t r = 0; r < f->rows[e]; ++r)
    std::memcpy(sub + (size_t)r * row, whole + ((size_t)e + (size_t)r * f->k) * row, row * sizeof(T));
}

size_t gf_npix(const ykgpu_group_film* f) { return (size_t)f->p.row_count * f->wt; }
size_t gf_sub_npix(const ykgpu_group_film* f, uint32_t e) { return (size_t)f->rows[e] * f->wt; }

// ykgpu_group_get_stats after an accumulate: every entry's last call, and the whole call's
void gf_stats(ykgpu_group_film* f, std::chrono::steady_clock::time_point t0) {
  ykgpu_group* g = f->g;
  yk_render_stats tot{};
  for (uint32_t e = 0; e < f->k; ++e) {
    g->st[e] = yk_render_stats{};
    if (!f->film[e]) continue;
    g->st[e] = g->ctx[e]->stats;
    add_entry_stats(tot, g->st[e], 0, 0);
  }
  tot.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  g->total = tot;
}

void gf_sync_all(const ykgpu_group_film* f) {
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    (void)hipSetDevice(f->g->ctx[e]->device);
    (void)hipStreamSynchronize(f->g->ctx[e]->stream);
  }
}

void gf_drop_bands(ykgpu_group_film* f) {
  for (ykgpu_film*& b : f->band) {
    ykgpu_film_destroy(b);
    b = nullptr;
  }
  f->have_bands = false;
}

// the band films for `halo`: film records without sample planes over band+halo of P's tile
void gf_make_bands(ykgpu_group_film* f, uint32_t halo, const std::vector<ykplan::Band>& bands) {
  if (f->have_bands && f->halo == halo) return;
  gf_drop_bands(f);
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!bands[e].count) continue;
    auto* b = new ykgpu_film();
    b->ctx = f->g->ctx[e];
    b->device = b->ctx->device;
    b->p = f->p;
    b->p.row_begin = (uint32_t)host_row_y(&f->p, bands[e].lo);  // (P's rows are consecutive)
    b->p.row_stride = 1;
    b->p.row_band_log2 = 0;
    b->p.row_count = bands[e].hi - bands[e].lo;
    b->scene_gen = f->gen[e];
    b->npix = (uint64_t)b->p.row_count * f->wt;
    b->hist[0] = b->npix;
    f->band[e] = b;
  }
  f->halo = halo;
  f->have_bands = true;
}

// n_samples of a sampled feature pass against the group film's target
int gf_check_n(const ykgpu_group_film* f, uint32_t n) {
  if (n < 1 || n > 256) return fail(YK_ERR_INVALID, "features: n_samples must be 1..256");
  if (n > f->p.samples_per_pixel) return fail(YK_ERR_INVALID, "features: n_samples is larger than the film's target");
  return YK_OK;
}

// Both filters.  fp: the guided filter's feature parameters, null for the colour-only one;
// n_samples != 0: the guides are the sampled pass's (fp->grid is not read).
int gf_denoise(ykgpu_group_film* f, const yk_denoise_params& dp, const yk_feature_params* fp, uint32_t n_samples,
               double* mean_host, uint8_t* rgb_host, yk_group_denoise_stats* stats) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = gf_ready(f)) return rc;
  if (int rc = denoise_params_check(dp)) return rc;
  if (fp) {
    if (int rc = feature_params_check(*fp)) return rc;
    if (int rc = gf_stale(f)) return rc;
  }
  if (!mean_host && !rgb_host) return fail(YK_ERR_INVALID, "denoise: mean_host and rgb_host are both null");
  const yk_render_params& P = f->p;
  if (host_row_y(&P, P.row_count - 1) != (uint64_t)P.row_begin + P.row_count - 1 ||
      host_col_x(&P, f->wt - 1) != (uint64_t)P.col_begin + f->wt - 1)
    return fail(YK_ERR_UNSUPPORTED, "denoise: the film's tile is not consecutive image rows and columns");
  if (gf_hist(f).begin()->first < 2) return fail(YK_ERR_INVALID, "denoise needs at least two samples in every pixel");

  const uint32_t k = f->k, wt = f->wt;
  std::vector<ykplan::Band> bands;
  std::vector<ykplan::Copy> copies;
  ykplan::group_film_plan(P.row_count, k, dp.radius + dp.patch, bands, copies);
  gf_make_bands(f, dp.radius + dp.patch, bands);
  ykgpu_group* g = f->g;

  // per entry: the moments' start and end on the render side; the exchange's start and end and the
  // filter's end on the band side
  enum { kM0, kM1, kX0, kX1, kF1, kEvents };
  std::vector<hipEvent_t> ev((size_t)k * kEvents, nullptr);
  std::vector<DenoiseBufs> sb(k), db(k);
  std::vector<const double*> feat(k, nullptr);
  double ms_feat = 0;
  const auto body = [&]() -> int {
    // the feature planes of every band+halo first: the pass is synchronous, the rest is not
    for (uint32_t e = 0; fp && e < k; ++e) {
      if (!f->band[e]) continue;
      double t = 0;
      if (n_samples) {
        yk_sampled_features_stats fs{};
        if (int rc = yk_film_features_sampled_ensure(f->band[e], n_samples, &feat[e], &fs)) return entry_fail(e, rc);
        t = fs.ms;
      } else if (int rc = yk_film_features_ensure(f->band[e], fp->grid, &feat[e], &t)) {
        return entry_fail(e, rc);
      }
      ms_feat = std::max(ms_feat, t);
    }
    // (a) the moments, on every entry's own film
    for (uint32_t e = 0; e < k; ++e) {
      if (!f->film[e]) continue;
      YK_HIP(hipSetDevice(g->ctx[e]->device));
      for (int q = 0; q < kEvents; ++q) YK_HIP(hipEventCreate(&ev[(size_t)e * kEvents + q]));
      if (int rc = denoise_buffers(f->film[e], &sb[e])) return entry_fail(e, rc);
      if (f->band[e])
        if (int rc = denoise_buffers(f->band[e], &db[e])) return entry_fail(e, rc);
      const hipStream_t st = g->ctx[e]->stream;
      YK_HIP(hipEventRecord(ev[(size_t)e * kEvents + kM0], st));
      YK_HIP(denoise_moments_enqueue(f->film[e], sb[e]));
      YK_HIP(hipEventRecord(ev[(size_t)e * kEvents + kM1], st));
    }
    // (b) the exchange and (c) the filter, on every band's stream; a band waits only for the
    // moments of the entries it receives rows from
    for (uint32_t d = 0; d < k; ++d) {
      if (!f->band[d]) continue;
      YK_HIP(hipSetDevice(g->ctx[d]->device));
      const hipStream_t st = g->ctx[d]->stream;
      for (const ykplan::Copy& c : copies)
        if (c.dst == d && c.src != d) YK_HIP(hipStreamWaitEvent(st, ev[(size_t)c.src * kEvents + kM1], 0));
      YK_HIP(hipEventRecord(ev[(size_t)d * kEvents + kX0], st));
      const size_t np_d = (size_t)f->band[d]->npix;
      for (const ykplan::Copy& c : copies) {
        if (c.dst != d) continue;
        const size_t np_s = gf_sub_npix(f, c.src);
        for (int pl = 0; pl < 6; ++pl)
          YK_HIP(hipMemcpy2DAsync(db[d].mv + pl * np_d + (size_t)c.dst_row * wt, (size_t)c.dst_pitch * wt * sizeof(double),
                                  sb[c.src].mv + pl * np_s + (size_t)c.src_row * wt, (size_t)wt * sizeof(double),
                                  (size_t)wt * sizeof(double), c.rows, hipMemcpyDefault, st));
      }
      YK_HIP(hipEventRecord(ev[(size_t)d * kEvents + kX1], st));
      YK_HIP(denoise_band_enqueue(f->band[d], db[d], dp, fp, feat[d], bands[d].begin - bands[d].lo, bands[d].count,
                                  rgb_host != nullptr));
      YK_HIP(hipEventRecord(ev[(size_t)d * kEvents + kF1], st));
    }
    for (uint32_t e = 0; e < k; ++e) {
      if (!f->film[e]) continue;
      YK_HIP(hipSetDevice(g->ctx[e]->device));
      YK_HIP(hipStreamSynchronize(g->ctx[e]->stream));
    }
    // (the counts were checked on the host: the moments' own counters only confirm it)
    for (uint32_t e = 0; e < k; ++e) {
      if (!f->film[e]) continue;
      unsigned long long low = 0;
      YK_HIP(hipSetDevice(g->ctx[e]->device));
      YK_HIP(hipMemcpy(&low, sb[e].low, sizeof low, hipMemcpyDeviceToHost));
      if (low) return entry_fail(e, YK_ERR_INVALID, "denoise needs at least two samples in every pixel");
    }
    // each band into its rows of the caller's arrays
    for (uint32_t d = 0; d < k; ++d) {
      if (!f->band[d]) continue;
      YK_HIP(hipSetDevice(g->ctx[d]->device));
      const size_t off = (size_t)(bands[d].begin - bands[d].lo) * wt * 3, at = (size_t)bands[d].begin * wt * 3;
      const size_t n = (size_t)bands[d].count * wt * 3;
      if (mean_host)
        YK_HIP(hipMemcpyAsync(mean_host + at, db[d].out + off, n * sizeof(double), hipMemcpyDeviceToHost, g->ctx[d]->stream));
      if (rgb_host) YK_HIP(hipMemcpyAsync(rgb_host + at, db[d].rgb + off, n, hipMemcpyDeviceToHost, g->ctx[d]->stream));
    }
    for (uint32_t d = 0; d < k; ++d) {
      if (!f->band[d]) continue;
      YK_HIP(hipSetDevice(g->ctx[d]->device));
      YK_HIP(hipStreamSynchronize(g->ctx[d]->stream));
    }
    if (stats) {
      yk_group_denoise_stats s{};
      for (uint32_t e = 0; e < k; ++e) {
        if (!f->film[e]) continue;
        hipEvent_t* v = &ev[(size_t)e * kEvents];
        float t = 0;
        YK_HIP(hipEventElapsedTime(&t, v[kM0], v[kM1]));
        s.moments_ms = std::max(s.moments_ms, (double)t);
        if (!f->band[e]) continue;
        YK_HIP(hipEventElapsedTime(&t, v[kX0], v[kX1]));
        s.exchange_ms = std::max(s.exchange_ms, (double)t);
        YK_HIP(hipEventElapsedTime(&t, v[kX1], v[kF1]));
        s.filter_ms = std::max(s.filter_ms, (double)t);
      }
      s.features_ms = ms_feat;
      s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      *stats = s;
    }
    return YK_OK;
  };
  const int rc = body();
  if (rc) gf_sync_all(f);  // (nothing of a failed call stays enqueued)
  for (hipEvent_t v : ev)
    if (v) (void)hipEventDestroy(v);
  return rc;
}

}  // namespace

extern "C" {

int ykgpu_group_film_create(ykgpu_group* g, const yk_render_params* params, ykgpu_group_film** out) {
  if (!out) return fail(YK_ERR_INVALID, "null out");
  *out = nullptr;
  if (!g || !params) return fail(YK_ERR_INVALID, "null group or params");
  const uint32_t k = (uint32_t)g->ctx.size();
  yk_render_params p = *params;
  p.flags &= YK_FLAG_LINEAR_SCAN;  // the diagnostic flags are not a film's
  if (int rc = check_params(g->ctx[0], &p)) return rc;
  if (k > 1 && p.row_band_log2 != 0)
    return fail(YK_ERR_UNSUPPORTED, "a group deals single rows: row_band_log2 must be 0");
  if (k > 1 && (uint64_t)p.row_stride * k >= (1ull << 32)) return fail(YK_ERR_INVALID, "row_stride * devices overflows");
  if (p.seed_mode == YK_SEED_RANDOM_DEVICE) {
    // one key for every entry and every chunk: the caller's, or one drawn now
    std::random_device rd;
    while (!p.seed_key) p.seed_key = ((uint64_t)rd() << 32) | rd();
  }
  auto* f = new ykgpu_group_film();
  f->g = g;
  f->p = p;
  f->k = k;
  f->wt = tile_width(&p);
  f->film.assign(k, nullptr);
  f->band.assign(k, nullptr);
  f->rows.assign(k, 0);
  f->gen.assign(k, 0);
  for (uint32_t e = 0; e < k; ++e) {
    f->gen[e] = g->ctx[e]->scene_gen;
    f->rows[e] = p.row_count > e ? (p.row_count - e + k - 1) / k : 0;
    if (!f->rows[e]) continue;
    yk_render_params sub = p;
    if (k > 1) {
      sub.row_begin = p.row_begin + e * p.row_stride;
      sub.row_stride = p.row_stride * k;
      sub.row_count = f->rows[e];
    }
    if (const int rc = ykgpu_film_create(g->ctx[e], &sub, &f->film[e])) {
      const std::string msg = last_error();
      ykgpu_group_film_destroy(f);
      return entry_fail(e, rc, msg);
    }
  }
  *out = f;
  return YK_OK;
}

int ykgpu_group_film_destroy(ykgpu_group_film* f) {
  if (!f) return YK_OK;
  gf_drop_bands(f);
  for (ykgpu_film* film : f->film) ykgpu_film_destroy(film);
  delete f;
  return YK_OK;
}

int ykgpu_group_film_params(const ykgpu_group_film* f, yk_render_params* out) {
  if (!f || !out) return fail(YK_ERR_INVALID, "null argument");
  *out = f->p;
  return YK_OK;
}

int ykgpu_group_film_accumulate(ykgpu_group_film* f, uint32_t n_samples) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = gf_ready(f)) return rc;
  if (int rc = gf_stale(f)) return rc;
  const GroupHist hist = gf_hist(f);
  if (hist.size() > 1)
    return fail(YK_ERR_INVALID,
                "the group film's pixels hold different sample counts: use ykgpu_group_film_accumulate_adaptive");
  if (n_samples == 0) return fail(YK_ERR_INVALID, "n_samples must be > 0");
  if (n_samples > f->p.samples_per_pixel - hist.begin()->first)
    return fail(YK_ERR_INVALID, "the chunk passes the film's target (samples_per_pixel)");
  // every entry's chunk enqueued on its own device before any wait: the devices run together
  f->torn = true;  // (until every entry's chunk is whole)
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (const int rc = film_accumulate_enqueue(f->film[e], n_samples)) {
      const std::string msg = last_error();
      gf_sync_all(f);
      return entry_fail(e, rc, msg);
    }
  }
  // (every entry is waited for, whatever another's fate; the first failure is the call's)
  int bad = YK_OK;
  std::string bad_msg;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    const int rc = film_accumulate_finish(f->film[e], n_samples, t0);
    if (rc && !bad) {
      bad = rc;
      bad_msg = "group film entry " + std::to_string(e) + ": " + last_error();
    }
  }
  if (bad) {
    gf_sync_all(f);
    return fail(bad, bad_msg);
  }
  gf_stats(f, t0);
  f->torn = false;
  return YK_OK;
}

int ykgpu_group_film_accumulate_adaptive(ykgpu_group_film* f, double threshold2, uint32_t n_samples, yk_film_pass* out) {
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = gf_ready(f)) return rc;
  if (int rc = gf_stale(f)) return rc;
  if (n_samples == 0) return fail(YK_ERR_INVALID, "n_samples must be > 0");
  const uint32_t k = f->k;
  std::vector<int> rcs(k, YK_OK);
  std::vector<std::string> msgs(k);
  std::vector<yk_film_pass> pass(k, yk_film_pass{});
  // A pass synchronises with the host between its count groups, so each entry's pass runs on a host
  // thread of its own (which selects the entry's device itself); the last error is per thread, so
  // the threads hand theirs back.  The selection is per pixel: no entry needs another's result.
  const auto run = [&](uint32_t e) {
    rcs[e] = ykgpu_film_accumulate_adaptive(f->film[e], threshold2, n_samples, &pass[e]);
    if (rcs[e]) msgs[e] = last_error();
  };
  std::vector<uint32_t> live;
  for (uint32_t e = 0; e < k; ++e)
    if (f->film[e]) live.push_back(e);
  if (live.size() == 1) {
    run(live[0]);
  } else {
    std::vector<std::thread> th;
    for (uint32_t e : live) th.emplace_back(run, e);
    for (std::thread& t : th) t.join();
  }
  for (uint32_t e : live)
    if (rcs[e]) {
      f->torn = true;  // (the other entries' passes are in: the tile holds part of a pass)
      return entry_fail(e, rcs[e], msgs[e]);
    }
  yk_film_pass sum{};
  for (uint32_t e : live) {
    sum.pixels_selected += pass[e].pixels_selected;
    sum.samples_added += pass[e].samples_added;
    sum.groups += pass[e].groups;
    sum.launches += pass[e].launches;
  }
  const GroupHist hist = gf_hist(f);
  sum.min_count = hist.begin()->first;
  sum.max_count = hist.rbegin()->first;
  gf_stats(f, t0);
  if (out) *out = sum;
  return YK_OK;
}

int ykgpu_group_film_resolve(ykgpu_group_film* f, uint8_t* rgb_host) {
  if (int rc = gf_ready(f)) return rc;
  if (!rgb_host) return fail(YK_ERR_INVALID, "null output");
  const GroupHist hist = gf_hist(f);
  if (hist.size() == 1 && hist.begin()->first < 1)
    return fail(YK_ERR_INVALID, "resolve needs at least one accumulated sample");
  std::vector<uint8_t> sub;
  for (uint32_t e = 0; e < f->k; ++e) {
    ykgpu_film* film = f->film[e];
    if (!film) continue;
    sub.assign(gf_sub_npix(f, e) * 3, 0);
    // (an entry whose pixels all hold no sample, on a film that is not uniform: black)
    if (!(film->uniform() && film->done == 0))
      if (const int rc = ykgpu_film_resolve(film, sub.data())) return entry_fail(e, rc);
    gf_scatter(f, e, sub.data(), rgb_host, 3);
  }
  return YK_OK;
}

int ykgpu_group_film_read(ykgpu_group_film* f, double* sums, double* sumsq, uint32_t* done) {
  if (int rc = gf_ready(f)) return rc;
  if (done) *done = gf_hist(f).begin()->first;
  if (!sums && !sumsq) return YK_OK;
  std::vector<double> a, b;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    a.resize(gf_sub_npix(f, e) * 3);
    b.resize(a.size());
    if (const int rc = ykgpu_film_read(f->film[e], sums ? a.data() : nullptr, sumsq ? b.data() : nullptr, nullptr))
      return entry_fail(e, rc);
    if (sums) gf_scatter(f, e, a.data(), sums, 3);
    if (sumsq) gf_scatter(f, e, b.data(), sumsq, 3);
  }
  return YK_OK;
}

int ykgpu_group_film_write(ykgpu_group_film* f, const double* sums, const double* sumsq, uint32_t done) {
  if (!f || !sums || !sumsq) return fail(YK_ERR_INVALID, "null argument");
  if (done > f->p.samples_per_pixel) return fail(YK_ERR_INVALID, "done passes the film's target (samples_per_pixel)");
  std::vector<double> a, b;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    a.resize(gf_sub_npix(f, e) * 3);
    b.resize(a.size());
    gf_gather(f, e, sums, a.data(), 3);
    gf_gather(f, e, sumsq, b.data(), 3);
    if (const int rc = ykgpu_film_write(f->film[e], a.data(), b.data(), done)) return entry_fail(e, rc);
  }
  f->torn = false;
  return YK_OK;
}

int ykgpu_group_film_counts(ykgpu_group_film* f, uint32_t* counts_host, uint32_t* min_count, uint32_t* max_count) {
  if (int rc = gf_ready(f)) return rc;
  const GroupHist hist = gf_hist(f);
  if (min_count) *min_count = hist.begin()->first;
  if (max_count) *max_count = hist.rbegin()->first;
  if (!counts_host) return YK_OK;
  std::vector<uint32_t> c;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    c.resize(gf_sub_npix(f, e));
    if (const int rc = ykgpu_film_counts(f->film[e], c.data(), nullptr, nullptr)) return entry_fail(e, rc);
    gf_scatter(f, e, c.data(), counts_host, 1);
  }
  return YK_OK;
}

int ykgpu_group_film_write_counts(ykgpu_group_film* f, const double* sums, const double* sumsq, const uint32_t* counts) {
  if (!f || !sums || !sumsq || !counts) return fail(YK_ERR_INVALID, "null argument");
  // (checked for the whole tile first: a refused call changes no entry)
  for (size_t i = 0, n = gf_npix(f); i < n; ++i)
    if (counts[i] > f->p.samples_per_pixel) return fail(YK_ERR_INVALID, "a count passes the film's target (samples_per_pixel)");
  std::vector<double> a, b;
  std::vector<uint32_t> c;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    a.resize(gf_sub_npix(f, e) * 3);
    b.resize(a.size());
    c.resize(gf_sub_npix(f, e));
    gf_gather(f, e, sums, a.data(), 3);
    gf_gather(f, e, sumsq, b.data(), 3);
    gf_gather(f, e, counts, c.data(), 1);
    if (const int rc = ykgpu_film_write_counts(f->film[e], a.data(), b.data(), c.data())) return entry_fail(e, rc);
  }
  f->torn = false;
  return YK_OK;
}

int ykgpu_group_film_error(ykgpu_group_film* f, double threshold2, double* e2_host, yk_film_stats* stats) {
  if (int rc = gf_ready(f)) return rc;
  const GroupHist hist = gf_hist(f);
  if (hist.size() == 1 && hist.begin()->first < 2)
    return fail(YK_ERR_INVALID, "the error map needs at least two accumulated samples");
  const double inf = std::numeric_limits<double>::infinity();
  uint64_t over = 0;
  double top = 0.0;
  std::vector<double> sub;
  for (uint32_t e = 0; e < f->k; ++e) {
    ykgpu_film* film = f->film[e];
    if (!film) continue;
    const size_t n = gf_sub_npix(f, e);
    yk_film_stats st{};
    if (film->uniform() && film->done < 2) {
      // (every pixel of the entry holds fewer than two samples, on a film that is not uniform: +inf)
      sub.assign(n, inf);
      st.pixels_over = inf > threshold2 ? n : 0;
      st.max_e2 = inf;
    } else {
      sub.resize(n);
      if (const int rc = ykgpu_film_error(film, threshold2, e2_host ? sub.data() : nullptr, &st)) return entry_fail(e, rc);
    }
    if (e2_host) gf_scatter(f, e, sub.data(), e2_host, 1);
    over += st.pixels_over;
    top = st.max_e2 > top ? st.max_e2 : top;
  }
  if (stats) {
    stats->pixels = gf_npix(f);
    stats->pixels_over = over;
    stats->max_e2 = top;
    stats->samples_done = hist.begin()->first;
    stats->samples_target = f->p.samples_per_pixel;
  }
  return YK_OK;
}

int ykgpu_group_film_features(ykgpu_group_film* f, uint32_t grid, double* mean_host, double* var_host, double* ms) {
  if (int rc = gf_ready(f)) return rc;
  if (grid < 1 || grid > 4) return fail(YK_ERR_INVALID, "features: grid must be 1..4");
  if (int rc = gf_stale(f)) return rc;
  const bool want = mean_host || var_host;
  std::vector<std::vector<double>> m(f->k), v(f->k);
  double t_max = 0;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (want) {
      m[e].resize(gf_sub_npix(f, e) * 7);
      v[e].resize(m[e].size());
    }
    double t = 0;
    if (const int rc = ykgpu_film_features(f->film[e], grid, want ? m[e].data() : nullptr, want ? v[e].data() : nullptr, &t))
      return entry_fail(e, rc);
    t_max = std::max(t_max, t);
  }
  // (the caller's arrays are written only once every entry's pass is in)
  for (uint32_t e = 0; want && e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (mean_host) gf_scatter(f, e, m[e].data(), mean_host, 7);
    if (var_host) gf_scatter(f, e, v[e].data(), var_host, 7);
  }
  if (ms) *ms = t_max;
  return YK_OK;
}

int ykgpu_group_film_denoise(ykgpu_group_film* f, const yk_denoise_params* params, double* mean_host, uint8_t* rgb_host,
                             yk_group_denoise_stats* stats) {
  yk_denoise_params dp;
  yk_denoise_defaults(&dp);
  if (params) dp = *params;
  return gf_denoise(f, dp, nullptr, 0, mean_host, rgb_host, stats);
}

int ykgpu_group_film_denoise_guided(ykgpu_group_film* f, const yk_denoise_params* colour, const yk_feature_params* feat,
                                    double* mean_host, uint8_t* rgb_host, yk_group_denoise_stats* stats) {
  yk_denoise_params dp;
  yk_feature_params fp;
  yk_guided_defaults(&dp, &fp);
  if (colour) dp = *colour;
  if (feat) fp = *feat;
  return gf_denoise(f, dp, &fp, 0, mean_host, rgb_host, stats);
}

int ykgpu_group_film_features_sampled(ykgpu_group_film* f, uint32_t n_samples, double* mean_host, double* var_host,
                                      yk_sampled_features_stats* stats) {
  if (int rc = gf_ready(f)) return rc;
  if (int rc = gf_check_n(f, n_samples)) return rc;
  if (int rc = gf_stale(f)) return rc;
  const bool want = mean_host || var_host;
  std::vector<std::vector<double>> m(f->k), v(f->k);
  yk_sampled_features_stats sum{};
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (want) {
      m[e].resize(gf_sub_npix(f, e) * 7);
      v[e].resize(m[e].size());
    }
    yk_sampled_features_stats st{};
    if (const int rc = ykgpu_film_features_sampled(f->film[e], n_samples, want ? m[e].data() : nullptr,
                                                   want ? v[e].data() : nullptr, &st))
      return entry_fail(e, rc);
    sum.ms = std::max(sum.ms, st.ms);
    sum.samples += st.samples;
    sum.hits += st.hits;
    sum.redo_pixels += st.redo_pixels;
  }
  // (the caller's arrays are written only once every entry's pass is in)
  for (uint32_t e = 0; want && e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (mean_host) gf_scatter(f, e, m[e].data(), mean_host, 7);
    if (var_host) gf_scatter(f, e, v[e].data(), var_host, 7);
  }
  if (stats) *stats = sum;
  return YK_OK;
}

int ykgpu_group_film_denoise_guided_sampled(ykgpu_group_film* f, const yk_denoise_params* colour,
                                            const yk_feature_params* feat, uint32_t n_samples, double* mean_host,
                                            uint8_t* rgb_host, yk_group_denoise_stats* stats) {
  yk_denoise_params dp;
  yk_feature_params fp;
  yk_guided_sampled_defaults(&dp, &fp, nullptr);
  if (colour) dp = *colour;
  if (feat) fp = *feat;
  fp.grid = 1;  // (not read, so not validated)
  if (int rc = gf_ready(f)) return rc;
  if (int rc = gf_check_n(f, n_samples)) return rc;
  return gf_denoise(f, dp, &fp, n_samples, mean_host, rgb_host, stats);
}

// The film mattes (include/ykgpu.h "film mattes"): a pixel's table depends on that pixel alone, so
// each entry runs the single film's call on the rows it was dealt and no halo is needed.
int ykgpu_group_film_mattes(ykgpu_group_film* f, uint32_t n_samples, yk_matte_pixel* table_host, yk_matte_stats* stats) {
  if (int rc = gf_ready(f)) return rc;
  if (n_samples > f->p.samples_per_pixel) return fail(YK_ERR_INVALID, "mattes: n_samples is larger than the film's target");
  if (int rc = gf_stale(f)) return rc;
  std::vector<std::vector<yk_matte_pixel>> t(f->k);
  yk_matte_stats sum{};
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (table_host) t[e].resize(gf_sub_npix(f, e));
    yk_matte_stats st{};
    if (const int rc = ykgpu_film_mattes(f->film[e], n_samples, table_host ? t[e].data() : nullptr, &st))
      return entry_fail(e, rc);
    sum.ms = std::max(sum.ms, st.ms);
    sum.samples += st.samples;
    sum.hits += st.hits;
    sum.other_samples += st.other_samples;
    sum.overflow_pixels += st.overflow_pixels;
    sum.redo_pixels += st.redo_pixels;
  }
  // (the caller's array is written only once every entry's pass is in)
  for (uint32_t e = 0; table_host && e < f->k; ++e)
    if (f->film[e]) gf_scatter(f, e, t[e].data(), table_host, 1);
  if (stats) *stats = sum;
  return YK_OK;
}

int ykgpu_group_film_matte_coverage(ykgpu_group_film* f, const uint32_t* ids, uint32_t n_ids, double* cov_host,
                                    uint8_t* grey_host, yk_matte_coverage_stats* stats) {
  if (int rc = gf_ready(f)) return rc;
  std::vector<std::vector<double>> c(f->k);
  std::vector<std::vector<uint8_t>> g(f->k);
  yk_matte_coverage_stats sum{};
  bool any = false;
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    any = true;
    if (cov_host) c[e].resize(gf_sub_npix(f, e));
    if (grey_host) g[e].resize(gf_sub_npix(f, e));
    yk_matte_coverage_stats st{};
    // (the entries hold tables of the same call and the same scene: a refusal is the first entry's)
    if (const int rc = ykgpu_film_matte_coverage(f->film[e], ids, n_ids, cov_host ? c[e].data() : nullptr,
                                                 grey_host ? g[e].data() : nullptr, &st))
      return entry_fail(e, rc);
    sum.ms = std::max(sum.ms, st.ms);
    sum.pixels_selected += st.pixels_selected;
    sum.pixels_uncertain += st.pixels_uncertain;
    sum.samples_selected += st.samples_selected;
  }
  if (!any) return fail(YK_ERR_INVALID, "matte coverage: the film holds no matte table");
  for (uint32_t e = 0; e < f->k; ++e) {
    if (!f->film[e]) continue;
    if (cov_host) gf_scatter(f, e, c[e].data(), cov_host, 1);
    if (grey_host) gf_scatter(f, e, g[e].data(), grey_host, 1);
  }
  if (stats) *stats = sum;
  return YK_OK;
}

}  // extern "C"

#endif
