// msckf_zupt_api.inc -- host side of include/msckf_zupt.h and of the cued update of include/msckf_standstill.h: the
// argument checks, the lazy workspace, the call's one input block and two launches, and the read of the records.  Included by msckf_api.hip behind msckf_map_api.inc,
// whose block helpers it uses.

namespace {

// The workspace and the records, made by the first msckf_zupt_batch of the context.
int zupt_ensure(msckf_ctx* c) {
    auto& z = c->zupt;
    if (z.on) return 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t B = (size_t)c->B;
    const size_t b_w = al(B * c->Dmax * ZUPT_M * sizeof(double)), b_app = al(B * sizeof(int)), b_gam = al(B * 8),
                 b_cnt = al(B * 8), b_cue = al(B * 4);
    HIPC(z.store.ensure(b_w + b_app + b_gam + b_cnt + 3 * b_cue));
    unsigned char* p = z.store.p;
    z.dev.W = reinterpret_cast<double*>(p);
    z.dev.applied = reinterpret_cast<int*>(p + b_w);
    z.dev.gamma = reinterpret_cast<double*>(p + b_w + b_app);
    z.dev.count = reinterpret_cast<long long*>(p + b_w + b_app + b_gam);
    z.dev.cue = reinterpret_cast<int*>(p + b_w + b_app + b_gam + b_cnt);
    z.dev.cue_n = reinterpret_cast<int*>(p + b_w + b_app + b_gam + b_cnt + b_cue);
    z.dev.cue_d2 = reinterpret_cast<float*>(p + b_w + b_app + b_gam + b_cnt + 2 * b_cue);
    // records: applied = 0, gamma = NaN (all bits set), count = 0; W is written before it is read
    HIPC(hipMemsetAsync(z.dev.applied, 0, b_app, c->stream));
    HIPC(hipMemsetAsync(z.dev.gamma, 0xff, b_gam, c->stream));
    HIPC(hipMemsetAsync(z.dev.count, 0, b_cnt, c->stream));
    // the cue records (msckf_standstill.h): cue = -1, cue_n = -1, cue_d2 = NaN (all bits set)
    HIPC(hipMemsetAsync(z.dev.cue, 0xff, 3 * b_cue, c->stream));
    z.on = true;
    return 0;
}

// The cue of a cued call (msckf_standstill.h) as do_zupt_batch takes it; null for msckf_zupt_batch.
struct ZuptCueHost {
    ZuptCueArgs q;           // the parameters, and rec for the device source
    const int32_t* head;     // [nfilt]: the lanes (-1: no valid record), or cue_n
    const float* d2;         // [nfilt], host source only
};

template <typename T>
int do_zupt_batch(msckf_ctx* c, int nfilt, const int32_t* filters, const double* gyro_mean, const double* acc_mean,
                  const ZuptArgs& a, const ZuptCueHost* cue) {
    if (int r = zupt_ensure(c)) return r;
    std::vector<double> means((size_t)nfilt * 6);
    int maxD = 21;
    for (int w = 0; w < nfilt; ++w) {
        for (int i = 0; i < 3; ++i) means[6 * w + i] = gyro_mean[3 * w + i], means[6 * w + 3 + i] = acc_mean[3 * w + i];
        maxD = std::max(maxD, 21 + 6 * c->h_ncams[filters[w]]);
    }
    MapBlock blk;
    const size_t o_fl = blk.add(filters, (size_t)nfilt * sizeof(int));
    const size_t o_mn = blk.add(means.data(), means.size() * sizeof(double));
    size_t o_hd = 0, o_d2 = 0;
    if (cue) {
        o_hd = blk.add(cue->head, (size_t)nfilt * sizeof(int));
        if (cue->d2) o_d2 = blk.add(cue->d2, (size_t)nfilt * sizeof(float));
    }
    if (int r = map_send(c, c->zupt.in, blk)) return r;
    const int* dfl = reinterpret_cast<const int*>(c->zupt.in.p + o_fl);
    const double* dmn = reinterpret_cast<const double*>(c->zupt.in.p + o_mn);
    if (cue) {
        ZuptCueArgs q = cue->q;
        const int* dhd = reinterpret_cast<const int*>(c->zupt.in.p + o_hd);
        if (q.rec) {
            q.lane = dhd;
        } else {
            q.n = dhd;
            q.d2 = reinterpret_cast<const float*>(c->zupt.in.p + o_d2);
        }
        c->timer.begin(c->stream, "zupt_gain_cued");
        launch_zupt_gain_cued<T>(c->stream, dev_state<T>(c), c->zupt.dev, a, q, nfilt, dfl, dmn);
    } else {
        c->timer.begin(c->stream, "zupt_gain");
        launch_zupt_gain<T>(c->stream, dev_state<T>(c), c->zupt.dev, a, nfilt, dfl, dmn);
    }
    c->timer.end(c->stream);
    HIPC(hipGetLastError());
    c->timer.begin(c->stream, "zupt_apply");
    launch_zupt_apply<T>(c->stream, dev_state<T>(c), c->zupt.dev, a.m, nfilt, dfl, maxD);
    c->timer.end(c->stream);
    HIPC(hipGetLastError());   // asynchronous: the next synchronising call waits for it
    return 0;
}

// the checks msckf_zupt_batch and msckf_zupt_batch_cued share; fills a
int zupt_check(msckf_ctx* c, int nfilt, const int32_t* filters, const double* gyro_mean, const double* acc_mean,
               const msckf_zupt_params_t* prm, ZuptArgs& a) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    if (!prm || (nfilt > 0 && (!gyro_mean || !acc_mean))) FAIL(-1, "null argument");
    const int all = MSCKF_ZUPT_VEL | MSCKF_ZUPT_GYRO | MSCKF_ZUPT_ACC;
    if (prm->rows == 0 || (prm->rows & ~all)) FAIL(-1, "bad row mask %d (a non-empty subset of %d)", prm->rows, all);
    a.noise[0] = prm->vel_noise, a.noise[1] = prm->gyro_noise, a.noise[2] = prm->acc_noise;
    static const char* group[3] = {"vel", "gyro", "acc"};
    for (int g = 0; g < 3; ++g)
        if (!(a.noise[g] > 0.0))
            FAIL(-1, "%s_noise = %g: a variance must be > 0", group[g], a.noise[g]);
    if (std::isnan(prm->chi2)) FAIL(-1, "chi2 is NaN");
    if (!(prm->max_speed >= 0.0)) FAIL(-1, "max_speed = %g must be >= 0", prm->max_speed);
    a.chi2 = prm->chi2, a.max_speed = prm->max_speed, a.rows = prm->rows;
    a.m = 3 * (((prm->rows >> 0) & 1) + ((prm->rows >> 1) & 1) + ((prm->rows >> 2) & 1));
    return 0;
}

}  // namespace

extern "C" {

int msckf_zupt_batch(msckf_ctx_t* c, int nfilt, const int32_t* filters, const double* gyro_mean,
                     const double* acc_mean, const msckf_zupt_params_t* prm) {
    ZuptArgs a{};
    if (int r = zupt_check(c, nfilt, filters, gyro_mean, acc_mean, prm, a)) return r;
    if (nfilt == 0) return 1;
    c->last_async = "msckf_zupt_batch";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_zupt_batch, c, nfilt, filters, gyro_mean, acc_mean, a, (const ZuptCueHost*)nullptr);
}

int msckf_zupt_batch_cued(msckf_ctx_t* c, mfe_ctx_t* fe, int nfilt, const int32_t* filters, const int32_t* lanes,
                          const int32_t* cue_n, const float* cue_d2, const double* gyro_mean, const double* acc_mean,
                          const msckf_zupt_params_t* prm, const msckf_zupt_cue_t* cue) {
    ZuptArgs a{};
    if (int r = zupt_check(c, nfilt, filters, gyro_mean, acc_mean, prm, a)) return r;
    if (!cue) FAIL(-1, "null cue");
    if (!(cue->max_px >= 0.0)) FAIL(-1, "max_px = %g must be >= 0", cue->max_px);
    if (cue->min_tracks < 1) FAIL(-1, "min_tracks = %d must be >= 1", cue->min_tracks);
    if (cue->mode != MSCKF_CUE_MODE_VETO && cue->mode != MSCKF_CUE_MODE_EITHER) FAIL(-1, "unknown cue mode %d", cue->mode);
    if (cue->unknown != MSCKF_CUE_UNKNOWN_IMU && cue->unknown != MSCKF_CUE_UNKNOWN_REJECT)
        FAIL(-1, "unknown policy %d for a frame without a cue", cue->unknown);
    ZuptCueHost hc{};
    hc.q.max_px2 = cue->max_px * cue->max_px;
    hc.q.min_tracks = cue->min_tracks, hc.q.mode = cue->mode, hc.q.unknown = cue->unknown;
    std::vector<int32_t> head;
    if (fe) {   // the lanes' records where they lie; an invalid one travels as lane -1 (UNKNOWN)
        TrackMotionView v;
        if (!mfe_track_motion(fe, v)) FAIL(-1, "the front-end context has no track tables (mfe_tracks_create)");
        if (v.device != c->device)
            FAIL(-1, "the front-end context is on device %d, the filter context on device %d", v.device, c->device);
        if (nfilt > 0 && !lanes) FAIL(-1, "null lanes");
        head.resize(nfilt);
        for (int w = 0; w < nfilt; ++w) {
            const int l = lanes[w];
            if (l < 0 || l >= v.n_lanes) FAIL(-1, "lanes[%d] = %d outside [0, %d)", w, l, v.n_lanes);
            for (int j = 0; j < w; ++j)
                if (lanes[j] == l) FAIL(-1, "lane %d is named twice (entries %d and %d)", l, j, w);
            head[w] = v.valid[l] ? l : -1;
        }
        hc.q.rec = v.rec;
        hc.head = head.data();
    } else {
        if (nfilt > 0 && (!cue_n || !cue_d2)) FAIL(-1, "null cue array (no front-end context was given)");
        hc.head = cue_n;
        hc.d2 = cue_d2;
    }
    if (nfilt == 0) return 1;
    c->last_async = "msckf_zupt_batch_cued";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_zupt_batch, c, nfilt, filters, gyro_mean, acc_mean, a, (const ZuptCueHost*)&hc);
}

int msckf_zupt_cue_results(msckf_ctx_t* c, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                           int64_t* count, int32_t* cue, int32_t* cue_n, float* cue_d2) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    if (!c->zupt.on) {   // no update was ever enqueued: the records' initial values, no allocation
        HIPSYNC(c, hipStreamSynchronize(c->stream));
        for (int w = 0; w < nfilt; ++w) {
            if (applied) applied[w] = 0;
            if (gamma) gamma[w] = std::nan("");
            if (count) count[w] = 0;
            if (cue) cue[w] = -1;
            if (cue_n) cue_n[w] = -1;
            if (cue_d2) cue_d2[w] = std::nanf("");
        }
        return 0;
    }
    const auto& z = c->zupt.dev;
    const size_t B = (size_t)c->B;
    DownList d;
    const size_t o_app = d.add(z.applied, B * sizeof(int)), o_gam = d.add(z.gamma, B * 8), o_cnt = d.add(z.count, B * 8),
                 o_cue = d.add(z.cue, B * 4), o_n = d.add(z.cue_n, B * 4), o_d2 = d.add(z.cue_d2, B * 4);
    HIPSYNC(c, d.run(c));   // one read for the six records
    const int* r_app = reinterpret_cast<const int*>(d.at(c, o_app));
    const double* r_gam = reinterpret_cast<const double*>(d.at(c, o_gam));
    const long long* r_cnt = reinterpret_cast<const long long*>(d.at(c, o_cnt));
    const int* r_cue = reinterpret_cast<const int*>(d.at(c, o_cue));
    const int* r_n = reinterpret_cast<const int*>(d.at(c, o_n));
    const float* r_d2 = reinterpret_cast<const float*>(d.at(c, o_d2));
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (applied) applied[w] = r_app[f];
        if (gamma) gamma[w] = r_gam[f];
        if (count) count[w] = (int64_t)r_cnt[f];
        if (cue) cue[w] = r_cue[f];
        if (cue_n) cue_n[w] = r_n[f];
        if (cue_d2) cue_d2[w] = r_d2[f];
    }
    return 0;
}

int msckf_zupt_results(msckf_ctx_t* c, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                       int64_t* count) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    if (!c->zupt.on) {   // no update was ever enqueued: the records' initial values, no allocation
        HIPSYNC(c, hipStreamSynchronize(c->stream));
        for (int w = 0; w < nfilt; ++w) {
            if (applied) applied[w] = 0;
            if (gamma) gamma[w] = std::nan("");
            if (count) count[w] = 0;
        }
        return 0;
    }
    const auto& z = c->zupt.dev;
    const size_t B = (size_t)c->B;
    DownList d;
    const size_t o_app = d.add(z.applied, B * sizeof(int)), o_gam = d.add(z.gamma, B * 8), o_cnt = d.add(z.count, B * 8);
    HIPSYNC(c, d.run(c));
    const int* r_app = reinterpret_cast<const int*>(d.at(c, o_app));
    const double* r_gam = reinterpret_cast<const double*>(d.at(c, o_gam));
    const long long* r_cnt = reinterpret_cast<const long long*>(d.at(c, o_cnt));
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (applied) applied[w] = r_app[f];
        if (gamma) gamma[w] = r_gam[f];
        if (count) count[w] = (int64_t)r_cnt[f];
    }
    return 0;
}

}  // extern "C"
