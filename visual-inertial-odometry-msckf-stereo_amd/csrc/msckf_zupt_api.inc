// msckf_zupt_api.inc -- host side of include/msckf_zupt.h: the argument checks, the lazy workspace, the call's one
// input block and two launches, and the read of the records.  Included by msckf_api.hip behind msckf_map_api.inc,
// whose block helpers it uses.

namespace {

// The workspace and the records, made by the first msckf_zupt_batch of the context.
int zupt_ensure(msckf_ctx* c) {
    auto& z = c->zupt;
    if (z.on) return 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t B = (size_t)c->B;
    const size_t b_w = al(B * c->Dmax * ZUPT_M * sizeof(double)), b_app = al(B * sizeof(int)), b_gam = al(B * 8),
                 b_cnt = al(B * 8);
    HIPC(z.store.ensure(b_w + b_app + b_gam + b_cnt));
    unsigned char* p = z.store.p;
    z.dev.W = reinterpret_cast<double*>(p);
    z.dev.applied = reinterpret_cast<int*>(p + b_w);
    z.dev.gamma = reinterpret_cast<double*>(p + b_w + b_app);
    z.dev.count = reinterpret_cast<long long*>(p + b_w + b_app + b_gam);
    // records: applied = 0, gamma = NaN (all bits set), count = 0; W is written before it is read
    HIPC(hipMemsetAsync(z.dev.applied, 0, b_app, c->stream));
    HIPC(hipMemsetAsync(z.dev.gamma, 0xff, b_gam, c->stream));
    HIPC(hipMemsetAsync(z.dev.count, 0, b_cnt, c->stream));
    z.on = true;
    return 0;
}

template <typename T>
int do_zupt_batch(msckf_ctx* c, int nfilt, const int32_t* filters, const double* gyro_mean, const double* acc_mean,
                  const ZuptArgs& a) {
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
    if (int r = map_send(c, c->zupt.in, blk)) return r;
    const int* dfl = reinterpret_cast<const int*>(c->zupt.in.p + o_fl);
    c->timer.begin(c->stream, "zupt_gain");
    launch_zupt_gain<T>(c->stream, dev_state<T>(c), c->zupt.dev, a, nfilt, dfl,
                        reinterpret_cast<const double*>(c->zupt.in.p + o_mn));
    c->timer.end(c->stream);
    HIPC(hipGetLastError());
    c->timer.begin(c->stream, "zupt_apply");
    launch_zupt_apply<T>(c->stream, dev_state<T>(c), c->zupt.dev, a.m, nfilt, dfl, maxD);
    c->timer.end(c->stream);
    HIPC(hipGetLastError());   // asynchronous: the next synchronising call waits for it
    return 0;
}

}  // namespace

extern "C" {

int msckf_zupt_batch(msckf_ctx_t* c, int nfilt, const int32_t* filters, const double* gyro_mean,
                     const double* acc_mean, const msckf_zupt_params_t* prm) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    if (!prm || (nfilt > 0 && (!gyro_mean || !acc_mean))) FAIL(-1, "null argument");
    const int all = MSCKF_ZUPT_VEL | MSCKF_ZUPT_GYRO | MSCKF_ZUPT_ACC;
    if (prm->rows == 0 || (prm->rows & ~all)) FAIL(-1, "bad row mask %d (a non-empty subset of %d)", prm->rows, all);
    ZuptArgs a{};
    a.noise[0] = prm->vel_noise, a.noise[1] = prm->gyro_noise, a.noise[2] = prm->acc_noise;
    static const char* group[3] = {"vel", "gyro", "acc"};
    for (int g = 0; g < 3; ++g)
        if (!(a.noise[g] > 0.0))
            FAIL(-1, "%s_noise = %g: a variance must be > 0", group[g], a.noise[g]);
    if (std::isnan(prm->chi2)) FAIL(-1, "chi2 is NaN");
    if (!(prm->max_speed >= 0.0)) FAIL(-1, "max_speed = %g must be >= 0", prm->max_speed);
    a.chi2 = prm->chi2, a.max_speed = prm->max_speed, a.rows = prm->rows;
    a.m = 3 * (((prm->rows >> 0) & 1) + ((prm->rows >> 1) & 1) + ((prm->rows >> 2) & 1));
    if (nfilt == 0) return 1;
    c->last_async = "msckf_zupt_batch";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_zupt_batch, c, nfilt, filters, gyro_mean, acc_mean, a);
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
