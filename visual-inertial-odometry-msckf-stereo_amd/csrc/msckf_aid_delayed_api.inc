// msckf_aid_delayed_api.inc -- host side of include/msckf_aid_delayed.h: the argument checks, the lazy workspace, the
// call's one input block and two launches, and the read of the records.  Included by msckf_api.hip behind
// msckf_map_api.inc, whose block helpers it uses.

namespace {

// The workspace and the records, made by the first msckf_aid_delayed_batch of the context.
int aid_delayed_ensure(msckf_ctx* c) {
    auto& z = c->aid_delayed;
    if (z.on) return 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t B = (size_t)c->B;
    const size_t b_w = al(B * c->Dmax * ADL_WS * sizeof(double)), b_app = al(B * sizeof(int)), b_gam = al(B * 8),
                 b_sta = al(B * sizeof(int)), b_row = al(B * sizeof(int)), b_cnt = al(B * 8);
    HIPC(z.store.ensure(b_w + b_app + b_gam + b_sta + b_row + b_cnt));
    unsigned char* p = z.store.p;
    z.dev.W = reinterpret_cast<double*>(p);
    z.dev.applied = reinterpret_cast<int*>(p + b_w);
    z.dev.gamma = reinterpret_cast<double*>(p + b_w + b_app);
    z.dev.status = reinterpret_cast<int*>(p + b_w + b_app + b_gam);
    z.dev.rows = reinterpret_cast<int*>(p + b_w + b_app + b_gam + b_sta);
    z.dev.count = reinterpret_cast<long long*>(p + b_w + b_app + b_gam + b_sta + b_row);
    // records: applied = 0, gamma = NaN and status = NONE = -1 (all bits set), rows = 0, count = 0; W is written
    // before it is read
    HIPC(hipMemsetAsync(z.dev.applied, 0, b_app, c->stream));
    HIPC(hipMemsetAsync(z.dev.gamma, 0xff, b_gam + b_sta, c->stream));
    HIPC(hipMemsetAsync(z.dev.rows, 0, b_row + b_cnt, c->stream));
    z.on = true;
    return 0;
}

template <typename T>
int do_aid_delayed_batch(msckf_ctx* c, int nfilt, const int32_t* filters, const msckf_aid_delayed_fix_t* fixes,
                         const msckf_aid_params_t& prm) {
    if (int r = aid_delayed_ensure(c)) return r;
    int maxD = 21;
    for (int w = 0; w < nfilt; ++w) maxD = std::max(maxD, 21 + 6 * c->h_ncams[filters[w]]);
    MapBlock blk;
    const size_t o_fl = blk.add(filters, (size_t)nfilt * sizeof(int));
    const size_t o_fx = blk.add(fixes, (size_t)nfilt * sizeof(msckf_aid_delayed_fix_t));
    if (int r = map_send(c, c->aid_delayed.in, blk)) return r;
    const int* dfl = reinterpret_cast<const int*>(c->aid_delayed.in.p + o_fl);
    c->timer.begin(c->stream, "aid_delayed_gain");
    launch_aid_delayed_gain<T>(c->stream, dev_state<T>(c), c->aid_delayed.dev, prm, nfilt, dfl,
                               reinterpret_cast<const msckf_aid_delayed_fix_t*>(c->aid_delayed.in.p + o_fx));
    c->timer.end(c->stream);
    HIPC(hipGetLastError());
    c->timer.begin(c->stream, "aid_delayed_apply");
    launch_aid_delayed_apply<T>(c->stream, dev_state<T>(c), c->aid_delayed.dev, nfilt, dfl, maxD);
    c->timer.end(c->stream);
    HIPC(hipGetLastError());   // asynchronous: the next synchronising call waits for it
    return 0;
}

}  // namespace

extern "C" {

int msckf_aid_delayed_batch(msckf_ctx_t* c, int nfilt, const int32_t* filters, const msckf_aid_delayed_fix_t* fixes,
                            const msckf_aid_params_t* prm) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    if (!prm || (nfilt > 0 && !fixes)) FAIL(-1, "null argument");
    int kept = 0;   // the union of the fixes' masks
    for (int w = 0; w < nfilt; ++w) {
        const msckf_aid_delayed_fix_t& fx = fixes[w];
        if (fx.rows == 0 || (fx.rows & ~0x3f)) FAIL(-1, "fix %d: bad row mask %d (a non-empty subset of 0x3f)", w, fx.rows);
        if (!(fx.lambda >= 0.0 && fx.lambda < 1.0)) FAIL(-1, "fix %d: lambda = %g must be in [0, 1)", w, fx.lambda);
        if (fx.slot < 0 || fx.slot >= c->Nmax)
            FAIL(-1, "fix %d: slot %d is outside the cam capacity %d", w, fx.slot, c->Nmax);
        int m = 0;
        for (int g = 0; g < ADL_M; ++g) {
            if (!((fx.rows >> g) & 1)) continue;
            ++m;
            if (!(fx.var[g] > 0.0)) FAIL(-1, "fix %d: var[%d] = %g: a variance must be > 0", w, g, fx.var[g]);
            if (std::isnan(fx.z[g])) FAIL(-1, "fix %d: z[%d] is NaN", w, g);
        }
        if (std::isnan(prm->chi2[m - 1])) FAIL(-1, "chi2[%d] is NaN and fix %d keeps %d rows", m - 1, w, m);
        kept |= fx.rows;
    }
    if (kept & MSCKF_AID_DELAYED_DIR) {
        const double* d = prm->dir_w;
        const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(std::fabs(n - 1.0) <= 1e-6)) FAIL(-1, "|dir_w| = %g is not 1 to 1e-6", n);
    }
    if (nfilt == 0) return 1;
    c->last_async = "msckf_aid_delayed_batch";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_aid_delayed_batch, c, nfilt, filters, fixes, *prm);
}

int msckf_aid_delayed_results(msckf_ctx_t* c, int nfilt, const int32_t* filters, int32_t* applied, double* gamma,
                              int32_t* rows, int32_t* status, int64_t* count) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    if (!c->aid_delayed.on) {   // no fix was ever enqueued: the records' initial values, no allocation
        HIPSYNC(c, hipStreamSynchronize(c->stream));
        for (int w = 0; w < nfilt; ++w) {
            if (applied) applied[w] = 0;
            if (gamma) gamma[w] = std::nan("");
            if (rows) rows[w] = 0;
            if (status) status[w] = MSCKF_AID_DELAYED_NONE;
            if (count) count[w] = 0;
        }
        return 0;
    }
    const auto& z = c->aid_delayed.dev;
    const size_t B = (size_t)c->B;
    DownList d;
    const size_t o_app = d.add(z.applied, B * sizeof(int)), o_gam = d.add(z.gamma, B * 8),
                 o_row = d.add(z.rows, B * sizeof(int)), o_sta = d.add(z.status, B * sizeof(int)),
                 o_cnt = d.add(z.count, B * 8);
    HIPSYNC(c, d.run(c));
    const int* r_app = reinterpret_cast<const int*>(d.at(c, o_app));
    const double* r_gam = reinterpret_cast<const double*>(d.at(c, o_gam));
    const int* r_row = reinterpret_cast<const int*>(d.at(c, o_row));
    const int* r_sta = reinterpret_cast<const int*>(d.at(c, o_sta));
    const long long* r_cnt = reinterpret_cast<const long long*>(d.at(c, o_cnt));
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (applied) applied[w] = r_app[f];
        if (gamma) gamma[w] = r_gam[f];
        if (rows) rows[w] = r_row[f];
        if (status) status[w] = r_sta[f];
        if (count) count[w] = (int64_t)r_cnt[f];
    }
    return 0;
}

}  // extern "C"
