// msckf_anchor_api.inc -- host side of include/msckf_anchor.h: the argument checks, the lazy workspace, the call's
// one input block and two launches, and the reads of the records.  Included by msckf_api.hip behind
// msckf_map_api.inc, whose block helpers it uses.

namespace {

// The workspace and the records, made by the first msckf_anchor_batch of the context.
int anchor_ensure(msckf_ctx* c) {
    auto& z = c->anchor;
    if (z.on) return 0;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t B = (size_t)c->B;
    const size_t b_w = al(B * c->Dmax * ANC_M * sizeof(double)), b_int = al(B * sizeof(int)), b_cnt = al(B * 8),
                 b_gam = al(B * ANC_K * 8), b_st = al(B * ANC_K);
    HIPC(z.store.ensure(b_w + 4 * b_int + b_cnt + b_gam + b_st));
    unsigned char* p = z.store.p;
    z.dev.W = reinterpret_cast<double*>(p);
    z.dev.gamma = reinterpret_cast<double*>(p + b_w);
    z.dev.count = reinterpret_cast<long long*>(p + b_w + b_gam);
    z.dev.applied = reinterpret_cast<int*>(p + b_w + b_gam + b_cnt);
    z.dev.used = reinterpret_cast<int*>(p + b_w + b_gam + b_cnt + b_int);
    z.dev.rows = reinterpret_cast<int*>(p + b_w + b_gam + b_cnt + 2 * b_int);
    z.dev.n = reinterpret_cast<int*>(p + b_w + b_gam + b_cnt + 3 * b_int);
    z.dev.status = p + b_w + b_gam + b_cnt + 4 * b_int;
    // records: applied = used = rows = count = 0 and no per-anchor entries (n = 0); W is written before it is read
    HIPC(hipMemsetAsync(p + b_w, 0, b_gam + b_cnt + 4 * b_int + b_st, c->stream));
    z.on = true;
    return 0;
}

template <typename T>
int do_anchor_batch(msckf_ctx* c, int nfilt, const int32_t* filters, const int32_t* off, const msckf_anchor_t* anchors,
                    const msckf_anchor_params_t& prm) {
    if (int r = anchor_ensure(c)) return r;
    int maxD = 21;
    for (int w = 0; w < nfilt; ++w) maxD = std::max(maxD, 21 + 6 * c->h_ncams[filters[w]]);
    AnchorPrm a{};
    a.obs_var = prm.obs_var, a.chi2 = prm.chi2, a.min_depth = prm.min_depth, a.min_anchors = prm.min_anchors;
    for (int i = 0; i < 9; ++i) a.R_cc[i] = c->cfg.R_cam0_cam1[i];
    for (int i = 0; i < 3; ++i) a.t_cc[i] = c->cfg.t_cam0_cam1[i];
    MapBlock blk;
    const size_t o_fl = blk.add(filters, (size_t)nfilt * sizeof(int));
    const size_t o_of = blk.add(off, (size_t)(nfilt + 1) * sizeof(int));
    const size_t o_an = blk.add(anchors, (size_t)off[nfilt] * sizeof(msckf_anchor_t));
    if (int r = map_send(c, c->anchor.in, blk)) return r;
    const int* dfl = reinterpret_cast<const int*>(c->anchor.in.p + o_fl);
    c->timer.begin(c->stream, "anchor_gain");
    launch_anchor_gain<T>(c->stream, dev_state<T>(c), c->anchor.dev, a, nfilt, dfl,
                          reinterpret_cast<const int*>(c->anchor.in.p + o_of),
                          reinterpret_cast<const msckf_anchor_t*>(c->anchor.in.p + o_an));
    c->timer.end(c->stream);
    HIPC(hipGetLastError());
    c->timer.begin(c->stream, "anchor_apply");
    launch_anchor_apply<T>(c->stream, dev_state<T>(c), c->anchor.dev, nfilt, dfl, maxD);
    c->timer.end(c->stream);
    HIPC(hipGetLastError());   // asynchronous: the next synchronising call waits for it
    return 0;
}

}  // namespace

extern "C" {

int msckf_anchor_batch(msckf_ctx_t* c, int nfilt, const int32_t* filters, const int32_t* off,
                       const msckf_anchor_t* anchors, const msckf_anchor_params_t* prm) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    if (!prm || !off) FAIL(-1, "null argument");
    if (!(prm->obs_var > 0.0) || !std::isfinite(prm->obs_var)) FAIL(-1, "obs_var = %g must be > 0", prm->obs_var);
    if (!(prm->min_depth > 0.0) || !std::isfinite(prm->min_depth)) FAIL(-1, "min_depth = %g must be > 0", prm->min_depth);
    if (prm->min_anchors < 1) FAIL(-1, "min_anchors = %d must be >= 1", prm->min_anchors);
    if (std::isnan(prm->chi2)) FAIL(-1, "chi2 is NaN");
    if (off[0] != 0) FAIL(-1, "off[0] = %d must be 0", off[0]);
    for (int w = 0; w < nfilt; ++w) {
        const int k = off[w + 1] - off[w];
        if (k < 0) FAIL(-1, "off decreases at %d", w + 1);
        if (k > MSCKF_ANCHOR_MAX) FAIL(-1, "filter %d has %d anchors (at most %d a call)", filters[w], k, MSCKF_ANCHOR_MAX);
    }
    if (off[nfilt] > 0 && !anchors) FAIL(-1, "null argument");
    for (int l = 0; l < off[nfilt]; ++l) {
        const msckf_anchor_t& an = anchors[l];
        bool fin = true;
        for (int i = 0; i < 3; ++i) fin = fin && std::isfinite(an.p_w[i]);
        for (int i = 0; i < 6; ++i) fin = fin && std::isfinite(an.cov[i]);
        for (int i = 0; i < 4; ++i) fin = fin && std::isfinite(an.z[i]);
        if (!fin) FAIL(-1, "anchor %d: p_w, cov and z must be finite", l);
        if (an.cov[0] < 0.0 || an.cov[3] < 0.0 || an.cov[5] < 0.0) FAIL(-1, "anchor %d: a negative variance", l);
    }
    if (nfilt == 0) return 1;
    c->last_async = "msckf_anchor_batch";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_anchor_batch, c, nfilt, filters, off, anchors, *prm);
}

int msckf_anchor_results(msckf_ctx_t* c, int nfilt, const int32_t* filters, int32_t* applied, int32_t* used,
                         int32_t* rows, int64_t* count) {
    if (!c) FAIL(-1, "null context");
    if (int r = check_list(c, nfilt, filters)) return r;
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    if (!c->anchor.on) {   // no anchor was ever enqueued: the records' initial values, no allocation
        HIPSYNC(c, hipStreamSynchronize(c->stream));
        for (int w = 0; w < nfilt; ++w) {
            if (applied) applied[w] = 0;
            if (used) used[w] = 0;
            if (rows) rows[w] = 0;
            if (count) count[w] = 0;
        }
        return 0;
    }
    const auto& z = c->anchor.dev;
    const size_t B = (size_t)c->B;
    DownList d;
    const size_t o_app = d.add(z.applied, B * sizeof(int)), o_use = d.add(z.used, B * sizeof(int)),
                 o_row = d.add(z.rows, B * sizeof(int)), o_cnt = d.add(z.count, B * 8);
    HIPSYNC(c, d.run(c));
    const int* r_app = reinterpret_cast<const int*>(d.at(c, o_app));
    const int* r_use = reinterpret_cast<const int*>(d.at(c, o_use));
    const int* r_row = reinterpret_cast<const int*>(d.at(c, o_row));
    const long long* r_cnt = reinterpret_cast<const long long*>(d.at(c, o_cnt));
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (applied) applied[w] = r_app[f];
        if (used) used[w] = r_use[f];
        if (rows) rows[w] = r_row[f];
        if (count) count[w] = (int64_t)r_cnt[f];
    }
    return 0;
}

int msckf_anchor_status(msckf_ctx_t* c, int filter, int cap, uint8_t* status, double* gamma, int32_t* n) {
    if (!c) FAIL(-1, "null context");
    if (filter < 0 || filter >= c->B) FAIL(-1, "filter slot %d out of range [0,%d)", filter, c->B);
    if (cap < 0) FAIL(-1, "cap = %d must be >= 0", cap);
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    if (!c->anchor.on) {
        HIPSYNC(c, hipStreamSynchronize(c->stream));
        if (n) *n = 0;
        return 0;
    }
    const auto& z = c->anchor.dev;
    DownList d;
    const size_t o_n = d.add(z.n + filter, sizeof(int)), o_st = d.add(z.status + (size_t)filter * ANC_K, ANC_K),
                 o_gam = d.add(z.gamma + (size_t)filter * ANC_K, ANC_K * 8);
    HIPSYNC(c, d.run(c));
    const int k = *reinterpret_cast<const int*>(d.at(c, o_n));
    const int take = std::min(k, cap);
    if (n) *n = k;
    if (status && take > 0) std::memcpy(status, d.at(c, o_st), (size_t)take);
    if (gamma && take > 0) std::memcpy(gamma, d.at(c, o_gam), (size_t)take * 8);
    return 0;
}

}  // extern "C"
