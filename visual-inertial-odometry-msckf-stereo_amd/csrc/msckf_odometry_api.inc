// msckf_odometry_api.inc -- host side of include/msckf_odometry.h: the landmark rings' allocation, the checks of
// an archive call against the context's record of the loaded batch (msckf_map_load leaves it, every other load
// and msckf_batch_update advance it), its one input block and launch, the read of a ring; msckf_readback_odom.
// Included by msckf_api.hip behind msckf_map_api.inc, whose helpers it uses.

namespace {

int lm_check(msckf_ctx* c) {
    if (!c) FAIL(-1, "null context");
    if (!c->lm.on) FAIL(-1, "the context has no landmark rings (msckf_landmarks_create)");
    return 0;
}

template <typename T>
int do_lm_archive(msckf_ctx* c, int nfilt, const int32_t* filters, const int32_t* stamps) {
    auto& lm = c->lm;
    auto& mp = c->map;
    std::vector<int> hdr((size_t)nfilt * LM_HDR, 0);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        int* h = &hdr[(size_t)w * LM_HDR];
        // the batch holds the features in ascending filter slot: filter f's begin at h_feat_off[f]
        h[0] = f, h[1] = mp.cur[f] ^ 1, h[2] = c->h_feat_off[f], h[3] = lm.feat_off[w + 1] - lm.feat_off[w];
        h[4] = stamps[w];
    }
    MapBlock blk;
    const size_t o_hdr = blk.add(hdr.data(), hdr.size() * sizeof(int));
    if (int r = map_send(c, lm.in, blk)) return r;
    c->timer.begin(c->stream, "landmarks_archive");
    launch_lm_archive<T>(c->stream, mp.dev, lm.dev, nfilt, reinterpret_cast<const int*>(lm.in.p + o_hdr),
                         reinterpret_cast<const int*>(mp.aux.p + mp.aux_rows), c->include,
                         reinterpret_cast<const T*>(c->p_w), reinterpret_cast<const T*>(c->gamma));
    c->timer.end(c->stream);
    HIPC(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int msckf_landmarks_create(msckf_ctx_t* c, int cap) {
    if (int r = map_check(c)) return r;
    if (c->lm.on) FAIL(-1, "the context already has landmark rings");
    if (cap < c->map.cap || cap > MSCKF_LANDMARKS_MAX_CAP)
        FAIL(-1, "landmark capacity %d outside [%d (the map's), %d]", cap, c->map.cap, MSCKF_LANDMARKS_MAX_CAP);
    HIPC(hipSetDevice(c->device));
    auto& lm = c->lm;
    const size_t rows = (size_t)c->B * cap;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_ids = al(rows * 8), b_pw = al(rows * 24), b_gam = al(rows * 8), b_nobs = al(rows * 4),
                 b_stamp = al(rows * 4), b_seq = al((size_t)c->B * 8);
    const size_t total = b_ids + b_pw + b_gam + b_nobs + b_stamp + b_seq;
    HIPC(lm.store.ensure(total));
    HIPC(hipMemset(lm.store.p, 0, total));
    unsigned char* p = lm.store.p;
    lm.dev.ids = reinterpret_cast<int64_t*>(p);
    lm.dev.pw = reinterpret_cast<double*>(p + b_ids);
    lm.dev.gamma = reinterpret_cast<double*>(p + b_ids + b_pw);
    lm.dev.nobs = reinterpret_cast<int*>(p + b_ids + b_pw + b_gam);
    lm.dev.stamp = reinterpret_cast<int*>(p + b_ids + b_pw + b_gam + b_nobs);
    lm.dev.seq = reinterpret_cast<long long*>(p + b_ids + b_pw + b_gam + b_nobs + b_stamp);
    lm.dev.cap = cap;
    lm.cap = cap;
    lm.on = true;
    return 0;
}

int msckf_landmarks_clear(msckf_ctx_t* c, int nfilt, const int32_t* filters) {
    if (int r = lm_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    c->last_async = "msckf_landmarks_clear";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    for (int w = 0; w < nfilt; ++w)
        HIPC(hipMemsetAsync(c->lm.dev.seq + filters[w], 0, sizeof(long long), c->stream));
    return 0;
}

int msckf_landmarks_archive(msckf_ctx_t* c, int nfilt, const int32_t* filters, const int32_t* feat_off,
                            const int32_t* rows, const int32_t* stamps) {
    if (int r = lm_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    auto& lm = c->lm;
    if (nfilt < 0 || !feat_off || (nfilt > 0 && !stamps)) FAIL(-1, "null argument");
    if (lm.state != 2)
        FAIL(-1, "msckf_landmarks_archive does not follow a lost-form msckf_map_load and its msckf_batch_update (%s)",
             lm.state == 1 ? "the batch was not updated" : "another batch is loaded, or this one was archived");
    if (nfilt != (int)lm.filters.size() || !std::equal(filters, filters + nfilt, lm.filters.begin()) ||
        !std::equal(feat_off, feat_off + nfilt + 1, lm.feat_off.begin()))
        FAIL(-1, "the filters or feature offsets are not the loaded batch's");
    const int ntot = lm.feat_off[nfilt];
    if (ntot && (!rows || !std::equal(rows, rows + ntot, lm.rows.begin()))) FAIL(-1, "the rows are not the loaded batch's");
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w], cnt = lm.feat_off[w + 1] - lm.feat_off[w];
        if (!c->map.lost_ok[f]) FAIL(-1, "filter %d: its lost table was given up since the load", f);
        if (cnt > lm.cap) FAIL(-1, "filter %d: %d features exceed the landmark capacity %d", f, cnt, lm.cap);
        if (c->h_feat_off[f + 1] - c->h_feat_off[f] != cnt) FAIL(-1, "filter %d: the loaded batch holds another count", f);
    }
    lm.state = 0;   // a batch is archived once
    if (nfilt == 0) return 0;
    c->last_async = "msckf_landmarks_archive";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);   // the update chain may have run as two lanes
    return DISPATCH(c, do_lm_archive, c, nfilt, filters, stamps);
}

int msckf_landmarks_get(msckf_ctx_t* c, int filter, int64_t first_seq, int max_rows, int64_t* seq_out,
                        int64_t* first_out, int64_t* ids, double* p_w, int32_t* n_obs, double* gamma, int32_t* stamp) {
    if (int r = lm_check(c)) return r;
    if (int r = check_ctx(c, filter)) return r;
    if (max_rows < 0 || !seq_out || !first_out) FAIL(-1, "bad argument");
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    const auto& L = c->lm.dev;
    const size_t cap = (size_t)L.cap, fb = (size_t)filter * cap;
    DownList d;
    const size_t o_seq = d.add(L.seq + filter, 8), o_ids = d.add(L.ids + fb, cap * 8), o_pw = d.add(L.pw + fb * 3, cap * 24);
    const size_t o_gam = d.add(L.gamma + fb, cap * 8), o_nobs = d.add(L.nobs + fb, cap * 4);
    const size_t o_stamp = d.add(L.stamp + fb, cap * 4);
    HIPSYNC(c, d.run(c));
    long long seq;
    std::memcpy(&seq, d.at(c, o_seq), 8);
    if (seq < 0) FAIL(-2, "filter %d: the landmark counter reads %lld", filter, seq);
    const long long lo = std::min<long long>(std::max<long long>({(long long)first_seq, seq - (long long)cap, 0LL}), seq);
    const int cnt = (int)std::min<long long>(max_rows, seq - lo);
    const int64_t* r_ids = reinterpret_cast<const int64_t*>(d.at(c, o_ids));
    const double* r_pw = reinterpret_cast<const double*>(d.at(c, o_pw));
    const double* r_gam = reinterpret_cast<const double*>(d.at(c, o_gam));
    const int32_t* r_nobs = reinterpret_cast<const int32_t*>(d.at(c, o_nobs));
    const int32_t* r_stamp = reinterpret_cast<const int32_t*>(d.at(c, o_stamp));
    for (int k = 0; k < cnt; ++k) {
        const size_t s = (size_t)((lo + k) % (long long)cap);
        if (ids) ids[k] = r_ids[s];
        if (p_w)
            for (int e = 0; e < 3; ++e) p_w[(size_t)k * 3 + e] = r_pw[s * 3 + e];
        if (gamma) gamma[k] = r_gam[s];
        if (n_obs) n_obs[k] = r_nobs[s];
        if (stamp) stamp[k] = r_stamp[s];
    }
    *seq_out = seq;
    *first_out = lo;
    return cnt;
}

int msckf_readback_odom(msckf_ctx_t* c, int nfilt, const int32_t* filters, double* imu_out, double* cams_out,
                        int32_t* ncams_out, int i0, int n, double* cov_out, uint8_t* accepted_out, double* gamma_out,
                        double* p_w_out, uint8_t* valid_out, int32_t* rows_out, const double* R_body,
                        double* pose_cov_out, double* vel_cov_out) {
    if (!c) FAIL(-1, "null context");
    if (!R_body || !pose_cov_out || !vel_cov_out) FAIL(-1, "null argument");
    JOIN_LANES(c);
    if (int r = check_list(c, nfilt, filters)) return r;
    return DISPATCH(c, do_readback, c, nfilt, filters, imu_out, cams_out, ncams_out, i0, n, cov_out, accepted_out,
                    gamma_out, p_w_out, valid_out, rows_out, R_body, pose_cov_out, vel_cov_out);
}

}  // extern "C"
