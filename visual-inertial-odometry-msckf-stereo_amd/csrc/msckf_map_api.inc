// msckf_map_api.inc -- host side of include/msckf_map.h and include/msckf_keyframes.h: argument checks, the
// host's record of every table (row count, which of the two sets is current),
// one input block and one H2D copy per call, the launches of msckf_map.hip.
// Included by msckf_api.hip, which owns the context and the batch loader's plan.

namespace {

int map_check(msckf_ctx* c) {
    if (!c) FAIL(-1, "null context");
    if (!c->map.on) FAIL(-1, "the context has no feature map (msckf_map_create)");
    return 0;
}

// A call's inputs, 16-byte aligned pieces of one block (one H2D copy).
struct MapBlock {
    std::vector<unsigned char> b;
    size_t add(const void* p, size_t bytes) {
        const size_t o = (b.size() + 15) & ~(size_t)15;
        b.resize(o + bytes);
        if (bytes) std::memcpy(b.data() + o, p, bytes);
        return o;
    }
};
int map_send(msckf_ctx* c, DBuf<unsigned char>& dst, const MapBlock& blk) {
    HIPC(dst.ensure(blk.b.size() + 16));
    HIPC(upload_raw(c, dst.p, blk.b.data(), blk.b.size()));
    return 0;
}

// The outputs of a select call: [out ints | descriptor ids | descriptor info], stride ds rows per filter.
struct MapOut {
    size_t o_id, o_info, total;
    MapOut(int nfilt, int ds) {
        o_id = ((size_t)nfilt * MAP_OUT * sizeof(int) + 255) & ~(size_t)255;
        o_info = o_id + (((size_t)nfilt * ds * sizeof(int64_t) + 255) & ~(size_t)255);
        total = o_info + (size_t)nfilt * ds * MAP_INFO * sizeof(int);
    }
};

// One copy back and one synchronisation; returns the block in the pinned buffer
// (valid until the context's next download) and the per-filter out ints.
const unsigned char* map_read_select(msckf_ctx* c, int nfilt, const MapOut& mo, std::vector<int>& out) {
    DownList d;
    const size_t o = d.add(c->map.out.p, mo.total);
    hipError_t e = d.run(c);
    if (e != hipSuccess) {
        char b[512];
        snprintf(b, sizeof(b), "reading a map call's results failed: %s (errors of asynchronous calls surface here "
                               "-- last asynchronous call: %s)", hipGetErrorString(e), c->last_async);
        g_err = b;
        return nullptr;
    }
    const unsigned char* p = d.at(c, o);
    out.assign(reinterpret_cast<const int*>(p), reinterpret_cast<const int*>(p) + (size_t)nfilt * MAP_OUT);
    return p;
}
// The first cnt descriptor entries of named filter w into the caller's arrays (stride cap).
void map_copy_desc(const msckf_ctx* c, const unsigned char* p, const MapOut& mo, int ds, int w, int cnt,
                   int64_t* desc_id, int32_t* desc_info) {
    const int cap = c->map.cap;
    cnt = std::min(std::max(cnt, 0), ds);
    std::memcpy(desc_id + (size_t)w * cap, p + mo.o_id + (size_t)w * ds * sizeof(int64_t), (size_t)cnt * sizeof(int64_t));
    std::memcpy(desc_info + (size_t)w * cap * MAP_INFO, p + mo.o_info + (size_t)w * ds * MAP_INFO * sizeof(int),
                (size_t)cnt * MAP_INFO * sizeof(int));
}

// msckf_map_add_lost and msckf_map_add_lost_tracks after their checks.  Filter w's message is rows
// [m0[w], m1[w]) of the message arrays: the host's ids / z (ntot rows, sent in the call's block), or -- with
// dev_ids / dev_z -- arrays that lie on the device already, and the block is the header alone.
int map_add_lost_run(msckf_ctx* c, int nfilt, const int32_t* filters, const int* m0, const int* m1, int ntot,
                     const int64_t* ids, const double* z, const int64_t* dev_ids, const double* dev_z,
                     int32_t* tracked_out, int32_t* n_before_out, int32_t* n_cand_out, int64_t* desc_id_out,
                     int32_t* desc_info_out) {
    auto& mp = c->map;
    int ds = 1;
    for (int w = 0; w < nfilt; ++w) ds = std::max(ds, mp.n[filters[w]]);
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    // the launch writes every named filter's other set, which is its lost table of the frame before:
    // that table is gone whether or not the call succeeds
    for (int w = 0; w < nfilt; ++w) mp.lost_ok[filters[w]] = 0;
    std::vector<int> hdr((size_t)nfilt * MAP_HDR, 0);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        int* h = &hdr[(size_t)w * MAP_HDR];
        h[0] = f, h[1] = mp.n[f], h[2] = mp.cur[f], h[3] = c->h_ncams[f] - 1, h[4] = m0[w], h[5] = m1[w];
        h[6] = ds;
    }
    MapBlock blk;
    const size_t o_hdr = blk.add(hdr.data(), hdr.size() * sizeof(int));
    size_t o_ids = 0, o_z = 0;
    if (!dev_ids) o_ids = blk.add(ids, (size_t)ntot * 8), o_z = blk.add(z, (size_t)ntot * 32);
    if (int r = map_send(c, mp.in, blk)) return r;
    const MapOut mo(nfilt, ds);
    HIPC(mp.out.ensure(mo.total + 16));
    launch_map_add_lost(c->stream, mp.dev, nfilt, reinterpret_cast<const int*>(mp.in.p + o_hdr),
                        dev_ids ? dev_ids : reinterpret_cast<const int64_t*>(mp.in.p + o_ids),
                        dev_ids ? dev_z : reinterpret_cast<const double*>(mp.in.p + o_z),
                        reinterpret_cast<int*>(mp.out.p), reinterpret_cast<int64_t*>(mp.out.p + mo.o_id),
                        reinterpret_cast<int*>(mp.out.p + mo.o_info));
    HIPC(hipGetLastError());
    std::vector<int> out;
    const unsigned char* res = map_read_select(c, nfilt, mo, out);
    if (!res) return -2;
    for (int w = 0; w < nfilt; ++w)
        if (out[w * MAP_OUT + 3])
            FAIL(-3, "filter %d: %d rows exceed the map capacity %d", filters[w], out[w * MAP_OUT + 1], mp.cap);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w], nc = out[w * MAP_OUT + 2];
        tracked_out[w] = out[w * MAP_OUT + 0];
        n_before_out[w] = mp.n[f];
        mp.nprev[f] = mp.n[f];
        n_cand_out[w] = nc;
        map_copy_desc(c, res, mo, ds, w, nc, desc_id_out, desc_info_out);
        mp.n[f] = out[w * MAP_OUT + 1];
        mp.cur[f] ^= 1;
        mp.lost_ok[f] = 1;
        mp.sel_ok[f] = 0;
    }
    return 0;
}

template <typename T>
int do_map_load(msckf_ctx* c, int mode, int nfilt, const int32_t* filters, const int32_t* feat_off,
                const int32_t* rows, const int32_t* counts, const double* p_w) {
    auto& mp = c->map;
    // arena order: ascending filter slot, each filter's features in the order given
    std::vector<int> where(c->B, -1);
    for (int w = 0; w < nfilt; ++w) where[filters[w]] = w;
    std::vector<int> full_off(c->B + 1, 0), frow, obs_off(1, 0), src;
    for (int b = 0; b < c->B; ++b) {
        full_off[b + 1] = full_off[b];
        const int w = where[b];
        if (w < 0) continue;
        for (int k = feat_off[w]; k < feat_off[w + 1]; ++k) {
            frow.push_back(rows[k]);
            src.push_back(k);
            obs_off.push_back(obs_off.back() + counts[k]);
        }
        full_off[b + 1] += feat_off[w + 1] - feat_off[w];
    }
    LoadPlan pl;
    if (int r = plan_counts(c, 0, full_off.data(), 0, obs_off.data(), pl)) return r;
    if (int r = plan_stage<T>(c, obs_off.data(), 0, pl)) return r;
    if (int r = plan_commit(c, obs_off.data(), pl)) return r;
    const int nf = pl.nf;
    std::vector<int> sel(c->B, 0);
    for (int b = 0; b < c->B; ++b) sel[b] = mode == MSCKF_MAP_LOAD_LOST ? mp.cur[b] ^ 1 : mp.cur[b];
    MapBlock blk;
    const size_t o_row = blk.add(frow.data(), frow.size() * sizeof(int));
    const size_t o_sel = blk.add(sel.data(), sel.size() * sizeof(int));
    const size_t o_rm = blk.add(mp.rm.data(), mp.rm.size() * sizeof(unsigned long long));
    size_t o_pw = 0;
    if (p_w && mode == MSCKF_MAP_LOAD_PRUNE_UPDATE) {
        std::vector<double> pw((size_t)nf * 3);
        for (int f = 0; f < nf; ++f)
            for (int k = 0; k < 3; ++k) pw[(size_t)f * 3 + k] = p_w[(size_t)src[f] * 3 + k];
        o_pw = blk.add(pw.data(), pw.size() * sizeof(double));
    }
    if (int r = map_send(c, mp.aux, blk)) return r;
    const unsigned char* a = mp.aux.p;
    launch_map_gather<T>(c->stream, mp.dev, mode, nf, c->feat_filter, c->obs_off,
                         reinterpret_cast<const int*>(a + o_row), reinterpret_cast<const int*>(a + o_sel),
                         reinterpret_cast<const unsigned long long*>(a + o_rm),
                         o_pw ? reinterpret_cast<const double*>(a + o_pw) : nullptr, mp.chi2.p, (T)1e300, c->obs_cam,
                         reinterpret_cast<T*>(c->obs_z), reinterpret_cast<T*>(c->chi2), c->valid,
                         reinterpret_cast<T*>(c->p_w));
    HIPC(hipGetLastError());
    mp.aux_rows = o_row;
    if (mode == MSCKF_MAP_LOAD_LOST) {   // what msckf_landmarks_archive has to name (msckf_odometry.h)
        auto& lm = c->lm;
        lm.filters.assign(filters, filters + nfilt);
        lm.feat_off.assign(feat_off, feat_off + nfilt + 1);
        lm.rows.assign(rows, rows + (nfilt ? feat_off[nfilt] : 0));
        lm.state = 1;
    }
    return 0;
}

// msckf_keyframe_select after its argument checks (include/msckf_keyframes.h): the launch, then ONE copy
// back for the slots, the counts, the descriptors and -- if asked -- the loaded batch's results.
template <typename T>
int do_keyframe_select(msckf_ctx* c, int nfilt, const int32_t* filters, const double* rate, double rot_thr,
                       double trans_thr, double rate_thr, int32_t* cam_slots_out, int32_t* n_inv_out,
                       int64_t* desc_id_out, int32_t* desc_info_out, uint8_t* accepted_out, double* gamma_out,
                       double* p_w_out, uint8_t* valid_out, int32_t* rows_out) {
    auto& mp = c->map;
    int ds = 1;
    for (int w = 0; w < nfilt; ++w) ds = std::max(ds, mp.n[filters[w]]);
    for (int w = 0; w < nfilt; ++w) mp.lost_ok[filters[w]] = 0;   // the launch overwrites the lost table
    std::vector<int> hdr((size_t)nfilt * MAP_HDR, 0);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        int* h = &hdr[(size_t)w * MAP_HDR];
        h[0] = f, h[1] = mp.n[f], h[2] = mp.cur[f], h[3] = c->h_ncams[f], h[6] = ds;
    }
    MapBlock blk;
    const size_t o_hdr = blk.add(hdr.data(), hdr.size() * sizeof(int));
    const size_t o_rate = blk.add(rate, (size_t)nfilt * sizeof(double));
    if (int r = map_send(c, mp.in, blk)) return r;
    const MapOut mo(nfilt, ds);
    HIPC(mp.out.ensure(mo.total + 16));
    launch_map_keyframe_select<T>(c->stream, mp.dev, nfilt, reinterpret_cast<const int*>(mp.in.p + o_hdr),
                                  reinterpret_cast<const double*>(mp.in.p + o_rate), rot_thr, trans_thr, rate_thr,
                                  reinterpret_cast<const T*>(c->cams.p), reinterpret_cast<int*>(mp.out.p),
                                  reinterpret_cast<int64_t*>(mp.out.p + mo.o_id),
                                  reinterpret_cast<int*>(mp.out.p + mo.o_info));
    HIPC(hipGetLastError());
    const bool res = accepted_out || gamma_out || p_w_out || valid_out || rows_out;
    DownList d;
    const size_t o_out = d.add(mp.out.p, mo.total);
    ResultsRead rr;
    if (res) rr = add_results<T>(c, d);
    HIPSYNC(c, d.run(c));
    if (res)   // an error of the batch: nothing was selected (no table becomes current)
        if (int r = unpack_results<T>(c, d, rr, accepted_out, gamma_out, p_w_out, valid_out, rows_out)) return r;
    const unsigned char* p = d.at(c, o_out);
    const int* out = reinterpret_cast<const int*>(p);
    for (int w = 0; w < nfilt; ++w) {
        const int a = out[w * MAP_OUT + 2], b = out[w * MAP_OUT + 3];
        if (a < 0 || a >= b || b >= c->h_ncams[filters[w]])
            FAIL(-2, "filter %d: the device chose the cam slots %d, %d of %d", filters[w], a, b, c->h_ncams[filters[w]]);
    }
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w], ni = out[w * MAP_OUT + 0], a = out[w * MAP_OUT + 2], b = out[w * MAP_OUT + 3];
        cam_slots_out[2 * w] = a;
        cam_slots_out[2 * w + 1] = b;
        n_inv_out[w] = ni;
        map_copy_desc(c, p, mo, ds, w, ni, desc_id_out, desc_info_out);
        mp.cur[f] ^= 1;
        mp.lost_ok[f] = 0;
        mp.sel_ok[f] = 1;
        mp.rm[2 * f] = mp.rm[2 * f + 1] = 0ull;
        mp.rm[2 * f + (a >> 6)] |= 1ull << (a & 63);
        mp.rm[2 * f + (b >> 6)] |= 1ull << (b & 63);
    }
    return 0;
}

}  // namespace

extern "C" {

int msckf_map_create(msckf_ctx_t* c, int cap, const double* chi2_table) {
    if (!c || !chi2_table) FAIL(-1, "null argument");
    if (c->map.on) FAIL(-1, "the context already has a feature map");
    if (cap < 1 || cap > MAP_MAX_CAP) FAIL(-1, "map capacity %d outside [1, %d]", cap, MAP_MAX_CAP);
    HIPC(hipSetDevice(c->device));
    auto& mp = c->map;
    const size_t rows = (size_t)c->B * cap;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_ids = al(rows * 8), b_mask = al(rows * 16), b_z = al(rows * c->Nmax * 32), b_pw = al(rows * 24),
                 b_init = al(rows);
    const size_t set = b_ids + b_mask + b_z + b_pw + b_init;
    HIPC(mp.store.ensure(2 * set));
    HIPC(hipMemset(mp.store.p, 0, 2 * set));
    for (int k = 0; k < 2; ++k) {
        unsigned char* p = mp.store.p + k * set;
        mp.dev.t[k].ids = reinterpret_cast<int64_t*>(p);
        mp.dev.t[k].mask = reinterpret_cast<unsigned long long*>(p + b_ids);
        mp.dev.t[k].z = reinterpret_cast<double*>(p + b_ids + b_mask);
        mp.dev.t[k].pw = reinterpret_cast<double*>(p + b_ids + b_mask + b_z);
        mp.dev.t[k].init = p + b_ids + b_mask + b_z + b_pw;
    }
    mp.dev.cap = cap;
    mp.dev.Nmax = c->Nmax;
    HIPC(mp.chi2.ensure(MSCKF_MAP_CHI2_LEN));
    HIPC(hipMemcpy(mp.chi2.p, chi2_table, MSCKF_MAP_CHI2_LEN * sizeof(double), hipMemcpyHostToDevice));
    mp.n.assign(c->B, 0);
    mp.cur.assign(c->B, 0);
    mp.nprev.assign(c->B, 0);
    mp.lost_ok.assign(c->B, 0);
    mp.sel_ok.assign(c->B, 0);
    mp.rm.assign((size_t)2 * c->B, 0ull);
    mp.cap = cap;
    mp.on = true;
    return 0;
}

int msckf_map_clear(msckf_ctx_t* c, int nfilt, const int32_t* filters) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        c->map.n[f] = 0;
        c->map.lost_ok[f] = c->map.sel_ok[f] = 0;
    }
    return 0;
}

int msckf_map_put(msckf_ctx_t* c, int filter, int n, const int64_t* ids, const uint64_t* mask, const double* z,
                  const double* p_w, const uint8_t* initialized) {
    if (int r = map_check(c)) return r;
    if (int r = check_ctx(c, filter)) return r;
    auto& mp = c->map;
    const int cap = mp.cap, Nmax = c->Nmax;
    if (n < 0 || n > cap) FAIL(-3, "%d rows exceed the map capacity %d", n, cap);
    if (n && (!ids || !mask || !z || !p_w || !initialized)) FAIL(-1, "null argument");
    {
        std::vector<int64_t> s(ids, ids + n);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) FAIL(-1, "the table's ids are not distinct");
    }
    for (int i = 0; i < n; ++i) {
        const uint64_t hi = Nmax >= 128 ? 0 : Nmax > 64 ? mask[2 * i + 1] >> (Nmax - 64) : mask[2 * i + 1];
        const uint64_t lo = Nmax >= 64 ? 0 : mask[2 * i] >> Nmax;
        if (hi || lo) FAIL(-1, "row %d observes a cam slot beyond the capacity %d", i, Nmax);
    }
    c->last_async = "msckf_map_put";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    const MapTab& t = mp.dev.t[mp.cur[filter] ^ 1];
    const size_t fb = (size_t)filter * cap;
    if (n) {
        HIPC(upload_raw(c, t.ids + fb, ids, (size_t)n * 8));
        HIPC(upload_raw(c, t.mask + fb * 2, mask, (size_t)n * 16));
        HIPC(upload_raw(c, t.z + fb * Nmax * 4, z, (size_t)n * Nmax * 32));
        HIPC(upload_raw(c, t.pw + fb * 3, p_w, (size_t)n * 24));
        HIPC(upload_raw(c, t.init + fb, initialized, (size_t)n));
    }
    mp.n[filter] = n;
    mp.cur[filter] ^= 1;
    mp.lost_ok[filter] = mp.sel_ok[filter] = 0;
    return 0;
}

int msckf_map_get(msckf_ctx_t* c, int filter, int32_t* n_out, int64_t* ids, uint64_t* mask, double* z, double* p_w,
                  uint8_t* initialized) {
    if (int r = map_check(c)) return r;
    if (int r = check_ctx(c, filter)) return r;
    if (!n_out) FAIL(-1, "null argument");
    auto& mp = c->map;
    const int cap = mp.cap, Nmax = c->Nmax, n = mp.n[filter];
    *n_out = n;
    if (!n) return 0;
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    const MapTab& t = mp.dev.t[mp.cur[filter]];
    const size_t fb = (size_t)filter * cap;
    DownList d;
    const size_t o_ids = d.add(t.ids + fb, (size_t)n * 8), o_mask = d.add(t.mask + fb * 2, (size_t)n * 16);
    const size_t o_z = d.add(t.z + fb * Nmax * 4, (size_t)n * Nmax * 32), o_pw = d.add(t.pw + fb * 3, (size_t)n * 24);
    const size_t o_init = d.add(t.init + fb, (size_t)n);
    HIPSYNC(c, d.run(c));
    std::vector<uint64_t> mk((size_t)n * 2);
    std::memcpy(mk.data(), d.at(c, o_mask), (size_t)n * 16);
    if (ids) std::memcpy(ids, d.at(c, o_ids), (size_t)n * 8);
    if (mask) std::memcpy(mask, mk.data(), (size_t)n * 16);
    if (p_w) std::memcpy(p_w, d.at(c, o_pw), (size_t)n * 24);
    if (initialized) std::memcpy(initialized, d.at(c, o_init), (size_t)n);
    if (z) {
        std::memcpy(z, d.at(c, o_z), (size_t)n * Nmax * 32);
        for (int i = 0; i < n; ++i)   // slots without an observation hold no defined value on the device
            for (int s = 0; s < Nmax; ++s)
                if (!((mk[2 * i + (s >> 6)] >> (s & 63)) & 1ull))
                    for (int k = 0; k < 4; ++k) z[((size_t)i * Nmax + s) * 4 + k] = 0.0;
    }
    return 0;
}

int msckf_map_add_lost(msckf_ctx_t* c, int nfilt, const int32_t* filters, const int32_t* msg_off, const int64_t* ids,
                       const double* z, int32_t* tracked_out, int32_t* n_before_out, int32_t* n_cand_out,
                       int64_t* desc_id_out, int32_t* desc_info_out) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    if (nfilt <= 0) return 1;
    if (!msg_off || !tracked_out || !n_before_out || !n_cand_out || !desc_id_out || !desc_info_out)
        FAIL(-1, "null argument");
    if (msg_off[0] != 0) FAIL(-1, "msg_off[0] must be 0");
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (msg_off[w + 1] < msg_off[w]) FAIL(-1, "msg_off not monotone");
        if (c->h_ncams[f] < 1) FAIL(-1, "filter %d has no cam state to observe from", f);
        std::vector<int64_t> s(ids + msg_off[w], ids + msg_off[w + 1]);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            FAIL(-1, "filter %d: an id is repeated within the message", f);
    }
    const int ntot = msg_off[nfilt];
    if (ntot && (!ids || !z)) FAIL(-1, "null argument");
    c->last_async = "msckf_map_add_lost";
    return map_add_lost_run(c, nfilt, filters, msg_off, msg_off + 1, ntot, ids, z, nullptr, nullptr, tracked_out,
                            n_before_out, n_cand_out, desc_id_out, desc_info_out);
}

int msckf_map_add_lost_tracks(msckf_ctx_t* c, mfe_ctx_t* fe, int nfilt, const int32_t* filters, const int32_t* lanes,
                              int32_t* tracked_out, int32_t* n_before_out, int32_t* n_cand_out, int64_t* desc_id_out,
                              int32_t* desc_info_out) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    TrackMsgView v;
    if (!mfe_track_messages(fe, v)) FAIL(-1, "the front-end context has no track tables (mfe_tracks_create)");
    if (v.device != c->device)
        FAIL(-1, "the front-end context is on device %d, the filter context on device %d", v.device, c->device);
    if (nfilt <= 0) return 1;
    if (!lanes || !tracked_out || !n_before_out || !n_cand_out || !desc_id_out || !desc_info_out)
        FAIL(-1, "null argument");
    std::vector<int> m0(nfilt), m1(nfilt);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w], l = lanes[w];
        if (l < 0 || l >= v.n_lanes) FAIL(-1, "lanes[%d] = %d outside [0, %d)", w, l, v.n_lanes);
        for (int j = 0; j < w; ++j)
            if (lanes[j] == l) FAIL(-1, "lane %d is named twice (entries %d and %d)", l, j, w);
        if (!v.valid[l]) FAIL(-1, "lane %d has no valid message", l);
        if (v.n[l] < 0 || v.n[l] > v.cap) FAIL(-1, "lane %d: a message of %d rows (cap %d)", l, v.n[l], v.cap);
        if (c->h_ncams[f] < 1) FAIL(-1, "filter %d has no cam state to observe from", f);
        m0[w] = l * v.cap;   // n_lanes cap <= MFE_MAX_SLOTS / 3 * MFE_RANSAC_MAX_SET_POINTS: an int holds it
        m1[w] = m0[w] + v.n[l];
    }
    c->last_async = "msckf_map_add_lost_tracks";
    return map_add_lost_run(c, nfilt, filters, m0.data(), m1.data(), 0, nullptr, nullptr, v.ids, v.uv, tracked_out,
                            n_before_out, n_cand_out, desc_id_out, desc_info_out);
}

int msckf_map_prune_select(msckf_ctx_t* c, int nfilt, const int32_t* filters, const int32_t* slot_off,
                           const int32_t* cam_slots, int32_t* n_inv_out, int64_t* desc_id_out,
                           int32_t* desc_info_out) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    if (nfilt <= 0) return 1;
    if (!slot_off || !n_inv_out || !desc_id_out || !desc_info_out) FAIL(-1, "null argument");
    if (slot_off[0] != 0) FAIL(-1, "slot_off[0] must be 0");
    auto& mp = c->map;
    std::vector<unsigned long long> rm((size_t)2 * nfilt, 0ull);
    int ds = 1;
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (slot_off[w + 1] < slot_off[w]) FAIL(-1, "slot_off not monotone");
        for (int k = slot_off[w]; k < slot_off[w + 1]; ++k) {
            const int s = cam_slots[k];
            if (s < 0 || s >= c->h_ncams[f]) FAIL(-1, "filter %d has no cam slot %d", f, s);
            if ((rm[2 * w + (s >> 6)] >> (s & 63)) & 1ull) FAIL(-1, "filter %d: cam slot %d listed twice", f, s);
            rm[2 * w + (s >> 6)] |= 1ull << (s & 63);
        }
        ds = std::max(ds, mp.n[f]);
    }
    c->last_async = "msckf_map_prune_select";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    for (int w = 0; w < nfilt; ++w) mp.lost_ok[filters[w]] = 0;   // the launch overwrites the lost table
    std::vector<int> hdr((size_t)nfilt * MAP_HDR, 0);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        int* h = &hdr[(size_t)w * MAP_HDR];
        h[0] = f, h[1] = mp.n[f], h[2] = mp.cur[f], h[6] = ds;
    }
    MapBlock blk;
    const size_t o_hdr = blk.add(hdr.data(), hdr.size() * sizeof(int));
    const size_t o_rm = blk.add(rm.data(), rm.size() * sizeof(unsigned long long));
    if (int r = map_send(c, mp.in, blk)) return r;
    const MapOut mo(nfilt, ds);
    HIPC(mp.out.ensure(mo.total + 16));
    launch_map_prune_select(c->stream, mp.dev, nfilt, reinterpret_cast<const int*>(mp.in.p + o_hdr),
                            reinterpret_cast<const unsigned long long*>(mp.in.p + o_rm),
                            reinterpret_cast<int*>(mp.out.p), reinterpret_cast<int64_t*>(mp.out.p + mo.o_id),
                            reinterpret_cast<int*>(mp.out.p + mo.o_info));
    HIPC(hipGetLastError());
    std::vector<int> out;
    const unsigned char* res = map_read_select(c, nfilt, mo, out);
    if (!res) return -2;
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w], ni = out[w * MAP_OUT + 0];
        n_inv_out[w] = ni;
        map_copy_desc(c, res, mo, ds, w, ni, desc_id_out, desc_info_out);
        mp.cur[f] ^= 1;
        mp.lost_ok[f] = 0;
        mp.sel_ok[f] = 1;
        mp.rm[2 * f] = rm[2 * w];
        mp.rm[2 * f + 1] = rm[2 * w + 1];
    }
    return 0;
}

int msckf_keyframe_select(msckf_ctx_t* c, int nfilt, const int32_t* filters, const double* tracking_rate,
                          double rot_thr, double trans_thr, double rate_thr, int32_t* cam_slots_out,
                          int32_t* n_inv_out, int64_t* desc_id_out, int32_t* desc_info_out, uint8_t* accepted_out,
                          double* gamma_out, double* p_w_out, uint8_t* valid_out, int32_t* rows_out) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    if (nfilt <= 0) return 1;
    if (!tracking_rate || !cam_slots_out || !n_inv_out || !desc_id_out || !desc_info_out) FAIL(-1, "null argument");
    for (int w = 0; w < nfilt; ++w)
        if (c->h_ncams[filters[w]] < 4)
            FAIL(-1, "filter %d has %d cam states: the keyframe choice needs 4", filters[w], c->h_ncams[filters[w]]);
    c->last_async = "msckf_keyframe_select";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_keyframe_select, c, nfilt, filters, tracking_rate, rot_thr, trans_thr, rate_thr,
                    cam_slots_out, n_inv_out, desc_id_out, desc_info_out, accepted_out, gamma_out, p_w_out, valid_out,
                    rows_out);
}

int msckf_map_load(msckf_ctx_t* c, int mode, int nfilt, const int32_t* filters, const int32_t* feat_off,
                   const int32_t* rows, const int32_t* counts, const double* p_w) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    if (mode < MSCKF_MAP_LOAD_LOST || mode > MSCKF_MAP_LOAD_PRUNE_UPDATE) FAIL(-1, "unknown load form %d", mode);
    if (nfilt < 0 || !feat_off || feat_off[0] != 0) FAIL(-1, "bad feature offsets");
    auto& mp = c->map;
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (feat_off[w + 1] < feat_off[w]) FAIL(-1, "feat_off not monotone");
        if (feat_off[w + 1] > feat_off[w] && (!rows || !counts)) FAIL(-1, "null argument");
        if (mode == MSCKF_MAP_LOAD_LOST ? !mp.lost_ok[f] : !mp.sel_ok[f])
            FAIL(-1, "filter %d: the load form %d does not follow its select call", f, mode);
        for (int k = feat_off[w]; k < feat_off[w + 1]; ++k) {
            if (rows[k] < 0 || rows[k] >= (mode == MSCKF_MAP_LOAD_LOST ? mp.nprev[f] : mp.n[f])) FAIL(-1, "filter %d: row %d outside the table", f, rows[k]);
            const int dof = mode == MSCKF_MAP_LOAD_LOST ? counts[k] - 1 : counts[k];
            if (counts[k] < 1 || counts[k] > c->Nmax) FAIL(-1, "filter %d: %d observations of a row", f, counts[k]);
            if (mode != MSCKF_MAP_LOAD_PRUNE_TRI && (dof < 1 || dof > MSCKF_MAP_CHI2_LEN))
                FAIL(-1, "filter %d: no chi-square threshold for %d degrees of freedom (1..%d)", f, dof,
                     MSCKF_MAP_CHI2_LEN);
        }
    }
    c->last_async = "msckf_map_load";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    return DISPATCH(c, do_map_load, c, mode, nfilt, filters, feat_off, rows, counts, p_w);
}

int msckf_map_prune_commit(msckf_ctx_t* c, int nfilt, const int32_t* filters, const int32_t* ent_off,
                           const int32_t* rows, const uint8_t* valid, const double* p_w) {
    if (int r = map_check(c)) return r;
    if (int r = check_list(c, nfilt, filters)) return r;
    if (nfilt <= 0) return 1;
    if (!ent_off || ent_off[0] != 0) FAIL(-1, "bad entry offsets");
    auto& mp = c->map;
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        if (ent_off[w + 1] < ent_off[w]) FAIL(-1, "ent_off not monotone");
        if (!mp.sel_ok[f]) FAIL(-1, "filter %d: no msckf_map_prune_select is open", f);
        if (ent_off[w + 1] > ent_off[w] && (!rows || !valid || !p_w)) FAIL(-1, "null argument");
        std::vector<int> s(rows + ent_off[w], rows + ent_off[w + 1]);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) FAIL(-1, "filter %d: a row is listed twice", f);
        if (!s.empty() && (s.front() < 0 || s.back() >= mp.n[f])) FAIL(-1, "filter %d: row outside the table", f);
    }
    c->last_async = "msckf_map_prune_commit";
    HIPC(hipSetDevice(c->device));
    JOIN_LANES(c);
    const int ne = ent_off[nfilt];
    std::vector<int> hdr((size_t)nfilt * MAP_HDR, 0), val(ne);
    std::vector<unsigned long long> rm((size_t)2 * nfilt);
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        int* h = &hdr[(size_t)w * MAP_HDR];
        h[0] = f, h[1] = mp.n[f], h[2] = mp.cur[f], h[4] = ent_off[w], h[5] = ent_off[w + 1];
        rm[2 * w] = mp.rm[2 * f];
        rm[2 * w + 1] = mp.rm[2 * f + 1];
    }
    for (int k = 0; k < ne; ++k) val[k] = valid[k] ? 1 : 0;
    MapBlock blk;
    const size_t o_hdr = blk.add(hdr.data(), hdr.size() * sizeof(int));
    const size_t o_rm = blk.add(rm.data(), rm.size() * sizeof(unsigned long long));
    const size_t o_row = blk.add(rows, (size_t)ne * sizeof(int)), o_val = blk.add(val.data(), (size_t)ne * sizeof(int));
    const size_t o_pw = blk.add(p_w, (size_t)ne * 24);
    if (int r = map_send(c, mp.in, blk)) return r;
    const unsigned char* a = mp.in.p;
    launch_map_prune_commit(c->stream, mp.dev, nfilt, reinterpret_cast<const int*>(a + o_hdr),
                            reinterpret_cast<const unsigned long long*>(a + o_rm),
                            reinterpret_cast<const int*>(a + o_row), reinterpret_cast<const int*>(a + o_val),
                            reinterpret_cast<const double*>(a + o_pw));
    HIPC(hipGetLastError());
    for (int w = 0; w < nfilt; ++w) {
        const int f = filters[w];
        mp.cur[f] ^= 1;
        mp.sel_ok[f] = mp.lost_ok[f] = 0;
    }
    return 0;
}

}  // extern "C"
