// Session host code: push, fire, snapshot and restore of the in-flight session lists (kernels: sessions.inc,
// sessions4.inc). Included by engine.hip behind snap_header.
//
// Sessions (DESIGN.md §2): classify -> route -> bulk gap-scan (sort by (kid, start), segmented max-scan,
// cluster ids, wave-segmented reduction) and the arrival-order walk for keys with order-sensitive records.
struct KidEq {                       // equal kid part of a (kid << tb | start - base) sort key
    int tb;
    __host__ __device__ bool operator()(unsigned long long x, unsigned long long y) const { return (x >> tb) == (y >> tb); }
};
struct MaxI64 {
    __host__ __device__ int64_t operator()(int64_t x, int64_t y) const { return x > y ? x : y; }
};

static int ensure_sort_tmp(fwa_engine* e, size_t bytes) {
    if (bytes <= e->sort_tmp_bytes) return FWA_OK;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (e->d_sort_tmp) HIPCHK(e, hipFree(e->d_sort_tmp));
    e->d_sort_tmp = nullptr;
    HIPCHK(e, hipMalloc(&e->d_sort_tmp, bytes + bytes / 4));
    e->sort_tmp_bytes = bytes + bytes / 4;
    return FWA_OK;
}

static int ensure_sess_lists(fwa_engine* e, int64_t need) {
    if (need <= e->ss_cap) return FWA_OK;
    const int64_t cap = std::max<int64_t>(need + need / 4, 1 << 12);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (int q = 0; q < 2; ++q) {
        SessList nl;
        nl.stride = cap;
        HIPCHK(e, hipMalloc(&nl.kid, 4 * (size_t)cap));
        HIPCHK(e, hipMalloc(&nl.start, 8 * (size_t)cap));
        HIPCHK(e, hipMalloc(&nl.end, 8 * (size_t)cap));
        HIPCHK(e, hipMalloc(&nl.acc, 8 * (size_t)cap * e->nacc));
        SessList& ol = e->ss[q];
        if (q == e->ss_cur && e->n_ss > 0) {             // keep the live sessions
            const size_t n = (size_t)e->n_ss;
            HIPCHK(e, hipMemcpy(nl.kid, ol.kid, 4 * n, hipMemcpyDeviceToDevice));
            HIPCHK(e, hipMemcpy(nl.start, ol.start, 8 * n, hipMemcpyDeviceToDevice));
            HIPCHK(e, hipMemcpy(nl.end, ol.end, 8 * n, hipMemcpyDeviceToDevice));
            for (int cc = 0; cc < e->nacc; ++cc)
                HIPCHK(e, hipMemcpy(nl.acc + (size_t)cc * cap, ol.acc + (size_t)cc * ol.stride, 8 * n, hipMemcpyDeviceToDevice));
        }
        for (void* p : {(void*)ol.kid, (void*)ol.start, (void*)ol.end, (void*)ol.acc}) if (p) HIPCHK(e, hipFree(p));
        ol = nl;
    }
    e->ss_cap = cap;
    return FWA_OK;
}

static int read_sess_ctr(fwa_engine* e) {
    HIPCHK(e, hipMemcpyAsync(e->h_sctr, e->d_sctr, sizeof(SessCtr), hipMemcpyDeviceToHost, e->stream));
    return sync_status(e);
}

// Staging buffers, the segment walk (sess2_segment_kernel, or sess3_segment_kernel over cell keys), the scan of the
// per-wave counts and the compaction into s.out.
static int launch_segments(fwa_engine* e, Sess2Args& s, int64_t nb, bool cells) {
    const int64_t nw = (nb + 63) / 64;
    if (nb > e->sg_cap || nw + 1 > e->sgw_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (e->d_sg) HIPCHK(e, hipFree(e->d_sg));
        e->d_sg = nullptr;
        e->sg_cap = std::max<int64_t>(nb + nb / 4, 1 << 14);
        e->sgw_cap = (e->sg_cap + 63) / 64 + 1;
        const size_t bytes = (size_t)e->sg_cap * (4 + 8 + 8 + 8 * (size_t)e->nacc) + (size_t)e->sgw_cap * (4 + 4 + 8) + 1024;
        HIPCHK(e, hipMalloc(&e->d_sg, bytes));
    }
    char* sp = (char*)e->d_sg;
    s.sg_start = (int64_t*)sp; sp += 8 * (size_t)e->sg_cap;
    s.sg_end = (int64_t*)sp; sp += 8 * (size_t)e->sg_cap;
    s.sg_acc = (unsigned long long*)sp; sp += 8 * (size_t)e->sg_cap * e->nacc;
    s.sg_h0 = (int64_t*)sp; sp += 8 * (size_t)e->sgw_cap;
    s.sg_kid = (uint32_t*)sp; sp += 4 * (size_t)e->sg_cap;
    s.sg_cnt = (uint32_t*)sp; sp += 4 * (size_t)e->sgw_cap;
    s.sg_off = (uint32_t*)sp;
    s.sg_cap = e->sg_cap;
    const unsigned sg = (unsigned)std::max<int64_t>(1, std::min<int64_t>((nb + 255) / 256, 1 << 16));
    switch (e->nacc) {
        case 1: if (cells) sess3_segment_kernel<1><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); else sess2_segment_kernel<1><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); break;
        case 2: if (cells) sess3_segment_kernel<2><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); else sess2_segment_kernel<2><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); break;
        case 3: if (cells) sess3_segment_kernel<3><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); else sess2_segment_kernel<3><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); break;
        case 4: if (cells) sess3_segment_kernel<4><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); else sess2_segment_kernel<4><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); break;
        default: if (cells) sess3_segment_kernel<5><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); else sess2_segment_kernel<5><<<sg, kBlock, 0, e->stream>>>(s, e->d_ec); break;
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemsetAsync(s.sg_cnt + nw, 0, 4, e->stream));
    size_t bytes = 0;
    HIPCHK(e, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, s.sg_cnt, s.sg_off, (int)(nw + 1), e->stream));
    int rc = ensure_sort_tmp(e, bytes);
    if (rc) return rc;
    bytes = e->sort_tmp_bytes;
    HIPCHK(e, hipcub::DeviceScan::ExclusiveSum(e->d_sort_tmp, bytes, s.sg_cnt, s.sg_off, (int)(nw + 1), e->stream));
    sess2_compact_kernel<<<1024, kBlock, 0, e->stream>>>(s, nw, e->nacc);
    HIPCHK(e, hipGetLastError());
    return FWA_OK;
}

#include "sessions4_host.inc"

static int push_session(fwa_engine* e, IngestArgs& a, int64_t* dropped_out) {
    const int64_t n = a.n;
    const int64_t n_in = e->n_ss;
    int rc = FWA_OK;
    if (n + n_in > e->sb_cap) {                           // sort / scan buffers for every element of the push
        HIPCHK(e, hipStreamSynchronize(e->stream));
        const int64_t cap = std::max<int64_t>((n + n_in) + (n + n_in) / 4, 1 << 14);
        auto re = [&](void** p, size_t elem) -> int {
            if (*p) HIPCHK(e, hipFree(*p));
            *p = nullptr;
            HIPCHK(e, hipMalloc(p, elem * (size_t)cap));
            return FWA_OK;
        };
        for (int q = 0; q < 4; ++q) {
            if ((rc = re((void**)&e->d_skey[q], 8))) return rc;
            if ((rc = re((void**)&e->d_sval[q], 4))) return rc;
        }
        if ((rc = re((void**)&e->d_send2, 8)) || (rc = re((void**)&e->d_smax, 8)) || (rc = re((void**)&e->d_scid, 4)) ||
            (rc = re((void**)&e->d_rkid, 4)) || (rc = re((void**)&e->d_spk, 8 * (size_t)e->nacc)) || (rc = re((void**)&e->d_spe, 8)))
            return rc;
        e->sb_cap = cap;
    }
    if ((rc = ensure_sess_lists(e, n_in + n))) return rc;
    SessCtr z;
    memset(&z, 0, sizeof(z));
    z.ts_min = ~0ull;
    if ((rc = upload(e, e->d_sctr, &z, sizeof(z)))) return rc;
    HIPCHK(e, hipMemsetAsync(e->d_kflag, 0, (size_t)e->capacity + 1, e->stream));
    if ((rc = reset_push_status(e))) return rc;

    Sess2Args s;
    memset(&s, 0, sizeof(s));
    s.keys = a.keys;
    s.ts = a.ts;
    if (!e->tz.empty() && n > 0) {                        // Table GROUP BY SESSION over a TIMESTAMP_LTZ rowtime:
        if (n > e->lts_cap) {                             // sessions are formed on local wall-clock time
            if (e->d_lts) HIPCHK(e, hipFree(e->d_lts));
            e->d_lts = nullptr;
            HIPCHK(e, hipMalloc(&e->d_lts, 8 * (size_t)n));
            e->lts_cap = n;
        }
        to_local_kernel<<<grid_for(n), kBlock, 0, e->stream>>>(a.ts, e->d_lts, n, e->d_ec);
        HIPCHK(e, hipGetLastError());
        s.ts = e->d_lts;
    }
    for (int c = 0; c < FWA_MAX_COLS; ++c) s.cols[c] = a.cols[c];
    s.key_hash = a.key_hash;
    s.gapc = (e->cfg.flags & FWA_CFG_DYNAMIC_GAP) ? (const int64_t*)a.cols[e->cfg.gap_col] : nullptr;
    s.n = n;
    s.wm = local_wm(e, e->wm);
    s.gap = e->cfg.gap_ms;
    s.lateness = e->lateness;
    s.key_table = e->d_keys;
    s.key_mask = (uint64_t)e->capacity - 1;
    s.seg_log = e->seg_log;
    s.part_bits = e->part_bits;
    s.capacity = e->capacity;
    s.rkid = e->d_rkid;
    s.kflag = e->d_kflag;
    s.in = e->ss[e->ss_cur];
    s.n_in = n_in;
    s.out = e->ss[e->ss_cur ^ 1];
    for (int cc = 0; cc <= kMaxAggsInt; ++cc) s.col_owner[cc] = -1;
    for (int j = 0; j < e->ec.naggs; ++j)
        if (e->ec.agg[j].acc > 0 && !e->ec.agg[j].alias) s.col_owner[e->ec.agg[j].acc] = j;
    for (int col = 0; col < FWA_MAX_COLS; ++col) s.nulls[col] = a.nulls[col];
    s.ctr = e->d_sctr;
    s.dropidx = a.dropidx;
    s.st = e->d_st;
    // cell path (sess3_*): fixed gap, 32-bit cell keys; redone on the general path below when a record is not
    // order-free or a start falls outside the cell range (then not tried again for 8 pushes)
    const int cb = 32 - e->kid_bits;
    // cell pre-aggregation (sessions4.inc) first; cells or sessions out of its range: the sort-based cell path
    bool s4_general = false;
    if (e->opt_cells != 0 && !s.gapc && e->nacc <= 5 && n > 0 && e->cell_skip <= 0 && n + n_in < ((int64_t)1 << 31) &&
        e->cfg.gap_ms > 0 && e->cfg.gap_ms <= ((int64_t)1 << 27) && e->capacity < ((int64_t)1 << 27) &&
        (e->capacity + 1 + kS4Kids - 1) / kS4Kids <= 24576) {
        int verdict = 1;
        if ((rc = push_session_s4(e, s, n, n_in, dropped_out, &verdict))) return rc;
        if (verdict == 0) { e->sess_path = 2; return FWA_OK; }
        s4_general = verdict == 2;
        memset(&z, 0, sizeof(z));
        z.ts_min = ~0ull;
        if ((rc = upload(e, e->d_sctr, &z, sizeof(z)))) return rc;
        if ((rc = reset_push_status(e))) return rc;
    }
    bool tried3 = false;
    if (e->opt_cells != 0 && !s4_general && !s.gapc && cb >= 1 && e->nacc <= 5 && n > 0 && e->cell_skip <= 0 &&
        n + n_in < ((int64_t)1 << 31)) {
        tried3 = true;
        Sess2Args t = s;
        t.tb = cb;
        t.gap_div = jm::udiv64_make((uint64_t)e->cfg.gap_ms);
        t.nb = n + n_in;
        t.bkey = e->d_skey[0];
        t.bval = e->d_sval[0];
        t.pk = e->d_spk;
        t.pkw = e->nacc;
        t.seg_out = 1;
        HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
        sess3_min_kernel<<<grid_for(n + n_in, 1024), kBlock, 0, e->stream>>>(t);
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(8192, (n + 2047) / 2048));   // >= 32 waves per CU (latency-bound probes)
        const int64_t chunk = ((n + G - 1) / G + 255) / 256 * 256;
        sess3_route_kernel<2><<<G, kBlock, 0, e->stream>>>(t, e->d_ec, chunk);
        if (n_in > 0) sess3_route_sessions_kernel<<<grid_for(n_in, 256 * 16), kBlock, 0, e->stream>>>(t);
        HIPCHK(e, hipGetLastError());
        size_t bytes = 0;
        const uint32_t* k0 = (const uint32_t*)e->d_skey[0];
        uint32_t* k1 = (uint32_t*)e->d_skey[1];
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k0, k1, (const uint32_t*)e->d_sval[0], e->d_sval[1],
                                                     (int)t.nb, 0, 32, e->stream));
        if ((rc = ensure_sort_tmp(e, bytes))) return rc;
        bytes = e->sort_tmp_bytes;
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(e->d_sort_tmp, bytes, k0, k1, (const uint32_t*)e->d_sval[0], e->d_sval[1],
                                                     (int)t.nb, 0, 32, e->stream));
        t.bkey = e->d_skey[1];
        t.bval = e->d_sval[1];
        if ((rc = launch_segments(e, t, t.nb, true))) return rc;
        HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
        if ((rc = read_sess_ctr(e))) return rc;
        if (e->h_st->error) return FWA_OK;                // reported by the caller
        if (e->h_sctr->n_special == 0 && e->h_sctr->n_redo == 0) {
            if ((rc = account_ingest(e))) return rc;
            e->ingest_launches++;
            e->ingest_records += n;
            e->n_ss = (int64_t)e->h_sctr->n_out_sp;
            e->ss_cur ^= 1;
            *dropped_out = (int64_t)e->h_st->dropped;
            e->sess_path = 1;
            return FWA_OK;
        }
        e->cell_skip = 8;                                 // the general path redoes the push (key inserts are idempotent)
        e->replay_records += n;
        memset(&z, 0, sizeof(z));
        z.ts_min = ~0ull;
        if ((rc = upload(e, e->d_sctr, &z, sizeof(z)))) return rc;
        HIPCHK(e, hipMemsetAsync(e->d_kflag, 0, (size_t)e->capacity + 1, e->stream));
        if ((rc = reset_push_status(e))) return rc;
    }
    e->sess_path = 0;
    if (s4_general) {
        e->cell_skip = 8;                                 // as the cell path: not tried again for 8 pushes
        e->replay_records += n;
    } else if (!tried3 && e->cell_skip > 0) {
        --e->cell_skip;
    }
    HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
    if (n > 0) sess2_classify_kernel<<<grid_for(n, 256 * 32), kBlock, 0, e->stream>>>(s, e->d_ec);
    if (n_in > 0) sess2_range_kernel<<<grid_for(n_in, 256 * 32), kBlock, 0, e->stream>>>(s);
    HIPCHK(e, hipGetLastError());
    if ((rc = read_sess_ctr(e))) return rc;
    if (e->h_st->error) return FWA_OK;                    // reported by the caller
    const SessCtr c1 = *e->h_sctr;
    if (n + n_in == 0 || c1.ts_min > c1.ts_max) {         // nothing to do (empty push, no sessions)
        *dropped_out = 0;
        return FWA_OK;
    }
    const int64_t lo = jm::unord_i64(c1.ts_min), hi = jm::unord_i64(c1.ts_max);
    const uint64_t span = (uint64_t)hi - (uint64_t)lo;
    int tb = 0;
    while (tb < 64 && (span >> tb) != 0) ++tb;
    s.base = lo;
    s.tb = tb;
    s.all_sp = e->kid_bits + tb > 64 ? 1 : 0;                // start range too wide for one sort key
    if (s.all_sp) s.tb = 0;
    s.bkey = e->d_skey[0];
    s.bval = e->d_sval[0];
    s.pk = e->d_spk;
    s.pe = e->d_spe;
    s.pkw = e->nacc;
    s.skey = e->d_skey[2];
    s.sval = e->d_sval[2];
    sess2_route_kernel<<<(unsigned)((n + n_in + (int64_t)kBlock * kRouteItems - 1) / ((int64_t)kBlock * kRouteItems)), kBlock, 0,
                         e->stream>>>(s, e->d_ec);
    HIPCHK(e, hipGetLastError());
    if ((rc = read_sess_ctr(e))) return rc;
    const int64_t nb = (int64_t)e->h_sctr->n_bulk, nsp = (int64_t)e->h_sctr->n_sp;
    s.nb = nb;
    s.nsp = nsp;
    s.bend = e->d_send2;
    s.bmax = e->d_smax;
    s.bcid = e->d_scid;
    if (nb > 0) {
        size_t bytes = 0;
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)e->d_skey[0], e->d_skey[1],
                                                     (const uint32_t*)e->d_sval[0], e->d_sval[1], (int)nb, 0, e->kid_bits + tb, e->stream));
        if ((rc = ensure_sort_tmp(e, bytes))) return rc;
        bytes = e->sort_tmp_bytes;
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(e->d_sort_tmp, bytes, (const unsigned long long*)e->d_skey[0], e->d_skey[1],
                                                     (const uint32_t*)e->d_sval[0], e->d_sval[1], (int)nb, 0, e->kid_bits + tb, e->stream));
        s.bkey = e->d_skey[1];
        s.bval = e->d_sval[1];
    }
    s.seg_out = e->nacc <= 5 ? 1 : 0;
    if (nb > 0 && s.seg_out) {
        if ((rc = launch_segments(e, s, nb, false))) return rc;
    } else if (nb > 0) {
        size_t bytes = 0;
        sess2_ends_kernel<<<grid_for(nb, 256 * 32), kBlock, 0, e->stream>>>(s);
        HIPCHK(e, hipGetLastError());
        KidEq eq{tb};
        bytes = 0;
        HIPCHK(e, hipcub::DeviceScan::InclusiveScanByKey(nullptr, bytes, (const unsigned long long*)s.bkey, (const int64_t*)s.bend,
                                                         s.bmax, MaxI64(), (int)nb, eq, e->stream));
        if ((rc = ensure_sort_tmp(e, bytes))) return rc;
        bytes = e->sort_tmp_bytes;
        HIPCHK(e, hipcub::DeviceScan::InclusiveScanByKey(e->d_sort_tmp, bytes, (const unsigned long long*)s.bkey, (const int64_t*)s.bend,
                                                         s.bmax, MaxI64(), (int)nb, eq, e->stream));
        Sess2Args h = s;
        h.bcid = e->d_sval[0];                               // head flags (the unsorted payload is dead)
        sess2_heads_kernel<<<grid_for(nb, 256 * 32), kBlock, 0, e->stream>>>(h);
        HIPCHK(e, hipGetLastError());
        bytes = 0;
        HIPCHK(e, hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const uint32_t*)h.bcid, s.bcid, (int)nb, e->stream));
        if ((rc = ensure_sort_tmp(e, bytes))) return rc;
        bytes = e->sort_tmp_bytes;
        HIPCHK(e, hipcub::DeviceScan::InclusiveSum(e->d_sort_tmp, bytes, (const uint32_t*)h.bcid, s.bcid, (int)nb, e->stream));
        sess2_init_kernel<<<grid_for(nb, 256 * 32), kBlock, 0, e->stream>>>(s, e->d_ec);
        sess2_reduce_kernel<<<grid_for(nb, 256 * 32), kBlock, 0, e->stream>>>(s, e->d_ec);
        HIPCHK(e, hipGetLastError());
    }
    if (nsp > 0) {
        if (nsp > e->sc_cap) {
            HIPCHK(e, hipStreamSynchronize(e->stream));
            if (e->d_sc) HIPCHK(e, hipFree(e->d_sc));
            e->d_sc = nullptr;
            e->sc_cap = nsp + nsp / 4 + 1024;
            HIPCHK(e, hipMalloc(&e->d_sc, 8 * (size_t)e->sc_cap * (2 + e->nacc)));
        }
        size_t bytes = 0;
        const int eb = std::min(64, 32 + e->kid_bits);
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const unsigned long long*)e->d_skey[2], e->d_skey[3],
                                                     (const uint32_t*)e->d_sval[2], e->d_sval[3], (int)nsp, 0, eb, e->stream));
        if ((rc = ensure_sort_tmp(e, bytes))) return rc;
        bytes = e->sort_tmp_bytes;
        HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(e->d_sort_tmp, bytes, (const unsigned long long*)e->d_skey[2], e->d_skey[3],
                                                     (const uint32_t*)e->d_sval[2], e->d_sval[3], (int)nsp, 0, eb, e->stream));
        s.skey = e->d_skey[3];
        s.sval = e->d_sval[3];
        s.sc_start = e->d_sc;
        s.sc_end = e->d_sc + nsp;
        s.sc_acc = (unsigned long long*)(e->d_sc + 2 * nsp);
        if ((rc = ensure_late_rows(e, e->late_rows + nsp))) return rc;
        if (!e->d_lr_n) HIPCHK(e, hipMalloc(&e->d_lr_n, 8));
        if ((rc = upload(e, e->d_lr_n, &e->late_rows, 8))) return rc;
        s.lr_key = e->lr_col[0];
        s.lr_start = e->lr_col[1];
        s.lr_end = e->lr_col[2];
        for (int j = 0; j < e->cfg.num_aggs; ++j) s.lr_agg[j] = e->lr_col[3 + j];
        s.lr_n = e->d_lr_n;
        s.lr_cap = e->lr_cap;
        sess2_ordered_kernel<<<grid_for(nsp, 256 * 32), kBlock, 0, e->stream>>>(s, e->d_ec);
        HIPCHK(e, hipGetLastError());
    }
    HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
    uint32_t ncl = 0;
    unsigned long long lrn = (unsigned long long)e->late_rows;
    if (nb > 0 && !s.seg_out) HIPCHK(e, hipMemcpyAsync(&ncl, e->d_scid + nb - 1, 4, hipMemcpyDeviceToHost, e->stream));
    if (nsp > 0) HIPCHK(e, hipMemcpyAsync(&lrn, e->d_lr_n, 8, hipMemcpyDeviceToHost, e->stream));
    if ((rc = read_sess_ctr(e))) return rc;
    if ((rc = account_ingest(e))) return rc;
    e->ingest_launches++;
    e->ingest_records += n;
    if (e->h_st->error) return FWA_OK;
    e->late_rows = (int64_t)lrn;
    e->n_ss = (int64_t)ncl + (int64_t)e->h_sctr->n_out_sp;
    e->ss_cur ^= 1;
    *dropped_out = (int64_t)e->h_st->dropped;
    return FWA_OK;
}

// Watermark advance for sessions: late-firing rows of the pushes since the last call first, then every
// session with prev < end - 1 <= wm; sessions past cleanup are dropped from the list.
static int fire_sessions(fwa_engine* e, int64_t wm, int64_t* nrows) {
    const int64_t n_in = e->n_ss;
    int rc = ensure_out(e, e->late_rows + n_in);
    if (rc) return rc;
    if (e->late_rows > 0 && (rc = emit_late_rows(e))) return rc;
    if ((rc = upload(e, &e->d_st->rows, &e->late_rows, 8))) return rc;
    e->rows_zero = false;
    SessCtr z;
    memset(&z, 0, sizeof(z));
    if ((rc = upload(e, e->d_sctr, &z, sizeof(z)))) return rc;
    if ((rc = ensure_sess_lists(e, n_in))) return rc;
    Sess2FireArgs f;
    memset(&f, 0, sizeof(f));
    f.in = e->ss[e->ss_cur];
    f.out = e->ss[e->ss_cur ^ 1];
    f.n_in = n_in;
    f.prev_wm = local_wm(e, e->wm);
    f.wm = local_wm(e, wm);
    f.lateness = e->lateness;
    f.key_table = e->d_keys;
    f.capacity = e->capacity;
    f.o_key = e->o_key;
    f.o_start = e->o_start;
    f.o_end = e->o_end;
    for (int j = 0; j < e->cfg.num_aggs; ++j) { f.o_agg[j] = e->o_agg[j]; f.o_null[j] = e->o_null[j]; }
    f.out_cap = e->out_cap;
    f.ctr = e->d_sctr;
    f.st = e->d_st;
    HIPCHK(e, hipEventRecord(e->ev[2], e->stream));
    if (n_in > 0)
        sess2_fire_kernel<<<(unsigned)((n_in + (int64_t)kBlock * kSessFireItems - 1) / ((int64_t)kBlock * kSessFireItems)), kBlock, 0,
                            e->stream>>>(f, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[3], e->stream));
    if ((rc = read_sess_ctr(e))) return rc;
    if (e->h_st->error) return fail(e, e->h_st->error, "session fire failed");
    *nrows = (int64_t)e->h_st->rows;
    e->n_ss = (int64_t)e->h_sctr->n_keep;
    e->ss_cur ^= 1;
    e->late_rows = 0;
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev[2], e->ev[3]));
    e->fire_ms += ms;
    e->fire_launches++;
    e->fire_rows += *nrows;
    return FWA_OK;
}
// Sessions: the blob's entries are the in-flight sessions (key, start, count, acc_j..., end) bucketed by
// key group -- the per-key MergingWindowSet mapping plus the window state of WindowOperator
// (WindowOperator.java:224-238 mergingSetsState / windowState), with the session end as a last column.
static int snapshot_sessions(fwa_engine* e, fwa_blob* out) {
    const int64_t n = e->n_ss;
    const int na = e->cfg.num_aggs, maxp = e->cfg.max_parallelism, nh = e->ec.naggs - e->ec.nout;
    const bool ph = e->cfg.key_kind == FWA_KEY_PREHASHED;   // + one column: each entry's key.hashCode()
    const int ncols = 4 + na + nh + (ph ? 1 : 0);
    const SessList& L = e->ss[e->ss_cur];
    std::vector<int32_t> khash(ph ? (size_t)e->capacity + 1 : 0);
    if (ph && n > 0) HIPCHK(e, hipMemcpy(khash.data(), e->d_khash, 4 * ((size_t)e->capacity + 1), hipMemcpyDeviceToHost));
    std::vector<uint32_t> kid((size_t)n);
    std::vector<int64_t> st((size_t)n), en((size_t)n), acc((size_t)n * e->nacc);
    std::vector<unsigned long long> table((size_t)e->capacity + 1);
    if (n > 0) {
        HIPCHK(e, hipMemcpy(kid.data(), L.kid, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(st.data(), L.start, 8 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(en.data(), L.end, 8 * (size_t)n, hipMemcpyDeviceToHost));
        for (int cc = 0; cc < e->nacc; ++cc)
            HIPCHK(e, hipMemcpy(acc.data() + (size_t)cc * n, L.acc + (size_t)cc * L.stride, 8 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(table.data(), e->d_keys, 8 * (size_t)e->capacity, hipMemcpyDeviceToHost));
    }
    std::vector<int32_t> kg((size_t)n);
    std::vector<int64_t> off((size_t)maxp + 1, 0), key((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        key[i] = (int64_t)kid[i] < e->capacity ? (int64_t)table[kid[i]] : LONG_MIN_J;
        kg[i] = jm::key_group_of(key[i], e->cfg.key_kind, ph ? khash[kid[i]] : 0, maxp);
        if (kg[i] < 0) return fail(e, FWA_E_STATE, "state holds a key outside every key group");
        off[kg[i] + 1]++;
    }
    for (int g = 0; g < maxp; ++g) off[g + 1] += off[g];
    std::vector<int64_t> dsec;                         // COUNT(DISTINCT): the set's live entries behind the body
    int64_t dm = 0;
    if (e->dist) { if (int rc = dist_snapshot_section(e, &dsec, &dm)) return rc; }
    const size_t words0 = kSnapHdr + (size_t)maxp + 1 + (size_t)n * ncols, words = words0 + dsec.size();
    int64_t* b = (int64_t*)malloc(words * 8);
    if (!b) return fail(e, FWA_E_OOM, "snapshot blob allocation failed");
    snap_header(e, b, n);
    b[28] = dm;
    if (!dsec.empty()) memcpy(b + words0, dsec.data(), 8 * dsec.size());
    memcpy(b + kSnapHdr, off.data(), 8 * ((size_t)maxp + 1));
    int64_t* body = b + kSnapHdr + maxp + 1;
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t d = cur[kg[i]]++;
        body[d] = key[i];
        body[(size_t)n + d] = st[i];
        body[(size_t)2 * n + d] = acc[i];                                  // COUNT(*)
        for (int j = 0; j < na; ++j) {
            const AggDesc& ad = e->ec.agg[j];
            body[(size_t)(3 + j) * n + d] = ad.acc > 0 ? acc[(size_t)ad.acc * n + i] : acc[i];
        }
        for (int h = 0; h < nh; ++h) body[(size_t)(3 + na + h) * n + d] = acc[(size_t)e->ec.agg[e->ec.nout + h].acc * n + i];
        body[(size_t)(3 + na + nh) * n + d] = en[i];
        if (ph) body[(size_t)(4 + na + nh) * n + d] = khash[kid[i]];
    }
    out->data = b;
    out->size = (int64_t)(words * 8);
    return FWA_OK;
}

__global__ void __launch_bounds__(kBlock) sess2_restore_kernel(Sess2Args a, const int64_t* keys, const int64_t* start,
                                                               const int64_t* end, const int64_t* const* accs, int64_t m,
                                                               int64_t at, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t kid = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, keys[i], a.st);
        if (kid < 0) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); continue; }
        const int64_t o = at + i;
        a.out.kid[o] = (uint32_t)kid;
        a.out.start[o] = start[i];
        a.out.end[o] = end[i];
        for (int cc = 0; cc < c.nacc; ++cc) a.out.acc[(int64_t)cc * a.out.stride + o] = (unsigned long long)accs[cc][i];
    }
}

// Restore sessions: the owned key groups' entries of every blob are appended to the in-flight list
// (a key lives in one subtask's snapshot, so the lists never overlap); watermark = MIN over the blobs.
static int restore_sessions(fwa_engine* e, const void* const* blobs, int32_t n_blobs) {
    const int na = e->cfg.num_aggs, maxp = e->cfg.max_parallelism, nh = e->ec.naggs - e->ec.nout;
    int64_t wm = LONG_MAX_J;
    for (int32_t b = 0; b < n_blobs; ++b) {
        const int64_t* h = (const int64_t*)blobs[b];
        const int64_t n = h[21];
        wm = std::min<int64_t>(wm, h[20]);
        const int64_t* off = h + kSnapHdr;
        const int64_t lo = off[e->cfg.kg_start], hi = off[e->cfg.kg_end + 1];
        if (lo < 0 || hi < lo || hi > n) return fail(e, FWA_E_ARG, "corrupt key-group offsets");
        if (e->dist) {   // the set's entries of this handle's key groups, folded back into block and bit
            const int ncols = 4 + na + nh + (e->cfg.key_kind == FWA_KEY_PREHASHED ? 1 : 0);
            if (int rcd = dist_restore_section(e, off + maxp + 1 + (size_t)n * ncols, h[28])) return rcd;
        }
        const int64_t m = hi - lo;
        if (m == 0) continue;
        const int64_t* body = off + maxp + 1;
        int rc = ensure_sess_lists(e, e->n_ss + m);
        if (rc) return rc;
        // device copies: key, start, end, one column per accumulator (COUNT, then each owner aggregate's)
        const int nc = 3 + e->nacc;
        int64_t* d = nullptr;
        HIPCHK(e, hipMalloc(&d, 8 * (size_t)m * nc));
        std::vector<const int64_t*> src(nc);
        src[0] = body + lo;
        src[1] = body + (size_t)n + lo;
        src[2] = body + (size_t)(3 + na + nh) * n + lo;
        src[3] = body + (size_t)2 * n + lo;
        for (int cc = 1; cc < e->nacc; ++cc) {
            for (int j = 0; j < na; ++j)
                if (e->ec.agg[j].acc == cc && !e->ec.agg[j].alias) src[3 + cc] = body + (size_t)(3 + j) * n + lo;
            for (int h = 0; h < nh; ++h)   // hidden non-NULL counters
                if (e->ec.agg[e->ec.nout + h].acc == cc) src[3 + cc] = body + (size_t)(3 + na + h) * n + lo;
        }
        std::vector<const int64_t*> hacc(e->nacc);
        for (int c = 0; c < nc; ++c) HIPCHK(e, hipMemcpy(d + (size_t)c * m, src[c], 8 * (size_t)m, hipMemcpyHostToDevice));
        for (int cc = 0; cc < e->nacc; ++cc) hacc[cc] = d + (size_t)(3 + cc) * m;
        const int64_t** dacc = nullptr;
        HIPCHK(e, hipMalloc(&dacc, sizeof(int64_t*) * e->nacc));
        HIPCHK(e, hipMemcpy(dacc, hacc.data(), sizeof(int64_t*) * e->nacc, hipMemcpyHostToDevice));
        Sess2Args s;
        memset(&s, 0, sizeof(s));
        s.key_table = e->d_keys;
        s.key_mask = (uint64_t)e->capacity - 1;
        s.seg_log = e->seg_log;
        s.part_bits = e->part_bits;
        s.out = e->ss[e->ss_cur];
        s.st = e->d_st;
        sess2_restore_kernel<<<grid_for(m), kBlock, 0, e->stream>>>(s, d, d + m, d + 2 * m, dacc, m, e->n_ss, e->d_ec);
        HIPCHK(e, hipGetLastError());
        if (e->d_khash) {                         // PREHASHED: the entries' key.hashCode() (last column) by kid
            std::vector<int32_t> hv((size_t)m);
            for (int64_t i = 0; i < m; ++i) hv[i] = (int32_t)body[(size_t)(4 + na + nh) * n + lo + i];
            int32_t* dh = nullptr;
            HIPCHK(e, hipMalloc(&dh, sizeof(int32_t) * (size_t)m));
            HIPCHK(e, hipMemcpyAsync(dh, hv.data(), sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, e->stream));
            khash_fill_kernel<<<grid_for(m), kBlock, 0, e->stream>>>(d, dh, m, e->d_keys, (uint64_t)e->capacity - 1,
                                                                     e->seg_log, e->part_bits, e->d_khash);
            HIPCHK(e, hipGetLastError());
            HIPCHK(e, hipStreamSynchronize(e->stream));
            (void)hipFree(dh);
        }
        rc = sync_status(e);
        (void)hipFree(d);
        (void)hipFree(dacc);
        if (rc) return rc;
        if (e->h_st->error) return fail(e, e->h_st->error, "key table full: raise fwa_config.key_capacity");
        e->n_ss += m;
    }
    if (n_blobs > 0) e->wm = wm;
    return FWA_OK;
}
