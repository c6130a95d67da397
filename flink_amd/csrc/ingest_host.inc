// Two-phase ingest, host side (included by engine.hip): a push's slice tables, its V2Shape (ingest_launch.inc), the
// kernel arguments and the two launches through the instantiation tables. Kernels: ingest.inc.

static int ensure_v2_buffers(fwa_engine* e, int64_t n, bool need_bn) {
    const int64_t per = n / ((int64_t)e->np * kSub);                 // expected records per sub-bucket
    const int64_t capb = per + per / 4 + 2048;
    if (capb > e->capb) {
        for (void* p : {(void*)e->d_bkey, (void*)e->d_brel, (void*)e->d_bn, (void*)e->d_bval[0], (void*)e->d_bval[1]}) if (p) HIPCHK(e, hipFree(p));
        e->d_bkey = nullptr;
        e->d_brel = nullptr;
        e->d_bn = nullptr;
        e->d_bval[0] = e->d_bval[1] = nullptr;
        const int64_t ent = capb * e->np * kSub + 8 * kMaxPart;  // + a trash area (partition3's masked stores)
        HIPCHK(e, hipMalloc(&e->d_bkey, (e->nv == 1 ? 12 : 8) * ent));   // 12: narrow {key, value, slice} entries
        HIPCHK(e, hipMalloc(&e->d_brel, 2 * ent));
        for (int v = 0; v < e->nv; ++v) HIPCHK(e, hipMalloc(&e->d_bval[v], 8 * ent));
        e->capb = capb;
    }
    if (need_bn && !e->d_bn) HIPCHK(e, hipMalloc(&e->d_bn, 2 * (e->capb * e->np * kSub + 8 * kMaxPart)));
    if (!e->d_bcnt) {
        HIPCHK(e, hipMalloc(&e->d_bcnt, sizeof(uint32_t) * kMaxPart * kSub));
        HIPCHK(e, hipMalloc(&e->d_rel2slot, (sizeof(int32_t) + 2) * kRelCap));   // rel2slot | relcode | relfresh
    }
    return FWA_OK;
}

// FWA_OPT_PROFILE: wait for a profiled kernel (events a, b) and print its per-block phase cycle counters (average
// over the nb blocks and the slowest block): Phase P marks 6 phases, Phase A 8.
static int print_phase_profile(fwa_engine* e, const char* tag, hipEvent_t a, hipEvent_t b, int nb, int nph) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, a, b));
    std::vector<long long> hp(8 * (size_t)nb);
    HIPCHK(e, hipMemcpy(hp.data(), e->d_prof, sizeof(long long) * 8 * nb, hipMemcpyDeviceToHost));
    double tot[8] = {0};
    int bmax = 0;
    long long bsum_max = -1;
    for (int blk = 0; blk < nb; ++blk) {
        long long bs = 0;
        for (int k = 0; k < nph; ++k) { tot[k] += (double)hp[blk * 8 + k] / nb; bs += hp[blk * 8 + k]; }
        if (bs > bsum_max) { bsum_max = bs; bmax = blk; }
    }
    fprintf(stderr, "[%s] kernel %.3f ms; per-block avg cycles:", tag, ms);
    for (int k = 0; k < nph; ++k) fprintf(stderr, " %.0f", tot[k]);
    fprintf(stderr, " | slowest block %d:", bmax);
    for (int k = 0; k < nph; ++k) fprintf(stderr, " %lld", hp[bmax * 8 + k]);
    fprintf(stderr, "\n");
    return FWA_OK;
}

// The push's V2Shape. *v2 = false: the batch keeps the v1 path (partial accumulators of an aggregate list the PRE
// buckets cannot carry).
static int plan_v2(fwa_engine* e, const IngestArgs& a, V2Shape* out, bool* v2) {
    V2Shape s;
    memset(&s, 0, sizeof(s));
    s.nv = e->nv;
    for (int v = 0; v < e->nv; ++v) s.vw |= e->vsize[v] == 8 ? 1 << v : 0;
    // combiner accumulator layout (compile-time in combine3) and the skew mode (PRE, partition3)
    // (layout 1 adds the carried value: not for a lone COUNT(col) over a nullable column, an ADD_I64 accumulator
    // without a value column, which the general layout feeds 1 per record)
    if (e->nacc_comb == 1) s.layout = 2;
    else if (e->nacc_comb == 2 && s.nv == 1 && e->ec.acc_kind[1] == ACC_ADD_I64) {
        for (int j = 0; j < e->cfg.num_aggs; ++j)
            if (e->ec.agg[j].acc == 1 && e->ec.agg[j].vslot == 0) s.layout = 1;
    }
    const bool pre_ok = (s.layout == 2 && s.nv == 0) || (s.layout == 1 && s.nv == 1 && (s.vw & 1));
    // partial accumulators (fwa_push_partials): the PRE buckets carry each row's record count, the value
    // column is the partial BIGINT sum; other aggregate lists keep the v1 path
    *v2 = !(a.pcount && (!pre_ok || e->cfg.nullable_cols || e->opt_partials_v1));
    if (!*v2) return FWA_OK;
    s.pre = a.pcount || (pre_ok && e->opt_pre != 0 && (e->opt_pre == 1 || e->pre));
    s.mp = e->opt_mp == 1 || (e->opt_mp != 0 && e->mp);   // combiner window passes (slices smaller than chunks)
    // ownership is checked per record unless the handle owns every key group; dictionary ids always (their key group
    // may be past max_parallelism: key group -1, rejected with FWA_E_KEYGROUP)
    const bool kg_all = e->cfg.kg_start == 0 && e->cfg.kg_end == e->cfg.max_parallelism - 1 &&
                        e->cfg.key_kind != FWA_KEY_GROUP_PREFIXED;
    s.kgm = kg_all ? 0 : (e->cfg.key_kind == FWA_KEY_PREHASHED ? 2 : 1);
    // (partial rows carry another value column, fill_part_args; they run PRE, which does not look at w16)
    auto al16 = [](const void* q) { return q == nullptr || ((uintptr_t)q & 15) == 0; };
    s.w16 = s.kgm == 0 && al16(a.keys) && al16(a.ts) &&
            (s.nv == 0 || ((uintptr_t)a.cols[e->vcol[0]] & ((s.vw & 1) ? 15 : 7)) == 0);
    // narrow bucket entries (partition3 / combine3 NW): COUNT + one BIGINT SUM over an 8-byte column, the paired-load
    // kernel; on by default until a push finds more than 1/64 of its records needing 64-bit keys or values
    const bool nw_on = e->opt_narrow != 0 && (e->opt_narrow == 1 || e->narrow) && !s.pre;
    s.narrow = nw_on && s.layout == 1 && s.nv == 1 && (s.vw & 1) && s.w16;
    // ... and for an 8-byte value column beside a 4-byte one (C5: DOUBLE and FLOAT): key and FLOAT bits share a word
    s.narrow2 = nw_on && s.layout == 0 && s.nv == 2 && s.vw == 1 && s.kgm == 0;
    s.roll = !(e->opt_variant & 1024);
    s.old_body = (e->opt_variant & 2) != 0;
    if (!v2_shape_valid(s)) return fail(e, FWA_E_INTERNAL, "two-phase ingest: the handle's shape breaks v2_shape_valid");
    e->narrow_used = s.narrow || s.narrow2;
    *out = s;
    return FWA_OK;
}

// rel2slot (combine), relcode (partition) and relfresh: the directory restricted to [q_base, q_base + kRelCap) with each
// slice's acceptance under the current watermark (WindowOperator.isWindowLate / SlicingWindowOperator lateness, as in
// ingest_kernel); by value for a narrow span, else uploaded. Resets the push status.
static int build_rel_tables(fwa_engine* e, const IngestArgs& a, const V2Shape& s, int64_t q_base) {
    std::vector<int32_t> r2s(kRelCap + kRelCap / 2, -1);
    uint8_t* code = (uint8_t*)(r2s.data() + kRelCap);
    memset(code, kCodeSlow, kRelCap);
    // slots no record reached yet hold their identities: the combiner's merge of such a slice stores without reading
    uint8_t* fresh = code + kRelCap;
    memset(fresh, 0, kRelCap);
    int64_t rel_hi = -1;                              // (rel_lo = 0: q_base is the first live slice)
    // stale slots (DESIGN.md section 5) under the slices of this push: the combiner overwrites them (fresh 2) when it
    // merges every slice of its window once and no other kernel writes slots first; otherwise they are reset here. Live
    // slices past the tables reach their slots through the v1 replay only: reset too.
    const bool lazy = !s.pre && !s.mp && !(e->opt_variant & (512 | 1));
    e->push_stale.clear();
    for (auto& kv : e->live) {
        const int64_t rel = kv.first - q_base;
        if (e->n_stale && e->stale[kv.second] && (!lazy || rel < 0 || rel >= kRelCap || e->touched[kv.second])) {
            e->stale[kv.second] = 0;
            e->n_stale--;
            e->pending_reset.push_back(kv.second);
        }
        if (rel < 0 || rel >= kRelCap) continue;
        rel_hi = rel;
        r2s[rel] = kv.second;
        fresh[rel] = (e->touched[kv.second] || (e->opt_variant & 1)) ? 0 : 1;   // variant bit 0: A/B without
        if (e->n_stale && e->stale[kv.second]) {
            fresh[rel] = 2;
            e->push_stale.push_back({kv.first, kv.second});
        }
        int64_t thr;
        bool always;
        accept_threshold(e, kv.first, &thr, &always);
        if (!always && !(a.wm < thr)) code[rel] = kCodeDrop;
        else if (e->lateness > 0 && a.wm >= trig(e, jm::wsub(first_window_end(e, kv.first), 1))) code[rel] = kCodeSlow;
        else code[rel] = kCodeAccept;
    }
    int rc = flush_resets(e);
    if (rc) return rc;
    if (rel_hi < kRelTabN && !(e->opt_variant & 256)) {   // a narrow span: the tables by value (variant bit 8: A/B)
        RelTab tab;
        memset(&tab, 0, sizeof(tab));
        tab.n = (int32_t)(rel_hi + 1);
        for (int32_t j = 0; j < tab.n; ++j) { tab.slot[j] = r2s[j]; tab.code[j] = code[j]; tab.fresh[j] = fresh[j]; }
        return reset_push_status(e, true, &tab);
    }
    if ((rc = upload(e, e->d_rel2slot, r2s.data(), (sizeof(int32_t) + 2) * kRelCap))) return rc;
    return reset_push_status(e, true);
}

static int fill_part_args(fwa_engine* e, const IngestArgs& a, const V2Shape& s, int64_t q_base, PartArgs& pa) {
    memset(&pa, 0, sizeof(pa));
    pa.keys = a.keys;
    pa.ts = a.ts;
    for (int c = 0; c < FWA_MAX_COLS; ++c) pa.cols[c] = a.cols[c];
    if (a.pcount) {                   // partial rows: cols[] is indexed by aggregate; the carried value is the
        pa.pcount = a.pcount;         // accumulator column of the BIGINT sum (layout 1)
        for (int j = 0; j < e->cfg.num_aggs; ++j)
            if (e->ec.agg[j].acc == 1 && s.layout == 1) pa.cols[e->vcol[0]] = a.cols[j];
    }
    pa.key_hash = a.key_hash;
    pa.n = a.n;
    pa.wm = a.wm;
    pa.relcode = (const uint8_t*)(e->d_rel2slot + kRelCap);
    pa.rel2slot = e->d_rel2slot;
    pa.touched = e->d_touched;
    pa.epoch = std::max<int32_t>(1, e->push_epoch);
    pa.spill = e->d_spill;
    pa.q_base = q_base;
    const jm::FastSlice fs = jm::fast_slice_make(e->g, kRelCap);
    if (!e->cfg.tz_n && fs.m && q_base > -(1ll << 40) && q_base < (1ll << 40)) {
        const __int128 b = (__int128)e->off + (__int128)q_base * e->g;
        if (b > (__int128)INT64_MIN / 2 && b < (__int128)INT64_MAX / 2) {
            pa.fast_sh = fs.sh;
            pa.fast_m = fs.m;
            pa.fast_lim = fs.lim;
            pa.base_ts = (int64_t)b;
            e->fast_slice_pushes++;
        }
    }
    pa.b_key = e->d_bkey;
    pa.b_rel = e->d_brel;
    pa.b_n = s.pre ? e->d_bn : nullptr;
    pa.key_table = e->d_keys;
    pa.key_mask = (uint64_t)e->capacity - 1;
    pa.seg_log = e->seg_log;
    pa.slot_base = e->d_slot_base;
    pa.stride = e->stride;
    pa.b_val0 = e->d_bval[0];
    pa.b_val1 = e->d_bval[1];
    pa.b_cnt = e->d_bcnt;
    pa.capb = e->capb;
    pa.trash = (uint64_t)e->capb * e->np * kSub;
    pa.spill_cap = e->spill_cap;
    pa.part_bits = e->part_bits;
    pa.np = e->np;
    pa.sub_major = (e->opt_variant & 4) ? 0 : 1;   // variant bit 2: partition-major buckets (A/B)
    pa.iota1 = e->ec.red_iota && e->nv == 2 && e->vcol[1] == kIotaCol && e->vsize[1] == 4 && !(e->opt_variant & 16);
    if (e->iota_pending && !pa.iota1) { int rc = ensure_iota(e); if (rc) return rc; }
    for (int v = 0; v < 2; ++v) { pa.vcol[v] = e->vcol[v]; pa.vsize[v] = e->vsize[v]; }
    pa.dropidx = a.pcount ? nullptr : a.dropidx;   // partial rows: no record indices (as in v1)
    for (int c = 0; c < FWA_MAX_COLS; ++c) { pa.nulls[c] = a.nulls[c]; pa.any_null |= a.nulls[c] != nullptr; }
    pa.st = e->d_st;
    if (e->opt_profile && !e->d_prof) HIPCHK(e, hipMalloc(&e->d_prof, sizeof(long long) * 8 * kMaxPart));
    pa.prof = e->opt_profile ? e->d_prof : nullptr;
    return FWA_OK;
}

// No host round trip between the phases: Phase P marks touched slots itself, spills bucket overflow to the v1 replay
// list, and the combiner applies stragglers in place.
static void fill_combine_args(const fwa_engine* e, const V2Shape& s, const PartArgs& pa, CombineArgs& ca) {
    memset(&ca, 0, sizeof(ca));
    ca.b_key = e->d_bkey;
    ca.b_rel = e->d_brel;
    ca.b_n = s.pre ? e->d_bn : nullptr;
    ca.key_table = e->d_keys;
    ca.b_val0 = e->d_bval[0];
    ca.b_val1 = e->d_bval[1];
    ca.b_cnt = e->d_bcnt;
    ca.capb = e->capb;
    ca.seg_log = e->seg_log;
    ca.np = e->np;
    ca.sl = e->sl;
    ca.sub_major = pa.sub_major;
    ca.rel2slot = e->d_rel2slot;
    // (not with PRE buckets: Phase P applies merged entries past a full sub-bucket to the slots with device atomics
    // before this merge -- tests/test_skew_gpu.py::test_pre_entries_past_bucket_end_applied_with_atomics)
    ca.relfresh = s.pre ? nullptr : (const uint8_t*)(e->d_rel2slot + kRelCap) + kRelCap;
    ca.stale = e->push_stale.empty() ? 0 : 1;
    ca.q_base = pa.q_base;
    ca.slot_base = e->d_slot_base;
    ca.stride = e->stride;
    ca.st = e->d_st;
    ca.prof = pa.prof;
}

// The instantiations of ingest_launch.inc's lists. A key without a row is an error, never another kernel.
struct P3Row { P3Key key; void (*fn)(PartArgs, const EngineConst*); };
struct C3Row { C3Key key; void (*fn)(CombineArgs, const EngineConst*); };
#define FWA_P3_ROW(NV, IT, VW, KG, PRE, W16, NW, ROLL) \
    {{NV, IT, VW, KG, PRE, W16, NW, ROLL, 0, 0}, partition3_kernel<NV, IT, 1024, VW, KG, PRE, W16, NW, ROLL>},
#define FWA_C3_ROW(IT, NV, LY, PRE, MP, NW, LEAN) \
    {{IT, NV, LY, PRE, MP, NW, LEAN}, combine3_kernel<IT, 2, NV, 1024, LY, PRE, MP, NW, LEAN>},
static const P3Row kP3Rows[] = {FWA_P3_INSTANCES(FWA_P3_ROW)};
static const C3Row kC3Rows[] = {FWA_C3_INSTANCES(FWA_C3_ROW)};
#undef FWA_P3_ROW
#undef FWA_C3_ROW

static int launch_partition3(fwa_engine* e, const V2Shape& s, const PartArgs& pa) {
    const P3Key k = p3_key(s);
    const P3Row* row = std::find_if(std::begin(kP3Rows), std::end(kP3Rows), [&](const P3Row& r) { return same_kernel(r.key, k); });
    if (row == std::end(kP3Rows)) {
        char msg[128];
        snprintf(msg, sizeof(msg), "no partition3_kernel<%d,%d,1024,%d,%d,%d,%d,%d,%d> in FWA_P3_INSTANCES", k.nv, k.items,
                 k.vw, k.kg, k.pre, k.w16, k.nw, k.roll);
        return fail(e, FWA_E_INTERNAL, msg);
    }
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((pa.n + k.tile - 1) / k.tile, k.max_grid));
    HIPCHK(e, hipEventRecord(e->ev[4], e->stream));
    row->fn<<<grid, 1024, 0, e->stream>>>(pa, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[5], e->stream));
    return e->opt_profile ? print_phase_profile(e, "pprof", e->ev[4], e->ev[5], grid, 6) : FWA_OK;
}

static int launch_combine3(fwa_engine* e, const V2Shape& s, const CombineArgs& ca) {
    const C3Key k = c3_key(s);
    const C3Row* row = std::find_if(std::begin(kC3Rows), std::end(kC3Rows), [&](const C3Row& r) { return same_kernel(r.key, k); });
    if (row == std::end(kC3Rows)) {
        char msg[128];
        snprintf(msg, sizeof(msg), "no combine3_kernel<%d,2,%d,1024,%d,%d,%d,%d,%d> in FWA_C3_INSTANCES", k.it, k.nv, k.layout,
                 k.pre, k.mp, k.nw, k.lean);
        return fail(e, FWA_E_INTERNAL, msg);
    }
    // LDS: the key segment, the 2-slice window of counts and of the other accumulators, the sub-bucket descriptors
    const size_t seg = (size_t)1 << e->seg_log;
    const size_t lds = seg * 8 + 2 * seg * 4 + (size_t)(e->nacc_comb - 1) * 2 * seg * 8 + 4 * 4 * kSub + 16;
    HIPCHK(e, hipEventRecord(e->ev[6], e->stream));
    row->fn<<<e->np, 1024, lds, e->stream>>>(ca, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[7], e->stream));
    e->v2_timing_pending = true;
    return e->opt_profile ? print_phase_profile(e, "aprof", e->ev[6], e->ev[7], e->np, 8) : FWA_OK;
}

// Two-phase ingest. Sets *ran = false (and leaves no state change besides key insertions) when the
// batch must take the v1 path instead.
static int push_v2(fwa_engine* e, IngestArgs& a, bool* ran) {
    *ran = false;
    V2Shape s;
    bool v2 = false;
    int rc = plan_v2(e, a, &s, &v2);
    if (rc || !v2) return rc;
    if ((rc = ensure_v2_buffers(e, a.n, s.pre))) return rc;
    const int64_t q_base = e->live.empty() ? 0 : e->live.begin()->first;
    if ((rc = build_rel_tables(e, a, s, q_base))) return rc;
    PartArgs pa;
    CombineArgs ca;
    if ((rc = fill_part_args(e, a, s, q_base, pa))) return rc;
    if ((rc = launch_partition3(e, s, pa))) return rc;
    fill_combine_args(e, s, pa, ca);
    if ((rc = launch_combine3(e, s, ca))) return rc;
    e->ingest_launches++;
    e->ingest_records += a.n;
    *ran = true;
    return FWA_OK;
}
