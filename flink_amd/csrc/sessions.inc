// Session kernels (merging windows): classify, route, bulk gap-scan, cell path, arrival-order walk, fire.
// Included by engine.hip inside its anonymous namespace, ahead of sessions4.inc; host side: sessions_host.inc.
// ------------------------------------------------------------------------------------------------
// sessions (merging windows): DataStream EventTimeSessionWindows + EventTimeTrigger (allowed lateness
// L >= 0) and the Table legacy GROUP BY SESSION (TR/operators/window/WindowOperator.java:331-398 with
// MergingWindowProcessFunction and EventTimeTriggers.afterEndOfWindow).
//
// State: a flat list of in-flight sessions {kid, start, end, acc[nacc]} (column 0 = COUNT), in no
// particular order; no per-key cap. A push rebuilds it (DESIGN.md §2 "Sessions"):
//  * Order-free records -- the lone window [ts, ts+gap) ends after the watermark (ts + gap - 1 > wm).
//    Such a record is never dropped, never fires on arrival, and merging is a union of intersecting
//    intervals, so the key's session set after the push is the connected components of (its in-flight
//    sessions + its new windows) regardless of arrival order (MergingWindowSet.addWindow :153-236,
//    TimeWindow.intersects/cover :116-124 -- touching windows merge). Bulk path: one radix sort by
//    (kid, start), a segmented max-scan of the ends (a new session starts where start > every earlier
//    end of the key), a cluster-id scan, and a wave-segmented reduction of the accumulators.
//  * A key with at least one order-sensitive record in the push (lone window already ends at or before
//    the watermark: it may be dropped, may fire on arrival with the session contents, or may be saved by
//    a session an earlier record of the push created) goes through an arrival-order walk instead: its
//    sessions and records sorted by (kid, arrival), one lane per key applying addWindow / isWindowLate /
//    EventTimeTrigger.onElement in order (WindowOperator.java:288-389). Late firings are written to the
//    late-row buffer (returned at the head of the next fwa_advance_watermark).
//  * Fire at a watermark advance prev -> wm: every session with prev < end - 1 <= wm emits a row
//    (EventTimeTrigger.onEventTime: sessions whose maxTimestamp <= prev already fired -- at a timer or
//    on an element); every session with cleanup = end - 1 + L <= wm is cleared (clearAllState).

struct SessCtr {                 // per-push device counters (zeroed by the host before a push / fire)
    unsigned long long ts_min, ts_max;   // ord-encoded, over records and in-flight session starts (cell pre-aggregation:
                                         // the smallest / largest cell number of the push)
    unsigned long long n_special;        // records whose lone window ends at or before the watermark
    unsigned long long n_bulk, n_sp;     // elements routed to the bulk / the arrival-order path
    unsigned long long n_out_sp;         // sessions written by the arrival-order path
    unsigned long long n_keep;           // fire: sessions kept
    unsigned long long n_redo;           // cell path: elements outside the cell range (the push is redone)
};

struct SessList {                // one in-flight session list (SoA)
    uint32_t* kid;
    int64_t* start;
    int64_t* end;
    unsigned long long* acc;     // [nacc][stride]
    int64_t stride;
};

struct Sess2Args {
    const int64_t* keys;
    const int64_t* ts;
    const void* cols[FWA_MAX_COLS];
    const int32_t* key_hash;
    const int64_t* gapc;         // per-record gaps (DynamicEventTimeSessionWindows) or nullptr: fixed `gap`
    const uint8_t* nulls[FWA_MAX_COLS];   // SQL NULL flags per value column (nullptr: no NULLs)
    int64_t n;
    int64_t wm, gap, lateness;
    unsigned long long* key_table;
    uint64_t key_mask;
    int32_t seg_log, part_bits;
    int64_t capacity;            // key-table capacity (side slot at capacity)
    uint32_t* rkid;              // [n] kid per record (0xffffffff: rejected)
    uint8_t* kflag;              // [capacity + 1] key has an order-sensitive record in this push
    SessList in;                 // in-flight sessions before the push
    int64_t n_in;
    SessList out;                // after the push
    // bulk path
    int64_t base;                // smallest start of the push (records and in-flight sessions)
    int32_t tb;                  // bits of (start - base) in the sort key (kid << tb | start - base)
    int32_t all_sp;              // 1: route everything through the arrival-order path
    unsigned long long* bkey;    // [nb] sort keys (then sorted)
    uint32_t* bval;              // [nb] payload: bulk position, | 0x80000000 when its end is in pe (sessions,
                                 // dynamic gaps)
    unsigned long long* pk;      // [nb][pkw] the element's COUNT + accumulator words, in bulk order (one row per
                                 // element gathered once after the sort, not one value column per accumulator)
    int64_t* pe;                 // [nb] end of a flagged element
    uint32_t* sg_kid;            // segment kernel staging: wave w's clusters at [h0(w), h0(w) + count(w)) (no atomics)
    int64_t* sg_start;
    int64_t* sg_end;
    unsigned long long* sg_acc;  // [nacc][cap]
    int64_t sg_cap;
    uint32_t* sg_cnt;            // [nw + 1] clusters per wave
    uint32_t* sg_off;            // [nw + 1] their exclusive sum
    int64_t* sg_h0;              // [nw] first owned position per wave
    int32_t pkw;
    jm::UDiv64 gap_div;          // cell path: cell = (start - base) / gap, base = ctr->ts_min
    int32_t seg_out;             // bulk sessions appended on ctr->n_out_sp by sess2_segment_kernel (the arrival-order
                                 // path appends after them on the same counter)
    int64_t* bend;               // [nb] window / session end per sorted element
    int64_t* bmax;               // [nb] inclusive max of bend over the key so far (segmented scan)
    uint32_t* bcid;              // [nb] head flags, then 1-based cluster ids (inclusive sum)
    int64_t nb;
    int32_t col_owner[1 + kMaxAggsInt];    // aggregate that feeds accumulator column c (-1: COUNT)
    // arrival-order path
    unsigned long long* skey;    // [ns] (kid << 32) | (0 for a session, 1 + record index)
    uint32_t* sval;
    int64_t nsp;
    int64_t* sc_start;           // [ns] scratch session lists, one region per key run
    int64_t* sc_end;
    unsigned long long* sc_acc;  // [nacc][ns]
    // late-firing rows
    int64_t* lr_key;
    int64_t* lr_start;
    int64_t* lr_end;
    void* lr_agg[FWA_MAX_AGGS];
    unsigned long long* lr_n;
    int64_t lr_cap;
    SessCtr* ctr;
    int32_t* dropidx;            // FWA_CFG_LATE_INDICES list (nullptr: not collected)
    DevStatus* st;
};

__device__ __forceinline__ int64_t sess_cleanup(int64_t max_ts, int64_t lateness) {   // WindowOperator.cleanupTime :647-654
    const int64_t ct = jm::wadd(max_ts, lateness);
    return ct >= max_ts ? ct : LONG_MAX_J;
}

__device__ __forceinline__ void wave_minmax(unsigned long long lo, unsigned long long hi, unsigned long long* dlo,
                                            unsigned long long* dhi) {
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const unsigned long long a = __shfl_xor(lo, sh), b = __shfl_xor(hi, sh);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) { atomicMin(dlo, lo); atomicMax(dhi, hi); }
}

// Pass 1 over the records: key-group check, kid, order-sensitivity flag per key, start range.
__global__ void __launch_bounds__(kBlock) sess2_classify_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    unsigned long long lo = ~0ull, hi = 0ull, nsp = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t key = a.keys[i];
        const int64_t ts = a.ts[i];
        a.rkid[i] = 0xffffffffu;
        const int32_t kg = jm::key_group_of(key, c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
        if (kg < c.kg_lo || kg > c.kg_hi) { raise_error(a.st, FWA_E_KEYGROUP); continue; }   // StateTable :300-307
        const int64_t gap = a.gapc ? a.gapc[i] : a.gap;
        if (gap <= 0) { raise_error(a.st, FWA_E_ARG); continue; }   // DynamicEventTimeSessionWindows.java:60-64
        const int64_t kid = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key, a.st);
        if (kid < 0) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); continue; }
        a.rkid[i] = (uint32_t)kid;
        if (jm::wsub(jm::wadd(ts, gap), 1) <= a.wm) { a.kflag[kid] = 1; ++nsp; }   // lone window maxTs <= wm
        const unsigned long long o = jm::ord_i64(ts);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
    wave_minmax(lo, hi, &a.ctr->ts_min, &a.ctr->ts_max);
    for (int sh = 32; sh >= 1; sh >>= 1) nsp += __shfl_xor(nsp, sh);
    if ((threadIdx.x & 63) == 0 && nsp) atomicAdd(&a.ctr->n_special, nsp);
}

__global__ void __launch_bounds__(kBlock) sess2_range_kernel(Sess2Args a) {
    unsigned long long lo = ~0ull, hi = 0ull;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_in; j += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long o = jm::ord_i64(a.in.start[j]);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
    wave_minmax(lo, hi, &a.ctr->ts_min, &a.ctr->ts_max);
}

// Pass 2: route every record and in-flight session to the bulk sort or the arrival-order sort. A block
// owns a contiguous chunk of kRouteItems * blockDim elements and reserves its two output runs with one
// atomic per list (a per-wave reservation on one counter serialised 1M waves per push: 12.8 ms on C5s).
constexpr int kRouteItems = 16;
__device__ __forceinline__ void route_elem(const Sess2Args& a, int64_t t, bool& valid, bool& sp, unsigned long long& bk,
                                           unsigned long long& sk, uint32_t& pay) {
    valid = false; sp = false; bk = 0; sk = 0; pay = 0;
    if (t < a.n) {
        const uint32_t kid = a.rkid[t];
        if (kid == 0xffffffffu) return;
        valid = true;
        sp = a.all_sp || a.kflag[kid];
        pay = (uint32_t)t;
        bk = ((unsigned long long)kid << a.tb) | (uint64_t)(a.ts[t] - a.base);
        sk = ((unsigned long long)kid << 32) | (uint64_t)(t + 1);
    } else if (t < a.n + a.n_in) {
        const int64_t j = t - a.n;
        const uint32_t kid = a.in.kid[j];
        valid = true;
        sp = a.all_sp || a.kflag[kid];
        pay = (uint32_t)j | 0x80000000u;
        bk = ((unsigned long long)kid << a.tb) | (uint64_t)(a.in.start[j] - a.base);
        sk = (unsigned long long)kid << 32;
    }
}

__global__ void __launch_bounds__(kBlock) sess2_route_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    constexpr int kW = kBlock / 64;
    __shared__ uint32_t s_wb[kW], s_ws[kW];
    __shared__ unsigned long long s_base[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kBlock * kRouteItems;
    uint32_t nbk = 0, nsp = 0;
    for (int j = 0; j < kRouteItems; ++j) {
        bool valid, sp; unsigned long long bk, sk; uint32_t pay;
        route_elem(a, c0 + (int64_t)j * kBlock + threadIdx.x, valid, sp, bk, sk, pay);
        nbk += (uint32_t)__popcll(__ballot(valid && !sp));
        nsp += (uint32_t)__popcll(__ballot(valid && sp));
    }
    if (lane == 0) { s_wb[wv] = nbk; s_ws[wv] = nsp; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tb = 0, ts = 0;
        for (int w = 0; w < kW; ++w) { const uint32_t x = s_wb[w], y = s_ws[w]; s_wb[w] = tb; s_ws[w] = ts; tb += x; ts += y; }
        s_base[0] = tb ? atomicAdd(&a.ctr->n_bulk, (unsigned long long)tb) : 0ull;
        s_base[1] = ts ? atomicAdd(&a.ctr->n_sp, (unsigned long long)ts) : 0ull;
    }
    __syncthreads();
    unsigned long long pb = s_base[0] + s_wb[wv], ps = s_base[1] + s_ws[wv];
    const unsigned long long lt = (1ull << lane) - 1;
    for (int j = 0; j < kRouteItems; ++j) {
        bool valid, sp; unsigned long long bk, sk; uint32_t pay;
        route_elem(a, c0 + (int64_t)j * kBlock + threadIdx.x, valid, sp, bk, sk, pay);
        const unsigned long long mb = __ballot(valid && !sp), ms = __ballot(valid && sp);
        if (valid && !sp) {
            const unsigned long long o = pb + __popcll(mb & lt);
            a.bkey[o] = bk;
            const bool sess = (pay & 0x80000000u) != 0;
            const bool flag = sess || a.gapc;
            a.bval[o] = (uint32_t)o | (flag ? 0x80000000u : 0u);
            unsigned long long* row = a.pk + (int64_t)o * a.pkw;
            const int64_t x = (int64_t)(pay & 0x7fffffffu);
            const EngineConst& c = *cp;
            auto word = [&](int cc) -> unsigned long long {
                if (sess) return a.in.acc[(int64_t)cc * a.in.stride + x];
                if (cc == 0) return 1ull;
                const AggDesc& d = c.agg[a.col_owner[cc]];
                return acc_input(d, a.cols[d.col], x, a.nulls[d.col]);
            };
            int cc = 0;
            if ((a.pkw & 1) == 0)                                  // 16-byte stores (rows stay 16-byte aligned)
                for (; cc < a.pkw; cc += 2) *reinterpret_cast<ulonglong2*>(row + cc) = make_ulonglong2(word(cc), word(cc + 1));
            for (; cc < a.pkw; ++cc) row[cc] = word(cc);
            if (sess) a.pe[o] = a.in.end[x];
            else if (a.gapc) a.pe[o] = jm::wadd(a.ts[x], a.gapc[x]);
        }
        if (valid && sp) { const unsigned long long o = ps + __popcll(ms & lt); a.skey[o] = sk; a.sval[o] = pay; }
        pb += __popcll(mb);
        ps += __popcll(ms);
    }
}

// Bulk: end of every sorted element (records: start + gap; sessions: their end).
__global__ void __launch_bounds__(kBlock) sess2_ends_kernel(Sess2Args a) {
    const uint64_t smask = a.tb >= 64 ? ~0ull : (((uint64_t)1 << a.tb) - 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t p = a.bval[i];
        const int64_t start = a.base + (int64_t)(a.bkey[i] & smask);
        a.bend[i] = (p & 0x80000000u) ? a.pe[p & 0x7fffffffu] : jm::wadd(start, a.gap);
    }
}

// Bulk: head flag = first element of a key, or start after every earlier end of the key.
__global__ void __launch_bounds__(kBlock) sess2_heads_kernel(Sess2Args a) {
    const uint64_t smask = (((uint64_t)1 << a.tb) - 1);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nb; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t h = 1;
        if (i > 0) {
            const unsigned long long k = a.bkey[i], kp = a.bkey[i - 1];
            h = ((k >> a.tb) != (kp >> a.tb) || a.base + (int64_t)(k & smask) > a.bmax[i - 1]) ? 1u : 0u;
        }
        a.bcid[i] = h;
    }
}


__device__ __forceinline__ void acc_atomic(int acc_kind, unsigned long long* p, unsigned long long v) {
    switch (acc_kind) {
        case ACC_NONE: case ACC_ADD_I64: atomicAdd(p, v); break;
        case ACC_ADD_F64: atomicAdd((double*)p, __longlong_as_double((long long)v)); break;
        case ACC_MIN_ORD: atomicMin(p, v); break;
        case ACC_MAX_ORD: atomicMax(p, v); break;
        default: break;
    }
}

__global__ void __launch_bounds__(kBlock) sess2_init_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int64_t ncl = a.nb > 0 ? (int64_t)a.bcid[a.nb - 1] : 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ncl; j += (int64_t)gridDim.x * blockDim.x)
        for (int cc = 0; cc < c.nacc; ++cc) a.out.acc[(int64_t)cc * a.out.stride + j] = cc == 0 ? 0ull : ident_of(c.acc_kind[cc]);
}

// Bulk: wave-segmented reduction of each cluster (COUNT + accumulator columns). The cluster's true
// head writes kid and start, its true tail the end (= the key's running max end there); accumulators
// of a cluster that lies inside one wave are written with plain stores, a cluster spanning waves is
// combined into identity-initialised columns with atomics.
__global__ void __launch_bounds__(kBlock) sess2_reduce_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int lane = threadIdx.x & 63;
    const uint64_t smask = (((uint64_t)1 << a.tb) - 1);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t w0 = (int64_t)blockIdx.x * blockDim.x; w0 < a.nb; w0 += stride) {   // uniform trips per wave
        const int64_t wb = w0 + (threadIdx.x & ~63);     // this wave's first element
        const int64_t i = w0 + threadIdx.x;
        const bool act = i < a.nb;
        const int64_t cid = act ? (int64_t)a.bcid[i] : -1 - lane;   // inactive lanes: distinct ids
        const uint32_t p = act ? a.bval[i] : 0u;
        const int64_t cid0 = __shfl(cid, 0);
        const bool head0 = wb < a.nb && (wb == 0 || a.bcid[wb] != a.bcid[wb - 1]);
        const int64_t cn = __shfl_down(cid, 1);
        const bool last = act && (i + 1 >= a.nb || a.bcid[i + 1] != (uint32_t)cid);   // cluster's true tail
        const bool tail = act && (lane == 63 || cn != cid);                          // its last lane here
        const bool whole = (cid != cid0 || head0) && (lane != 63 || last);
        const int64_t cl = cid - 1;
        if (act && (i == 0 || a.bcid[i - 1] != (uint32_t)cid)) {
            a.out.kid[cl] = (uint32_t)(a.bkey[i] >> a.tb);
            a.out.start[cl] = a.base + (int64_t)(a.bkey[i] & smask);
        }
        if (last) a.out.end[cl] = a.bmax[i];
        for (int cc = 0; cc < c.nacc; ++cc) {
            const int ak = cc == 0 ? ACC_ADD_I64 : c.acc_kind[cc];
            unsigned long long v = act ? a.pk[(int64_t)(p & 0x7fffffffu) * a.pkw + cc] : 0ull;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned long long y = __shfl_up(v, d);
                const int64_t yc = __shfl_up(cid, d);
                if (lane >= d && yc == cid) v = acc_combine(ak, v, y);
            }
            if (!tail) continue;
            unsigned long long* dst = &a.out.acc[(int64_t)cc * a.out.stride + cl];
            if (whole) *dst = v;
            else acc_atomic(ak, dst, v);
        }
    }
}

// Bulk sessions after the (kid, start) sort in one pass, replacing ends / scan-by-key / heads / cluster-id scan /
// reduce: wave w owns the keys whose first sorted element lies in positions [64w, 64w + 64) and walks each owned key
// to its end in 64-element chunks, carrying the open cluster (the session being built) from chunk to chunk. Per chunk:
// the ends (start + gap, or the element's own end), the key's running max end (segmented shuffle scan; lane 0 joins
// the carried key), cluster heads (a new key, or a start after every earlier end of the key: TimeWindow.intersects is
// inclusive, so touching windows merge), the accumulators per cluster (segmented shuffle scans over the packed
// rows) and the completed clusters appended to the output list (one reservation per wave and chunk).
template <int NA>
__global__ void __launch_bounds__(kBlock) sess2_segment_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int lane = threadIdx.x & 63;
    const uint64_t smask = ((uint64_t)1 << a.tb) - 1;              // tb <= 63 - kid bits on this path
    const int64_t nb = a.nb;
    const int64_t nw = (nb + 63) >> 6;
    const int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int ak[NA];
#pragma unroll
    for (int cc = 0; cc < NA; ++cc) ak[cc] = cc == 0 ? ACC_ADD_I64 : c.acc_kind[cc];
    const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // lanes <= this one
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const int64_t p0 = w << 6;
        // a window of 128 sorted positions (this wave's 64 and the next 64) and the element before, loaded at once:
        // the heads, the end of the last owned key and the first two chunks come from it (one round trip)
        const int64_t pa = p0 + lane, pb = p0 + 64 + lane;
        const unsigned long long kA = pa < nb ? a.bkey[pa] : 0ull, kB = pb < nb ? a.bkey[pb] : 0ull;
        const uint32_t vA = pa < nb ? a.bval[pa] : 0u, vB = pb < nb ? a.bval[pb] : 0u;
        const unsigned long long kprev = p0 > 0 ? a.bkey[p0 - 1] : 0ull;
        const uint32_t kidA = (uint32_t)(kA >> a.tb), kidB = (uint32_t)(kB >> a.tb);
        const uint32_t kup = __shfl_up(kidA, 1);
        const bool hd = pa < nb && (lane == 0 ? (p0 == 0 || (uint32_t)(kprev >> a.tb) != kidA) : kidA != kup);
        const unsigned long long hm = __ballot(hd);
        if (!hm) {                                                  // inside a key owned by an earlier wave
            if (lane == 0) a.sg_cnt[w] = 0u;
            continue;
        }
        const int64_t h0 = p0 + (__ffsll((long long)hm) - 1);
        uint32_t wc = 0;                                            // clusters this wave wrote (staging h0 + i)
        int64_t h1 = min(p0 + 64, nb);
        if (h1 < nb) {                                              // the last owned key may run past the range
            const uint32_t kl = __shfl(kidA, 63);
            const unsigned long long dm = __ballot(pb >= nb || kidB != kl);
            if (dm) h1 = p0 + 64 + (__ffsll((long long)dm) - 1);
            else
                for (int64_t q = p0 + 128;; q += 64) {
                    const int64_t pp = q + lane;
                    const unsigned long long dq = __ballot(pp >= nb || (uint32_t)(a.bkey[pp] >> a.tb) != kl);
                    if (dq) { h1 = q + (__ffsll((long long)dq) - 1); break; }
                }
        }
        // chunk loads: key, payload, end, accumulator row of position base + lane (window or memory)
        auto fetch = [&](int64_t base, unsigned long long& bk, uint32_t& pay, int64_t& en, unsigned long long* x) {
            const int64_t q = base + lane;
            const int64_t d = q - p0;
            if (base + 63 - p0 < 128) {                             // inside the window
                const int src = (int)(d & 63);
                const unsigned long long ka = __shfl(kA, src), kb = __shfl(kB, src);
                const uint32_t va = __shfl(vA, src), vb = __shfl(vB, src);
                bk = d < 64 ? ka : kb;
                pay = d < 64 ? va : vb;
            } else {
                bk = q < h1 ? a.bkey[q] : 0ull;
                pay = q < h1 ? a.bval[q] : 0u;
            }
            const bool v = q < h1;
            const int64_t st = a.base + (int64_t)(bk & smask);
            en = !v ? LONG_MIN_J : (pay & 0x80000000u) ? a.pe[pay & 0x7fffffffu] : jm::wadd(st, a.gap);
            const uint32_t o = pay & 0x7fffffffu;
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) x[cc] = v ? a.pk[(int64_t)o * a.pkw + cc] : 0ull;
        };
        uint32_t ck = 0u;                                           // the carried open cluster
        int64_t cmax = LONG_MIN_J, cst = 0;
        unsigned long long cacc[NA];
#pragma unroll
        for (int cc = 0; cc < NA; ++cc) cacc[cc] = 0ull;
        bool copen = false;
        unsigned long long nbk, nx[NA];                             // the next chunk, in flight (software pipeline)
        uint32_t npay;
        int64_t nen;
        fetch(h0, nbk, npay, nen, nx);
        for (int64_t base = h0; base < h1; base += 64) {
            const int64_t q = base + lane;
            const bool v = q < h1;
            const unsigned long long bk = nbk;
            const int64_t en = nen;
            unsigned long long acc[NA];
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) acc[cc] = nx[cc];
            if (base + 64 < h1) fetch(base + 64, nbk, npay, nen, nx);
            const uint32_t kk = (uint32_t)(bk >> a.tb);
            const int64_t st = a.base + (int64_t)(bk & smask);
            const uint32_t kp = __shfl_up(kk, 1);
            const bool kc = v && (lane == 0 ? (!copen || kk != ck) : kk != kp);
            const unsigned long long km = __ballot(kc) & below;
            const int ks = km ? 63 - __clzll((long long)km) : 0;   // first lane of this lane's key in the chunk
            int64_t m = en;                                         // running max end of the key (inclusive)
            for (int d = 1; d < 64; d <<= 1) {
                const int64_t y = __shfl_up(m, d);
                if (lane - d >= ks && y > m) m = y;
            }
            if (km == 0 && copen && cmax > m) m = cmax;            // the key continues from the previous chunk
            int64_t mprev = __shfl_up(m, 1);
            if (lane == 0) mprev = cmax;
            const bool head = v && (kc || st > mprev);
            const unsigned long long hb = __ballot(head) & below;
            const int cs = hb ? 63 - __clzll((long long)hb) : 0;   // first lane of this lane's cluster in the chunk
            const bool ccont = hb == 0;                            // still the carried cluster
            const int64_t hst = __shfl(st, cs);
            const int64_t cstart = ccont ? cst : hst;
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) {
                unsigned long long x = acc[cc];
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned long long y = __shfl_up(x, d);
                    if (lane - d >= cs) x = acc_combine(ak[cc], x, y);
                }
                if (ccont && copen) x = acc_combine(ak[cc], cacc[cc], x);
                acc[cc] = x;
            }
            const bool nxt = __shfl_down(head ? 1 : 0, 1) != 0;
            const bool tail = v && (q + 1 == h1 || (lane < 63 && nxt));
            const bool emit_c = copen && __shfl(head ? 1 : 0, 0) != 0;   // the carried cluster ended before lane 0
            if (emit_c && lane == 0) {
                const int64_t sc = h0 + (int64_t)wc;
                a.sg_kid[sc] = ck;
                a.sg_start[sc] = cst;
                a.sg_end[sc] = cmax;
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) a.sg_acc[(int64_t)cc * a.sg_cap + sc] = cacc[cc];
            }
            wc += emit_c ? 1u : 0u;
            const unsigned long long tm = __ballot(tail);
            if (tail) {
                const int64_t so = h0 + (int64_t)wc + __popcll(tm & ((1ull << lane) - 1ull));
                a.sg_kid[so] = kk;
                a.sg_start[so] = cstart;
                a.sg_end[so] = m;                                   // the key's max end at the cluster's last element
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) a.sg_acc[(int64_t)cc * a.sg_cap + so] = acc[cc];
            }
            wc += (uint32_t)__popcll(tm);
            ck = __shfl(kk, 63);
            cmax = __shfl(m, 63);
            cst = __shfl(cstart, 63);
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) cacc[cc] = __shfl(acc[cc], 63);
            copen = true;
        }
        if (lane == 0) { a.sg_cnt[w] = wc; a.sg_h0[w] = h0; }
    }
}

// The segment kernel's clusters, moved from each wave's staging range to the output list at the exclusive sum of the
// per-wave counts (one thread per wave; the arrival-order path appends after them on ctr->n_out_sp).
// One thread per output session (coalesced stores): the staging wave w that owns output dst is the last one with
// sg_off[w] <= dst (a binary search over the scanned counts, which stay cache-resident); a thread per wave copying its
// ~1.4 clusters serially took 0.24 ms per C5s push.
__global__ void __launch_bounds__(kBlock) sess2_compact_kernel(Sess2Args a, int64_t nw, int nacc) {
    const int64_t tot = a.sg_off[nw];
    for (int64_t dst = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; dst < tot; dst += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nw;                          // invariant: sg_off[lo] <= dst < sg_off[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)a.sg_off[mid] <= dst) lo = mid; else hi = mid;
        }
        const int64_t src = a.sg_h0[lo] + (dst - (int64_t)a.sg_off[lo]);
        a.out.kid[dst] = a.sg_kid[src];
        a.out.start[dst] = a.sg_start[src];
        a.out.end[dst] = a.sg_end[src];
        for (int cc = 0; cc < nacc; ++cc) a.out.acc[(int64_t)cc * a.out.stride + dst] = a.sg_acc[(int64_t)cc * a.sg_cap + src];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.ctr->n_out_sp = (unsigned long long)tot;
}

// ---- Cell path: fixed gap, every record of the push order-free ------------------------------------------------------
// The time axis is cut into cells of width gap starting at base = the smallest start of the push. Two windows whose
// starts lie in one cell intersect (s2 - s1 < gap <= end1 - s1, TimeWindow.intersects), so the elements of one
// (kid, cell) group end in one session whatever their order: sorting by the 32-bit key kid << cb | cell (cb = 32 -
// kid_bits) replaces the (kid, start) sort (4 one-byte passes over 8-byte pairs instead of 5 over 12-byte pairs), and
// the segment walk reduces each group (min start, max end, accumulators) before chaining the key's groups in cell
// order. Records go to the sort at their input position (no compaction); a record that is not order-free or a start
// outside the cell range is counted and the host redoes the push on the general path (sess2_*).
constexpr uint32_t kCellSent = 0xffffffffu;        // sorts last; its kid (all ones in kid_bits) is never a real kid

__global__ void __launch_bounds__(kBlock) sess3_min_kernel(Sess2Args a) {
    __shared__ unsigned long long s_lo[kBlock / 64];
    unsigned long long lo = ~0ull;
    const int64_t tot = a.n + a.n_in;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long o = jm::ord_i64(t < a.n ? a.ts[t] : a.in.start[t - a.n]);
        lo = o < lo ? o : lo;
    }
    for (int sh = 32; sh >= 1; sh >>= 1) { const unsigned long long y = __shfl_xor(lo, sh); lo = y < lo ? y : lo; }
    if ((threadIdx.x & 63) == 0) s_lo[threadIdx.x >> 6] = lo;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) lo = s_lo[w] < lo ? s_lo[w] : lo;
        if (lo != ~0ull) atomicMin(&a.ctr->ts_min, lo);
    }
}

// Probe of the key's first 8-slot bucket (one 64-byte read); -1 when the key is not there (then key_slot, which also
// inserts). Loads only: the caller issues several before using any.
__device__ __forceinline__ int64_t key_probe8(const unsigned long long* table, int seg_log, int part_bits, int64_t key,
                                             ulonglong2 (&bk)[4], uint64_t& i0) {
    const uint64_t h = jm::mix64((uint64_t)key);
    const uint64_t smask = ((uint64_t)1 << seg_log) - 1;
    i0 = seg_base(h, seg_log, part_bits) | (h & smask & ~(uint64_t)(kBucket - 1));
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(table + i0);
#pragma unroll
    for (int j = 0; j < 4; ++j) bk[j] = p[j];
    return 0;
}
__device__ __forceinline__ int64_t key_probe8_find(const ulonglong2 (&bk)[4], uint64_t i0, int64_t key) {
    const unsigned long long k = (unsigned long long)key;
    int64_t r = -1;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        if (bk[j].y == k) r = (int64_t)(i0 + 2 * j + 1);
        if (bk[j].x == k) r = (int64_t)(i0 + 2 * j);
    }
    return r;
}

// Records: block b routes its chunk [b * chunk, (b + 1) * chunk): key-group check, kid (U records' bucket probes in
// flight at once), 32-bit cell key and payload (the row position) at the record's input position, and the packed row
// [ts, acc_1 .. acc_{nacc-1}] (COUNT is 1 for a record) at the same position.
template <int U>
__global__ void __launch_bounds__(kBlock) sess3_route_kernel(Sess2Args a, const EngineConst* __restrict__ cp, int64_t chunk) {
    __shared__ uint32_t s_c[2];
    const EngineConst& c = *cp;
    if (threadIdx.x == 0) { s_c[0] = 0u; s_c[1] = 0u; }
    __syncthreads();
    const int cb = a.tb;
    const uint64_t ncell = (uint64_t)1 << cb;
    const uint64_t base = (uint64_t)jm::unord_i64(a.ctr->ts_min);
    uint32_t nsp = 0, nredo = 0;
    uint32_t* bkey = reinterpret_cast<uint32_t*>(a.bkey);
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(a.n, r0 + chunk);
    for (int64_t t0 = r0 + threadIdx.x; t0 < r1; t0 += (int64_t)blockDim.x * U) {
        int64_t key[U], ts[U], kid[U];
        ulonglong2 bk[U][4];
        uint64_t i0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t t = t0 + (int64_t)u * blockDim.x;
            key[u] = t < r1 ? a.keys[t] : 0;
            ts[u] = t < r1 ? a.ts[t] : 0;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) key_probe8(a.key_table, a.seg_log, a.part_bits, key[u], bk[u], i0[u]);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t t = t0 + (int64_t)u * blockDim.x;
            if (t >= r1) continue;
            uint32_t k32 = kCellSent;
            kid[u] = -1;
            const int32_t kg = jm::key_group_of(key[u], c.key_kind, a.key_hash ? a.key_hash[t] : 0, c.max_par);
            if (kg < c.kg_lo || kg > c.kg_hi) {
                raise_error(a.st, FWA_E_KEYGROUP);                     // StateTable :300-307
            } else {
                kid[u] = (uint64_t)key[u] == kEmptyKey ? -1 : key_probe8_find(bk[u], i0[u], key[u]);
                if (kid[u] < 0) kid[u] = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key[u], a.st);
                if (kid[u] < 0) {
                    a.st->key_full = 1;
                    raise_error(a.st, FWA_E_OOM);
                } else if (jm::wsub(jm::wadd(ts[u], a.gap), 1) <= a.wm) {   // order-sensitive: the general path
                    a.kflag[kid[u]] = 1;
                    ++nsp;
                } else {
                    const uint64_t cell = jm::udiv64((uint64_t)ts[u] - base, a.gap_div);
                    if (cell >= ncell) ++nredo;
                    else k32 = ((uint32_t)kid[u] << cb) | (uint32_t)cell;
                }
            }
            uint32_t pos = 0u;
            if (k32 != kCellSent) {
                pos = (uint32_t)t;
                unsigned long long* row = a.pk + (int64_t)pos * a.pkw;
                const int64_t tsu = ts[u];
                auto word = [&](int cc) -> unsigned long long {
                    if (cc == 0) return (unsigned long long)tsu;
                    const AggDesc& d = c.agg[a.col_owner[cc]];
                    return acc_input(d, a.cols[d.col], t, a.nulls[d.col]);
                };
                int cc = 0;
                if ((a.pkw & 1) == 0)
                    for (; cc < a.pkw; cc += 2) *reinterpret_cast<ulonglong2*>(row + cc) = make_ulonglong2(word(cc), word(cc + 1));
                for (; cc < a.pkw; ++cc) row[cc] = word(cc);
            }
            bkey[t] = k32;
            a.bval[t] = pos;
        }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) { nsp += __shfl_xor(nsp, sh); nredo += __shfl_xor(nredo, sh); }
    if ((threadIdx.x & 63) == 0 && (nsp | nredo)) { atomicAdd(&s_c[0], nsp); atomicAdd(&s_c[1], nredo); }
    __syncthreads();
    if (threadIdx.x == 0 && s_c[0]) atomicAdd(&a.ctr->n_special, (unsigned long long)s_c[0]);
    if (threadIdx.x == 0 && s_c[1]) atomicAdd(&a.ctr->n_redo, (unsigned long long)s_c[1]);
}

// In-flight sessions at sort positions n + j: cell key of their start, payload j | 0x80000000.
__global__ void __launch_bounds__(kBlock) sess3_route_sessions_kernel(Sess2Args a) {
    const int cb = a.tb;
    const uint64_t ncell = (uint64_t)1 << cb;
    const uint64_t base = (uint64_t)jm::unord_i64(a.ctr->ts_min);
    uint32_t* bkey = reinterpret_cast<uint32_t*>(a.bkey);
    uint32_t nredo = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_in; j += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t cell = jm::udiv64((uint64_t)a.in.start[j] - base, a.gap_div);
        uint32_t k32 = kCellSent;
        if (cell >= ncell) ++nredo;
        else k32 = (a.in.kid[j] << cb) | (uint32_t)cell;
        bkey[a.n + j] = k32;
        a.bval[a.n + j] = (uint32_t)j | 0x80000000u;
    }
    for (int sh = 32; sh >= 1; sh >>= 1) nredo += __shfl_xor(nredo, sh);
    if ((threadIdx.x & 63) == 0 && nredo) atomicAdd(&a.ctr->n_redo, (unsigned long long)nredo);
}

__device__ __forceinline__ uint32_t perm32(int dst4, uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_permute(dst4, (int)v); }
__device__ __forceinline__ unsigned long long perm64(int dst4, unsigned long long v) {
    const uint32_t lo = perm32(dst4, (uint32_t)v), hi = perm32(dst4, (uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// Cross-lane moves on the VALU (DPP) instead of the LDS crossbar: row_shr:n = 0x110 + n, row_bcast:15 = 0x142,
// row_bcast:31 = 0x143, wave_shl:1 = 0x130, wave_shr:1 = 0x138 (lanes without a source get 0)
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ uint32_t dpp32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, 0xf, false);
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ unsigned long long dpp64(unsigned long long v) {
    return ((unsigned long long)dpp32<CTRL, RM>((uint32_t)(v >> 32)) << 32) | dpp32<CTRL, RM>((uint32_t)v);
}
__device__ __forceinline__ unsigned long long rdlane64(unsigned long long v, int l) {   // wave-uniform l
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t rdlane32(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// Segmented inclusive scans: lane L combines the lanes [gs(L), L] (gs = first lane of L's segment) with the earlier
// part as the second operand. Hillis-Steele inside rows of 16 (row_shr 1, 2, 4, 8), then the row totals (row_bcast 15
// / 31); one accumulator kind per scan, branch-free (selects; the kind switch is taken once per scan, not per step).
template <int K>
__device__ __forceinline__ unsigned long long comb_k(unsigned long long x, unsigned long long y) {
    if constexpr (K == ACC_ADD_I64) return x + y;
    else if constexpr (K == ACC_ADD_F64)
        return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)x) + __longlong_as_double((long long)y));
    else if constexpr (K == ACC_MIN_ORD) return y < x ? y : x;
    else if constexpr (K == ACC_MAX_ORD) return y > x ? y : x;
    else return x;
}
template <int K>
__device__ __forceinline__ unsigned long long seg_scan_k(unsigned long long x, int lane, int gs) {
    unsigned long long y, r;
    y = dpp64<0x111>(x); r = comb_k<K>(x, y); x = ((lane & 15) >= 1 && lane - 1 >= gs) ? r : x;
    y = dpp64<0x112>(x); r = comb_k<K>(x, y); x = ((lane & 15) >= 2 && lane - 2 >= gs) ? r : x;
    y = dpp64<0x114>(x); r = comb_k<K>(x, y); x = ((lane & 15) >= 4 && lane - 4 >= gs) ? r : x;
    y = dpp64<0x118>(x); r = comb_k<K>(x, y); x = ((lane & 15) >= 8 && lane - 8 >= gs) ? r : x;
    y = dpp64<0x142, 0xa>(x); r = comb_k<K>(x, y); x = ((lane & 16) != 0 && gs < (lane & ~15)) ? r : x;
    y = dpp64<0x143, 0xc>(x); r = comb_k<K>(x, y); x = (lane >= 32 && gs < 32) ? r : x;
    return x;
}
__device__ __forceinline__ unsigned long long seg_scan_acc(int k, unsigned long long x, int lane, int gs) {
    switch (k) {
        case ACC_ADD_I64: return seg_scan_k<ACC_ADD_I64>(x, lane, gs);
        case ACC_ADD_F64: return seg_scan_k<ACC_ADD_F64>(x, lane, gs);
        case ACC_MIN_ORD: return seg_scan_k<ACC_MIN_ORD>(x, lane, gs);
        case ACC_MAX_ORD: return seg_scan_k<ACC_MAX_ORD>(x, lane, gs);
        default: return x;
    }
}
__device__ __forceinline__ int64_t seg_min64(int64_t x, int lane, int gs) {   // ord encoding: unsigned min
    return jm::unord_i64(seg_scan_k<ACC_MIN_ORD>(jm::ord_i64(x), lane, gs));
}
__device__ __forceinline__ int64_t seg_max64(int64_t x, int lane, int gs) {
    return jm::unord_i64(seg_scan_k<ACC_MAX_ORD>(jm::ord_i64(x), lane, gs));
}

// The cell-sorted elements in one pass. Ownership as in sess2_segment_kernel (wave w owns the keys whose first sorted
// element lies in [64w, 64w + 64) and walks each to its end). Per 64-element chunk: (1) segmented scans over the
// (kid, cell) groups -- min start, max end, accumulators -- joined with the group carried from the previous chunk;
// (2) the groups that end in the chunk are packed to the low lanes (ds_permute) and chained as sess2_segment_kernel
// chains elements: a group opens a session if it starts a key or starts after the key's running max end.
template <int NA>
__global__ void __launch_bounds__(kBlock) sess3_segment_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int lane = threadIdx.x & 63;
    const int cb = a.tb;
    const uint32_t* bkey = reinterpret_cast<const uint32_t*>(a.bkey);
    const int64_t nb = a.nb;
    const int64_t nw = (nb + 63) >> 6;
    const int64_t wstride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    int ak[NA];
    unsigned long long idn[NA];
#pragma unroll
    for (int cc = 0; cc < NA; ++cc) { ak[cc] = cc == 0 ? ACC_ADD_I64 : c.acc_kind[cc]; idn[cc] = ident_of(ak[cc]); }
    const unsigned long long below = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);   // lanes <= this one
    const unsigned long long before = (1ull << lane) - 1ull;                          // lanes < this one
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const int64_t p0 = w << 6;
        const int64_t pa = p0 + lane, pb = p0 + 64 + lane;
        const uint32_t kA = pa < nb ? bkey[pa] : kCellSent, kB = pb < nb ? bkey[pb] : kCellSent;
        const uint32_t vA = pa < nb ? a.bval[pa] : 0u, vB = pb < nb ? a.bval[pb] : 0u;
        const uint32_t kprev = p0 > 0 ? bkey[p0 - 1] : kCellSent;
        const uint32_t kidA = kA >> cb;
        const uint32_t kup = __shfl_up(kidA, 1);
        const bool okA = kA != kCellSent;
        const bool hd = okA && (lane == 0 ? (p0 == 0 || (kprev >> cb) != kidA) : kidA != kup);
        const unsigned long long hm = __ballot(hd);
        if (!hm) {
            if (lane == 0) a.sg_cnt[w] = 0u;
            continue;
        }
        const int64_t h0 = p0 + (__ffsll((long long)hm) - 1);
        int64_t h1;
        const unsigned long long sa = __ballot(!okA);               // sentinels / the end inside this range
        if (sa) {
            h1 = p0 + (__ffsll((long long)sa) - 1);
        } else {                                                    // the last owned key may run past the range
            const uint32_t kl = __shfl(kidA, 63);
            const unsigned long long dm = __ballot((kB >> cb) != kl);   // a sentinel's kid differs from every kid
            if (dm) h1 = p0 + 64 + (__ffsll((long long)dm) - 1);
            else
                for (int64_t q = p0 + 128;; q += 64) {
                    const int64_t pp = q + lane;
                    const uint32_t kq = pp < nb ? bkey[pp] : kCellSent;
                    const unsigned long long dq = __ballot((kq >> cb) != kl);
                    if (dq) { h1 = q + (__ffsll((long long)dq) - 1); break; }
                }
        }
        auto fetch = [&](int64_t base, uint32_t& bk, int64_t& st, int64_t& en, unsigned long long* x) {
            const int64_t q = base + lane;
            const int64_t d = q - p0;
            uint32_t pay;
            if (base + 63 - p0 < 128) {                             // inside the loaded window
                const int src = (int)(d & 63);
                const uint32_t ka = __shfl(kA, src), kb = __shfl(kB, src);
                const uint32_t va = __shfl(vA, src), vb = __shfl(vB, src);
                bk = d < 64 ? ka : kb;
                pay = d < 64 ? va : vb;
            } else {
                bk = q < h1 ? bkey[q] : kCellSent;
                pay = q < h1 ? a.bval[q] : 0u;
            }
            const uint32_t o = pay & 0x7fffffffu;
            if (q >= h1) {
                bk = kCellSent;
                st = LONG_MAX_J;
                en = LONG_MIN_J;
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) x[cc] = idn[cc];
            } else if (pay & 0x80000000u) {                         // in-flight session
                st = a.in.start[o];
                en = a.in.end[o];
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) x[cc] = a.in.acc[(int64_t)cc * a.in.stride + o];
            } else {                                                // record: packed row [ts, acc_1 ..]
                const unsigned long long* row = a.pk + (int64_t)o * NA;
                unsigned long long wv[NA];
                if constexpr ((NA & 1) == 0) {
#pragma unroll
                    for (int cc = 0; cc < NA; cc += 2) {
                        const ulonglong2 p = reinterpret_cast<const ulonglong2*>(row)[cc >> 1];
                        wv[cc] = p.x;
                        wv[cc + 1] = p.y;
                    }
                } else {
#pragma unroll
                    for (int cc = 0; cc < NA; ++cc) wv[cc] = row[cc];
                }
                st = (int64_t)wv[0];
                en = jm::wadd(st, a.gap);
                x[0] = 1ull;
#pragma unroll
                for (int cc = 1; cc < NA; ++cc) x[cc] = wv[cc];
            }
        };
        // Carries (wave-uniform): the pending group (its last element not seen yet: its session is undecided) and the
        // open session (every group before the pending one that belongs to it).
        bool gopen = false, copen = false;
        uint32_t gkey = 0u, ck = 0u;
        int64_t gmin = 0, gmax = 0, cmaxe = LONG_MIN_J, cst = 0;
        unsigned long long gacc[NA], cacc[NA];
#pragma unroll
        for (int cc = 0; cc < NA; ++cc) { gacc[cc] = 0ull; cacc[cc] = 0ull; }
        uint32_t wc = 0;                                            // sessions this wave wrote (staging h0 + i)
        uint32_t nbk;
        int64_t nst, nen;
        unsigned long long nx[NA];
        fetch(h0, nbk, nst, nen, nx);
        for (int64_t base = h0; base < h1; base += 64) {
            const int64_t q = base + lane;
            const bool v = q < h1;
            const uint32_t bk = nbk;
            int64_t st = nst, en = nen;
            unsigned long long x[NA];
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) x[cc] = nx[cc];
            const bool more = base + 64 < h1;
            if (more) fetch(base + 64, nbk, nst, nen, nx);
            // (1) groups: min start / max end per (kid, cell) run, joined with the pending group at lane 0
            const uint32_t gup = dpp32<0x138>(bk);                  // lane - 1
            const bool cont0 = gopen && rdlane32(bk, 0) == gkey;    // lane 0 continues the pending group
            const bool gf = v && (lane == 0 ? !cont0 : bk != gup);
            const unsigned long long GF = __ballot(gf);
            const unsigned long long gm = GF & below;
            const int gs = gm ? 63 - __clzll((long long)gm) : 0;
            st = seg_min64(st, lane, gs);
            en = seg_max64(en, lane, gs);
            if (gm == 0 && cont0) {
                st = gmin < st ? gmin : st;
                en = gmax > en ? gmax : en;
            }
            const uint32_t nk0 = rdlane32(nbk, 0);                  // the next chunk's first key (when `more`)
            const uint32_t gdn = dpp32<0x130>(bk);                  // lane + 1
            const bool gt = v && (q + 1 == h1 || (lane < 63 ? gdn != bk : nk0 != bk));   // the group's last element
            const int lv = (int)min<int64_t>(63, h1 - 1 - base);   // last valid lane
            const unsigned long long P = __ballot(gt);
            const bool pend = ((P >> lv) & 1ull) == 0;              // the last group continues in the next chunk
            // (2) chain the groups that end here, packed to lanes [0, np): heads and session tails
            const int np = __popcll(P);
            uint32_t kk = 0u;
            int64_t gst = 0, m = LONG_MIN_J, cstart = 0;
            bool head = false, ptail = false;
            unsigned long long H = 0ull;
            if (np) {
                const int dst = gt ? __popcll(P & before) : np + __popcll(~P & before);
                kk = perm32(dst * 4, bk >> cb);
                gst = (int64_t)perm64(dst * 4, (unsigned long long)st);
                const int64_t gen = (int64_t)perm64(dst * 4, (unsigned long long)en);
                const bool range_end = base + lv + 1 == h1;         // the last packed group closes the walk
                const bool pv = lane < np;
                const uint32_t kp = dpp32<0x138>(kk);
                const bool kc = pv && (lane == 0 ? (!copen || kk != ck) : kk != kp);
                const unsigned long long km = __ballot(kc) & below;
                const int ks = km ? 63 - __clzll((long long)km) : 0;
                m = seg_max64(pv ? gen : LONG_MIN_J, lane, ks);     // running max end of the key (inclusive)
                if (km == 0 && copen && cmaxe > m) m = cmaxe;       // the key continues from the open session
                int64_t mprev = (int64_t)dpp64<0x138>((unsigned long long)m);
                if (lane == 0) mprev = cmaxe;
                head = pv && (kc || gst > mprev);
                H = __ballot(head);
                const unsigned long long hb = H & below;
                const int cs = hb ? 63 - __clzll((long long)hb) : 0;
                const int64_t hst = __shfl(gst, cs);
                cstart = hb == 0 ? cst : hst;
                ptail = pv && (lane == np - 1 ? range_end : (lane < 63 && ((H >> ((lane + 1) & 63)) & 1ull) != 0));
            }
            // (3) accumulators once, per element, segmented by session: a segment starts at lane 0, at the first
            // element of every head group, and at the first element of the pending group
            const unsigned long long Pge = P & ~before;             // groups ending at or after this lane
            const int tl = Pge ? __ffsll((long long)Pge) - 1 : 64;  // this lane's group tail (64: pending group)
            const int rk = __popcll(P & ((tl < 64) ? ((1ull << tl) - 1ull) : ~0ull));   // its packed rank
            const bool ghead = tl < 64 && ((H >> rk) & 1ull) != 0;
            const unsigned long long SS = __ballot(v && gf && (tl == 64 || ghead)) | 1ull;
            const unsigned long long sm = SS & below;
            const int ss = 63 - __clzll((long long)sm);
            // prefix of the first segment: the open session unless its first group is a head, then the pending group
            // that lane 0 continues
            const bool g0end = (P & ~0ull) != 0;                    // the group at lane 0 ends in this chunk
            const bool pre_c = copen && g0end && (H & 1ull) == 0;
            const bool pre_g = cont0;
#pragma unroll
            for (int cc = 0; cc < NA; ++cc) {
                unsigned long long xx = seg_scan_acc(ak[cc], x[cc], lane, ss);
                if (ss == 0 && pre_g) xx = acc_combine(ak[cc], xx, gacc[cc]);
                if (ss == 0 && pre_c) xx = acc_combine(ak[cc], xx, cacc[cc]);
                x[cc] = xx;
            }
            // the open session ended before the first group here
            const bool emit_c = copen && np > 0 && (H & 1ull) != 0;
            if (emit_c && lane == 0) {
                const int64_t sc = h0 + (int64_t)wc;
                a.sg_kid[sc] = ck;
                a.sg_start[sc] = cst;
                a.sg_end[sc] = cmaxe;
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) a.sg_acc[(int64_t)cc * a.sg_cap + sc] = cacc[cc];
            }
            wc += emit_c ? 1u : 0u;
            // sessions ending at an element lane (the tail of a packed group whose session ends)
            const int rsrc = gt ? __popcll(P & before) : 0;
            const int ptl = __shfl(ptail ? 1 : 0, rsrc);           // every lane takes part in the shuffle
            const bool etail = gt && ptl != 0;
            const int64_t e_start = __shfl(cstart, rsrc);
            const int64_t e_end = __shfl(m, rsrc);
            const unsigned long long tm = __ballot(etail);
            if (etail) {
                const int64_t so = h0 + (int64_t)wc + __popcll(tm & before);
                a.sg_kid[so] = bk >> cb;
                a.sg_start[so] = e_start;
                a.sg_end[so] = e_end;
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) a.sg_acc[(int64_t)cc * a.sg_cap + so] = x[cc];
            }
            wc += (uint32_t)__popcll(tm);
            // carries
            if (np) {
                const int tlast = 63 - __clzll((long long)P);       // element lane of the last ended group
                ck = rdlane32(kk, np - 1);
                cmaxe = (int64_t)rdlane64((unsigned long long)m, np - 1);
                cst = (int64_t)rdlane64((unsigned long long)cstart, np - 1);
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) cacc[cc] = rdlane64(x[cc], tlast);
                copen = true;
            }
            gopen = pend;
            if (pend) {
                gkey = rdlane32(bk, lv);
                gmin = (int64_t)rdlane64((unsigned long long)st, lv);
                gmax = (int64_t)rdlane64((unsigned long long)en, lv);
#pragma unroll
                for (int cc = 0; cc < NA; ++cc) gacc[cc] = rdlane64(x[cc], lv);
            }
        }
        if (lane == 0) { a.sg_cnt[w] = wc; a.sg_h0[w] = h0; }
    }
}

__device__ __forceinline__ int64_t sess_key_of(const unsigned long long* key_table, int64_t capacity, uint32_t kid) {
    return (int64_t)kid < capacity ? (int64_t)key_table[kid] : LONG_MIN_J;   // side slot: the sentinel key
}

// Arrival-order path: one lane per key run of the (kid, arrival)-sorted list; its in-flight sessions
// come first (low word 0), then its records in arrival order. The run's scratch region [t, t + len)
// holds its session list (a run of len elements never has more than len sessions).
__global__ void __launch_bounds__(kBlock) sess2_ordered_kernel(Sess2Args a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int nacc = c.nacc;
    const bool table = c.sem == FWA_SEM_TABLE;
    const int64_t ncl = (a.seg_out || a.nb == 0) ? 0 : (int64_t)a.bcid[a.nb - 1];
    unsigned long long dropped = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.nsp; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t kid = (uint32_t)(a.skey[t] >> 32);
        if (t > 0 && (uint32_t)(a.skey[t - 1] >> 32) == kid) continue;   // not the head of the key's run
        int64_t* ss = a.sc_start + t;
        int64_t* se = a.sc_end + t;
        auto acc = [&](int cc, int64_t s) -> unsigned long long& { return a.sc_acc[(int64_t)cc * a.nsp + t + s]; };
        int64_t ns = 0;
        bool failed = false;
        for (int64_t j = t; j < a.nsp && (uint32_t)(a.skey[j] >> 32) == kid && !failed; ++j) {
            const uint32_t p = a.sval[j];
            if (p & 0x80000000u) {                              // an in-flight session of this key
                const int64_t q = p & 0x7fffffffu;
                ss[ns] = a.in.start[q];
                se[ns] = a.in.end[q];
                for (int cc = 0; cc < nacc; ++cc) acc(cc, ns) = a.in.acc[(int64_t)cc * a.in.stride + q];
                ++ns;
                continue;
            }
            const int64_t r = p;
            const int64_t ts = a.ts[r];
            const int64_t ws = ts, we = jm::wadd(ts, a.gapc ? a.gapc[r] : a.gap);   // EventTimeSessionWindows.assignWindows :61-63
            // MergingWindowSet.addWindow: the in-flight sessions intersecting the new window
            int64_t first = -1, nm = 0, cs = ws, ce = we;
            bool covers = false;
            for (int64_t s = 0; s < ns; ++s) {
                if (!(ss[s] <= we && se[s] >= ws)) continue;    // TimeWindow.intersects
                ++nm;
                if (first < 0) first = s;
                cs = ss[s] < cs ? ss[s] : cs;                   // TimeWindow.cover
                ce = se[s] > ce ? se[s] : ce;
                covers = covers || (ss[s] <= ws && se[s] >= we);
            }
            int64_t act = first;
            if (nm > 1 || (nm == 1 && !covers)) {               // MergeFunction.merge (WindowOperator.java:296-349)
                if (jm::wadd(jm::wsub(ce, 1), a.lateness) <= a.wm) { raise_error(a.st, FWA_E_MERGE_LATE); failed = true; break; }
                for (int64_t s = ns - 1; s >= 0; --s) {         // mergeNamespaces into the first, drop the rest
                    if (s == first || !(ss[s] <= we && se[s] >= ws)) continue;
                    for (int cc = 0; cc < nacc; ++cc)
                        acc(cc, first) = acc_combine(cc == 0 ? ACC_ADD_I64 : c.acc_kind[cc], acc(cc, first), acc(cc, s));
                    --ns;
                    if (s != ns) {
                        ss[s] = ss[ns]; se[s] = se[ns];
                        for (int cc = 0; cc < nacc; ++cc) acc(cc, s) = acc(cc, ns);
                        if (first == ns) first = s;
                    }
                }
                act = first;
                ss[act] = cs;
                se[act] = ce;
            }
            const int64_t aw_end = act >= 0 ? se[act] : we;
            if (sess_cleanup(jm::wsub(aw_end, 1), a.lateness) <= a.wm) {   // isWindowLate -> retireWindow, skip
                if (act >= 0) {
                    --ns;
                    if (act != ns) { ss[act] = ss[ns]; se[act] = se[ns]; for (int cc = 0; cc < nacc; ++cc) acc(cc, act) = acc(cc, ns); }
                }
                // Table: every skipped record counts (WindowOperator.java:386-389); DataStream: only if
                // isElementLate (WindowOperator.java:425-433, :597-601)
                if (table || jm::wadd(ts, a.lateness) <= a.wm) {
                    ++dropped;
                    if (a.dropidx) a.dropidx[atomicAdd(&a.st->drop_n, 1ull)] = (int32_t)r;
                }
                continue;
            }
            if (act < 0) {                                      // new self-contained session
                act = ns++;
                ss[act] = ws;
                se[act] = we;
                acc(0, act) = 0ull;
                for (int cc = 1; cc < nacc; ++cc) acc(cc, act) = ident_of(c.acc_kind[cc]);
            }
            acc(0, act) += 1ull;                                // windowState.add (AggregateFunction.add)
            for (int cc = 1; cc < nacc; ++cc)
                acc(cc, act) = acc_combine(c.acc_kind[cc], acc(cc, act),
                                           acc_input(c.agg[a.col_owner[cc]], a.cols[c.agg[a.col_owner[cc]].col], r,
                                                     a.nulls[c.agg[a.col_owner[cc]].col]));
            if (jm::wsub(se[act], 1) <= a.wm) {                 // EventTimeTrigger.onElement: FIRE at once
                const unsigned long long row = atomicAdd(a.lr_n, 1ull);
                if ((int64_t)row >= a.lr_cap) { raise_error(a.st, FWA_E_STATE); continue; }
                a.lr_key[row] = sess_key_of(a.key_table, a.capacity, kid);
                a.lr_start[row] = ss[act];
                a.lr_end[row] = se[act];
                for (int jj = 0; jj < c.nout; ++jj) {
                    const AggDesc d = c.agg[jj];
                    write_agg(d, acc(0, act), d.acc > 0 ? acc(d.acc, act) : 0ull, d.nn > 0 ? acc(d.nn, act) : 0ull,
                              a.lr_agg[jj], nullptr, (int64_t)row);
                }
            }
        }
        for (int64_t s = 0; s < ns; ++s) {                      // the key's sessions after the push
            const int64_t o = ncl + (int64_t)atomicAdd(&a.ctr->n_out_sp, 1ull);
            a.out.kid[o] = kid;
            a.out.start[o] = ss[s];
            a.out.end[o] = se[s];
            for (int cc = 0; cc < nacc; ++cc) a.out.acc[(int64_t)cc * a.out.stride + o] = acc(cc, s);
        }
    }
    for (int sh = 32; sh >= 1; sh >>= 1) dropped += __shfl_xor(dropped, sh);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&a.st->dropped, dropped);
}

struct Sess2FireArgs {
    SessList in, out;
    int64_t n_in;
    int64_t prev_wm, wm, lateness;
    const unsigned long long* key_table;
    int64_t capacity;
    int64_t* o_key;
    int64_t* o_start;
    int64_t* o_end;
    void* o_agg[FWA_MAX_AGGS];
    uint8_t* o_null[FWA_MAX_AGGS];
    int64_t out_cap;
    SessCtr* ctr;
    DevStatus* st;
};

// Watermark advance prev -> wm: emit every session with prev < end - 1 <= wm (EventTimeTrigger.onEventTime
// / AfterEndOfWindow); keep every session whose cleanup time is still after wm (clearAllState otherwise).
// A block owns a contiguous chunk of kSessFireItems * kBlock sessions and reserves its emitted rows and kept sessions
// with one atomic per counter (a per-wave reservation on the two counters serialised ~23 K waves per fire: 0.33 ms on
// C5s); the flags are computed twice, once to count and once to write.
constexpr int kSessFireItems = 16;
__global__ void __launch_bounds__(kBlock) sess2_fire_kernel(Sess2FireArgs f, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    constexpr int kW = kBlock / 64;
    __shared__ uint32_t s_wr[kW], s_wk[kW];
    __shared__ unsigned long long s_base[2];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c0 = (int64_t)blockIdx.x * kBlock * kSessFireItems;
    auto flags = [&](int64_t j, int64_t& end, bool& fire, bool& keep) {
        const bool act = j < f.n_in;
        end = act ? f.in.end[j] : 0;
        const int64_t mt = jm::wsub(end, 1);
        fire = act && mt > f.prev_wm && mt <= f.wm;
        keep = act && !(sess_cleanup(mt, f.lateness) <= f.wm);
    };
    uint32_t nr = 0, nk = 0;
    for (int it = 0; it < kSessFireItems; ++it) {
        int64_t end; bool fire, keep;
        flags(c0 + (int64_t)it * kBlock + threadIdx.x, end, fire, keep);
        nr += (uint32_t)__popcll(__ballot(fire));
        nk += (uint32_t)__popcll(__ballot(keep));
    }
    if (lane == 0) { s_wr[wv] = nr; s_wk[wv] = nk; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tr = 0, tk = 0;
        for (int w = 0; w < kW; ++w) { const uint32_t x = s_wr[w], y = s_wk[w]; s_wr[w] = tr; s_wk[w] = tk; tr += x; tk += y; }
        s_base[0] = tr ? atomicAdd(&f.st->rows, (unsigned long long)tr) : 0ull;
        s_base[1] = tk ? atomicAdd(&f.ctr->n_keep, (unsigned long long)tk) : 0ull;
    }
    __syncthreads();
    unsigned long long pr = s_base[0] + s_wr[wv], pk = s_base[1] + s_wk[wv];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int it = 0; it < kSessFireItems; ++it) {
        const int64_t j = c0 + (int64_t)it * kBlock + threadIdx.x;
        int64_t end; bool fire, keep;
        flags(j, end, fire, keep);
        const unsigned long long mf = __ballot(fire), mk = __ballot(keep);
        if (fire) {
            const unsigned long long row = pr + __popcll(mf & lt);
            if ((int64_t)row >= f.out_cap) raise_error(f.st, FWA_E_STATE);
            else {
                const uint32_t kid = f.in.kid[j];
                f.o_key[row] = sess_key_of(f.key_table, f.capacity, kid);
                f.o_start[row] = f.in.start[j];
                f.o_end[row] = end;
                const uint64_t cnt = f.in.acc[j];
                for (int jj = 0; jj < c.nout; ++jj) {
                    const AggDesc d = c.agg[jj];
                    write_agg(d, cnt, d.acc > 0 ? f.in.acc[(int64_t)d.acc * f.in.stride + j] : 0ull,
                              d.nn > 0 ? f.in.acc[(int64_t)d.nn * f.in.stride + j] : 0ull, f.o_agg[jj], f.o_null[jj], (int64_t)row);
                }
            }
        }
        if (keep) {
            const unsigned long long k = pk + __popcll(mk & lt);
            f.out.kid[k] = f.in.kid[j];
            f.out.start[k] = f.in.start[j];
            f.out.end[k] = end;
            for (int cc = 0; cc < c.nacc; ++cc) f.out.acc[(int64_t)cc * f.out.stride + k] = f.in.acc[(int64_t)cc * f.in.stride + j];
        }
        pr += __popcll(mf);
        pk += __popcll(mk);
    }
}
