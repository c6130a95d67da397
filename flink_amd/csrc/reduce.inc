// DataStream built-in reductions (FWA_CFG_REDUCE, include/flink_amd.h) -- included by engine.hip.
//
// Reference: WindowedStream.sum / min / max / minBy / maxBy(pos) (WindowedStream.java:680-890) are reduce() with
// SumAggregator (SumAggregator.java:66-76) or ComparableAggregator (ComparableAggregator.java:83-107); the window
// state is a ReducingState folded in arrival order (HeapReducingState.add: stored = reduce(stored, element)). The
// result is value1 with field pos replaced, so every other field is the window's FIRST element's, and minBy / maxBy
// keep the whole element whose pos field is extremal, ties to the first (or, first = false, the last) element.
//
// Design: the aggregated field is an ordinary accumulator column (SUM: wrapping add, MIN / MAX: ordered key in Java
// compareTo order, MINBY / MAXBY: the by-field's ordered key), COUNT(*) as always; the "selected element" (the first
// element, or the by-winner) is identified by its arrival sequence number seq = records before the push + batch
// index, kept per (key, slice) in a hidden column SELQ, and its other fields are copied into payload columns
// (ACC_PAYLOAD). Without a by-field (the first element; FWA_CFG_BY_LAST: the last) SELQ is an ordinary MIN (MAX)
// accumulator over an arrival-sequence column the push generates (red_iota: stored as the ordered key, taken by the
// two-phase ingest like any other aggregate), and one dense pass over the live slots copies the selected element's
// fields (red_iota_payload_kernel). MINBY / MAXBY select in passes over the records after the ingest (two-phase when
// every reduced field is a BIGINT / DOUBLE-SUM one the combiner carries, else the v1 atomics) applied the accumulators:
//   red_index_kernel    the (kid, slot) of every record the ingest accepted;
//   red_stale_kernel    MINBY / MAXBY: a slot whose by-value improved in this push (SELV != SELK, the value the stored
//                       selection was made at) drops its stored selection (SELQ := identity);
//   red_pick_kernel     records at the slot's (new) best value, or every record for the first-element rule, take
//                       atomicMin (first) / atomicMax (last) of seq into SELQ; SELK := SELV;
//   red_payload_kernel  the one record with seq == SELQ (per slot touched by it) writes its fields.
// An older selection at the same value keeps its smaller seq under atomicMin (ties go to the first element) and loses
// under atomicMax (ties to the last), exactly the arrival-order fold. The fire (red_fire_kernel) merges the slices of
// a window (SLIDE: slices of gcd(size, slide)): sums add, MIN / MAX fold, and the selection is the slice whose
// (by-value, seq) is best -- the element the window's own ReducingState would hold. Records that fire a window already
// past its trigger (allowed lateness > 0) are applied one by one in arrival order by red_late_fire_kernel. TUMBLE and
// SLIDE windows, and session windows of a Tuple2<key, field> (validate()); integer sums wrap like Java, a Float SUM is
// summed in double and rounded once unless the handle asks for the float32 arrival-order fold (FWA_CFG_F32_FOLD,
// f32fold.inc).

namespace {

__device__ __forceinline__ bool red_resolve(const IngestArgs& a, const EngineConst& c, int64_t i, int64_t* kid,
                                            int32_t* slot) {
    const int64_t key = a.keys[i];
    const int64_t ts = a.ts[i];
    const int32_t kg = jm::key_group_of(key, c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
    if (kg < c.kg_lo || kg > c.kg_hi || ts == LONG_MIN_J) return false;
    const int64_t d = jm::wsub(ts, c.off);
    const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
    const uint64_t uq = jm::udiv64(ud, c.g_div);
    const int64_t q = d >= 0 ? (int64_t)uq : ((uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1);
    const DirEntry* e = dir_find(a.dir, a.dir_mask, q);
    if (e == nullptr || e->slot < 0 || !((e->flags & 2) || a.wm < e->thr)) return false;   // dropped as late
    if (c.lateness_pos && a.wm >= e->first_maxts) return false;   // a late firing: red_late_fire_kernel applies it
    *kid = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key, a.st);           // present: the ingest
    *slot = e->slot;                                                                         // inserted it
    return *kid >= 0;
}

__global__ void __launch_bounds__(kBlock) red_index_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                           unsigned long long* rk) {
    const EngineConst& c = *cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t kid;
        int32_t slot;
        rk[i] = red_resolve(a, c, i, &kid, &slot) ? ((unsigned long long)kid | ((unsigned long long)slot << 40)) : ~0ull;
    }
}

__device__ __forceinline__ unsigned long long* red_col(const IngestArgs& a, unsigned long long r, int acc) {
    const int64_t kid = (int64_t)(r & ((1ull << 40) - 1));
    return a.slot_base[(int32_t)(r >> 40)] + (int64_t)acc * a.stride + kid;
}

__global__ void __launch_bounds__(kBlock) red_stale_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                           const unsigned long long* rk) {
    const EngineConst& c = *cp;
    const AggDesc by = c.agg[c.red_by];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long r = rk[i];
        if (r == ~0ull) continue;
        const unsigned long long selv = *red_col(a, r, by.acc);
        if (load_ord(a.cols[by.col], i, by.kind, 1) == selv && *red_col(a, r, c.red_selk) != selv)
            *red_col(a, r, c.red_selq) = c.red_last ? 0ull : ~0ull;    // the stored selection was made at a worse value
    }
}

__global__ void __launch_bounds__(kBlock) red_pick_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                          const unsigned long long* rk, int64_t seq0) {
    const EngineConst& c = *cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long r = rk[i];
        if (r == ~0ull) continue;
        if (c.red_by >= 0) {
            const AggDesc by = c.agg[c.red_by];
            const unsigned long long selv = *red_col(a, r, by.acc);
            if (load_ord(a.cols[by.col], i, by.kind, 1) != selv) continue;
            *red_col(a, r, c.red_selk) = selv;                         // every writer stores the same value
        }
        const unsigned long long seq = (unsigned long long)(seq0 + i);
        if (c.red_last) atomicMax(red_col(a, r, c.red_selq), seq);
        else atomicMin(red_col(a, r, c.red_selq), seq);
    }
}

__global__ void __launch_bounds__(kBlock) red_payload_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                             const unsigned long long* rk, int64_t seq0) {
    const EngineConst& c = *cp;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long r = rk[i];
        if (r == ~0ull || *red_col(a, r, c.red_selq) != (unsigned long long)(seq0 + i)) continue;
        for (int j = 0; j < c.nout; ++j) {                             // the selected element's fields
            const AggDesc d = c.agg[j];
            if (d.acc_kind != ACC_PAYLOAD || d.alias) continue;
            *red_col(a, r, d.acc) = (d.kind == FWA_FIRST_32 || d.kind == FWA_SEL_32)
                                        ? (unsigned long long)((const uint32_t*)a.cols[d.col])[i]
                                        : ((const unsigned long long*)a.cols[d.col])[i];
        }
    }
}

// MINBY / MAXBY selection, one pass over the records after the ingest settled (the by-accumulator holds each slot's
// best value v*): every record at v* takes atomicMin (first) / atomicMax (last) of its arrival sequence into the
// slot's scratch column SCR; red_by_payload_kernel then settles each slot from SCR alone. (Was: an index pass, a pass
// dropping stale selections, a pick pass and a payload pass over the records -- four random accesses per record.)
__global__ void __launch_bounds__(kBlock) red_by_kernel(IngestArgs a, const EngineConst* __restrict__ cp, int64_t seq0) {
    constexpr int U = 2;                                // records whose key-bucket probes are in flight together
    const EngineConst& c = *cp;
    const AggDesc by = c.agg[c.red_by];
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < a.n; i0 += U * step) {
        int64_t key[U], ts[U];
        unsigned long long v[U];
        ulonglong2 bk[U][4];
        uint64_t h0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {                   // clamped index: unconditional loads
            const int64_t i = min(i0 + (int64_t)u * step, a.n - 1);
            key[u] = a.keys[i];
            ts[u] = a.ts[i];
            v[u] = load_ord(a.cols[by.col], i, by.kind, 1);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) key_probe8(a.key_table, a.seg_log, a.part_bits, key[u], bk[u], h0[u]);
        int64_t kid[U];
        unsigned long long* slotb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            kid[u] = -1;
            slotb[u] = nullptr;
            const int64_t i = i0 + (int64_t)u * step;
            if (i >= a.n) continue;
            const int32_t kg = jm::key_group_of(key[u], c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
            if (kg < c.kg_lo || kg > c.kg_hi || ts[u] == LONG_MIN_J) continue;
            const int64_t d = jm::wsub(ts[u], c.off);
            const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
            const uint64_t uq = jm::udiv64(ud, c.g_div);
            const int64_t q = d >= 0 ? (int64_t)uq : ((uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1);
            const DirEntry* e = dir_find(a.dir, a.dir_mask, q);
            if (e == nullptr || e->slot < 0 || !((e->flags & 2) || a.wm < e->thr)) continue;   // dropped as late
            if (c.lateness_pos && a.wm >= e->first_maxts) continue;                              // a late firing
            int64_t k = (uint64_t)key[u] == kEmptyKey ? -1 : key_probe8_find(bk[u], h0[u], key[u]);
            if (k < 0) k = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key[u], a.st);   // present
            kid[u] = k;
            slotb[u] = a.slot_base[e->slot];
        }
        unsigned long long best[U];
#pragma unroll
        for (int u = 0; u < U; ++u) best[u] = kid[u] >= 0 ? slotb[u][(int64_t)by.acc * a.stride + kid[u]] : 0ull;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (kid[u] < 0 || v[u] != best[u]) continue;
            unsigned long long* scr = slotb[u] + (int64_t)c.red_scr * a.stride + kid[u];
            const unsigned long long seq = (unsigned long long)(seq0 + i0 + (int64_t)u * step) + 1ull;   // + 1: never 0
            if (c.red_last) atomicMax(scr, seq);
            else atomicMin(scr, seq);
        }
    }
}

// Per (slot, kid) of the live slots whose SCR names an element of this push: that element becomes the selection --
// unless (first-element rule) the slot already holds a selection made at the same best value, which arrived earlier --
// and its fields are copied; SCR goes back to its identity.
__global__ void __launch_bounds__(kBlock) red_by_payload_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                                const int32_t* slots, int64_t seq0, int64_t nkid) {
    const EngineConst& c = *cp;
    unsigned long long* base = a.slot_base[slots[blockIdx.y]];
    const unsigned long long ident = c.red_last ? 0ull : ~0ull;
    const int64_t st = a.stride;
    const AggDesc by = c.agg[c.red_by];
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nkid; k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long q = base[(int64_t)c.red_scr * st + k];
        if (q == ident) continue;
        base[(int64_t)c.red_scr * st + k] = ident;
        const unsigned long long vs = base[(int64_t)by.acc * st + k];
        const unsigned long long old = base[(int64_t)c.red_selq * st + k];
        if (!c.red_last && old != ident && base[(int64_t)c.red_selk * st + k] == vs) continue;   // ties: the first
        const int64_t i = (int64_t)q - 1 - seq0;
        if (i < 0 || i >= a.n) continue;                   // (cannot happen: SCR only holds this push's elements)
        base[(int64_t)c.red_selq * st + k] = q - 1ull;
        base[(int64_t)c.red_selk * st + k] = vs;
        for (int j = 0; j < c.nout; ++j) {
            const AggDesc d = c.agg[j];
            if (d.acc_kind != ACC_PAYLOAD || d.alias) continue;
            base[(int64_t)d.acc * st + k] = (d.kind == FWA_FIRST_32 || d.kind == FWA_SEL_32)
                                                ? (unsigned long long)((const uint32_t*)a.cols[d.col])[i]
                                                : ((const unsigned long long*)a.cols[d.col])[i];
        }
    }
}

// One output value of a reduce handle from its merged accumulator word.
__device__ __forceinline__ void red_write(int kind, unsigned long long x, uint64_t cnt, void* out, int64_t row) {
    switch (kind) {
        case FWA_COUNT: ((int64_t*)out)[row] = (int64_t)cnt; break;
        case FWA_SUM_I32: case FWA_FIRST_32: case FWA_SEL_32: ((uint32_t*)out)[row] = (uint32_t)x; break;
        case FWA_SUM_F32: ((float*)out)[row] = (float)__longlong_as_double((long long)x); break;
        case FWA_MIN_I32: case FWA_MAX_I32: case FWA_MINBY_I32: case FWA_MAXBY_I32:
            ((int32_t*)out)[row] = (int32_t)jm::unord_i64(x); break;
        case FWA_MIN_I64: case FWA_MAX_I64: case FWA_MINBY_I64: case FWA_MAXBY_I64:
            ((int64_t*)out)[row] = jm::unord_i64(x); break;
        case FWA_MIN_F32: case FWA_MAX_F32: case FWA_MINBY_F32: case FWA_MAXBY_F32:
            ((float*)out)[row] = (float)__longlong_as_double((long long)jm::unord_bits64(x)); break;
        case FWA_MIN_F64: case FWA_MAX_F64: case FWA_MINBY_F64: case FWA_MAXBY_F64:
            ((unsigned long long*)out)[row] = jm::unord_bits64(x); break;
        default: ((unsigned long long*)out)[row] = x; break;          // SUM_I64, SUM_F64 bits, FIRST_64, SEL_64
    }
}

// The reduced state of key k over a window's slices (base_of(s): slice s's slot columns, or nullptr for a slice without
// state): the count, and the selected slice -- the one whose (by-value, seq) wins, i.e. the element the window's own
// ReducingState would hold -- with its arrival sequence.
template <class BaseOf>
__device__ __forceinline__ uint64_t red_window(const EngineConst& c, int nslots, BaseOf base_of, int64_t k, int64_t stride,
                                               const unsigned long long** sel, unsigned long long* selq) {
    uint64_t cnt = 0;
    bool have = false;
    unsigned long long bv = 0, bq = 0;
    *sel = nullptr;
    for (int s = 0; s < nslots; ++s) {
        const unsigned long long* base = base_of(s);
        if (base == nullptr) continue;
        const uint64_t cs = base[k];
        if (cs == 0) continue;
        cnt += cs;
        const unsigned long long q = base[(int64_t)c.red_selq * stride + k];
        const unsigned long long v = c.red_by >= 0 ? base[(int64_t)c.agg[c.red_by].acc * stride + k] : 0ull;
        bool better = !have;
        if (!better) {
            if (v != bv) better = c.red_max ? v > bv : v < bv;
            else better = c.red_last ? q > bq : q < bq;
        }
        if (better) { have = true; *sel = base; bv = v; bq = q; }
    }
    *selq = bq;
    return cnt;
}

// Output field j of that window's reduced element: the selected element's own field, or the reduced field over the
// slices (sums add, MIN / MAX fold).
template <class BaseOf>
__device__ __forceinline__ unsigned long long red_field(const EngineConst& c, int j, int nslots, BaseOf base_of, int64_t k,
                                                        int64_t stride, const unsigned long long* sel) {
    const AggDesc d = c.agg[j];
    if (d.acc_kind == ACC_PAYLOAD || j == c.red_by) return sel[(int64_t)d.acc * stride + k];
    unsigned long long x = 0;
    if (d.acc <= 0) return x;
    bool first = true;
    for (int s = 0; s < nslots; ++s) {
        const unsigned long long* base = base_of(s);
        if (base == nullptr || base[k] == 0) continue;
        const unsigned long long y = base[(int64_t)d.acc * stride + k];
        if (first) { x = y; first = false; continue; }
        switch (d.acc_kind) {
            case ACC_ADD_I64: x += y; break;
            case ACC_ADD_F64:
                x = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)x) +
                                                             __longlong_as_double((long long)y));
                break;
            case ACC_MIN_ORD: x = y < x ? y : x; break;
            case ACC_MAX_ORD: x = y > x ? y : x; break;
            default: break;
        }
    }
    return x;
}

// Fire of a reduce handle: a block per (window, 4096-kid chunk), kFireJ kids per thread; the window's slices are merged
// (see the file comment). One row reservation per block (a per-wave reservation on the one row counter serialised the
// fire: 2.7 ms per C2-sized step); rows past out_cap are counted, not written (the host grows the output and
// relaunches). raw (fwa_snapshot): every field as an 8-byte cell (4-byte fields zero-extended) and o_count = the
// arrival sequence of the selected element, which orders the restore (red_restore).
__global__ void __launch_bounds__(kBlock) red_fire_kernel(FireArgs f, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int32_t w = blockIdx.x / f.blocks_per_win;
    const int64_t k0 = (int64_t)(blockIdx.x % f.blocks_per_win) * kBlock * kFireJ;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    constexpr int kWaves = kBlock / 64;
    __shared__ uint32_t woff[kFireJ][kWaves];
    __shared__ unsigned long long s_base;
    const FireWindow win = f.win[w];
    const int64_t nk = f.capacity + 1;
    auto base_of = [&](int s) -> const unsigned long long* { return f.slot_base[f.win_slots[win.slot_off + s]]; };
    unsigned long long masks[kFireJ];
#pragma unroll
    for (int j = 0; j < kFireJ; ++j) {
        const int64_t k = k0 + (int64_t)j * kBlock + tid;
        bool present = false;
        if (k < nk) {
            const unsigned long long kv = f.key_table[k];
            present = (k < f.capacity) ? (kv != kEmptyKey) : (kv == 1ull);
        }
        uint64_t cnt = 0;
        if (present) for (int s = 0; s < win.nslots; ++s) cnt += base_of(s)[k];
        masks[j] = __ballot(present && cnt != 0);
        if (lane == 0) woff[j][wid] = (uint32_t)__popcll(masks[j]);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t run = 0;
        for (int j = 0; j < kFireJ; ++j)
            for (int v = 0; v < kWaves; ++v) { const uint32_t t = woff[j][v]; woff[j][v] = run; run += t; }
        s_base = run ? atomicAdd(&f.st->rows, (unsigned long long)run) : 0ull;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int j = 0; j < kFireJ; ++j) {
        if (!((masks[j] >> lane) & 1ull)) continue;
        const int64_t k = k0 + (int64_t)j * kBlock + tid;
        const int64_t row = (int64_t)s_base + woff[j][wid] + __popcll(masks[j] & lt);
        if (row >= f.out_cap) continue;
        const unsigned long long* sel = nullptr;
        unsigned long long bq = 0;
        const uint64_t cnt = red_window(c, win.nslots, base_of, k, f.stride, &sel, &bq);
        // every field's loads before the row's stores (a store could alias a later load: each field would wait)
        unsigned long long xs[FWA_MAX_AGGS];
#pragma unroll
        for (int jj = 0; jj < FWA_MAX_AGGS; ++jj) xs[jj] = jj < c.nout ? red_field(c, jj, win.nslots, base_of, k, f.stride, sel) : 0ull;
        f.o_key[row] = (k < f.capacity) ? (int64_t)f.key_table[k] : LONG_MIN_J;
        f.o_start[row] = win.start;
        f.o_end[row] = win.end;
#pragma unroll
        for (int jj = 0; jj < FWA_MAX_AGGS; ++jj) {
            if (jj >= c.nout) break;
            const AggDesc d = c.agg[jj];
            const unsigned long long x = xs[jj];
            if (f.raw && type_size_dev(d.kind) == 4) {    // fwa_snapshot: a 4-byte field zero-extended in an 8-byte cell
                red_write(d.kind, x, cnt, f.o_agg[jj], 2 * row);
                ((uint32_t*)f.o_agg[jj])[2 * row + 1] = 0u;
            } else {
                red_write(d.kind, x, cnt, f.o_agg[jj], row);
            }
        }
        if (f.raw && f.o_count) f.o_count[row] = (int64_t)bq;
        if (f.raw) for (int h = 0; h < c.naggs - c.nout; ++h) if (f.o_hid[h]) f.o_hid[h][row] = (int64_t)bq;   // SELQ
    }
}

// red_iota: the push's record index column (i; a push holds < 2^31 records), read by the scratch MIN / MAX accumulator
__global__ void __launch_bounds__(kBlock) iota_kernel(int32_t* out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = (int32_t)i;
}

// red_iota selection pass: after the push's accumulators settled, every (slot, kid) whose scratch accumulator (SCR: MIN /
// MAX of the push's record index, a 4-byte column the two-phase ingest carries in its narrow entries) took a record of
// this push selects it -- the first element when the slice had none before (SELQ at its identity), the last always --
// copies its fields into the payload columns and resets SCR: one dense pass over the live slots and a gather of one
// element per (key, slice), instead of a key probe per record.
__global__ void __launch_bounds__(kBlock) red_iota_payload_kernel(IngestArgs a, const EngineConst* __restrict__ cp,
                                                                  const int32_t* slots, int64_t seq0, int64_t nkid) {
    const EngineConst& c = *cp;
    unsigned long long* base = a.slot_base[slots[blockIdx.y]];
    unsigned long long* selq = base + (int64_t)c.red_selq * a.stride;
    unsigned long long* scr = base + (int64_t)c.red_scr * a.stride;
    const unsigned long long ident = c.red_last ? 0ull : ~0ull;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < nkid; k += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long q = scr[k];
        if (q == ident) continue;
        scr[k] = ident;
        if (!c.red_last && selq[k] != ~0ull) continue;                // the slice's first element came earlier
        const int64_t i = jm::unord_i64(q);
        selq[k] = (unsigned long long)(seq0 + i);
        for (int j = 0; j < c.nout; ++j) {
            const AggDesc d = c.agg[j];
            if (d.acc_kind != ACC_PAYLOAD || d.alias) continue;
            base[(int64_t)d.acc * a.stride + k] = (d.kind == FWA_FIRST_32 || d.kind == FWA_SEL_32)
                                                      ? (unsigned long long)((const uint32_t*)a.cols[d.col])[i]
                                                      : ((const unsigned long long*)a.cols[d.col])[i];
        }
    }
}

// Late firings of a reduce handle (allowed lateness > 0; late_fire_kernel's contract: the deferred records of a push,
// in arrival order, by one lane). Each record is folded into its slice as HeapReducingState.add folds it -- the
// selection moves to it when it is the slice's first element, or (MINBY / MAXBY) when its by-value is better, or equal
// under FWA_CFG_BY_LAST (ComparableAggregator.java:83-104) -- and every window of the record already past its trigger
// emits its reduced element at once (EventTimeTrigger.onElement FIRE, WindowOperator.java:391-431).
__global__ void __launch_bounds__(64) red_late_fire_kernel(LateArgs L, const EngineConst* __restrict__ cp, int64_t seq0) {
    const EngineConst& c = *cp;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const IngestArgs& a = L.in;
    auto slice_q = [&](int64_t t) -> int64_t {                      // floor((t - off) / g), Java wrap arithmetic
        const int64_t d = jm::wsub(t, c.off);
        const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
        const uint64_t uq = jm::udiv64(ud, c.g_div);
        return d >= 0 ? (int64_t)uq : ((uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1);
    };
    unsigned long long nrow = *L.rows;
    for (int64_t t = 0; t < L.n; ++t) {
        const int64_t i = L.order[t];
        const int64_t key = a.keys[i];
        const int64_t q = slice_q(a.ts[i]);
        const DirEntry* e = dir_find(a.dir, a.dir_mask, q);
        if (e == nullptr || e->slot < 0) { raise_error(a.st, FWA_E_STATE); return; }   // host allocated it
        const int64_t kid = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key, a.st);
        if (kid < 0) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); return; }
        unsigned long long* base = a.slot_base[e->slot];
        a.touched[e->slot] = 1;
        const uint64_t before = base[kid];
        bool sel = before == 0 || (c.red_by < 0 && c.red_last);
        unsigned long long v = 0;
        if (c.red_by >= 0) {
            const AggDesc by = c.agg[c.red_by];
            v = load_ord(a.cols[by.col], i, by.kind, 1);
            const unsigned long long old = base[(int64_t)by.acc * a.stride + kid];
            if (!sel) sel = v != old ? (c.red_max ? v > old : v < old) : c.red_last;
        }
        base[kid] = before + 1;                                       // state.add
        for (int j = 0; j < c.naggs; ++j) {
            const AggDesc dsc = c.agg[j];
            if (dsc.acc == 0 || dsc.alias || dsc.acc_kind == ACC_PAYLOAD || (c.red_iota && dsc.col == kIotaCol)) continue;
            unsigned long long* col = base + (int64_t)dsc.acc * a.stride + kid;
            *col = acc_combine(dsc.acc_kind, *col, acc_input(dsc, a.cols[dsc.col], i));
        }
        if (sel) {
            base[(int64_t)c.red_selq * a.stride + kid] = (unsigned long long)(seq0 + i);
            if (c.red_by >= 0) base[(int64_t)c.red_selk * a.stride + kid] = v;
            for (int j = 0; j < c.nout; ++j) {
                const AggDesc d = c.agg[j];
                if (d.acc_kind != ACC_PAYLOAD || d.alias) continue;
                base[(int64_t)d.acc * a.stride + kid] = (d.kind == FWA_FIRST_32 || d.kind == FWA_SEL_32)
                                                            ? (unsigned long long)((const uint32_t*)a.cols[d.col])[i]
                                                            : ((const unsigned long long*)a.cols[d.col])[i];
            }
        }
        // windows of the record (TimeWindow.getWindowStartWithOffset + Tumbling/SlidingEventTimeWindows)
        const int64_t sa = jm::wadd(c.off, (int64_t)((uint64_t)q * (uint64_t)c.g));
        for (int64_t ws = jm::window_start(sa, c.off, L.slide_div); ws > jm::wsub(sa, L.size); ws = jm::wsub(ws, L.slide)) {
            const int64_t we = jm::wadd(ws, L.size);
            const int64_t mt = jm::wsub(we, 1);
            int64_t cleanup = jm::wadd(mt, L.lateness);
            if (cleanup < mt) cleanup = LONG_MAX_J;
            if (cleanup <= a.wm || mt > a.wm) continue;              // late window / timer still pending
            const int64_t q0 = slice_q(ws);
            const int ns = (int)((uint64_t)(we - ws) / (uint64_t)c.g);
            auto base_of = [&](int s) -> const unsigned long long* {
                const DirEntry* ee = dir_find(a.dir, a.dir_mask, q0 + s);
                return (ee == nullptr || ee->slot < 0) ? nullptr : a.slot_base[ee->slot];
            };
            const unsigned long long* sb = nullptr;
            unsigned long long bq = 0;
            const uint64_t cnt = red_window(c, ns, base_of, kid, a.stride, &sb, &bq);
            L.o_key[nrow] = key;
            L.o_start[nrow] = ws;
            L.o_end[nrow] = we;
            for (int j = 0; j < c.nout; ++j)
                red_write(c.agg[j].kind, red_field(c, j, ns, base_of, kid, a.stride, sb), cnt, L.o_agg[j], (int64_t)nrow);
            ++nrow;
        }
    }
    *L.rows = nrow;
}

}  // namespace

// Restore of a reduce handle (fwa_restore, after the blobs were validated): every owned (key, slice) entry is pushed
// back as one element -- the slice's selected element with its reduced field -- in the order of the original arrival
// sequence of those elements (the count column), so the first-element and tie rules see the same order; the restored
// watermark is set after them.
static int push_body(fwa_engine* e, const int64_t* keys, const int64_t* ts, const void* const* val_cols,
                     const uint8_t* const* null_cols, const int32_t* key_hash, int64_t n, int32_t flags,
                     int64_t* late_dropped_out);
static int retire_slices(fwa_engine* e, int64_t wm);
static int account_ingest(fwa_engine* e);
static int red_restore(fwa_engine* e, const void* const* blobs, int32_t n_blobs) {
    const int na = e->cfg.num_aggs, maxp = e->cfg.max_parallelism;
    int64_t wm = LONG_MAX_J;
    std::vector<std::pair<uint64_t, std::pair<int32_t, int64_t>>> ord;   // (seq, (blob, entry))
    for (int32_t b = 0; b < n_blobs; ++b) {
        const int64_t* h = (const int64_t*)blobs[b];
        wm = std::min<int64_t>(wm, h[20]);
        const int64_t* off = h + kSnapHdr;
        const int64_t lo = off[e->cfg.kg_start], hi = off[e->cfg.kg_end + 1];
        if (lo < 0 || hi < lo || hi > h[21]) return fail(e, FWA_E_ARG, "corrupt key-group offsets");
        const int64_t* cnt = off + maxp + 1 + 2 * h[21];
        for (int64_t i = lo; i < hi; ++i) ord.push_back({(uint64_t)cnt[i], {b, i}});
    }
    if (n_blobs == 0) return FWA_OK;
    const int64_t n = (int64_t)ord.size();
    if (n == 0) { e->wm = wm; e->dir_dirty = true; return FWA_OK; }
    std::stable_sort(ord.begin(), ord.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    const bool ph = e->cfg.key_kind == FWA_KEY_PREHASHED;   // the blobs' last column: each key's key.hashCode()
    std::vector<int64_t> keys((size_t)n), ts((size_t)n);
    std::vector<int32_t> kh(ph ? (size_t)n : 0);
    std::vector<std::vector<int64_t>> c64(FWA_MAX_COLS);
    std::vector<std::vector<int32_t>> c32(FWA_MAX_COLS);
    const void* cols[FWA_MAX_COLS] = {};
    for (int j = 0; j < na; ++j) {
        const int col = e->cfg.aggs[j].col;
        if (type_size(e->cfg.aggs[j].kind) == 4) { c32[col].resize((size_t)n); cols[col] = c32[col].data(); }
        else { c64[col].resize((size_t)n); cols[col] = c64[col].data(); }
    }
    for (int64_t r = 0; r < n; ++r) {
        const int64_t* h = (const int64_t*)blobs[ord[r].second.first];
        const int64_t i = ord[r].second.second, m = h[21];
        const int64_t* body = h + kSnapHdr + maxp + 1;
        keys[r] = body[i];
        if (ph) kh[r] = (int32_t)body[(size_t)(3 + na + (e->ec.naggs - e->ec.nout)) * m + i];
        ts[r] = jm::wadd(body[m + i], e->g - 1);            // the slice's last timestamp: lands in that slice
        for (int j = 0; j < na; ++j) {
            const int col = e->cfg.aggs[j].col;
            const int64_t v = body[(size_t)(3 + j) * m + i];
            if (type_size(e->cfg.aggs[j].kind) == 4) c32[col][r] = (int32_t)(uint32_t)v;
            else c64[col][r] = v;
        }
    }
    // pushed before the watermark moves (nothing is late or fires late then), then the watermark is restored as
    // fwa_restore does it: windows with maxTimestamp <= wm fired before the snapshot and do not fire again, and slices
    // kept only for allowed lateness stay for later late firings
    int64_t late = 0;
    int rc = push_body(e, keys.data(), ts.data(), cols, nullptr, ph ? kh.data() : nullptr, n, 0, &late);
    if (rc) return rc;
    if (late) return fail(e, FWA_E_STATE, "restored elements were dropped as late");
    if (wm > e->wm) {
        if ((rc = retire_slices(e, wm))) return rc;
        e->wm = wm;
    }
    e->red_seq_base += e->records_in;                  // later elements stay after the restored ones
    e->records_in = 0;                                 // metrics are not part of the snapshot
    e->late_dropped = 0;
    return FWA_OK;
}

// The selection passes of one push (after its ingest and miss replays settled). seq0: records before this push.
static int red_select(fwa_engine* e, IngestArgs& a, int64_t n, int64_t seq0) {
    if (n <= 0) return FWA_OK;
    if (n > e->rk_cap) {
        if (e->d_rk) HIPCHK(e, hipFree(e->d_rk));
        e->d_rk = nullptr;
        HIPCHK(e, hipMalloc(&e->d_rk, 8 * (size_t)n));
        e->rk_cap = n;
    }
    if (e->ec.red_iota) {   // SELQ is an accumulator: only the payload of this push's selections is left
        std::vector<int32_t> sl;
        for (auto& kv : e->live) if (e->touched[kv.second]) sl.push_back(kv.second);
        if (sl.empty()) return FWA_OK;
        if ((int64_t)sl.size() > e->rslots_cap) {
            if (e->d_rslots) HIPCHK(e, hipFree(e->d_rslots));
            e->d_rslots = nullptr;
            HIPCHK(e, hipMalloc(&e->d_rslots, 4 * sl.size()));
            e->rslots_cap = (int64_t)sl.size();
        }
        HIPCHK(e, hipMemcpyAsync(e->d_rslots, sl.data(), 4 * sl.size(), hipMemcpyHostToDevice, e->stream));
        a.n = n;
        a.slot_base = e->d_slot_base;
        a.stride = e->stride;
        const int64_t nkid = e->capacity + 1;
        HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
        red_iota_payload_kernel<<<dim3((unsigned)std::min<int64_t>((nkid + 4 * kBlock - 1) / (4 * kBlock), 2048),
                                       (unsigned)sl.size()), kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rslots, seq0, nkid);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
        int rc = stream_sync(e);
        return rc ? rc : account_ingest(e);
    }
    if (e->ec.red_by >= 0 && !(e->opt_variant & 64)) {   // variant bit 6: the four record passes below (A/B)
        std::vector<int32_t> sl;
        for (auto& kv : e->live) if (e->touched[kv.second]) sl.push_back(kv.second);
        if (sl.empty()) return FWA_OK;
        if ((int64_t)sl.size() > e->rslots_cap) {
            if (e->d_rslots) HIPCHK(e, hipFree(e->d_rslots));
            e->d_rslots = nullptr;
            HIPCHK(e, hipMalloc(&e->d_rslots, 4 * sl.size()));
            e->rslots_cap = (int64_t)sl.size();
        }
        if (e->dir_dirty) { int rc = publish_dir(e); if (rc) return rc; }
        HIPCHK(e, hipMemcpyAsync(e->d_rslots, sl.data(), 4 * sl.size(), hipMemcpyHostToDevice, e->stream));
        a.idx = nullptr;
        a.n = n;
        a.key_table = e->d_keys;
        a.key_mask = (uint64_t)e->capacity - 1;
        a.seg_log = e->seg_log;
        a.part_bits = e->part_bits;
        a.dir = e->d_dir;
        a.dir_mask = e->dir_cap - 1;
        a.slot_base = e->d_slot_base;
        a.stride = e->stride;
        a.st = e->d_st;
        const int64_t nkid = e->capacity + 1;
        HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
        red_by_kernel<<<grid_for(n, 256 * 32), kBlock, 0, e->stream>>>(a, e->d_ec, seq0);
        red_by_payload_kernel<<<dim3((unsigned)std::min<int64_t>((nkid + 4 * kBlock - 1) / (4 * kBlock), 2048),
                                     (unsigned)sl.size()), kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rslots, seq0, nkid);
        HIPCHK(e, hipGetLastError());
        HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
        int rc = stream_sync(e);
        return rc ? rc : account_ingest(e);
    }
    if (e->dir_dirty) { int rc = publish_dir(e); if (rc) return rc; }
    a.idx = nullptr;
    a.n = n;
    a.key_table = e->d_keys;
    a.key_mask = (uint64_t)e->capacity - 1;
    a.seg_log = e->seg_log;
    a.part_bits = e->part_bits;
    a.dir = e->d_dir;
    a.dir_mask = e->dir_cap - 1;
    a.slot_base = e->d_slot_base;
    a.stride = e->stride;
    a.st = e->d_st;
    const int grid = grid_for(n, 256 * 32);
    HIPCHK(e, hipEventRecord(e->ev[0], e->stream));
    red_index_kernel<<<grid, kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rk);
    if (e->ec.red_by >= 0) red_stale_kernel<<<grid, kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rk);
    red_pick_kernel<<<grid, kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rk, seq0);
    red_payload_kernel<<<grid, kBlock, 0, e->stream>>>(a, e->d_ec, e->d_rk, seq0);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[1], e->stream));
    int rc = stream_sync(e);    // the inputs may be the caller's (valid only during the call)
    return rc ? rc : account_ingest(e);   // the selection passes count as ingest device time
}
