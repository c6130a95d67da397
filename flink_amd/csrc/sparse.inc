// sparse.inc -- record-list window state for key spaces far larger than a window's records (C4: 1e8 keys, each
// key ~0.1-0.7 times per window). Included by engine.hip (it uses the engine's structures and helpers).
//
// The dense layout (one accumulator per (kid, slice) in per-slot SoA columns behind a key table) costs a random
// key-table probe and memory-side atomics per record and a fire scan over every kid when keys barely repeat. Here a
// TUMBLE window's state is the list of its accepted records (key + accumulator words), bucketed on arrival by
// (window, coarse hash partition), and the aggregation happens once, when the window fires -- the same function
// (HeapAggregatingState.add per record, then AggregateFunction.getResult per key at onEventTime,
// WindowOperator.java:393-417,459-505) evaluated in a different order. Semantics kept from the dense engine:
// key-group ownership (StateTable.getMapForKeyGroup), Long.MIN_VALUE timestamps (DataStream), late records
// (isWindowLate, lateness 0 / TimeWindowUtil.isWindowFired), per-record drop indices, partial accumulators
// (fwa_push_partials / fwa_drain_partials), snapshot / restore through the FWASNAP1 blob.
//
// push  (one pass per <= kSpW windows):   sp_range_kernel  : ownership / timestamp checks, late drops, window range
//                                          sp_hist_kernel   : per block, LDS histogram over (window, partition)
//        (after the first watermark the range pass is folded into the histogram: the windows are the kSpW from the
//         first one the watermark leaves open, and a record past them sends the push back to the two-pass form)
//                                          sp_scan_kernel   : bucket offsets
//                                          sp_scatter_kernel: per block, reserve each bucket's run, scatter entries
// fire  (per watermark, all due windows): sp_refine_kernel: one workgroup per (window, partition) holding more than
//                                          one LDS table's worth of entries: counting sort of the partition's
//                                          entries (gathered from every run) into fine buckets (scratch)
//                                          sp_agg_kernel   : one workgroup per fine bucket (or per small partition,
//                                          straight from the runs): LDS open-addressing table (key, COUNT,
//                                          accumulators; LDS atomics), one row per key
// Bound: HBM streaming (~48 B/record in, 16-24 B/record list write, 2 x list read + scratch write/read, rows out).

constexpr int kSpPBits = 10, kSpP = 1 << kSpPBits;   // coarse hash partitions per window
constexpr int kSpW = 16;                              // windows per push pass (LDS histogram: kSpW * kSpP)
constexpr int kSpBlock = 1024;
constexpr int kSpPushBlocks = 1024;                 // two 1024-thread blocks per CU
constexpr int kSpU = 4;                               // records in flight per thread (independent loads)
constexpr int kSpMaxF = 4096;                         // fine buckets per (window, partition)
constexpr int kSpAccCols = 1 + kMaxAggsInt;

// An entry is W = 1 + has_cnt + (nacc - 1) consecutive words: key, [COUNT], accumulators 1..nacc-1 (AoS: one
// 16-byte store per entry for COUNT + one accumulator, so each scattered entry dirties one partial line, not two).
struct SpRun {                      // one push pass: accepted entries bucketed by (window, partition)
    int64_t n = 0;                  // entries
    int32_t nq = 0;
    int64_t qs[kSpW] = {};          // slice numbers of its windows
    int32_t alive = 0;              // windows with entries not yet fired
    bool has_cnt = false;           // rows stand for several records (partials / restore)
    void* mem = nullptr;
    size_t bytes = 0;               // allocation size (pool bookkeeping)
    unsigned long long* ent = nullptr;   // [n][W]
    int32_t W = 1;
    bool nw = false;                // narrow entries: one word (int32 key | int32 BIGINT sum << 32), W = 1
    uint32_t* off = nullptr;        // [nq * kSpP + 1]
    std::vector<uint32_t> hoff;
};

struct SpWin {
    std::vector<std::pair<int32_t, int32_t>> parts;   // (run id, window index in the run)
    int64_t entries = 0;
    int64_t base = 0;                                 // entries right after its last compaction (0: never compacted)
};

struct SpState {
    std::vector<SpRun*> runs;
    std::vector<std::pair<size_t, void*>> pool;   // freed run buffers (size, ptr), reused by later pushes
    std::map<int64_t, SpWin> wins;   // live windows by slice number
    uint32_t* d_ghist = nullptr;
    size_t ghist_cap = 0;
    uint32_t* d_cursor = nullptr;    // [kSpW * kSpP]
    uint32_t* d_off = nullptr;       // [kSpW * kSpP + 1]
    char* d_scratch = nullptr;
    size_t scratch_cap = 0;
    char* d_desc = nullptr;
    size_t desc_cap = 0;
    int32_t T = 4096;                // LDS table slots
    size_t lds = 0;                  // fire kernel dynamic LDS
    size_t budget = 0;               // live list bytes above which growing windows are compacted (sp_compact)
    int32_t fmax = 0;                // max fine buckets per (window, partition) at fire (0: kSpMaxF)
    bool compacting = false;
    int64_t compactions = 0;
    bool narrow = true;              // narrow entries while every key and BIGINT value of a push fits 32 bits
};

namespace {

struct SpPushArgs {
    const int64_t* keys;
    const int64_t* ts;
    const int32_t* key_hash;
    const unsigned long long* pcount;     // partial accumulators: COUNT per row (cols are accumulator words)
    const void* col[kSpAccCols];          // source of accumulator column c (1..nacc-1)
    int32_t aggi[kSpAccCols];             // aggregate descriptor feeding column c
    int64_t n, wm, per;
    int32_t nq, check_kg;
    int32_t fused, nw;                    // fused: histogram pass also checks / drops, windows qs[0] + w (contiguous);
                                          // nw: narrow entries (a record that does not fit counts st->wide_n)
    int64_t qs[kSpW];
    uint32_t* ghist;                      // [blocks][nq * kSpP]
    uint32_t* cursor;                     // [nq * kSpP]
    uint32_t* off;                        // [nq * kSpP + 1]
    unsigned long long* oent;             // [ocap][ow]
    int64_t ocap;
    int32_t ow;
    unsigned long long* want;             // collect the distinct accepted windows (wide pushes)
    int32_t* dropidx;
    DevStatus* st;
};

__device__ __forceinline__ int64_t sp_slice(const EngineConst& c, int64_t ts) {   // TimeWindow.getWindowStartWithOffset
    const int64_t d = jm::wsub(ts, c.off);
    const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
    const uint64_t uq = jm::udiv64(ud, c.g_div);
    if (d >= 0) return (int64_t)uq;
    return (uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1;
}

// TUMBLE window q accepts records iff its maxTimestamp is past the watermark (lateness 0: isWindowLate /
// !isWindowFired); a Table window ending at Long.MAX_VALUE always accepts
__device__ __forceinline__ bool sp_accepts(const EngineConst& c, int64_t q, int64_t wm) {
    const int64_t start = jm::wadd(c.off, (int64_t)((uint64_t)q * (uint64_t)c.g));
    const int64_t end = jm::wadd(start, c.g);
    if (c.sem == FWA_SEM_TABLE && end == LONG_MAX_J) return true;
    return wm < jm::wsub(end, 1);
}

__device__ __forceinline__ int sp_local_window(const SpPushArgs& a, int64_t q) {
    if (a.fused) {
        const uint64_t w = (uint64_t)q - (uint64_t)a.qs[0];
        return w < (uint64_t)a.nq ? (int)w : -1;
    }
    for (int w = 0; w < a.nq; ++w) if (a.qs[w] == q) return w;
    return -1;
}

__device__ __forceinline__ uint32_t sp_part(int64_t key) { return (uint32_t)(jm::mix64((uint64_t)key) >> (64 - kSpPBits)); }

__global__ void __launch_bounds__(kBlock) sp_range_kernel(SpPushArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    unsigned long long qmax = 0, qmin = ~0ull, dropped = 0;
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < a.n; i0 += kSpU * gstride) {
      int64_t tv[kSpU];
#pragma unroll
      for (int u = 0; u < kSpU; ++u) tv[u] = i0 + u * gstride < a.n ? a.ts[i0 + u * gstride] : 0;
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        const int64_t i = i0 + u * gstride;
        if (i >= a.n) break;
        const int64_t ts = tv[u];
        bool drop = false;
        if (a.check_kg) {
            const int32_t kg = jm::key_group_of(a.keys[i], c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
            if (kg < c.kg_lo || kg > c.kg_hi) raise_error(a.st, FWA_E_KEYGROUP);
        }
        if (c.sem == FWA_SEM_DATASTREAM && ts == LONG_MIN_J && !a.pcount) {
            raise_error(a.st, FWA_E_TS_MIN);
        } else {
            const int64_t q = sp_slice(c, ts);
            if (sp_accepts(c, q, a.wm)) {
                const uint64_t oq = jm::ord_i64(q);
                qmax = oq > qmax ? oq : qmax;
                qmin = oq < qmin ? oq : qmin;
                if (a.want) want_insert(a.want, a.st, q);
            } else {
                drop = true;
                dropped += a.pcount ? a.pcount[i] : 1ull;
            }
        }
        note_drop(a.pcount ? nullptr : a.dropidx, a.st, drop, i);
      }
    }
    for (int s = 32; s > 0; s >>= 1) {
        const unsigned long long x = __shfl_xor(qmax, s), y = __shfl_xor(qmin, s), z = __shfl_xor(dropped, s);
        qmax = x > qmax ? x : qmax;
        qmin = y < qmin ? y : qmin;
        dropped += z;
    }
    __shared__ unsigned long long r[3][kBlock / 64];   // one set of device atomics per block: same-address
    const int wv = threadIdx.x >> 6;                    // atomics from every wave serialised the kernel
    if ((threadIdx.x & 63) == 0) { r[0][wv] = qmax; r[1][wv] = qmin; r[2][wv] = dropped; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kBlock / 64; ++k) {
            qmax = r[0][k] > qmax ? r[0][k] : qmax;
            qmin = r[1][k] < qmin ? r[1][k] : qmin;
            dropped += r[2][k];
        }
        if (qmax) atomicMax(&a.st->max_q, qmax);
        if (qmin != ~0ull) atomicMin(&a.st->min_q, qmin);
        if (dropped) atomicAdd(&a.st->dropped, dropped);
    }
}

__global__ void __launch_bounds__(kSpBlock) sp_hist_kernel(SpPushArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    __shared__ uint32_t h[kSpW * kSpP];
    __shared__ unsigned long long s_drop;
    __shared__ uint32_t s_out;
    const int nb = a.nq * kSpP;
    for (int k = threadIdx.x; k < nb; k += kSpBlock) h[k] = 0;
    if (threadIdx.x == 0) { s_drop = 0ull; s_out = 0u; }
    __syncthreads();
    unsigned long long dropped = 0;
    uint32_t outside = 0;
    const int64_t lo = (int64_t)blockIdx.x * a.per, hi = min(lo + a.per, a.n);
    for (int64_t i0 = lo + threadIdx.x; i0 < hi; i0 += kSpU * kSpBlock) {
        int64_t t[kSpU], k[kSpU];
#pragma unroll
        for (int u = 0; u < kSpU; ++u) {   // clamped index: unconditional loads
            const int64_t i = min(i0 + (int64_t)u * kSpBlock, hi - 1);
            t[u] = a.ts[i];
            k[u] = a.keys[i];
        }
#pragma unroll
        for (int u = 0; u < kSpU; ++u) {
            const int64_t i = i0 + (int64_t)u * kSpBlock;
            if (i >= hi) continue;
            const int64_t q = sp_slice(c, t[u]);
            const int w = sp_local_window(a, q);
            if (a.fused) {   // sp_range_kernel's checks, on the same loads
                if (a.check_kg) {
                    const int32_t kg = jm::key_group_of(k[u], c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
                    if (kg < c.kg_lo || kg > c.kg_hi) raise_error(a.st, FWA_E_KEYGROUP);
                }
                if (c.sem == FWA_SEM_DATASTREAM && t[u] == LONG_MIN_J) { raise_error(a.st, FWA_E_TS_MIN); continue; }
                const bool drop = !sp_accepts(c, q, a.wm);
                dropped += drop ? 1ull : 0ull;
                note_drop(a.dropidx, a.st, drop, i);
                if (drop) continue;
                if (w < 0) { ++outside; continue; }
            }
            if (w >= 0) atomicAdd(&h[w * kSpP + sp_part(k[u])], 1u);
        }
    }
    if (a.fused) {
        for (int sh = 32; sh > 0; sh >>= 1) { dropped += __shfl_xor(dropped, sh); outside += __shfl_xor(outside, sh); }
        if ((threadIdx.x & 63) == 0 && (dropped | outside)) { atomicAdd(&s_drop, dropped); atomicAdd(&s_out, outside); }
    }
    __syncthreads();
    if (a.fused && threadIdx.x == 0) {
        if (s_drop) atomicAdd(&a.st->dropped, s_drop);
        if (s_out) atomicAdd(&a.st->spill_n, (int32_t)s_out);   // records past the pass's windows
    }
    uint32_t* g = a.ghist + (int64_t)blockIdx.x * nb;
    for (int k = threadIdx.x; k < nb; k += kSpBlock) {
        g[k] = h[k];
        if (h[k]) atomicAdd(&a.cursor[k], h[k]);
    }
}

// exclusive scan of the bucket totals into off[], cursors reset to the bucket starts (one block)
__global__ void __launch_bounds__(kSpBlock) sp_scan_kernel(uint32_t* cursor, uint32_t* off, int nb) {
    __shared__ uint32_t part[kSpBlock];
    const int per = (nb + kSpBlock - 1) / kSpBlock;
    const int k0 = threadIdx.x * per;
    uint32_t s = 0;
    for (int k = k0; k < min(k0 + per, nb); ++k) s += cursor[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < kSpBlock; d <<= 1) {
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;
    for (int k = k0; k < min(k0 + per, nb); ++k) {
        const uint32_t v = cursor[k];
        off[k] = run;
        cursor[k] = run;
        run += v;
    }
    if (threadIdx.x == kSpBlock - 1) off[nb] = part[kSpBlock - 1];
}

// NA: accumulator columns when known at compile time (1..4: the per-entry values stay in registers), 0: any
template <int NA>
__global__ void __launch_bounds__(kSpBlock) sp_scatter_kernel(SpPushArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int nacc = NA ? NA : c.nacc;
    __shared__ uint32_t cur[kSpW * kSpP];
    const int nb = a.nq * kSpP;
    const uint32_t* g = a.ghist + (int64_t)blockIdx.x * nb;
    for (int k = threadIdx.x; k < nb; k += kSpBlock) {
        const uint32_t n = g[k];
        cur[k] = n ? atomicAdd(&a.cursor[k], n) : 0u;
    }
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * a.per, hi = min(lo + a.per, a.n);
    for (int64_t i0 = lo + threadIdx.x; i0 < hi; i0 += kSpU * kSpBlock) {
      // every load of the kSpU records first, at clamped indices (a load under a per-record condition -- the range
      // test, acc_input's kind switch -- made hipcc wait for each one, and the value load came after the slot's LDS
      // atomic), then the slots and the stores
      int64_t t[kSpU], k[kSpU], ic[kSpU];
      constexpr int NV = NA ? NA : 1;
      unsigned long long v[kSpU][NV], pc[kSpU];
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
          ic[u] = min(i0 + (int64_t)u * kSpBlock, hi - 1);
          t[u] = a.ts[ic[u]];
          k[u] = a.keys[ic[u]];
          pc[u] = a.pcount ? a.pcount[ic[u]] : 0ull;
      }
      if constexpr (NA > 0) {
#pragma unroll
          for (int cc = 1; cc < NA; ++cc) {
              const AggDesc& d = c.agg[a.aggi[cc]];
              const void* col = a.col[cc];
              if (a.pcount || type_size_dev(d.kind) == 8) {
#pragma unroll
                  for (int u = 0; u < kSpU; ++u) v[u][cc] = ((const unsigned long long*)col)[ic[u]];
              } else {
#pragma unroll
                  for (int u = 0; u < kSpU; ++u) v[u][cc] = ((const uint32_t*)col)[ic[u]];
              }
              if (!a.pcount) {
#pragma unroll
                  for (int u = 0; u < kSpU; ++u) v[u][cc] = acc_of_raw(d, v[u][cc], false);
              }
          }
      }
#pragma unroll
      for (int u = 0; u < kSpU; ++u) {
        const int64_t i = i0 + (int64_t)u * kSpBlock;
        if (i >= hi) continue;
        const int w = sp_local_window(a, sp_slice(c, t[u]));
        if (w < 0) continue;
        const int64_t key = k[u];
        const int64_t pos = atomicAdd(&cur[w * kSpP + sp_part(key)], 1u);
        if (pos >= a.ocap) { raise_error(a.st, FWA_E_STATE); continue; }
        unsigned long long* e = a.oent + pos * a.ow;
        auto accv = [&](int cc) -> unsigned long long {
            if constexpr (NA > 0) return v[u][cc];
            return a.pcount ? ((const unsigned long long*)a.col[cc])[i] : acc_input(c.agg[a.aggi[cc]], a.col[cc], i, nullptr);
        };
        if (NA == 2 && a.nw) {
            const int64_t val = (int64_t)accv(1);
            if ((int64_t)(int32_t)key != key || (int64_t)(int32_t)val != val) {   // the host redoes the push wide
                atomicAdd(&a.st->wide_n, 1);
                continue;
            }
            *e = ((unsigned long long)key & 0xffffffffull) | ((unsigned long long)val << 32);
        } else if (a.ow == 2) {
            *(ulonglong2*)e = make_ulonglong2((unsigned long long)key, a.pcount ? pc[u] : accv(1));
        } else {
            const int hc = a.pcount ? 1 : 0;
            e[0] = (unsigned long long)key;
            if (hc) e[1] = pc[u];
#pragma unroll 4
            for (int cc = 1; cc < nacc; ++cc) e[hc + cc] = accv(cc);
        }
      }
    }
}

struct SpRunDesc {
    const unsigned long long* ent;
    const uint32_t* off;
    int32_t W, has_cnt;
    int32_t nw, pad;                   // narrow entries (SpRun::nw)
};
struct SpWinDesc {
    int64_t start, end;
    int32_t seg0, nseg;
};
struct SpSeg {
    int32_t run, wl;
};

struct SpFireArgs {
    const SpRunDesc* runs;
    const SpWinDesc* wins;
    const SpSeg* segs;
    const int64_t* task_base;          // [tasks + 1]: scratch offset of each (window, partition)
    const int64_t* fbase;              // [tasks + 1]: first fine bucket of each task (F_t = fbase[t+1] - fbase[t])
    uint32_t* fend;                    // [fine buckets]: end of each fine bucket, relative to its task's base
    int64_t ntasks;
    int64_t sn;                        // scratch entries (column stride)
    unsigned long long* sent;          // scratch entries [sn][sw] (key, [COUNT], accumulators)
    int32_t sw, scnt;                  // words per scratch entry; 1: they carry a COUNT word
    int32_t T, raw;                    // LDS table slots; raw accumulators
    int64_t* o_key;
    int64_t* o_start;
    int64_t* o_end;
    int64_t* o_count;
    void* o_agg[FWA_MAX_AGGS];
    int64_t out_cap;
    DevStatus* st;
};

template <int NA>
__device__ __forceinline__ void sp_apply(unsigned long long* tc, int stride, const EngineConst& c, int s, unsigned long long cnt,
                                         const unsigned long long* v) {
    atomicAdd(&tc[s], cnt);
    const int nacc = NA ? NA : c.nacc;
#pragma unroll 4
    for (int cc = 1; cc < nacc; ++cc) {
        unsigned long long* p = &tc[(int64_t)cc * stride + s];
        switch (c.acc_kind[cc]) {
            case ACC_ADD_I64: atomicAdd(p, v[cc]); break;
            case ACC_ADD_F64: atomicAdd((double*)p, __longlong_as_double((long long)v[cc])); break;
            case ACC_MIN_ORD: atomicMin(p, v[cc]); break;
            case ACC_MAX_ORD: atomicMax(p, v[cc]); break;
            default: break;
        }
    }
}

// entry i of an AoS list with W words per entry (key, [COUNT if has_cnt], accumulators)
__device__ __forceinline__ void sp_load_ent(const unsigned long long* ent, int W, int has_cnt, int64_t i, int nacc,
                                            int64_t& key, unsigned long long& cnt, unsigned long long* v, int nw = 0) {
    if (nw) {                          // (int32 key | int32 BIGINT sum << 32), one record
        const unsigned long long x = ent[i];
        key = (int64_t)(int32_t)(uint32_t)x;
        cnt = 1ull;
        v[1] = (unsigned long long)(int64_t)(int32_t)(uint32_t)(x >> 32);
        return;
    }
    const unsigned long long* e = ent + i * W;
    if (W == 2) {
        const ulonglong2 p = *(const ulonglong2*)e;
        key = (int64_t)p.x;
        if (has_cnt) cnt = p.y; else { cnt = 1ull; v[1] = p.y; }
        return;
    }
    key = (int64_t)e[0];
    cnt = has_cnt ? e[1] : 1ull;
#pragma unroll 4
    for (int cc = 1; cc < nacc; ++cc) v[cc] = e[has_cnt + cc];
}
__device__ __forceinline__ void sp_load(const SpRunDesc& r, int64_t i, int nacc, int64_t& key, unsigned long long& cnt,
                                        unsigned long long* v) {
    sp_load_ent(r.ent, r.W, r.has_cnt, i, nacc, key, cnt, v, r.nw);
}
__device__ __forceinline__ int64_t sp_key(const SpRunDesc& r, int64_t i) {
    return r.nw ? (int64_t)(int32_t)(uint32_t)r.ent[i] : (int64_t)r.ent[i * r.W];
}

__device__ __forceinline__ void sp_seg(const SpFireArgs& f, const SpWinDesc& win, int p, int s, SpRunDesc& r, int64_t& s0,
                                       int64_t& s1) {
    const SpSeg sg = f.segs[win.seg0 + s];
    r = f.runs[sg.run];
    const uint32_t* off = r.off + (int64_t)sg.wl * kSpP + p;
    s0 = off[0];
    s1 = off[1];
}

__device__ __forceinline__ int sp_fine(int64_t key, int fbits) {
    return fbits ? (int)((jm::mix64((uint64_t)key) >> (64 - kSpPBits - fbits)) & (uint64_t)((1 << fbits) - 1)) : 0;
}

// Refine: one workgroup per (window, coarse partition) with F_t > 1 fine buckets: counting sort of the partition's
// entries (gathered from every run) by the hash bits below the coarse partition's into the scratch copy.
template <int NA>
__global__ void __launch_bounds__(kSpBlock) sp_refine_kernel(SpFireArgs f, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    __shared__ uint32_t fh[kSpMaxF];
    const int tid = threadIdx.x, nacc = NA ? NA : c.nacc;
    const int64_t task = blockIdx.x;
    const int F = (int)(f.fbase[task + 1] - f.fbase[task]);
    if (F <= 1) return;
    int fbits = 0;
    while ((1 << fbits) < F) ++fbits;
    const int32_t w = (int32_t)(task >> kSpPBits), p = (int32_t)(task & (kSpP - 1));
    const SpWinDesc win = f.wins[w];
    const int64_t base = f.task_base[task];
    for (int k = tid; k < F; k += kSpBlock) fh[k] = 0;
    __syncthreads();
    for (int s = 0; s < win.nseg; ++s) {
        SpRunDesc r;
        int64_t s0, s1;
        sp_seg(f, win, p, s, r, s0, s1);
        for (int64_t i = s0 + tid; i < s1; i += kSpBlock) atomicAdd(&fh[sp_fine(sp_key(r, i), fbits)], 1u);
    }
    __syncthreads();
    if (tid < 64) {   // exclusive scan of the fine counts by one wave (F / 64 consecutive counts per lane)
        const int per = (F + 63) / 64, k0 = tid * per, k1 = min(F, k0 + per);
        uint32_t sum = 0;
        for (int k = k0; k < k1; ++k) sum += fh[k];
        uint32_t x = sum;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d); if (tid >= d) x += y; }
        uint32_t run = x - sum;
        for (int k = k0; k < k1; ++k) { const uint32_t t = fh[k]; fh[k] = run; run += t; }
    }
    __syncthreads();
    unsigned long long v[kSpAccCols];
    for (int s = 0; s < win.nseg; ++s) {
        SpRunDesc r;
        int64_t s0, s1;
        sp_seg(f, win, p, s, r, s0, s1);
        for (int64_t i = s0 + tid; i < s1; i += kSpBlock) {
            int64_t key;
            unsigned long long cnt;
            sp_load(r, i, nacc, key, cnt, v);
            const int64_t o = base + atomicAdd(&fh[sp_fine(key, fbits)], 1u);
            unsigned long long* e = f.sent + o * f.sw;
            if (f.sw == 2) *(ulonglong2*)e = make_ulonglong2((unsigned long long)key, f.scnt ? cnt : v[1]);
            else {
                e[0] = (unsigned long long)key;
                if (f.scnt) e[1] = cnt;
#pragma unroll 4
                for (int cc = 1; cc < nacc; ++cc) e[f.scnt + cc] = v[cc];
            }
        }
    }
    __syncthreads();
    uint32_t* fe = f.fend + f.fbase[task];
    for (int k = tid; k < F; k += kSpBlock) fe[k] = fh[k];   // after the scatter: the end of fine bucket k
}

constexpr int kSpAggBlock = 512;

// Aggregate: one workgroup per fine bucket (or per task whose entries fit one table: straight from the runs).
// LDS: table keys [T+1] (slot T: the Long.MIN_VALUE key's flag), accumulator columns [nacc][T+1] (column 0 = COUNT).
template <int NA>
__global__ void __launch_bounds__(kSpAggBlock) sp_agg_kernel(SpFireArgs f, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    extern __shared__ unsigned long long sp_lds[];
    const int T = f.T, stride = T + 1, nacc = NA ? NA : c.nacc;
    unsigned long long* tk = sp_lds;
    unsigned long long* tc = sp_lds + stride;
    __shared__ uint32_t nocc, ovf, ectr, dead;
    __shared__ unsigned long long rbase;
    __shared__ uint32_t smod[40], srem[40];
    __shared__ int32_t sp;
    const int tid = threadIdx.x;
    // fine bucket b -> its task (binary search over fbase)
    const int64_t b = blockIdx.x;
    int64_t lo = 0, hi = f.ntasks;   // fbase[lo] <= b < fbase[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (f.fbase[mid] <= b) lo = mid; else hi = mid;
    }
    const int64_t task = lo;
    const int64_t k = b - f.fbase[task];
    const int F = (int)(f.fbase[task + 1] - f.fbase[task]);
    const int32_t w = (int32_t)(task >> kSpPBits), p = (int32_t)(task & (kSpP - 1));
    const SpWinDesc win = f.wins[w];
    const int64_t base = f.task_base[task];
    int64_t a0 = 0, a1 = 0;
    if (F > 1) {
        a0 = base + (k ? f.fend[f.fbase[task] + k - 1] : 0u);
        a1 = base + f.fend[f.fbase[task] + k];
        if (a1 == a0) return;
    }
    const uint32_t ovf_lim = (uint32_t)(T - T / 8);
    if (tid == 0) dead = 0;

    auto clear_table = [&]() {
        for (int s = tid; s < stride; s += kSpAggBlock) {
            tk[s] = s < T ? kEmptyKey : 0ull;
            for (int cc = 0; cc < nacc; ++cc) tc[(int64_t)cc * stride + s] = ident_of(c.acc_kind[cc]);
        }
        if (tid == 0) { nocc = 0; ovf = 0; ectr = 0; }
    };
    auto insert = [&](int64_t key, unsigned long long cnt, const unsigned long long* v) {
        int s;
        if ((uint64_t)key == kEmptyKey) {
            s = T;
            if (tk[T] == 0ull && atomicCAS(&tk[T], 0ull, 1ull) == 0ull) atomicAdd(&nocc, 1u);
        } else {
            s = (int)(jm::mix64((uint64_t)key) & (uint64_t)(T - 1));
            for (int probe = 0;; ++probe) {
                if (probe >= T) { ovf = 1; return; }
                const unsigned long long cur = tk[s];
                if (cur == (unsigned long long)key) break;
                if (cur == kEmptyKey) {
                    const unsigned long long old = atomicCAS(&tk[s], kEmptyKey, (unsigned long long)key);
                    if (old == kEmptyKey) {
                        if (atomicAdd(&nocc, 1u) + 1 >= ovf_lim) ovf = 1;
                        break;
                    }
                    if (old == (unsigned long long)key) break;
                }
                s = (s + 1) & (T - 1);
            }
        }
        sp_apply<NA>(tc, stride, c, s, cnt, v);
    };
    auto emit = [&]() {
        __syncthreads();
        if (tid == 0) rbase = atomicAdd(&f.st->rows, (unsigned long long)nocc);
        __syncthreads();
        const int lane = tid & 63;
        for (int s0 = tid - lane; s0 < stride; s0 += kSpAggBlock) {   // wave-uniform loop: ballot-ranked rows
            const int s = s0 + lane;
            const bool occ = s < stride && (s < T ? tk[s] != kEmptyKey : tk[T] != 0ull);
            const unsigned long long m = __ballot(occ);
            if (!m) continue;
            uint32_t wb = 0;
            if (lane == 0) wb = atomicAdd(&ectr, (uint32_t)__popcll(m));
            wb = __shfl(wb, 0);
            if (!occ) continue;
            const int64_t row = (int64_t)rbase + wb + __popcll(m & ((1ull << lane) - 1));
            if (row >= f.out_cap) continue;
            const unsigned long long cnt = tc[s];
            f.o_key[row] = s < T ? (int64_t)tk[s] : LONG_MIN_J;
            f.o_start[row] = win.start;
            f.o_end[row] = win.end;
            if (f.o_count) f.o_count[row] = (int64_t)cnt;
            for (int j = 0; j < c.nout; ++j) {
                const AggDesc d = c.agg[j];
                const unsigned long long x = d.acc > 0 ? tc[(int64_t)d.acc * stride + s] : cnt;
                if (f.raw) ((unsigned long long*)f.o_agg[j])[row] = x;
                else write_agg(d, cnt, x, 0, f.o_agg[j], nullptr, row);
            }
        }
    };
    // split stack: pass (mod, rem) takes the entries whose hash bits 32.. are rem modulo mod; a pass whose distinct
    // keys would crowd the table is redone as two half passes
    auto aggregate = [&](auto&& for_each) {
        if (tid == 0) { smod[0] = 1; srem[0] = 0; sp = 1; }
        __syncthreads();
        while (sp > 0) {
            const uint32_t mod = smod[sp - 1], rem = srem[sp - 1];
            __syncthreads();
            if (tid == 0) --sp;
            clear_table();
            __syncthreads();
            for_each([&](int64_t key, unsigned long long cnt, const unsigned long long* v) {
                if (*(volatile uint32_t*)&ovf) return;
                if (((uint32_t)(jm::mix64((uint64_t)key) >> 32) & (mod - 1)) != rem) return;
                insert(key, cnt, v);
            });
            __syncthreads();
            if (ovf) {
                if (tid == 0) {
                    if (mod >= (1u << 20) || sp + 2 > 40) { raise_error(f.st, FWA_E_STATE); dead = 1; }
                    else { smod[sp] = 2 * mod; srem[sp] = rem + mod; smod[sp + 1] = 2 * mod; srem[sp + 1] = rem; sp += 2; }
                }
                __syncthreads();
                if (dead) return;
                continue;
            }
            emit();
            __syncthreads();
        }
    };

    unsigned long long v[kSpAccCols];
    if (F <= 1) {   // the task fits one table: straight from the run segments
        aggregate([&](auto&& fn) {
            for (int s = 0; s < win.nseg; ++s) {
                SpRunDesc r;
                int64_t s0, s1;
                sp_seg(f, win, p, s, r, s0, s1);
                for (int64_t i = s0 + tid; i < s1; i += kSpAggBlock) {
                    int64_t key;
                    unsigned long long cnt;
                    sp_load(r, i, nacc, key, cnt, v);
                    fn(key, cnt, v);
                }
            }
        });
        return;
    }
    aggregate([&](auto&& fn) {
        for (int64_t i = a0 + tid; i < a1; i += kSpAggBlock) {
            int64_t key;
            unsigned long long cnt;
            sp_load_ent(f.sent, f.sw, f.scnt, i, nacc, key, cnt, v);
            fn(key, cnt, v);
        }
    });
}

}  // namespace

// ---- host side ----

static bool sp_eligible(const fwa_config* cfg) {
    return cfg->window_kind == FWA_TUMBLE && cfg->nullable_cols == 0 && cfg->tz_n == 0 &&
           !(cfg->flags & FWA_CFG_DYNAMIC_GAP) && (cfg->semantics == FWA_SEM_TABLE || cfg->allowed_lateness_ms == 0);
}

static void sp_free_run(SpRun* r) {
    if (r->mem) (void)hipFree(r->mem);
    delete r;
}

// run buffers are recycled: a steady stream allocates its lists once instead of hipMalloc / hipFree per push
static void sp_release_run(SpState* s, SpRun* r) {
    if (r->mem) {
        s->pool.push_back({r->bytes, r->mem});
        r->mem = nullptr;
        if (s->pool.size() > 4) {   // keep the 4 largest
            std::sort(s->pool.begin(), s->pool.end());
            (void)hipFree(s->pool.front().second);
            s->pool.erase(s->pool.begin());
        }
    }
    delete r;
}

static void* sp_alloc_run(SpState* s, size_t bytes, size_t* got) {
    int best = -1;
    for (int i = 0; i < (int)s->pool.size(); ++i)
        if (s->pool[i].first >= bytes && s->pool[i].first <= 2 * bytes + (64u << 20) &&
            (best < 0 || s->pool[i].first < s->pool[best].first)) best = i;
    if (best >= 0) {
        void* p = s->pool[best].second;
        *got = s->pool[best].first;
        s->pool.erase(s->pool.begin() + best);
        return p;
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {   // give the pool back to the device and retry once
        for (auto& x : s->pool) (void)hipFree(x.second);
        s->pool.clear();
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    }
    *got = bytes;
    return p;
}

static void sp_destroy(fwa_engine* e) {
    SpState* s = e->sp;
    if (!s) return;
    for (SpRun* r : s->runs) if (r) sp_free_run(r);
    for (auto& x : s->pool) (void)hipFree(x.second);
    for (void* p : {(void*)s->d_ghist, (void*)s->d_cursor, (void*)s->d_off, (void*)s->d_scratch, (void*)s->d_desc})
        if (p) (void)hipFree(p);
    delete s;
    e->sp = nullptr;
}

static int sp_init(fwa_engine* e) {
    SpState* s = new SpState();
    e->sp = s;
    const size_t per_slot = 8 * (size_t)(1 + e->nacc);
    int T = 2048;   // ~49 KB at COUNT + one accumulator: three aggregate workgroups per CU
    while (T > 256 && (size_t)(T + 1) * per_slot > 72 * 1024) T >>= 1;
    s->T = T;
    s->lds = (size_t)(T + 1) * per_slot;
    size_t fr = 0, tot = 0;   // compaction budget: a quarter of the device's memory (FWA_OPT_SP_BUDGET: bytes, tests)
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) tot = (size_t)64 << 30;
    s->budget = tot / 4;
    HIPCHK(e, hipMalloc(&s->d_cursor, 4 * (size_t)kSpW * kSpP));
    HIPCHK(e, hipMalloc(&s->d_off, 4 * ((size_t)kSpW * kSpP + 1)));
    return FWA_OK;
}

// FWA_OPT_SP_TABLE (before the first push: the LDS table size, rounded down to a power of two >= 64; tests force
// split passes with small tables), FWA_OPT_SP_FMAX, FWA_OPT_SP_BUDGET
static int sp_set_option(fwa_engine* e, int32_t opt, int64_t v) {
    SpState* s = e->sp;
    if (!s) return FWA_E_UNSUPPORTED;
    if (opt == FWA_OPT_SP_TABLE) {
        if (!s->runs.empty() || !s->wins.empty()) return FWA_E_STATE;
        const size_t per_slot = 8 * (size_t)(1 + e->nacc);
        int t = 64;
        while (2 * t <= v && (size_t)(2 * t + 1) * per_slot <= 150 * 1024) t *= 2;
        s->T = t;
        s->lds = (size_t)(t + 1) * per_slot;
    } else if (opt == FWA_OPT_SP_FMAX) {
        s->fmax = (int32_t)std::max<int64_t>(1, std::min<int64_t>(kSpMaxF, v));
    } else {
        s->budget = (size_t)std::max<int64_t>(1, v);
    }
    return FWA_OK;
}

static int sp_live_windows(const fwa_engine* e) { return e->sp ? (int)e->sp->wins.size() : 0; }

// one push pass over the windows qs (sorted, <= kSpW): bucket, allocate the run, scatter
static int sp_status_error(fwa_engine* e);

// redo (the fused form: pa.fused, single): set when a record fell past the pass's windows -- nothing is kept and the
// caller pushes again in the two-pass form; errors and drops are read from the status here.
static int sp_push_pass(fwa_engine* e, SpPushArgs pa, const std::vector<int64_t>& qs, double* ms, bool single,
                        bool* redo = nullptr) {
    SpState* s = e->sp;
    pa.nq = (int32_t)qs.size();
    for (int w = 0; w < pa.nq; ++w) pa.qs[w] = qs[w];
    pa.want = nullptr;
    const int nb = pa.nq * kSpP;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(kSpPushBlocks, (pa.n + 8191) / 8192));
    pa.per = (pa.n + blocks - 1) / blocks;
    const size_t gh = (size_t)blocks * nb;
    if (gh > s->ghist_cap) {
        if (s->d_ghist) HIPCHK(e, hipFree(s->d_ghist));
        s->d_ghist = nullptr;
        HIPCHK(e, hipMalloc(&s->d_ghist, 4 * gh));
        s->ghist_cap = gh;
    }
    pa.ghist = s->d_ghist;
    pa.cursor = s->d_cursor;
    pa.off = s->d_off;
    HIPCHK(e, hipMemsetAsync(s->d_cursor, 0, 4 * (size_t)nb, e->stream));
    HIPCHK(e, hipEventRecord(e->ev[6], e->stream));
    sp_hist_kernel<<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec);
    sp_scan_kernel<<<1, kSpBlock, 0, e->stream>>>(s->d_cursor, s->d_off, nb);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[7], e->stream));
    SpRun* r = new SpRun();
    r->hoff.resize((size_t)nb + 1);
    r->nq = pa.nq;
    for (int w = 0; w < pa.nq; ++w) r->qs[w] = qs[w];
    r->has_cnt = pa.pcount != nullptr;
    r->W = 1 + (r->has_cnt ? 1 : 0) + (e->nacc - 1);
    // narrow entries: a fused single pass of COUNT + one BIGINT sum (the handle's steady state) while the handle has
    // seen no key or value past 32 bits; a push that has one is redone with 64-bit entries, which then stay
    if (single && pa.fused && s->narrow && e->opt_narrow != 0 && e->nacc == 2 && !pa.pcount && e->ec.acc_kind[1] == ACC_ADD_I64 &&
        input_class(e->ec.agg[pa.aggi[1]].kind) == 0) {
        r->nw = true;
        r->W = 1;
    }
    pa.nw = r->nw ? 1 : 0;
    float t = 0.f;
    int64_t total;
    // one pass covers the push (the common case): the run is sized for every record of the push, so the scatter
    // follows the scan without a host round trip; several passes size each run exactly (a host sync per pass)
    if (single) {
        const size_t bytes = 8 * (size_t)pa.n * (size_t)r->W + 4 * ((size_t)nb + 1);
        r->mem = sp_alloc_run(s, bytes, &r->bytes);
        if (!r->mem) { delete r; return fail(e, FWA_E_OOM, "out of device memory (window record lists)"); }
        total = pa.n;
    } else {
        HIPCHK(e, hipMemcpyAsync(r->hoff.data(), s->d_off, 4 * ((size_t)nb + 1), hipMemcpyDeviceToHost, e->stream));
        if (int rc = stream_sync(e)) { delete r; return rc; }
        total = r->hoff[nb];
        if (total == 0) { delete r; return FWA_OK; }
        const size_t bytes = 8 * (size_t)total * (size_t)r->W + 4 * ((size_t)nb + 1);
        r->mem = sp_alloc_run(s, bytes, &r->bytes);
        if (!r->mem) { delete r; return fail(e, FWA_E_OOM, "out of device memory (window record lists)"); }
    }
    char* m = (char*)r->mem;
    r->ent = (unsigned long long*)m; m += 8 * (size_t)total * (size_t)r->W;
    r->off = (uint32_t*)m;
    HIPCHK(e, hipMemcpyAsync(r->off, s->d_off, 4 * ((size_t)nb + 1), hipMemcpyDeviceToDevice, e->stream));
    pa.oent = r->ent;
    pa.ocap = total;
    pa.ow = r->W;
    HIPCHK(e, hipEventRecord(e->ev[8], e->stream));
    switch (e->nacc) {
        case 1: sp_scatter_kernel<1><<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec); break;
        case 2: sp_scatter_kernel<2><<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec); break;
        case 3: sp_scatter_kernel<3><<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec); break;
        case 4: sp_scatter_kernel<4><<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec); break;
        default: sp_scatter_kernel<0><<<blocks, kSpBlock, 0, e->stream>>>(pa, e->d_ec); break;
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[9], e->stream));
    if (single) HIPCHK(e, hipMemcpyAsync(r->hoff.data(), s->d_off, 4 * ((size_t)nb + 1), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipEventSynchronize(e->ev[9]));
    if (redo) {                                  // fused: the pass's own checks decide whether it stands
        *redo = false;
        if (int rc = sync_status(e)) { sp_release_run(s, r); return rc; }
        if (e->h_st->error) { sp_release_run(s, r); return sp_status_error(e); }
        if (e->h_st->spill_n) { sp_release_run(s, r); *redo = true; return FWA_OK; }
        if (r->nw && e->h_st->wide_n) { s->narrow = false; sp_release_run(s, r); *redo = true; return FWA_OK; }
    }
    if (single) {
        if (int rc = stream_sync(e)) { sp_release_run(s, r); return rc; }
        if (r->hoff[nb] == 0) { sp_release_run(s, r); return FWA_OK; }
    }
    r->n = r->hoff[nb];
    HIPCHK(e, hipEventElapsedTime(&t, e->ev[6], e->ev[7]));
    *ms += t;
    HIPCHK(e, hipEventElapsedTime(&t, e->ev[8], e->ev[9]));
    *ms += t;
    int32_t rid = -1;   // reuse a freed run id (a steady stream would otherwise grow the table by one id per pass)
    for (int32_t i = 0; i < (int32_t)s->runs.size(); ++i) if (!s->runs[i]) { rid = i; break; }
    if (rid < 0) {
        if (s->runs.size() >= (size_t)INT32_MAX) { sp_release_run(s, r); return fail(e, FWA_E_OOM, "too many record-list runs"); }
        rid = (int32_t)s->runs.size();
        s->runs.push_back(r);
    } else {
        s->runs[(size_t)rid] = r;
    }
    for (int w = 0; w < pa.nq; ++w) {
        const int64_t cnt = (int64_t)r->hoff[(size_t)(w + 1) * kSpP] - (int64_t)r->hoff[(size_t)w * kSpP];
        if (cnt == 0) continue;
        SpWin& sw = s->wins[qs[w]];
        sw.parts.push_back({rid, w});
        sw.entries += cnt;
        r->alive++;
    }
    return FWA_OK;
}

static int sp_status_error(fwa_engine* e) {
    const int err = e->h_st->error;
    return fail(e, err, err == FWA_E_KEYGROUP ? "Key group is not in the owned KeyGroupRange (StateTable.getMapForKeyGroup)"
                      : err == FWA_E_TS_MIN ? "Record has Long.MIN_VALUE timestamp (= no timestamp marker)."
                      : err == FWA_E_OOM ? "too many distinct windows in one push"
                                         : "record-list state inconsistency");
}

static int sp_compact(fwa_engine* e);

static int sp_push(fwa_engine* e, IngestArgs& a, int64_t n, int64_t* late_dropped_out) {
    SpState* s = e->sp;
    SpPushArgs pa;
    memset(&pa, 0, sizeof(pa));
    pa.keys = a.keys;
    pa.ts = a.ts;
    pa.key_hash = a.key_hash;
    pa.pcount = a.pcount;
    pa.n = n;
    pa.wm = e->wm;
    pa.dropidx = a.dropidx;
    pa.st = e->d_st;
    pa.check_kg = !(e->cfg.kg_start == 0 && e->cfg.kg_end == e->cfg.max_parallelism - 1) ||
                  e->cfg.key_kind == FWA_KEY_GROUP_PREFIXED;
    for (int j = 0; j < e->ec.naggs; ++j) {   // accumulator column -> its (first) aggregate and source column
        const AggDesc& d = e->ec.agg[j];
        if (d.acc <= 0 || d.alias) continue;
        pa.aggi[d.acc] = j;
        pa.col[d.acc] = a.pcount ? a.cols[j] : a.cols[d.col];
    }
    if (int rc = reset_push_status(e)) return rc;
    double ms = 0;   // device time of the push kernels (host syncs between them excluded)
    // fused form: the kSpW windows from the first one the watermark leaves open, checked and bucketed in one pass
    // over the keys and timestamps (sp_hist_kernel); a record past them (a push spanning more windows) sends the
    // push to the two-pass form below
    if (!a.pcount && e->wm != LONG_MIN_J) {
        int64_t q0 = slice_q(e, e->wm);
        const int64_t end0 = jm::wadd(slice_start(e, q0), e->g);
        if (!(e->cfg.semantics == FWA_SEM_TABLE && end0 == LONG_MAX_J) && !(e->wm < jm::wsub(end0, 1))) ++q0;
        std::vector<int64_t> qs;
        for (int w = 0; w < kSpW; ++w) qs.push_back(q0 + w);
        SpPushArgs pf = pa;
        pf.fused = 1;
        bool redo = false;
        if (int rc = sp_push_pass(e, pf, qs, &ms, true, &redo)) return rc;
        if (!redo) {
            const int64_t dropped = (int64_t)e->h_st->dropped;
            e->ingest_ms += ms;
            e->partition_ms += ms;
            e->ingest_launches++;
            e->ingest_records += n;
            if (a.dropidx) {   // FWA_CFG_LATE_INDICES
                unsigned long long m = 0;
                HIPCHK(e, hipMemcpy(&m, &e->d_st->drop_n, 8, hipMemcpyDeviceToHost));
                e->late_idx.resize((size_t)m);
                if (m) HIPCHK(e, hipMemcpy(e->late_idx.data(), e->d_dropidx, 4 * (size_t)m, hipMemcpyDeviceToHost));
                std::sort(e->late_idx.begin(), e->late_idx.end());
            }
            e->records_in += n;
            e->late_dropped += dropped;
            if (late_dropped_out) *late_dropped_out = dropped;
            if (!s->compacting) {
                s->compacting = true;
                const int rc = sp_compact(e);
                s->compacting = false;
                if (rc) return rc;
            }
            return FWA_OK;
        }
        ms = 0;                                   // the two-pass form redoes the push
        if (int rc = reset_push_status(e)) return rc;
        if (a.dropidx) HIPCHK(e, hipMemsetAsync(&e->d_st->drop_n, 0, 8, e->stream));
    }
    HIPCHK(e, hipEventRecord(e->ev[4], e->stream));
    sp_range_kernel<<<grid_for(n, 1024), kBlock, 0, e->stream>>>(pa, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[5], e->stream));
    if (int rc = sync_status(e)) return rc;
    if (e->h_st->error) return sp_status_error(e);
    {
        float t = 0.f;
        HIPCHK(e, hipEventElapsedTime(&t, e->ev[4], e->ev[5]));
        ms += t;
    }
    const DevStatus st = *e->h_st;
    if (st.max_q != 0 || st.min_q != ~0ull) {
        const int64_t qmin = jm::unord_i64(st.min_q), qmax = jm::unord_i64(st.max_q);
        std::vector<int64_t> qs;
        if ((uint64_t)qmax - (uint64_t)qmin < (uint64_t)kSpW) {
            for (int64_t q = qmin;; ++q) { qs.push_back(q); if (q == qmax) break; }
        } else {   // a wide push: collect its distinct windows first
            HIPCHK(e, hipMemsetAsync(e->d_want, 0, sizeof(unsigned long long) * kWantCap, e->stream));
            SpPushArgs pw = pa;
            pw.want = e->d_want;
            pw.dropidx = nullptr;
            sp_range_kernel<<<grid_for(n, 1024), kBlock, 0, e->stream>>>(pw, e->d_ec);
            HIPCHK(e, hipGetLastError());
            std::vector<unsigned long long> want(kWantCap);
            HIPCHK(e, hipMemcpyAsync(want.data(), e->d_want, sizeof(unsigned long long) * kWantCap, hipMemcpyDeviceToHost, e->stream));
            if (int rc = sync_status(e)) return rc;
            if (e->h_st->error) return sp_status_error(e);
            for (unsigned long long x : want) if (x) qs.push_back(jm::unord_i64(x - 1ull));
            std::sort(qs.begin(), qs.end());
        }
        for (size_t i = 0; i < qs.size(); i += kSpW) {
            std::vector<int64_t> chunk(qs.begin() + i, qs.begin() + std::min(qs.size(), i + kSpW));
            if (int rc = sp_push_pass(e, pa, chunk, &ms, qs.size() <= (size_t)kSpW)) return rc;
        }
    }
    if (int rc = sync_status(e)) return rc;
    if (e->h_st->error) return sp_status_error(e);
    e->ingest_ms += ms;
    e->partition_ms += ms;
    e->ingest_launches++;
    e->ingest_records += n;
    if (a.dropidx) {   // FWA_CFG_LATE_INDICES
        unsigned long long m = 0;
        HIPCHK(e, hipMemcpy(&m, &e->d_st->drop_n, 8, hipMemcpyDeviceToHost));
        e->late_idx.resize((size_t)m);
        if (m) HIPCHK(e, hipMemcpy(e->late_idx.data(), e->d_dropidx, 4 * (size_t)m, hipMemcpyDeviceToHost));
        std::sort(e->late_idx.begin(), e->late_idx.end());
    }
    const int64_t dropped = (int64_t)st.dropped;
    e->records_in += n;
    e->late_dropped += dropped;
    if (late_dropped_out) *late_dropped_out = dropped;
    if (!s->compacting) {
        s->compacting = true;
        const int rc = sp_compact(e);
        s->compacting = false;
        if (rc) return rc;
    }
    return FWA_OK;
}

// Aggregate the windows qs (live) into the output columns: raw = 1 writes COUNT and the accumulator words
// (snapshot / partials); retire = drop their record lists afterwards.
static int sp_fire(fwa_engine* e, const std::vector<int64_t>& qs, int raw, bool retire, int64_t* nrows) {
    SpState* s = e->sp;
    *nrows = 0;
    if (qs.empty()) return FWA_OK;
    std::vector<SpRunDesc> rd;
    std::vector<int32_t> rmap(s->runs.size(), -1);
    std::vector<SpWinDesc> wd;
    std::vector<SpSeg> sg;
    std::vector<int64_t> tb((size_t)qs.size() * kSpP + 1, 0);
    bool has_cnt = false;
    for (size_t w = 0; w < qs.size(); ++w) {
        const SpWin& sw = s->wins.at(qs[w]);
        SpWinDesc d;
        d.start = slice_start(e, qs[w]);
        d.end = jm::wadd(d.start, e->g);
        d.seg0 = (int32_t)sg.size();
        d.nseg = (int32_t)sw.parts.size();
        for (auto& pr : sw.parts) {
            SpRun* r = s->runs[pr.first];
            if (rmap[pr.first] < 0) {
                rmap[pr.first] = (int32_t)rd.size();
                rd.push_back({r->ent, r->off, r->W, r->has_cnt ? 1 : 0, r->nw ? 1 : 0, 0});
            }
            has_cnt = has_cnt || r->has_cnt;
            sg.push_back({rmap[pr.first], pr.second});
            for (int p = 0; p < kSpP; ++p)
                tb[w * kSpP + p + 1] += (int64_t)r->hoff[(size_t)pr.second * kSpP + p + 1] - (int64_t)r->hoff[(size_t)pr.second * kSpP + p];
        }
        wd.push_back(d);
    }
    // fine buckets per task: one table's worth of entries (T/2) on average; a task that fits one table is
    // aggregated straight from the runs
    const int64_t ntasks = (int64_t)qs.size() * kSpP, tcap = s->T * 3 / 4;
    const int fmax = s->fmax > 0 ? std::min(kSpMaxF, s->fmax) : kSpMaxF;
    std::vector<int64_t> fb((size_t)ntasks + 1, 0);
    for (int64_t t = 0; t < ntasks; ++t) {
        const int64_t E = tb[t + 1];
        int64_t F = E == 0 ? 0 : 1;
        while (F > 0 && F * tcap < E && F < fmax) F <<= 1;
        fb[t + 1] = fb[t] + F;
    }
    const int64_t nfine = fb.back();
    for (size_t t = 0; t + 1 < tb.size(); ++t) tb[t + 1] += tb[t];
    const int64_t total = tb.back();
    // device descriptors, scratch, output (rows <= entries)
    const size_t b_rd = sizeof(SpRunDesc) * rd.size(), b_wd = sizeof(SpWinDesc) * wd.size(), b_sg = sizeof(SpSeg) * sg.size();
    const size_t b_tb = 8 * tb.size(), b_fb = 8 * fb.size(), b_fe = 4 * (size_t)std::max<int64_t>(nfine, 1);
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t need = al(b_rd) + al(b_wd) + al(b_sg) + al(b_tb) + al(b_fb) + al(b_fe);
    if (need > s->desc_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (s->d_desc) HIPCHK(e, hipFree(s->d_desc));
        s->d_desc = nullptr;
        HIPCHK(e, hipMalloc(&s->d_desc, need * 2));
        s->desc_cap = need * 2;
    }
    char* dp = s->d_desc;
    SpFireArgs f;
    memset(&f, 0, sizeof(f));
    f.runs = (const SpRunDesc*)dp; if (int rc = upload(e, dp, rd.data(), b_rd)) return rc; dp += al(b_rd);
    f.wins = (const SpWinDesc*)dp; if (int rc = upload(e, dp, wd.data(), b_wd)) return rc; dp += al(b_wd);
    f.segs = (const SpSeg*)dp; if (int rc = upload(e, dp, sg.data(), b_sg)) return rc; dp += al(b_sg);
    f.task_base = (const int64_t*)dp; if (int rc = upload(e, dp, tb.data(), b_tb)) return rc; dp += al(b_tb);
    f.fbase = (const int64_t*)dp; if (int rc = upload(e, dp, fb.data(), b_fb)) return rc; dp += al(b_fb);
    f.fend = (uint32_t*)dp;
    f.ntasks = ntasks;
    const size_t sbytes = 8 * (size_t)total * (1 + (has_cnt ? 1 : 0) + (size_t)(e->nacc - 1));
    if (sbytes > s->scratch_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (s->d_scratch) HIPCHK(e, hipFree(s->d_scratch));
        s->d_scratch = nullptr;
        const size_t cap = sbytes + sbytes / 4;
        HIPCHK(e, hipMalloc(&s->d_scratch, cap));
        s->scratch_cap = cap;
    }
    f.sn = total;
    f.sent = (unsigned long long*)s->d_scratch;
    f.scnt = has_cnt ? 1 : 0;
    f.sw = 1 + f.scnt + (e->nacc - 1);
    f.T = s->T;
    f.raw = raw;
    if (int rc = ensure_out(e, std::max<int64_t>(total, 1))) return rc;
    f.o_key = e->o_key;
    f.o_start = e->o_start;
    f.o_end = e->o_end;
    f.o_count = raw ? e->o_count : nullptr;
    for (int j = 0; j < e->cfg.num_aggs; ++j) f.o_agg[j] = e->o_agg[j];
    f.out_cap = e->out_cap;
    f.st = e->d_st;
    HIPCHK(e, hipMemsetAsync(&e->d_st->rows, 0, 8, e->stream));
    e->rows_zero = false;
    HIPCHK(e, hipEventRecord(e->ev[2], e->stream));
    auto launch = [&](auto na) {
        constexpr int NA = decltype(na)::value;
        sp_refine_kernel<NA><<<(unsigned)ntasks, kSpBlock, 0, e->stream>>>(f, e->d_ec);
        if (nfine > 0) sp_agg_kernel<NA><<<(unsigned)nfine, kSpAggBlock, s->lds, e->stream>>>(f, e->d_ec);
    };
    switch (e->nacc) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 3: launch(std::integral_constant<int, 3>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        default: launch(std::integral_constant<int, 0>()); break;
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(e->ev[3], e->stream));
    if (int rc = sync_status(e)) return rc;
    if (e->h_st->error) return sp_status_error(e);
    *nrows = (int64_t)e->h_st->rows;
    if (*nrows > e->out_cap) return fail(e, FWA_E_STATE, "record-list fire emitted more rows than entries");
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev[2], e->ev[3]));
    e->fire_ms += ms;
    e->fire_launches++;
    e->fire_rows += *nrows;
    if (retire) {
        for (int64_t q : qs) {
            auto it = s->wins.find(q);
            for (auto& pr : it->second.parts) {
                SpRun*& r = s->runs[pr.first];
                if (--r->alive == 0) { sp_release_run(s, r); r = nullptr; }
            }
            s->wins.erase(it);
        }
        while (!s->runs.empty() && s->runs.back() == nullptr) s->runs.pop_back();
    }
    return FWA_OK;
}

// Memory bound of the record lists (state is O(accepted records per live window)): once the live lists exceed the
// budget, every live window whose list grew to at least twice its size after its last compaction is folded into one
// pre-aggregated run -- its raw fire (key, COUNT, accumulator words per distinct key, what fwa_drain_partials
// exports) pushed back as partial accumulators. Windows whose keys repeat shrink to their distinct keys; a window of
// distinct keys is compacted at most once per doubling. Statistics are left as the caller's push made them.
static int sp_compact(fwa_engine* e) {
    SpState* s = e->sp;
    size_t live = 0;
    for (const SpRun* r : s->runs) if (r) live += r->bytes;
    if (live <= s->budget) return FWA_OK;
    std::vector<int64_t> qs;
    for (auto& kv : s->wins)
        if (kv.second.entries >= 2 * std::max<int64_t>(kv.second.base, 1)) qs.push_back(kv.first);
    if (qs.empty()) return FWA_OK;
    const int64_t c_in = e->records_in, c_late = e->late_dropped, c_il = e->ingest_launches, c_ir = e->ingest_records;
    const double c_ims = e->ingest_ms, c_pms = e->partition_ms, c_fms = e->fire_ms;
    const int64_t c_fl = e->fire_launches, c_fr = e->fire_rows;
    int64_t nrows = 0;
    int rc = sp_fire(e, qs, 1, true, &nrows);
    if (!rc && nrows > 0) {
        IngestArgs a;
        memset(&a, 0, sizeof(a));
        a.n = nrows;
        a.wm = e->wm;
        a.keys = e->o_key;
        a.ts = e->o_start;                             // the window start: assigns each row to its window again
        a.pcount = (const unsigned long long*)e->o_count;
        for (int j = 0; j < e->ec.naggs; ++j) if (e->ec.agg[j].acc > 0) a.cols[j] = e->o_agg[j];
        rc = sp_push(e, a, nrows, nullptr);
    }
    for (int64_t q : qs) { auto it = s->wins.find(q); if (it != s->wins.end()) it->second.base = it->second.entries; }
    e->records_in = c_in; e->late_dropped = c_late; e->ingest_launches = c_il; e->ingest_records = c_ir;
    e->ingest_ms = c_ims; e->partition_ms = c_pms; e->fire_ms = c_fms; e->fire_launches = c_fl; e->fire_rows = c_fr;
    s->compactions++;
    return rc;
}

// windows whose maxTimestamp is <= wm (all: wm == Long.MAX_VALUE)
static std::vector<int64_t> sp_due(const fwa_engine* e, int64_t wm) {
    std::vector<int64_t> qs;
    for (auto& kv : e->sp->wins) {
        const int64_t end = jm::wadd(slice_start(e, kv.first), e->g);
        if (wm == LONG_MAX_J || jm::wsub(end, 1) <= wm) qs.push_back(kv.first);
    }
    return qs;
}

// drop the lists of windows past wm without emitting them (restore: they fired before the snapshot)
static void sp_retire(fwa_engine* e, int64_t wm) {
    SpState* s = e->sp;
    for (int64_t q : sp_due(e, wm)) {
        auto it = s->wins.find(q);
        for (auto& pr : it->second.parts) {
            SpRun*& r = s->runs[pr.first];
            if (--r->alive == 0) { sp_release_run(s, r); r = nullptr; }
        }
        s->wins.erase(it);
    }
}
