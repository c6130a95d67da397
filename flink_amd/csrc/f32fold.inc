// SUM(FLOAT) as the reference's float32 arrival-order fold (include/flink_amd.h, FWA_CFG_F32_FOLD) -- included by
// engine.hip.
//
// Reference: the Table SUM(FLOAT) keeps a FLOAT buffer and adds each record to it (SumAggFunction.java:133-139), the
// DataStream sum(pos) on a Float field reduces in arrival order (SumAggregator.java:66-76). The result of a
// (key, window) is therefore acc = +0.0f; acc = (float)(acc + v) for every accepted non-NULL record in arrival order,
// which the oracle computes (fwa_oracle.c: x->f = x->f + v). The engine's own SUM_F32 adds in f64 with atomics and
// rounds once: deterministic, close, and not those bits.
//
// Design: the handle keeps everything it has -- the f64 accumulator of SUM_F32 still runs and supplies the row, its
// NULL flag and every ingest path, record list and snapshot body unchanged -- and, beside it, a device-resident
// open-addressing set with one entry per live (key, slice) (TUMBLE: a slice is a window) carrying one float per folded
// source column. Every push first runs the fold pass over the batch, once, ahead of the ingest (slice-miss and overflow
// replays of the ingest never come back here):
//   fold_resolve_kernel  one thread per record: the slice as the ingest computes it, sp_slice(assign_ts(ts)); a record
//                        of a slice below q_min (its window fired: the ingest drops it) gets the sentinel slot,
//                        every other record upserts (key, slice) and gets its entry's slot number;
//   a stable radix sort  of (slot, record index) over the bits a slot number needs (hipcub::DeviceRadixSort): equal
//                        slots become one contiguous run and, the sort being stable, keep their arrival order;
//   fold_heads_kernel    the first position of every run (one atomic per wave reserves room in the head list; the
//                        list's order does not matter, runs are independent);
//   fold_runs_kernel     one lane per run: load the slot's accumulator, walk the run's record indices in order,
//                        acc = __fadd_rn(acc, v[idx]) for the non-NULL ones, store once. No atomics on an
//                        accumulator, no '+' the compiler could contract or reassociate.
// A float32 fold cannot be split or tree-reduced without changing its bits ((a + b) + c != a + (b + c)), so a run is
// serial by nature and a hot key's run takes one lane as long as it is; the balance is across runs only. The gathers
// v[idx] are the traffic and the walk is latency-bound: the lane issues four index loads and four value loads before
// the four dependent adds. Results do not depend on the launch shape.
// The q >= q_min filter is the argument of TUMBLE COUNT(DISTINCT): q_min comes from accept_threshold at the handle's
// watermark (dist_qmin), as the ingest's thresholds do, and within a window acceptance only ever turns off, so with no
// allowed lateness a record is accepted iff its slice is not below q_min. Where q_min is unknown nothing is filtered: a
// record folded into a fired window's entry changes nothing anybody reads.
//
// The set. 16 bytes per slot: word 0 the key (a zero key is stored as 1 with tag bit 0 set), word 1 the tag
// q << 2 | 2 | key-was-zero (bit 1 keeps a tag from being 0 = EMPTY; q keeps 62 bits, so windows shorter than 4 ms are
// refused). Words are claimed in order with atomicCAS(word, EMPTY, mine) and never change afterwards, as in
// distinct.inc: exactly one lane creates an entry, nothing waits for another lane. The float accumulators live in a
// plan-owned array [column][slot], +0.0f (all bits 0) from the allocation on. Capacity: the host keeps an upper bound
// of occupied slots (previous bound + records, corrected by the count of entries the last pass created) at <= slots / 2
// and otherwise rebuilds the set from the entries of windows that have not fired (the live cut at q_min), carrying
// their accumulators, into a table of 2 x (live + this batch) slots. Firing costs nothing: a fired window's entries are
// garbage that the next rebuild drops.
//
// At the fire fold_rows_kernel (one thread per row and folded aggregate) takes the slice from the row's win_start,
// finds the entry and writes its float into a plan-owned column that fill_out substitutes for the f64-summed one (never
// in place: fill_out may run twice over the same rows). It runs inside fwa_advance_watermark, so no later push can have
// rebuilt the set; a handle with the flag completes its fire inside fwa_advance_watermark_async. A row whose SUM_F32 is
// not NULL and has no entry is a broken invariant: FWA_E_INTERNAL.

struct FoldPlan {
    int32_t nc = 0;                        // folded source columns
    int32_t src[FWA_MAX_COLS] = {};        // folded column c: the caller's value column
    int32_t col_of[FWA_MAX_AGGS] = {};     // caller's aggregate j: its folded column, -1: not a SUM_F32
    int64_t mask = 0;                      // bit j: the caller's aggregate j is folded (snapshot header word 29)
    int32_t nullable = 0;                  // the caller's nullable_cols
    fwa_config ucfg;                       // the caller's configuration (host pushes stage every input column)
    unsigned long long* d_tab = nullptr;   // the set, [slots][2]
    float* d_acc = nullptr;                // the accumulators, [nc][slots]
    int64_t slots = 0, first_slots = 0;    // first_slots: FWA_OPT_F32_FOLD_SLOTS (0: sized from the first push)
    int64_t bound = 0;                     // upper bound of occupied slots
    int64_t live = 0, rebuilds = 0;        // entries counted at the last rebuild; rebuilds so far
    int64_t last_add = 0;                  // the last pass's share of `bound`, until its exact count replaces it
    uint32_t* d_rec = nullptr;             // per push, [5][rec_cap]: slot, index, sorted slot, sorted index, run heads
    int64_t rec_cap = 0;
    char* d_stage = nullptr;               // host pushes: every input column, staged once
    size_t stage_bytes = 0;
    unsigned long long* d_ctr = nullptr;   // [0] entries counted / moved, [1] inserts that found no slot, [2] entries the
    unsigned long long* h_ctr = nullptr;   // last pass created, [3] run heads, [4] non-NULL rows without an entry
    float* d_out[FWA_MAX_AGGS] = {};       // the folded results of the fired rows per folded aggregate, [out_cap]
    int64_t out_cap = 0;
    hipEvent_t ev[5] = {};                 // the pass: begin, resolve end, sort end, fold end; its created-count copy
    hipEvent_t rev[2] = {};                // the fire's lookup: begin, end
    bool timing = false;                   // ev[0..3] hold a pass not yet added to ingest_ms
    double resolve_ms = 0.0, sort_ms = 0.0, fold_ms = 0.0, rows_ms = 0.0;   // device time so far
};

static int ensure_sort_tmp(fwa_engine* e, size_t bytes);   // sessions_host.inc

namespace {

const char* const kFoldNoPartials = "FWA_CFG_F32_FOLD: partial accumulators of a float32 arrival-order fold are not "
                                    "supported (a fold split across ranks is the two-phase plan, which has no single "
                                    "float32 result)";
constexpr int64_t kFoldMinSlots = 1 << 12;
constexpr int64_t kFoldMinSize = 4;        // ms: the tag keeps 62 bits of the slice number

__device__ __forceinline__ uint64_t fold_hash(uint64_t k, uint64_t t) { return jm::mix64(k ^ jm::mix64(t)); }
__host__ __device__ __forceinline__ uint64_t fold_tag(int64_t q, uint64_t key) {
    return ((uint64_t)q << 2) | 2ull | (key == 0 ? 1ull : 0ull);
}
__host__ __device__ __forceinline__ int64_t fold_tag_q(uint64_t tag) { return (int64_t)tag >> 2; }

// 1: this call created the entry, 0: it was there, -1: no slot (the host's bound makes that impossible); *slot: where
__device__ __forceinline__ int fold_upsert(unsigned long long* tab, uint64_t smask, uint64_t k, uint64_t t, uint64_t* slot) {
    uint64_t i = fold_hash(k, t) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe, i = (i + 1) & smask) {
        unsigned long long* s = tab + 2 * i;
        const ulonglong2 kt = *reinterpret_cast<const ulonglong2*>(s);
        unsigned long long c = kt.x;
        if (c == 0ull) { c = atomicCAS(s, 0ull, (unsigned long long)k); if (c == 0ull) c = k; }
        if (c != k) continue;
        c = kt.y;
        *slot = i;
        if (c == 0ull) { c = atomicCAS(s + 1, 0ull, (unsigned long long)t); if (c == 0ull) return 1; }
        if (c == t) return 0;
    }
    return -1;
}

// Read-only probe: the slot of (k, t) or -1. It may stop at a slot whose key word is 0: words never change between
// rebuilds, every upsert of an earlier launch ran to its end, and none runs beside the caller.
__device__ __forceinline__ int64_t fold_find(const unsigned long long* tab, uint64_t smask, uint64_t k, uint64_t t) {
    uint64_t i = fold_hash(k, t) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe, i = (i + 1) & smask) {
        const ulonglong2 kt = *reinterpret_cast<const ulonglong2*>(tab + 2 * i);
        if (kt.x == 0ull) return -1;
        if (kt.x == k && kt.y == t) return (int64_t)i;
    }
    return -1;
}

struct FoldPushArgs {
    const int64_t* keys;
    const int64_t* ts;
    const float* val[FWA_MAX_COLS];        // folded column c: its values
    const uint8_t* nul[FWA_MAX_COLS];      // ... and NULL flags (nullptr: none)
    int32_t nc;
    int64_t n;
    int64_t q_min;                         // first slice whose window has not fired at the handle's watermark
    unsigned long long* tab;
    uint64_t smask;                        // slots - 1; the sentinel slot is slots
    float* acc;                            // [nc][slots]
    uint32_t* slot;                        // [n] per record, then sorted
    uint32_t* idx;
    uint32_t* sslot;
    uint32_t* sidx;
    uint32_t* heads;
    unsigned long long* ctr;
};

// One thread per record: its slot number (the sentinel for a record of a fired window) and its own index as the
// sort's value. Entries created are counted with one atomic per wave.
__global__ void __launch_bounds__(256) fold_resolve_kernel(FoldPushArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const uint32_t sentinel = (uint32_t)(a.smask + 1);
    unsigned int created = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = sp_slice(c, assign_ts(c, a.ts[i]));
        uint32_t s = sentinel;
        if (q >= a.q_min) {
            const uint64_t key = (uint64_t)a.keys[i];
            uint64_t slot = 0;
            const int r = fold_upsert(a.tab, a.smask, key ? key : 1ull, fold_tag(q, key), &slot);
            if (r < 0) atomicAdd(a.ctr + 1, 1ull);
            else s = (uint32_t)slot;
            created += r > 0 ? 1u : 0u;
        }
        a.slot[i] = s;
        a.idx[i] = (uint32_t)i;
    }
    for (int o = 32; o > 0; o >>= 1) created += __shfl_down(created, o);    // the whole wave is back here
    if ((threadIdx.x & 63) == 0 && created) atomicAdd(a.ctr + 2, (unsigned long long)created);
}

// The first position of every run of equal slots in the sorted batch (the sentinel's run, sorted last, is none). Every
// lane takes every iteration, so the ballot sees whole waves; one atomic per wave reserves its heads' places.
__global__ void __launch_bounds__(256) fold_heads_kernel(FoldPushArgs a) {
    const uint32_t sentinel = (uint32_t)(a.smask + 1);
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.n; i0 += stride) {   // (uniform per block)
        const int64_t i = i0 + threadIdx.x;
        bool head = false;
        if (i < a.n) {
            const uint32_t s = a.sslot[i];
            head = s != sentinel && (i == 0 || a.sslot[i - 1] != s);
        }
        const unsigned long long b = __ballot(head);
        if (!b) continue;                                  // (wave-uniform)
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(a.ctr + 3, (unsigned long long)__popcll(b));
        base = __shfl(base, 0);
        if (head) a.heads[base + __popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
}

// One lane per run. The run [p, e) of slot s: e by bisection (the slots are sorted), then per folded column the slot's
// accumulator continues over the run's records in their sorted = arrival order. Four indices and four values are in
// flight ahead of the four dependent adds; __fadd_rn is the IEEE add that is neither contracted nor reordered, and the
// build keeps float32 subnormals.
__global__ void __launch_bounds__(256) fold_runs_kernel(FoldPushArgs a) {
    const int64_t nh = (int64_t)a.ctr[3];
    const int64_t slots = (int64_t)a.smask + 1;
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < nh; h += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = a.heads[h];
        const uint32_t s = a.sslot[p];
        int64_t lo = p, hi = a.n;                          // sslot[lo] == s, sslot[hi] > s (or hi == n)
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.sslot[mid] == s) lo = mid; else hi = mid;
        }
        const int64_t e = hi;
        for (int c = 0; c < a.nc; ++c) {
            const float* __restrict__ v = a.val[c];
            const uint8_t* __restrict__ z = a.nul[c];
            float acc = a.acc[(int64_t)c * slots + s];
            int64_t j = p;
            for (; j + 4 <= e; j += 4) {
                const uint32_t i0 = a.sidx[j], i1 = a.sidx[j + 1], i2 = a.sidx[j + 2], i3 = a.sidx[j + 3];
                const float v0 = v[i0], v1 = v[i1], v2 = v[i2], v3 = v[i3];
                const bool z0 = z && z[i0], z1 = z && z[i1], z2 = z && z[i2], z3 = z && z[i3];
                acc = z0 ? acc : __fadd_rn(acc, v0);
                acc = z1 ? acc : __fadd_rn(acc, v1);
                acc = z2 ? acc : __fadd_rn(acc, v2);
                acc = z3 ? acc : __fadd_rn(acc, v3);
            }
            for (; j < e; ++j) {
                const uint32_t i0 = a.sidx[j];
                if (!(z && z[i0])) acc = __fadd_rn(acc, v[i0]);
            }
            a.acc[(int64_t)c * slots + s] = acc;
        }
    }
}

// Entries of windows that have not fired, one atomic per wave.
__global__ void __launch_bounds__(256) fold_count_kernel(const unsigned long long* tab, int64_t slots, int64_t q_min,
                                                        unsigned long long* ctr) {
    unsigned int mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long t = tab[2 * i + 1];
        mine += (t != 0ull && fold_tag_q(t) >= q_min) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(ctr, (unsigned long long)mine);
}

// Rebuild into a new table: the entries of unfired windows re-inserted, their accumulators carried; ctr[0] receives
// the entries created there (the exact live count).
__global__ void __launch_bounds__(256) fold_rebuild_kernel(const unsigned long long* tab, const float* acc, int64_t slots,
                                                          int64_t q_min, int32_t nc, unsigned long long* ntab,
                                                          float* nacc, uint64_t nsmask, unsigned long long* ctr) {
    unsigned int made = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 kt = *reinterpret_cast<const ulonglong2*>(tab + 2 * i);
        if (kt.y == 0ull || fold_tag_q(kt.y) < q_min) continue;
        uint64_t slot = 0;
        const int r = fold_upsert(ntab, nsmask, kt.x, kt.y, &slot);
        if (r <= 0) { atomicAdd(ctr + 1, 1ull); continue; }       // (an entry is in the old table once)
        for (int c = 0; c < nc; ++c) nacc[(int64_t)c * (int64_t)(nsmask + 1) + (int64_t)slot] = acc[(int64_t)c * slots + i];
        made += 1u;
    }
    for (int o = 32; o > 0; o >>= 1) made += __shfl_down(made, o);
    if ((threadIdx.x & 63) == 0 && made) atomicAdd(ctr, (unsigned long long)made);
}

// Restore: entries given as (stored key, tag, column, accumulator bits), w[4][n]; the (key, slice) is upserted (its
// columns arrive as separate entries) and the accumulator set.
__global__ void __launch_bounds__(256) fold_restore_kernel(const unsigned long long* w, int64_t n, unsigned long long* tab,
                                                          float* acc, uint64_t smask, unsigned long long* ctr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t slot = 0;
        const int r = fold_upsert(tab, smask, w[i], w[n + i], &slot);
        if (r < 0) { atomicAdd(ctr + 1, 1ull); continue; }
        acc[(int64_t)w[2 * n + i] * (int64_t)(smask + 1) + (int64_t)slot] = __uint_as_float((unsigned int)w[3 * n + i]);
    }
}

struct FoldRowDesc {
    int32_t col;                           // the folded column of this aggregate
    float* out;                            // its plan-owned result column
    const uint8_t* nul;                    // the aggregate's NULL flags as fired (nullptr: never NULL)
};
struct FoldRowsArgs {
    FoldRowDesc d[FWA_MAX_AGGS];
    const int64_t* o_key;
    const int64_t* o_start;
    int64_t n;
    const unsigned long long* tab;         // nullptr: nothing was ever folded
    const float* acc;
    uint64_t smask;
    int32_t canon_nan;                     // reductions return a NaN canonical
    unsigned long long* ctr;
};

// One thread per (row, folded aggregate): the slice from the row's window start, the entry's float. A NULL row (no
// non-NULL input) may have an entry or none and reads as +0.0f behind its NULL flag either way.
__global__ void __launch_bounds__(256) fold_rows_kernel(FoldRowsArgs f, const EngineConst* __restrict__ cp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.n) return;
    const FoldRowDesc& d = f.d[blockIdx.y];
    const uint64_t key = (uint64_t)f.o_key[i];
    const int64_t q = sp_slice(*cp, f.o_start[i]);
    const int64_t slot = f.tab ? fold_find(f.tab, f.smask, key ? key : 1ull, fold_tag(q, key)) : -1;
    float r = 0.0f;
    if (slot >= 0) r = f.acc[(int64_t)d.col * (int64_t)(f.smask + 1) + slot];
    else if (!(d.nul && d.nul[i])) atomicAdd(f.ctr + 4, 1ull);
    if (f.canon_nan && r != r) r = __uint_as_float(0x7fc00000u);
    d.out[i] = r;
}

// ---- host ----

// The plan of a handle created with FWA_CFG_F32_FOLD: 0 with P->nc == 0 when no SUM_F32 aggregate makes the flag do
// anything, 0 with the folded columns, or FWA_E_UNSUPPORTED with *why naming the flag.
int fold_plan(const fwa_config* u, FoldPlan* P, std::string* why) {
    P->ucfg = *u;
    P->nullable = u->nullable_cols;
    for (int j = 0; j < FWA_MAX_AGGS; ++j) P->col_of[j] = -1;
    if (u->num_aggs < 0 || u->num_aggs > FWA_MAX_AGGS) return FWA_OK;     // (validate refuses it)
    for (int j = 0; j < u->num_aggs; ++j) {
        const fwa_agg_spec& s = u->aggs[j];
        if (s.kind != FWA_SUM_F32) continue;
        if (s.col < 0 || s.col >= FWA_MAX_COLS) return FWA_OK;            // (validate refuses it)
        int c = -1;
        for (int i = 0; i < P->nc; ++i) if (P->src[i] == s.col) c = i;    // aggregates over one column share a fold
        if (c < 0) { c = P->nc++; P->src[c] = s.col; }
        P->col_of[j] = c;
        P->mask |= (int64_t)1 << j;
    }
    if (!P->nc) return FWA_OK;
    auto no = [&](const char* m) { *why = std::string("FWA_CFG_F32_FOLD: ") + m; return FWA_E_UNSUPPORTED; };
    if (u->window_kind == FWA_SLIDE && u->semantics == FWA_SEM_DATASTREAM)
        return no("DataStream SLIDE windows are not supported (the reference folds per window, the engine keeps slices, "
                  "and a window's arrival-order fold is not a function of per-slice folds)");
    if (u->window_kind != FWA_TUMBLE)
        return no("only TUMBLE windows (HOP / CUMULATE / SESSION need the reference's slice and namespace merge order)");
    if (u->allowed_lateness_ms > 0)
        return no("allowed lateness is not supported (a late firing shows the state after each late element)");
    if (u->key_kind == FWA_KEY_PREHASHED)
        return no("PREHASHED keys are not supported (the set keeps no hash per entry to place it in a key group)");
    if (has_distinct(u))
        return no("a handle that also has DISTINCT aggregates is not supported (two plans would stage the same columns)");
    if (u->size_ms > 0 && u->size_ms < kFoldMinSize) return no("windows shorter than 4 ms are not supported");
    return FWA_OK;
}

void fold_free(FoldPlan* P) {
    if (!P) return;
    for (void* p : {(void*)P->d_tab, (void*)P->d_acc, (void*)P->d_rec, (void*)P->d_stage, (void*)P->d_ctr})
        if (p) (void)hipFree(p);
    for (int j = 0; j < FWA_MAX_AGGS; ++j) if (P->d_out[j]) (void)hipFree(P->d_out[j]);
    if (P->h_ctr) (void)hipHostFree(P->h_ctr);
    for (hipEvent_t ev : P->ev) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : P->rev) if (ev) (void)hipEventDestroy(ev);
    delete P;
}

int fold_counters(fwa_engine* e) {
    FoldPlan* P = e->fold;
    if (P->d_ctr) return FWA_OK;
    HIPCHK(e, hipMalloc(&P->d_ctr, 64));
    HIPCHK(e, hipHostMalloc((void**)&P->h_ctr, 64));
    memset(P->h_ctr, 0, 64);
    HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 64, e->stream));
    for (hipEvent_t& ev : P->ev) HIPCHK(e, hipEventCreate(&ev));
    for (hipEvent_t& ev : P->rev) HIPCHK(e, hipEventCreate(&ev));
    return FWA_OK;
}

// Read ctr[0] (and check ctr[1]) after the work enqueued so far; synchronises.
int fold_read_counter(fwa_engine* e, int64_t* out) {
    FoldPlan* P = e->fold;
    HIPCHK(e, hipMemcpyAsync(P->h_ctr, P->d_ctr, 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (P->h_ctr[1]) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the set overflowed its bound");
    *out = (int64_t)P->h_ctr[0];
    return FWA_OK;
}

int fold_alloc(fwa_engine* e, int64_t slots, int32_t nc, unsigned long long** tab, float** acc) {
    *tab = nullptr;
    *acc = nullptr;
    HIPCHK(e, hipMalloc(tab, 16 * (size_t)slots));
    hipError_t r = hipMalloc(acc, 4 * (size_t)nc * (size_t)slots);
    if (r == hipSuccess) r = hipMemsetAsync(*tab, 0, 16 * (size_t)slots, e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(*acc, 0, 4 * (size_t)nc * (size_t)slots, e->stream);   // +0.0f
    if (r != hipSuccess) {
        (void)hipFree(*tab);
        if (*acc) (void)hipFree(*acc);
        *tab = nullptr;
        *acc = nullptr;
        HIPCHK(e, r);
    }
    return FWA_OK;
}

// Make room for `add` more upserts: bound + add <= slots / 2, rebuilding the set from its live entries otherwise
// (always into a new allocation: the accumulators move with their entries, and the old table is freed behind it).
int fold_reserve(fwa_engine* e, int64_t add) {
    FoldPlan* P = e->fold;
    if (int rc = fold_counters(e)) return rc;
    if (!P->d_tab) {
        const int64_t slots = P->first_slots > 0 ? P->first_slots : dist_pow2(std::max<int64_t>(2 * add, kFoldMinSlots));
        if (slots > ((int64_t)1 << 31)) return fail(e, FWA_E_OOM, "FWA_CFG_F32_FOLD: the set would exceed 2^31 slots");
        if (int rc = fold_alloc(e, slots, P->nc, &P->d_tab, &P->d_acc)) return rc;
        P->slots = slots;
        P->bound = 0;
    }
    if (P->last_add) {   // the last pass's exact count (its copy was enqueued behind it) replaces its estimate
        HIPCHK(e, hipEventSynchronize(P->ev[4]));
        if (P->h_ctr[1]) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the set overflowed its bound");
        const int64_t made = (int64_t)P->h_ctr[2];
        if (made >= 0 && made <= P->last_add) P->bound -= P->last_add - made;
        P->last_add = 0;
    }
    if (P->bound + add <= P->slots / 2) { P->bound += add; return FWA_OK; }
    const int64_t q_min = dist_qmin(e);
    const int grid = grid_for(P->slots, 4096);
    int64_t livee = 0;
    HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 16, e->stream));
    fold_count_kernel<<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, P->d_ctr);
    HIPCHK(e, hipGetLastError());
    if (int rc = fold_read_counter(e, &livee)) return rc;
    const int64_t nslots = dist_pow2(std::max<int64_t>(2 * (livee + add), 64));
    if (nslots > ((int64_t)1 << 31)) return fail(e, FWA_E_OOM, "FWA_CFG_F32_FOLD: the set would exceed 2^31 slots");
    unsigned long long* ntab = nullptr;
    float* nacc = nullptr;
    if (int rc = fold_alloc(e, nslots, P->nc, &ntab, &nacc)) return rc;
    hipError_t r = hipMemsetAsync(P->d_ctr, 0, 16, e->stream);
    if (r == hipSuccess) {
        fold_rebuild_kernel<<<grid, 256, 0, e->stream>>>(P->d_tab, P->d_acc, P->slots, q_min, P->nc, ntab, nacc,
                                                         (uint64_t)nslots - 1, P->d_ctr);
        r = hipGetLastError();
    }
    int64_t moved = 0;
    int rc = r == hipSuccess ? fold_read_counter(e, &moved) : fail(e, FWA_E_DEVICE, hipGetErrorString(r));
    if (rc || moved != livee) {
        (void)hipFree(ntab);
        (void)hipFree(nacc);
        return rc ? rc : fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the rebuild lost entries");
    }
    HIPCHK(e, hipFree(P->d_tab));
    HIPCHK(e, hipFree(P->d_acc));
    P->d_tab = ntab;
    P->d_acc = nacc;
    P->slots = nslots;
    P->live = moved;
    P->bound = moved + add;
    P->rebuilds++;
    return FWA_OK;
}

// The pass's device time, once its events completed, goes to ingest_ms (like the marking pass of COUNT(DISTINCT)).
void fold_collect_timing(fwa_engine* e) {
    FoldPlan* P = e->fold;
    if (!P || !P->timing || hipEventQuery(P->ev[3]) != hipSuccess) return;
    float ms[3] = {0.f, 0.f, 0.f};
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && hipEventElapsedTime(&ms[k], P->ev[k], P->ev[k + 1]) == hipSuccess;
    if (ok) {
        P->resolve_ms += ms[0];
        P->sort_ms += ms[1];
        P->fold_ms += ms[2];
        e->ingest_ms += ms[0] + ms[1] + ms[2];
    }
    P->timing = false;
}

// The fold pass of one push. On return *keys / *ts, vals[] and nulls[] are device pointers (host inputs are staged
// once, here, every input column of the caller's configuration), laid out as the caller passed them.
int fold_pass(fwa_engine* e, const int64_t** keys, const int64_t** ts, const void* const* val_cols,
              const uint8_t* const* null_cols, int64_t n, bool device, const void** vals, const uint8_t** nulls) {
    FoldPlan* P = e->fold;
    const fwa_config& u = P->ucfg;
    fold_collect_timing(e);
    for (int c = 0; c < FWA_MAX_COLS; ++c) { vals[c] = nullptr; nulls[c] = nullptr; }
    size_t width[FWA_MAX_COLS] = {};
    for (int j = 0; j < u.num_aggs; ++j) {
        const fwa_agg_spec& s = u.aggs[j];
        if (s.kind == FWA_COUNT || s.kind == FWA_COUNT_COL) continue;
        if (!val_cols || !val_cols[s.col]) return fail(e, FWA_E_ARG, "missing value column");
        vals[s.col] = val_cols[s.col];
        width[s.col] = std::max(width[s.col], dist_in_width(s.kind));
    }
    for (int c = 0; c < FWA_MAX_COLS; ++c) if (null_cols && ((u.nullable_cols >> c) & 1)) nulls[c] = null_cols[c];
    if (!device) {
        size_t need = 2 * ((((size_t)n * 8) + 255) & ~(size_t)255);
        for (int c = 0; c < FWA_MAX_COLS; ++c) {
            if (vals[c]) need += ((size_t)n * width[c] + 255) & ~(size_t)255;
            if (nulls[c]) need += ((size_t)n + 255) & ~(size_t)255;
        }
        if (need > P->stage_bytes) {
            if (P->d_stage) HIPCHK(e, hipFree(P->d_stage));
            P->d_stage = nullptr;
            P->stage_bytes = 0;
            HIPCHK(e, hipMalloc(&P->d_stage, need));
            P->stage_bytes = need;
        }
        char* p = P->d_stage;
        hipError_t err = hipSuccess;
        auto put = [&](const void* src, size_t bytes) -> const void* {
            void* dst = p;
            const hipError_t r = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream);
            if (r != hipSuccess) err = r;
            p += (bytes + 255) & ~(size_t)255;
            return dst;
        };
        *keys = (const int64_t*)put(*keys, (size_t)n * 8);
        *ts = (const int64_t*)put(*ts, (size_t)n * 8);
        for (int c = 0; c < FWA_MAX_COLS; ++c) {
            if (vals[c]) vals[c] = put(vals[c], (size_t)n * width[c]);
            if (nulls[c]) nulls[c] = (const uint8_t*)put(nulls[c], (size_t)n);
        }
        HIPCHK(e, err);
    }
    if (n > P->rec_cap) {
        if (P->d_rec) HIPCHK(e, hipFree(P->d_rec));
        P->d_rec = nullptr;
        P->rec_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 1 << 16);
        HIPCHK(e, hipMalloc(&P->d_rec, sizeof(uint32_t) * 5 * (size_t)cap));
        P->rec_cap = cap;
    }
    if (int rc = fold_reserve(e, n)) return rc;
    FoldPushArgs a;
    memset(&a, 0, sizeof(a));
    a.keys = *keys;
    a.ts = *ts;
    a.nc = P->nc;
    a.n = n;
    a.q_min = dist_qmin(e);
    a.tab = P->d_tab;
    a.smask = (uint64_t)P->slots - 1;
    a.acc = P->d_acc;
    a.slot = P->d_rec;
    a.idx = P->d_rec + (size_t)P->rec_cap;
    a.sslot = P->d_rec + 2 * (size_t)P->rec_cap;
    a.sidx = P->d_rec + 3 * (size_t)P->rec_cap;
    a.heads = P->d_rec + 4 * (size_t)P->rec_cap;
    a.ctr = P->d_ctr;
    for (int c = 0; c < P->nc; ++c) {
        a.val[c] = (const float*)vals[P->src[c]];
        a.nul[c] = nulls[P->src[c]];
    }
    int bits = 1;                                          // the slot numbers and the sentinel `slots`
    while (((int64_t)1 << bits) <= P->slots) ++bits;
    size_t tmp = 0;
    HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, a.slot, a.sslot, a.idx, a.sidx, (int)n, 0, bits, e->stream));
    if (int rc = ensure_sort_tmp(e, tmp)) return rc;
    tmp = e->sort_tmp_bytes;
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 1, 0, 24, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[0], e->stream));
    fold_resolve_kernel<<<grid_for(n, 1 << 16), 256, 0, e->stream>>>(a, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->ev[1], e->stream));
    // a radix sort is stable: records of one slot stay in batch = arrival order, which is what the fold is defined over
    HIPCHK(e, hipcub::DeviceRadixSort::SortPairs(e->d_sort_tmp, tmp, a.slot, a.sslot, a.idx, a.sidx, (int)n, 0, bits, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[2], e->stream));
    fold_heads_kernel<<<grid_for(n, 1 << 12), 256, 0, e->stream>>>(a);
    HIPCHK(e, hipGetLastError());
    fold_runs_kernel<<<grid_for(n, 1 << 14), 256, 0, e->stream>>>(a);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->ev[3], e->stream));
    P->timing = true;
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 1, P->d_ctr + 1, 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[4], e->stream));
    P->last_add = n;
    return FWA_OK;
}

// The folded results of the nrows fired rows into P->d_out (fill_out substitutes them). On the handle's stream behind
// the fire, inside the watermark call: no push can have rebuilt the set. Synchronises.
int fold_rows(fwa_engine* e, int64_t nrows) {
    FoldPlan* P = e->fold;
    if (int rc = fold_counters(e)) return rc;
    if (nrows > P->out_cap || !P->out_cap) {
        const int64_t cap = std::max<int64_t>(nrows + nrows / 4, 1 << 12);
        for (int j = 0; j < P->ucfg.num_aggs; ++j) {
            if (P->col_of[j] < 0) continue;
            if (P->d_out[j]) HIPCHK(e, hipFree(P->d_out[j]));
            P->d_out[j] = nullptr;
            HIPCHK(e, hipMalloc(&P->d_out[j], 4 * (size_t)cap));
        }
        P->out_cap = cap;
    }
    if (nrows == 0) return FWA_OK;
    FoldRowsArgs f;
    memset(&f, 0, sizeof(f));
    int na = 0;
    for (int j = 0; j < P->ucfg.num_aggs; ++j) {
        if (P->col_of[j] < 0) continue;
        const int ij = e->dec ? e->dec->umap[j] : j;       // (a DECIMAL plan renumbers the internal aggregates)
        if (ij < 0) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: a folded aggregate has no output column");
        f.d[na].col = P->col_of[j];
        f.d[na].out = P->d_out[j];
        f.d[na].nul = e->o_null[ij];
        ++na;
    }
    f.o_key = e->o_key;
    f.o_start = e->o_start;
    f.n = nrows;
    f.tab = P->d_tab;
    f.acc = P->d_acc;
    f.smask = (uint64_t)P->slots - 1;
    f.canon_nan = e->red ? 1 : 0;
    f.ctr = P->d_ctr;
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 4, 0, 8, e->stream));
    HIPCHK(e, hipEventRecord(P->rev[0], e->stream));
    fold_rows_kernel<<<dim3((unsigned)((nrows + 255) / 256), (unsigned)na), 256, 0, e->stream>>>(f, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->rev[1], e->stream));
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 4, P->d_ctr + 4, 8, hipMemcpyDeviceToHost, e->stream));
    if (int rc = stream_sync(e)) return rc;
    if (P->h_ctr[1]) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the set overflowed its bound");
    if (P->h_ctr[4]) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: a fired row with a non-NULL SUM_F32 has no fold entry");
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, P->rev[0], P->rev[1]));
    P->rows_ms += ms;
    e->fire_ms += ms;
    return FWA_OK;
}

// ---- engine snapshot / restore: the set's live entries as a section behind everything else in the FWASNAP1 blob ----
// off[max_parallelism + 1], then key[m], slice_start[m], column[m] (the folded column's ordinal: the SUM_F32 source
// columns in first-use order), acc_bits[m] (the float's 32 bits, zero-extended), bucketed by key group like the body.
int fold_snapshot_section(fwa_engine* e, std::vector<int64_t>* sec, int64_t* m_out) {
    FoldPlan* P = e->fold;
    const int maxp = e->cfg.max_parallelism;
    std::vector<unsigned long long> tab;
    std::vector<uint32_t> acc;
    std::vector<int64_t> lv;                              // the live slots
    if (P->d_tab) {
        HIPCHK(e, hipStreamSynchronize(e->stream));
        if (P->h_ctr && P->h_ctr[1]) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the set overflowed its bound");
        tab.resize(2 * (size_t)P->slots);
        acc.resize((size_t)P->nc * (size_t)P->slots);
        HIPCHK(e, hipMemcpy(tab.data(), P->d_tab, 16 * (size_t)P->slots, hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(acc.data(), P->d_acc, 4 * acc.size(), hipMemcpyDeviceToHost));
        const int64_t q_min = dist_qmin(e);
        for (int64_t i = 0; i < P->slots; ++i)
            if (tab[2 * i + 1] != 0ull && fold_tag_q(tab[2 * i + 1]) >= q_min) lv.push_back(i);
    }
    const int64_t m = (int64_t)lv.size() * P->nc;
    std::vector<int32_t> kg(lv.size());
    std::vector<int64_t> off((size_t)maxp + 1, 0);
    for (size_t i = 0; i < lv.size(); ++i) {
        const uint64_t t = tab[2 * lv[i] + 1];
        const int64_t key = (t & 1) ? 0 : (int64_t)tab[2 * lv[i]];
        kg[i] = jm::key_group_of(key, e->cfg.key_kind, 0, maxp);
        if (kg[i] < 0) return fail(e, FWA_E_INTERNAL, "FWA_CFG_F32_FOLD: the set holds a key outside every key group");
        off[kg[i] + 1] += P->nc;
    }
    for (int g = 0; g < maxp; ++g) off[g + 1] += off[g];
    sec->assign((size_t)maxp + 1 + 4 * (size_t)m, 0);
    memcpy(sec->data(), off.data(), 8 * ((size_t)maxp + 1));
    int64_t* body = sec->data() + maxp + 1;
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (size_t i = 0; i < lv.size(); ++i) {
        const uint64_t t = tab[2 * lv[i] + 1];
        for (int c = 0; c < P->nc; ++c) {
            const int64_t d = cur[kg[i]]++;
            body[d] = (t & 1) ? 0 : (int64_t)tab[2 * lv[i]];
            body[m + d] = slice_start(e, fold_tag_q(t));
            body[2 * m + d] = c;
            body[3 * m + d] = (int64_t)acc[(size_t)c * (size_t)P->slots + (size_t)lv[i]];
        }
    }
    *m_out = m;
    return FWA_OK;
}

// Insert the entries of this handle's key groups from one blob's section, with their accumulators.
int fold_restore_section(fwa_engine* e, const int64_t* sec, int64_t m) {
    FoldPlan* P = e->fold;
    const int maxp = e->cfg.max_parallelism;
    const int64_t lo = sec[e->cfg.kg_start], hi = sec[e->cfg.kg_end + 1];
    if (lo < 0 || hi < lo || hi > m) return fail(e, FWA_E_ARG, "corrupt FWA_CFG_F32_FOLD key-group offsets");
    const int64_t n = hi - lo;
    if (n == 0) return FWA_OK;
    const int64_t* body = sec + maxp + 1;
    std::vector<unsigned long long> w(4 * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = (uint64_t)body[lo + i];
        const int64_t c = body[2 * m + lo + i];
        if (c < 0 || c >= P->nc) return fail(e, FWA_E_ARG, "corrupt FWA_CFG_F32_FOLD entry");
        w[i] = key ? key : 1ull;
        w[n + i] = fold_tag(slice_q(e, body[m + lo + i]), key);
        w[2 * n + i] = (unsigned long long)c;
        w[3 * n + i] = (unsigned long long)body[3 * m + lo + i] & 0xffffffffull;
    }
    if (int rc = fold_reserve(e, n)) return rc;
    unsigned long long* dw = nullptr;
    HIPCHK(e, hipMalloc(&dw, 32 * (size_t)n));
    hipError_t r = hipMemcpyAsync(dw, w.data(), 32 * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) {
        fold_restore_kernel<<<grid_for(n), 256, 0, e->stream>>>(dw, n, P->d_tab, P->d_acc, (uint64_t)P->slots - 1, P->d_ctr);
        r = hipGetLastError();
    }
    const hipError_t rs = hipStreamSynchronize(e->stream);
    (void)hipFree(dw);
    if (r != hipSuccess || rs != hipSuccess) return fail(e, FWA_E_DEVICE, "FWA_CFG_F32_FOLD restore failed");
    return FWA_OK;
}

}  // namespace
