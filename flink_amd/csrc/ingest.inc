// Ingest kernels (Phase P partition3, Phase A combine3, v1 ingest) and the device definitions they share;
// included by engine.hip inside its anonymous namespace, and by tools/regprobe.hip (register / spill report of the
// hot kernels without compiling the whole engine).

// Per-phase clock64 profile of partition3 / combine3 (FWA_OPT_PROFILE): compiled in only with -DFWA_KPROF. Its
// accumulators cost the hot kernels registers they do not have (VGPR spills, DESIGN.md section 4 "Skewed keys").
#ifdef FWA_KPROF
#define KPROF(p) ((p) != nullptr)
#else
#define KPROF(p) false
#endif

constexpr int kBlock = 256;
constexpr uint64_t kEmptyKey = 0x8000000000000000ull;  // key-table sentinel (INT64_MIN); that key uses a side slot
constexpr int kBucket = 8;                              // key-table probe bucket: 8 slots = 64 B
constexpr int32_t kWantCap = 1 << 14;                   // distinct missing slices reported per launch

// ------------------------------------------------------------------------------------------------
// device-side structures

struct DirEntry {               // slice directory entry (32 B), read-only during a launch
    int64_t q;                  // slice number
    int32_t slot;               // accumulator slot, -1: not allocated
    int32_t flags;              // bit0 occupied, bit1 always accepted (last window end == LONG_MAX)
    int64_t thr;                // a record is accepted iff wm < thr (or bit1)
    int64_t first_maxts;        // maxTimestamp of the earliest window containing the slice
};

struct DevStatus {
    int32_t error;              // first fwa_status error code raised by a kernel (0 = none)
    int32_t spill_n;            // records whose slice had no slot (replayed)
    int32_t want_n;             // distinct slice numbers in want[]
    int32_t key_full;
    unsigned long long dropped;
    unsigned long long n_keys;  // distinct keys in the key table (incl. side slot)
    unsigned long long late_fire;
    unsigned long long rows;    // fire kernel output counter
    unsigned long long max_q;   // ord-encoded max / min slice number accepted this push
    unsigned long long min_q;
    int32_t pad;                // host-side scratch (straggler count copy)
    int32_t pad2;
    unsigned long long sess_live;  // sessions: in-flight sessions (rows a fire can emit at most)
    unsigned long long drop_n;     // FWA_CFG_LATE_INDICES: entries in the dropped-record index list this push
    int32_t ovf_n;                 // Phase P: bucket entries past their sub-bucket's end this push (skew signal)
    int32_t strag_n;               // Phase A: entries older than their combiner's LDS window this push
    int32_t wide_n;                // Phase P narrow entries: accepted records whose key or value needs 64 bits (replayed)
    int32_t pad3;
};

// FWA_CFG_LATE_INDICES: record index of a late-dropped record (lateDataOutputTag / lateRecordsDroppedRate),
// appended with one reservation per wave; list capacity = the push's record count.
__device__ __forceinline__ void note_drop(int32_t* list, DevStatus* st, bool drop, int64_t i) {
    if (!list) return;
    const unsigned long long m = __ballot(drop);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    const int ld = __ffsll((long long)m) - 1;
    unsigned long long b = 0;
    if (lane == ld) b = atomicAdd(&st->drop_n, (unsigned long long)__popcll(m));
    b = __shfl(b, ld);
    if (drop) list[b + __popcll(m & ((1ull << lane) - 1))] = (int32_t)i;
}

// ACC_PAYLOAD: raw field bits of one selected element (FWA_FIRST_* / FWA_SEL_*, reduce.inc); not updated by the ingest
enum AccKind : int32_t { ACC_NONE = 0, ACC_ADD_I64 = 1, ACC_ADD_F64 = 2, ACC_MIN_ORD = 3, ACC_MAX_ORD = 4, ACC_PAYLOAD = 5 };

struct AggDesc {
    int32_t kind;               // fwa_agg_kind
    int32_t col;                // input column
    int32_t acc;                // accumulator column (>=1) or 0 for COUNT
    int32_t acc_kind;
    int32_t vslot;              // partitioned path: which carried value column feeds this aggregate
    int32_t alias;              // 1: shares the accumulator column of an earlier aggregate (e.g. SUM(d) and
                                // AVG(d) keep one double sum): read at fire, never updated through it
    int32_t nn;                 // accumulator column counting the non-NULL inputs of a nullable column (0: none)
    int32_t jcmp;               // FWA_CFG_REDUCE: Java compareTo order for a float MIN / MAX (NaN canonical, greatest)
};
constexpr int kMaxAggsInt = FWA_MAX_AGGS + FWA_MAX_COLS;   // user aggregates + hidden non-NULL counters

struct EngineConst {
    jm::UDiv64 g_div;           // slice size
    int64_t g, off;
    int32_t sem, lateness_pos;  // lateness_pos: DataStream allowed lateness > 0
    int32_t key_kind, max_par, kg_lo, kg_hi;
    int32_t naggs, nacc;        // naggs: user + hidden aggregates; nacc = 1 (count) + stateful agg columns
    int32_t nout, nullable;     // nout: user aggregates (output columns); nullable: fwa_config.nullable_cols
    AggDesc agg[kMaxAggsInt];
    int32_t acc_kind[1 + kMaxAggsInt];
    const int64_t* tz;          // shift time zone table (device copy of fwa_config.tz), tz_n pairs
    int32_t tz_n, pad_tz;
    // FWA_CFG_REDUCE (reduce.inc): red = 1; red_by = the MINBY / MAXBY aggregate (-1: the first element is selected);
    // red_max: it is a MAXBY; red_last: ties select the last element; red_selq / red_selk: accumulator columns of the
    // selected element's arrival sequence and of the by-value it was selected at
    int32_t red, red_by, red_max, red_last, red_selq, red_selk;
    int32_t red_scr, pad_scr;   // MINBY / MAXBY: this push's first (last) arrival at the slot's best value (reduce.inc)
    // accumulator columns the two-phase combiner merges: 0 .. nacc_comb - 1 (all of them, except a reduce handle's
    // selected-element columns -- payload fields, SELQ, SELK -- which come after and only the selection passes write)
    int32_t nacc_comb;
    // red_iota: a first- / last-element reduction selecting through an ordinary MIN / MAX accumulator (red_scr) over
    // the engine's 4-byte record-index column kIotaCol; the payload pass moves it into SELQ (reduce.inc)
    int32_t red_iota;
};
constexpr int kIotaCol = FWA_MAX_COLS - 1;

// Slice-assignment timestamp: the record's local wall-clock time under a Table shift time zone
// (AbstractSliceAssigner.assignSliceEnd -> TimeWindowUtil.toUtcTimestampMills), else the timestamp.
__device__ __forceinline__ int64_t assign_ts(const EngineConst& c, int64_t ts) {
    return c.tz_n ? jm::tz_to_local(c.tz, c.tz_n, ts) : ts;
}

struct IngestArgs {
    const int64_t* keys;
    const int64_t* ts;
    const void* cols[FWA_MAX_AGGS + FWA_MAX_COLS];   // value columns; partials: aggregate j's accumulator column
                                                     // (hidden non-NULL counters after the user aggregates)
    const int32_t* key_hash;
    const int32_t* idx;         // optional index list (miss replay)
    const unsigned long long* pcount;  // partial accumulators (fwa_push_partials): COUNT per row; cols[j] = acc of agg j
    int64_t n;
    int64_t wm;
    unsigned long long* key_table;
    uint64_t key_mask;          // capacity-1 (power of two); side slot at capacity
    int32_t seg_log, part_bits; // key-table segmentation (see key_slot)
    const DirEntry* dir;
    uint32_t dir_mask;
    unsigned long long* want;   // open-addressing set of ord(q), kWantCap entries, 0 = empty
    int32_t* spill;
    int32_t* late;              // DataStream late firings (window fired, within allowed lateness): deferred
    int32_t* touched;           // per slot: 0 untouched, else the epoch of the last push that touched it
    int32_t epoch;              // this push's epoch (>= 1)
    unsigned long long* const* slot_base;
    int64_t stride;             // elements per accumulator column
    int64_t spill_cap;          // entries of spill[] and late[] (a store past it raises FWA_E_STATE instead)
    int32_t* dropidx;           // FWA_CFG_LATE_INDICES: dropped-record indices (nullptr: not collected)
    const uint8_t* nulls[FWA_MAX_COLS];   // SQL NULL flags per value column (nullptr: no NULLs)
    DevStatus* st;
};

__device__ __forceinline__ void raise_error(DevStatus* st, int code) { atomicCAS(&st->error, 0, code); }

// Bounds-checked scatter of a record index into a spill / late list: an index past the list's capacity
// would be a logic error upstream; it is reported (FWA_E_STATE) instead of faulting the device.
__device__ __forceinline__ void put_idx(int32_t* list, int64_t pos, int64_t cap, int32_t v, DevStatus* st) {
    if (pos >= 0 && pos < cap) list[pos] = v;
    else raise_error(st, FWA_E_STATE);
}

// Key table: SEGMENTED open addressing. h = mix64(key); segment p = top part_bits of h (the v2
// combiner's partition), probe linearly inside the segment from the kBucket-aligned home
// (h & (SEG-1)) & ~(kBucket-1); CAS insert. The aligned home lets the combiner read a key's whole
// home bucket (64 B) with one LDS round instead of walking the probe sequence slot by slot: linear
// probing's displacement tail (~20 slots at load 0.5 over a 4096-slot segment) made a wave's probe
// loop run for the worst of its 256 records (r01 clock64 profile: 75 % of combine time).
// A stale EMPTY read only sends us to the CAS, which returns the winner's key: no hand-off needed.
__device__ __forceinline__ uint64_t seg_base(uint64_t h, int seg_log, int part_bits) {
    return part_bits ? ((h >> (64 - part_bits)) << seg_log) : 0ull;
}
__device__ __forceinline__ int64_t key_slot(unsigned long long* table, uint64_t mask, int seg_log, int part_bits,
                                            int64_t key, DevStatus* st) {
    if ((uint64_t)key == kEmptyKey) {
        const unsigned long long side = mask + 1;
        if (table[side] != 1ull && atomicCAS(&table[side], 0ull, 1ull) == 0ull) atomicAdd(&st->n_keys, 1ull);
        return (int64_t)side;
    }
    const uint64_t h = jm::mix64((uint64_t)key);
    const uint64_t base = seg_base(h, seg_log, part_bits);
    const uint64_t smask = ((uint64_t)1 << seg_log) - 1;
    const uint64_t home = h & smask & ~(uint64_t)(kBucket - 1);   // probing starts at a bucket boundary
    for (uint64_t probe = 0; probe <= smask; ++probe) {
        const uint64_t i = base | ((home + probe) & smask);
        const unsigned long long cur = table[i];
        if (cur == (unsigned long long)key) return (int64_t)i;
        if (cur == kEmptyKey) {
            const unsigned long long old = atomicCAS(&table[i], kEmptyKey, (unsigned long long)key);
            if (old == kEmptyKey) {
                atomicAdd(&st->n_keys, 1ull);
                return (int64_t)i;
            }
            if (old == (unsigned long long)key) return (int64_t)i;
        }
    }
    return -1;
}

__device__ __forceinline__ const DirEntry* dir_find(const DirEntry* dir, uint32_t mask, int64_t q) {
    uint32_t i = (uint32_t)jm::mix64((uint64_t)q) & mask;
    for (uint32_t probe = 0; probe <= mask; ++probe) {
        const DirEntry* e = &dir[i];
        if (!(e->flags & 1)) return nullptr;
        if (e->q == q) return e;
        i = (i + 1) & mask;
    }
    return nullptr;
}

__device__ __forceinline__ void want_insert(unsigned long long* want, DevStatus* st, int64_t q) {
    const unsigned long long key = jm::ord_i64(q) + 1ull;  // never 0: |q| <= 2^63/g < LONG_MAX for g >= 2
    uint32_t i = (uint32_t)jm::mix64((uint64_t)q) & (kWantCap - 1);
    for (int probe = 0; probe < kWantCap; ++probe) {
        unsigned long long cur = want[i];
        if (cur == key) return;
        if (cur == 0ull) {
            unsigned long long old = atomicCAS(&want[i], 0ull, key);
            if (old == 0ull) { atomicAdd(&st->want_n, 1); return; }
            if (old == key) return;
        }
        i = (i + 1) & (kWantCap - 1);
    }
    raise_error(st, FWA_E_OOM);
}

__device__ __forceinline__ bool is_i32_kind(int kind) {
    return kind == FWA_SUM_I32 || kind == FWA_MIN_I32 || kind == FWA_MAX_I32 || kind == FWA_MINBY_I32 || kind == FWA_MAXBY_I32;
}
__device__ __forceinline__ bool is_f32_kind(int kind) {
    return kind == FWA_MIN_F32 || kind == FWA_MAX_F32 || kind == FWA_MINBY_F32 || kind == FWA_MAXBY_F32;
}
__device__ __forceinline__ bool is_i64_ord_kind(int kind) {
    return kind == FWA_MIN_I64 || kind == FWA_MAX_I64 || kind == FWA_MINBY_I64 || kind == FWA_MAXBY_I64;
}
// Order-preserving u64 key of a MIN / MAX / MINBY / MAXBY input. jcmp (reduce handles): Double.compare / Float.compare
// order, every NaN is the canonical one (doubleToLongBits), above +Inf; -0.0 < 0.0 holds for the bit order anyway.
__device__ __forceinline__ uint64_t load_ord(const void* col, int64_t i, int kind, int jcmp = 0) {
    if (is_i64_ord_kind(kind)) return jm::ord_i64(((const int64_t*)col)[i]);
    if (is_i32_kind(kind)) return jm::ord_i64((int64_t)((const int32_t*)col)[i]);
    double v = is_f32_kind(kind) ? (double)((const float*)col)[i] : ((const double*)col)[i];
    uint64_t b = (uint64_t)__double_as_longlong(v);
    if (jcmp && v != v) b = 0x7ff8000000000000ull;
    return jm::ord_bits64(b);
}

// One input value in its accumulator domain (i64 bits, f64 bits, or ordered key). A SQL NULL input (nul[i])
// contributes the accumulator's identity; a hidden non-NULL counter (COUNT_COL) contributes 1 or 0.
__device__ __forceinline__ unsigned long long acc_input(const AggDesc& d, const void* col, int64_t i,
                                                        const uint8_t* nul = nullptr) {
    if (d.acc_kind == ACC_PAYLOAD) return 0ull;       // written by the reduce selection (reduce.inc)
    const bool isnull = nul && nul[i];
    if (d.kind == FWA_COUNT_COL) return isnull ? 0ull : 1ull;
    if (isnull) return d.acc_kind == ACC_MIN_ORD ? ~0ull : 0ull;
    switch (d.acc_kind) {
        case ACC_ADD_I64:                             // Integer SUM: sign-extended, the fire keeps the low 32 bits
            return d.kind == FWA_SUM_I32 ? (unsigned long long)(int64_t)((const int32_t*)col)[i]
                                         : ((const unsigned long long*)col)[i];
        case ACC_ADD_F64: {
            const double v = (d.kind == FWA_SUM_F32 || d.kind == FWA_AVG_F32) ? (double)((const float*)col)[i]
                                                                               : ((const double*)col)[i];
            return (unsigned long long)__double_as_longlong(v);
        }
        default: return load_ord(col, i, d.kind, d.jcmp);
    }
}

template <bool kIdx>
__global__ void __launch_bounds__(kBlock) ingest_kernel(IngestArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    const int lane = threadIdx.x & 63;
    __shared__ unsigned long long s_red[kBlock / 64][1 + kMaxAggsInt];   // hot-key group reduction
    const int64_t stride_grid = (int64_t)gridDim.x * blockDim.x;
    unsigned long long qmax = 0, qmin = ~0ull;
    unsigned long long dropped = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.n; t += stride_grid) {
        const int64_t i = kIdx ? (int64_t)a.idx[t] : t;
        const int64_t key = a.keys[i];
        const int64_t ts = a.ts[i];
        // key-group ownership (StateTable.getMapForKeyGroup :300-307)
        const int32_t kg = jm::key_group_of(key, c.key_kind, a.key_hash ? a.key_hash[i] : 0, c.max_par);
        if (kg < c.kg_lo || kg > c.kg_hi) { raise_error(a.st, FWA_E_KEYGROUP); continue; }
        if (c.sem == FWA_SEM_DATASTREAM && ts == LONG_MIN_J) { raise_error(a.st, FWA_E_TS_MIN); continue; }
        // slice number q = floor((ts - off) / g), Java wrap arithmetic (TimeWindow.java:264-272)
        const int64_t d = jm::wsub(a.pcount ? ts : assign_ts(c, ts), c.off);   // partial rows: slice start, already local
        const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
        const uint64_t uq = jm::udiv64(ud, c.g_div);
        int64_t q;
        if (d >= 0) q = (int64_t)uq;
        else q = (uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1;
        const DirEntry* e = dir_find(a.dir, a.dir_mask, q);
        if (e == nullptr) {                                     // slice unknown to the host: replay
            want_insert(a.want, a.st, q);
            const unsigned long long m = __ballot(1);
            const int leader = __ffsll((long long)m) - 1;
            int32_t base = 0;
            if (lane == leader) base = atomicAdd(&a.st->spill_n, __popcll(m));
            base = __shfl(base, leader);
            put_idx(a.spill, base + __popcll(m & ((1ull << lane) - 1)), a.spill_cap, (int32_t)i, a.st);
            continue;
        }
        const unsigned long long cadd = a.pcount ? a.pcount[i] : 1ull;   // records this row stands for
        const bool accepted = (e->flags & 2) || a.wm < e->thr;
        if (!accepted) { dropped += cadd; if (a.dropidx && !a.pcount) a.dropidx[atomicAdd(&a.st->drop_n, 1ull)] = (int32_t)i; continue; }
        if (e->slot < 0) {                                      // known slice without slot: replay
            want_insert(a.want, a.st, q);
            const int32_t si = atomicAdd(&a.st->spill_n, 1);
            put_idx(a.spill, si, a.spill_cap, (int32_t)i, a.st);
            continue;
        }
        if (c.lateness_pos && a.wm >= e->first_maxts) {        // some window of the slice fired already:
            const unsigned long long li = atomicAdd(&a.st->late_fire, 1ull);   // EventTimeTrigger.onElement
            put_idx(a.late, (int64_t)li, a.spill_cap, (int32_t)i, a.st);        // FIRE -> late_fire_kernel
            continue;
        }
        const uint64_t oq = jm::ord_i64(q);
        qmax = oq > qmax ? oq : qmax;
        qmin = oq < qmin ? oq : qmin;
        const int64_t kid = key_slot(a.key_table, a.key_mask, a.seg_log, a.part_bits, key, a.st);
        if (kid < 0) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); continue; }
        const int32_t slot = e->slot;
        unsigned long long* base = a.slot_base[slot];
        if (a.touched[slot] != a.epoch) a.touched[slot] = a.epoch;
        // Hot keys (skew: e.g. the bucket-overflow replay of a Zipf head key, where most lanes of a wave
        // carry the same key): the lanes sharing the wave leader's (kid, slot) combine in LDS first, so
        // the group costs one set of global atomics instead of one per lane on the same address.
        // Replay launches only (kIdx): the plain v1 pass over a large uniform key space (C4) is
        // latency-bound and lost half its rate to the extra registers.
        if constexpr (kIdx) {
            const unsigned long long act = __ballot(1);
            const int leader = __ffsll((long long)act) - 1;
            const long long lkid = __shfl((long long)kid, leader);
            const int lslot = __shfl(slot, leader);
            const bool grp = kid == lkid && slot == lslot;
            const unsigned long long gm = __ballot(grp);
            if (grp && __popcll(gm) > 1) {
                unsigned long long* r = s_red[threadIdx.x >> 6];
                if (lane == leader) {
                    r[0] = cadd;
                    for (int j = 0; j < c.naggs; ++j) {
                        const AggDesc dsc = c.agg[j];
                        if (dsc.acc == 0 || dsc.alias) continue;
                        r[dsc.acc] = a.pcount ? ((const unsigned long long*)a.cols[j])[i] : acc_input(dsc, a.cols[dsc.col], i, a.nulls[dsc.col]);
                    }
                }
                __threadfence_block();
                __builtin_amdgcn_wave_barrier();
                if (lane != leader) {
                    atomicAdd(&r[0], cadd);
                    for (int j = 0; j < c.naggs; ++j) {
                        const AggDesc dsc = c.agg[j];
                        if (dsc.acc == 0 || dsc.alias) continue;
                        const unsigned long long x = a.pcount ? ((const unsigned long long*)a.cols[j])[i]
                                                              : acc_input(dsc, a.cols[dsc.col], i, a.nulls[dsc.col]);
                        unsigned long long* rp = &r[dsc.acc];
                        switch (dsc.acc_kind) {
                            case ACC_ADD_I64: atomicAdd(rp, x); break;
                            case ACC_ADD_F64: atomicAdd((double*)rp, __longlong_as_double((long long)x)); break;
                            case ACC_MIN_ORD: atomicMin(rp, x); break;
                            case ACC_MAX_ORD: atomicMax(rp, x); break;
                            default: break;
                        }
                    }
                }
                __threadfence_block();
                __builtin_amdgcn_wave_barrier();
                if (lane == leader) {
                    atomicAdd(&base[kid], r[0]);
                    for (int j = 0; j < c.naggs; ++j) {
                        const AggDesc dsc = c.agg[j];
                        if (dsc.acc == 0 || dsc.alias) continue;
                        unsigned long long* col = base + (int64_t)dsc.acc * a.stride + kid;
                        const unsigned long long x = r[dsc.acc];
                        switch (dsc.acc_kind) {
                            case ACC_ADD_I64: atomicAdd(col, x); break;
                            case ACC_ADD_F64: atomicAdd((double*)col, __longlong_as_double((long long)x)); break;
                            case ACC_MIN_ORD: atomicMin(col, x); break;
                            case ACC_MAX_ORD: atomicMax(col, x); break;
                            default: break;
                        }
                    }
                }
                continue;
            }
        }
        atomicAdd(&base[kid], cadd);                            // COUNT(*)
#pragma unroll
        for (int j = 0; j < kMaxAggsInt; ++j) {
            if (j >= c.naggs) break;
            const AggDesc dsc = c.agg[j];
            if (dsc.acc == 0 || dsc.alias) continue;
            unsigned long long* col = base + (int64_t)dsc.acc * a.stride + kid;
            const unsigned long long x = a.pcount ? ((const unsigned long long*)a.cols[j])[i]   // accumulator
                                                  : acc_input(dsc, a.cols[dsc.col], i, a.nulls[dsc.col]);
            switch (dsc.acc_kind) {
                case ACC_ADD_I64: atomicAdd(col, x); break;
                case ACC_ADD_F64: atomicAdd((double*)col, __longlong_as_double((long long)x)); break;
                case ACC_MIN_ORD: atomicMin(col, x); break;
                case ACC_MAX_ORD: atomicMax(col, x); break;
                default: break;
            }
        }
    }
    // wave-level reductions of the per-thread tallies, one atomic per wave
    for (int s = 32; s >= 1; s >>= 1) {
        dropped += __shfl_xor(dropped, s);
        unsigned long long x = __shfl_xor(qmax, s);
        qmax = x > qmax ? x : qmax;
        unsigned long long y = __shfl_xor(qmin, s);
        qmin = y < qmin ? y : qmin;
    }
    if (lane == 0) {
        if (dropped) atomicAdd(&a.st->dropped, (unsigned long long)dropped);
        if (qmax) atomicMax(&a.st->max_q, qmax);
        if (qmin != ~0ull) atomicMin(&a.st->min_q, qmin);
    }
}

// ------------------------------------------------------------------------------------------------
// v2 ingest: two phases, no global atomics (DESIGN.md §4) -- Flink's LocalSlicingWindowAggOperator /
// GlobalAggCombiner split (TwoStageOptimizedWindowAggregateRule.java:88-103) done on-chip.
//
// Phase P (partition_kernel): a pure streaming pass. Per tile of records: Java key-group check,
//   slice number + lateness via the read-only directory, partition p = top bits of mix64(key) (= the
//   key-table segment that will hold the key), LDS counting sort of the tile by p, one global cursor
//   reservation per (tile, partition), coalesced stores of the bucket runs. Carried record (SoA):
//   key u64, up to 2 raw 8-byte value columns, rel u16 (slice number - q_base).
// Phase A (combine_kernel): one workgroup owns one partition = one SEG-slot key-table segment. It
//   loads the segment into LDS, streams its bucket once, finds/inserts keys in LDS (ds_cmpst_b64),
//   accumulates into an LDS window of `sl` slices with LDS atomics, and merges a slice that leaves
//   the window into HBM with plain coalesced read-modify-write (exclusive ownership: no atomics).
//   Records older than the window ("stragglers") are applied in place with global atomics.

constexpr int kMaxPart = 1024;
constexpr int kRelCap = 4096;                      // slice numbers relative to q_base
constexpr int kSub = 16;                           // sub-buckets per partition (spread cursor contention)
// Phase P's per-launch verdict for a relative slice (built by the host from the directory and the
// watermark): accept into a bucket, count as late-dropped, or hand to the v1 replay (directory miss,
// slice without slot, late firing within allowed lateness, errors -- everything rare).
constexpr uint8_t kCodeSlow = 0, kCodeAccept = 1, kCodeDrop = 2;

struct PartArgs {
    const int64_t* keys;
    const int64_t* ts;
    const void* cols[FWA_MAX_COLS];
    const int32_t* key_hash;
    int64_t n;
    int64_t wm;
    const uint8_t* relcode;            // [kRelCap] per relative slice: kCodeAccept / kCodeDrop / kCodeSlow
    const int32_t* rel2slot;           // [kRelCap] slot of each relative slice (touched marking)
    int32_t* touched;                  // per slot: the epoch of the last push that touched it (0: none)
    int32_t epoch;
    int32_t* spill;
    int64_t q_base;
    int64_t base_ts;                   // off + q_base * g: first timestamp of slice q_base (fast path)
    uint64_t fast_lim;                 // kRelCap * g (< 2^32) or 0
    uint64_t fast_m;                   // ceil(2^fast_sh / g): exact floor(dd / g) for dd < fast_lim; 0 = no fast path
    int32_t fast_sh, pad_fast;
    unsigned long long* b_key;         // [np][capb]
    unsigned long long* b_val0;
    unsigned long long* b_val1;
    uint16_t* b_rel;
    uint16_t* b_n;                     // PRE: records each bucket entry stands for (tile pre-aggregation)
    uint32_t* b_cnt;                   // [np]
    int64_t capb;
    uint64_t trash;                    // bucket index of a kMaxPart-entry scratch area past the buckets
    int64_t spill_cap;
    int32_t part_bits, np;
    int32_t sub_major;                 // bucket layout (bucket_base)
    int32_t iota1;                     // value column 1 is the reduce record index (kIotaCol): taken from i, not loaded
    int32_t vcol[2];
    int32_t vsize[2];                  // 4 or 8 bytes
    int32_t* dropidx;                  // FWA_CFG_LATE_INDICES list (nullptr: not collected)
    const uint8_t* nulls[FWA_MAX_COLS];   // SQL NULL flags of the push (records with a NULL take the v1 path)
    int32_t any_null;                  // some nulls[] is set
    const unsigned long long* pcount;  // fwa_push_partials (PRE only): records each row stands for (bucket n);
                                       // rows are not merged in the tile, counts > 65535 take the v1 path
    // PRE: a pre-aggregated entry past its sub-bucket's end is applied at once with global atomics
    unsigned long long* key_table;
    uint64_t key_mask;
    int32_t seg_log, pad_p;
    unsigned long long* const* slot_base;
    int64_t stride;
    DevStatus* st;
    long long* prof;                   // optional per-block phase cycle counters (FWA_OPT_PROFILE)
};

// Sub-bucket (p, sub)'s place in the bucket arrays, in units of capb entries. Sub-major (default): the 512-1024
// partitions' regions a Phase P block appends to (its sub = blockIdx % kSub) lie next to each other, so a tile's
// scattered run stores touch np x capb x 8 bytes of address space instead of 16x that (partition-major: 1.5 MB apart
// per partition for C2 -- a TLB page per partition).
__device__ __forceinline__ uint64_t bucket_base(int p, int sub, int np, int sub_major) {
    return sub_major ? (uint64_t)sub * (uint64_t)np + (uint64_t)p : (uint64_t)p * kSub + (uint64_t)sub;
}

__device__ __forceinline__ bool row_has_null(const PartArgs& a, int64_t i) {
    bool r = false;
#pragma unroll
    for (int col = 0; col < FWA_MAX_COLS; ++col) r = r || (a.nulls[col] && a.nulls[col][i]);
    return r;
}

__device__ __forceinline__ unsigned long long load_raw(const void* col, int64_t i, int size) {
    return size == 4 ? (unsigned long long)((const uint32_t*)col)[i] : ((const unsigned long long*)col)[i];
}

// Make the compiler wait for a loaded register HERE, on every path (see partition3).
__device__ __forceinline__ void consume(unsigned long long x) {
    asm volatile("" : : "v"((uint32_t)x), "v"((uint32_t)(x >> 32)));
}
__device__ __forceinline__ void consume(int64_t x) { consume((unsigned long long)x); }
__device__ __forceinline__ void consume(int32_t x) { asm volatile("" : : "v"(x)); }
__device__ __forceinline__ void consume(uint32_t x) { asm volatile("" : : "v"(x)); }

// partition3 (Phase P): the tile is staged in LDS in arrival order (x_*), a counting sort by partition writes only a
// permutation (s_src) and the store loop gathers through it, so the load registers are free for the next tile's
// loads as soon as the tile is classified; the run reservations are issued before those loads (below). The
// key-group check and key-hash loads are compiled in only when needed (KG: 0 whole range owned, 1 hash of the key,
// 2 supplied key.hashCode()).
// PRE (skewed keys, COUNT [+ one BIGINT SUM] layouts): equal (key, slice) records of a tile are first merged
// in an LDS hash table -- the wavefront/workgroup hot-key reduction of Flink's local pre-aggregation
// (LocalSlicingWindowAggOperator) -- so a Zipf head key costs one bucket entry per tile instead of one
// per record: no sub-bucket overflow into the v1 replay, no same-address LDS atomics in the combiner.
// Entries carry their record count (b_n) and the partial BIGINT sum in the value column.
// inlined: as a call it made the PRE kernels spill VGPRs around the call site (DESIGN.md section 4, "Skewed keys")
__device__ __forceinline__ void pre_apply_global(unsigned long long* table, uint64_t mask, int seg_log, int part_bits,
                                              unsigned long long* base, int64_t stride, int has_sum, int64_t key,
                                              unsigned long long n, unsigned long long sum, DevStatus* st) {
    const int64_t kid = key_slot(table, mask, seg_log, part_bits, key, st);
    if (kid < 0) { st->key_full = 1; raise_error(st, FWA_E_OOM); return; }
    atomicAdd(&base[kid], n);
    if (has_sum) atomicAdd(&base[stride + kid], sum);
}

// W16: the tile's columns are read with 16-byte loads (two records per lane per column; 8-byte loads reach
// roughly 0.6x the 16-byte rate, MI355X_MICROARCH.md): item j of a lane is record 2 * ((j / 2) * THREADS + tid) + j % 2.
// NW = 2 (two value columns, the second a 4-byte one, e.g. FLOAT beside DOUBLE): the key's 32 bits and the 4-byte
// value's bits share one u64, the 8-byte value keeps its own (18 instead of 26 bytes per entry).
// NW: narrow bucket entries -- key and BIGINT value as two sign-extended 32-bit halves of one u64 (10 instead of 18
// bytes per entry with the u16 slice); a record whose key or value needs 64 bits takes the v1 replay.
// ROLL (W16, not PRE; DESIGN.md section 5 "Rolling tile loads"): the next tile's loads are issued pair by pair from
// inside the classify loop, each as soon as the registers of its pair are dead, instead of in one burst behind the
// scan; the wait is per pair too, ahead of the pair's classify. No register set, tile or LDS more: only where the
// loads are issued moves. The cold branches of classify (NULL flags, late-index list, spill list, the time-zone table
// on the 64-bit division's branch) wait vmcnt(0) as before and then drain the loads in flight as well.
template <int NV, int ITEMS, int THREADS, int VW, int KG, int PRE = 0, int W16 = 0, int NW = 0, int ROLL = 0>
__global__ void __launch_bounds__(THREADS, 1) partition3_kernel(PartArgs a, const EngineConst* __restrict__ cp) {
    static_assert(!ROLL || (W16 && !PRE), "rolling issue: paired loads; PRE reads the load registers behind a barrier");
    static_assert(THREADS == kMaxPart && ITEMS <= 8, "one partition cursor per thread; trash area of 8 x kMaxPart");
    static_assert(!PRE || NV <= 1, "pre-aggregation: COUNT [+ one BIGINT sum]");
    static_assert(!W16 || (ITEMS % 2 == 0 && KG != 2 && NV <= 1), "paired loads: even ITEMS, no key-hash column");
    static_assert(NW != 1 || (NV == 1 && !PRE && (VW & 1) && W16), "narrow entries: one 8-byte value column, paired loads");
    static_assert(NW != 2 || (NV == 2 && !PRE && VW == 1 && !W16), "narrow entries: an 8-byte and a 4-byte value column");
    constexpr int XV = NW == 1 ? 0 : (NW == 2 ? 1 : NV);   // value columns staged apart from the packed key word
    constexpr int kTile = THREADS * ITEMS;
    constexpr int kHt = 2 * kTile;                     // PRE: (key, slice) hash table, load <= 0.5
    constexpr int kHtLog = __builtin_ctz(kHt);
    const EngineConst& c = *cp;
    __shared__ uint32_t hist[kMaxPart];
    __shared__ uint32_t toff[kMaxPart];
    __shared__ uint32_t gbase[kMaxPart];
    __shared__ uint32_t sbase[kMaxPart];   // spill-list base of the tile's overflow records, per partition
    __shared__ unsigned long long x_key[kTile];
    // NW: x_key holds the packed entry (key | value << 32) and x_val is not used (half the staging LDS)
    __shared__ unsigned long long x_val[XV > 0 ? XV : 1][XV > 0 ? kTile : 1];
    __shared__ uint16_t x_rel[kTile];
    __shared__ uint16_t s_part[kTile];
    __shared__ uint16_t s_src[kTile];
    __shared__ uint32_t wsum[THREADS / 64];
    __shared__ uint32_t s_total;
    __shared__ uint8_t s_code[kRelCap];
    __shared__ uint32_t ht[PRE ? kHt : 1];             // PRE: 1 + staging index of the (key, slice)'s representative
    __shared__ uint32_t x_n[PRE ? kTile : 1];          // PRE: records merged into the representative
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    unsigned dropped = 0, wide = 0;
    uint32_t relmax = 0, relmin = ~0u;
    const bool ds = c.sem == FWA_SEM_DATASTREAM;
    for (int r = tid; r < kRelCap / 4; r += THREADS) ((uint32_t*)s_code)[r] = ((const uint32_t*)a.relcode)[r];
    const int64_t ntiles = (a.n + kTile - 1) / kTile;
    const int sub = blockIdx.x % kSub;
    // one tile's loaded columns
    struct Regs { unsigned long long key[ITEMS], v0[ITEMS], v1[ITEMS]; int64_t ts[ITEMS]; int32_t kh[ITEMS]; };
    // Column pointers resolved once (uniform, SGPRs): indexing the kernel-argument array per load
    // made hipcc fetch the pointer with a vector load and wait vmcnt(0) before every value load,
    // serialising the tile's loads item by item.
    const int64_t* __restrict__ pkeys = a.keys;
    const int64_t* __restrict__ pts = a.ts;
    const void* pc0 = NV > 0 ? a.cols[a.vcol[0]] : nullptr;
    const void* pc1 = NV > 1 ? a.cols[a.vcol[1]] : nullptr;
    constexpr bool w0 = (VW & 1) != 0, w1 = (VW & 2) != 0;
    const int32_t* __restrict__ pkh = a.key_hash;
    const int64_t n = a.n;
    // every load of a tile is issued before any is used; uniform branches sit outside the item loops
    // (a per-item select between a 4- and an 8-byte load made hipcc wait vmcnt(0) at every join)
    auto xof = [&](int j) -> int { return W16 ? 2 * ((j >> 1) * THREADS + tid) + (j & 1) : j * THREADS + tid; };
    // W16: pair jj of tile t into items 2jj, 2jj+1 of R. Pair p = records 2p, 2p+1 of the tile; a pair reaching past n
    // is not loaded (its record n-1, if any, goes to the slow path below).
    auto load_pair = [&](Regs& R, int64_t t, int jj) {
        const int64_t pi = t * (kTile / 2) + (int64_t)jj * THREADS + tid;
        const int64_t ip = 2 * pi + 1 < n ? pi : 0;
        const ulonglong2 kk = reinterpret_cast<const ulonglong2*>(pkeys)[ip];
        const longlong2 tt = reinterpret_cast<const longlong2*>(pts)[ip];
        R.key[2 * jj] = kk.x; R.key[2 * jj + 1] = kk.y;
        R.ts[2 * jj] = tt.x; R.ts[2 * jj + 1] = tt.y;
        if constexpr (NV > 0) {
            if constexpr (w0) {
                const ulonglong2 vv = reinterpret_cast<const ulonglong2*>(pc0)[ip];
                R.v0[2 * jj] = vv.x; R.v0[2 * jj + 1] = vv.y;
            } else {
                const uint2 vv = reinterpret_cast<const uint2*>(pc0)[ip];
                R.v0[2 * jj] = vv.x; R.v0[2 * jj + 1] = vv.y;
            }
        }
        R.kh[2 * jj] = 0; R.kh[2 * jj + 1] = 0;
    };
    auto load = [&](Regs& R, int64_t t) {
        if constexpr (W16) {
#pragma unroll
            for (int jj = 0; jj < ITEMS / 2; ++jj) load_pair(R, t, jj);
            return;
        }
        int64_t ic[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const int64_t i = t * kTile + (int64_t)j * THREADS + tid;
            ic[j] = i < n ? i : 0;
        }
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) { R.key[j] = (unsigned long long)pkeys[ic[j]]; R.ts[j] = pts[ic[j]]; }
        if constexpr (NV > 0) {
            if constexpr (w0) {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) R.v0[j] = ((const unsigned long long*)pc0)[ic[j]];
            } else {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) R.v0[j] = ((const uint32_t*)pc0)[ic[j]];
            }
        }
        if constexpr (NV > 1) {
            if constexpr (w1) {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) R.v1[j] = ((const unsigned long long*)pc1)[ic[j]];
            } else if (a.iota1) {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) R.v1[j] = (uint32_t)ic[j];
            } else {
#pragma unroll
                for (int j = 0; j < ITEMS; ++j) R.v1[j] = ((const uint32_t*)pc1)[ic[j]];
            }
        }
        if constexpr (KG == 2) {
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) R.kh[j] = pkh[ic[j]];
        } else {
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) R.kh[j] = 0;
        }
    };
    long long pt = clock64();
    long long pacc[6] = {0, 0, 0, 0, 0, 0};
    // phases: 0 classify (ROLL: with the waits per pair and the issue of the next tile's first pairs), 1 barrier
    // behind classify, reservation (ROLL: and the issue of the last pair) and scan (not ROLL: and the issue of the
    // next tile), 2 LDS scatter and the wait for the reservation, 3 stores, 4 barrier at the end of the tile, 5 the
    // wait for the whole tile at the top (ROLL: empty)
#define QMARK(k) do { if (KPROF(a.prof)) { const long long _t = clock64(); pacc[k] += _t - pt; pt = _t; } } while (0)
    Regs ra;
    const int64_t G = gridDim.x;
    load(ra, blockIdx.x < ntiles ? (int64_t)blockIdx.x : 0);
    // the memory operations of one store phase, to the trash area: hipcc's waitcnt analysis merges the
    // loop entry with the back-edge, so an entry without the stores made the header wait vmcnt(0) on
    // every trip (draining the previous tile's stores)
#pragma unroll
    for (int jj = 0; jj < ITEMS; ++jj) {
        const uint64_t o = a.trash + (uint64_t)(jj * THREADS + tid);   // distinct: not merged by the compiler
        a.b_key[o] = 0ull;
        a.b_rel[o] = 0;
        if constexpr (PRE) a.b_n[o] = 0;
        if (XV > 0) a.b_val0[o] = 0ull;
        if (XV > 1) a.b_val1[o] = 0ull;
    }
    // one tile: classify R, scan, reserve, issue the loads of tile `nx` into R, scatter, store
    // the partition counts start at zero; each tile's owner thread p clears hist[p] once it has read it (below)
    for (int i = tid; i < kMaxPart; i += THREADS) hist[i] = 0;
    if constexpr (PRE) for (int i = tid; i < kHt / 4; i += THREADS) ((uint4*)ht)[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    auto step = [&](Regs& R, int64_t tile, int64_t nx) {
        QMARK(5);
        const int64_t t0 = tile * kTile;
        uint32_t r_pos[ITEMS];   // (p << 16 | rank) or ~0u when the record does not go to a bucket
        // wait for the whole tile HERE, on every path: a loaded register consumed only on some paths (the
        // value, staged for accepted records only) stays "pending" in hipcc's waitcnt analysis, and the
        // next reuse of that register then waited vmcnt(0) -- draining the stores and the prefetch
        // ROLL: the wait is per pair, just ahead of the pair's own classify (below) -- the later pairs of the tile
        // are still landing while the first is classified
        if constexpr (!ROLL) {
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                consume(R.key[j]);
                consume(R.ts[j]);
                if constexpr (NV > 0) consume(R.v0[j]);
                if constexpr (NV > 1) consume(R.v1[j]);
                if constexpr (KG == 2) consume(R.kh[j]);
            }
        }
        const int64_t nxt = nx < ntiles ? nx : tile;    // a block's last tile reloads itself (fixed count of loads)
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            if constexpr (ROLL != 0) {
                if ((j & 1) == 0) {                     // every register of the pair, on every path (as above)
                    consume(R.key[j]); consume(R.key[j + 1]);
                    consume(R.ts[j]); consume(R.ts[j + 1]);
                    if constexpr (NV > 0) { consume(R.v0[j]); consume(R.v0[j + 1]); }
                }
            }
            const int64_t i = t0 + xof(j);
            const int64_t key = (int64_t)R.key[j];
            const int64_t ts = R.ts[j];
            // slice relative to q_base: a timestamp within kRelCap slices of the base takes a 32-bit division
            // (one 32 x 33-bit multiply); anything else (and shift time zones) the exact 64-bit floor division
            uint64_t rel;
            const uint64_t dd = (uint64_t)ts - (uint64_t)a.base_ts;
            if (a.fast_m && dd < a.fast_lim) {
                rel = (dd * a.fast_m) >> a.fast_sh;
            } else {
                const int64_t d = jm::wsub(PRE && a.pcount ? ts : assign_ts(c, ts), c.off);
                const uint64_t ud = d < 0 ? (uint64_t)0 - (uint64_t)d : (uint64_t)d;
                const uint64_t uq = jm::udiv64(ud, c.g_div);
                const int64_t q = d >= 0 ? (int64_t)uq : ((uq * c.g_div.d == ud) ? -(int64_t)uq : -(int64_t)uq - 1);
                rel = (uint64_t)(q - a.q_base);
            }
            uint32_t code = rel < (uint64_t)kRelCap ? s_code[rel] : kCodeSlow;
            if constexpr (KG != 0) {
                const int32_t kg = jm::key_group_of(key, c.key_kind, R.kh[j], c.max_par);
                if (kg < c.kg_lo || kg > c.kg_hi) code = kCodeSlow;
            }
            if (ds && ts == LONG_MIN_J) code = kCodeSlow;
            if (a.any_null && i < a.n && row_has_null(a, i)) code = kCodeSlow;   // SQL NULLs: the v1 path
            if ((uint64_t)key == kEmptyKey) code = kCodeSlow;
            if (W16 && i == a.n - 1 && (a.n & 1)) code = kCodeSlow;     // unpaired last record: the v1 replay
            uint32_t rn = 1;                                          // records this row stands for
            if constexpr (PRE) {
                if (a.pcount && i < a.n) {
                    const unsigned long long pc = a.pcount[i];
                    rn = (uint32_t)pc;
                    if (pc == 0 || pc > 0xFFFFull) code = kCodeSlow;  // does not fit a bucket's u16 count
                }
            }
            if constexpr (NW) {   // (INT32_MIN and INT32_MIN + 1 are the narrow combiner's LDS markers: v1 path too)
                if (code == kCodeAccept && ((int64_t)(int32_t)key != key || (uint32_t)key - 0x80000000u <= 1u ||
                                            (NW == 1 && (int64_t)(int32_t)R.v0[j] != (int64_t)R.v0[j]))) {
                    code = kCodeSlow;
                    ++wide;
                }
            }
            if (i >= a.n) code = 0xff;
            dropped += code == kCodeDrop ? rn : 0u;
            note_drop(a.dropidx, a.st, code == kCodeDrop, i);
            const bool slow = code == kCodeSlow;
            const unsigned long long mk = __ballot(slow);
            if (mk) {
                const int leader = __ffsll((long long)mk) - 1;
                int32_t sb = 0;
                if (lane == leader) sb = atomicAdd(&a.st->spill_n, __popcll(mk));
                sb = __shfl(sb, leader);
                if (slow) put_idx(a.spill, sb + __popcll(mk & ((1ull << lane) - 1)), a.spill_cap, (int32_t)i, a.st);
            }
            r_pos[j] = ~0u;
            if (code == kCodeAccept) {
                relmax = max(relmax, (uint32_t)rel);
                relmin = min(relmin, (uint32_t)rel);
                const uint64_t h = jm::mix64((uint64_t)key);
                const uint32_t p = a.part_bits ? (uint32_t)(h >> (64 - a.part_bits)) : 0u;
                const int x = xof(j);
                x_key[x] = R.key[j];
                x_rel[x] = (uint16_t)rel;
                if constexpr (NW == 1) x_key[x] = (R.key[j] & 0xffffffffull) | (R.v0[j] << 32);
                else if constexpr (NW == 2) x_key[x] = (R.key[j] & 0xffffffffull) | ((R.v1[j] & 0xffffffffull) << 32);
                if (XV > 0) x_val[0][x] = R.v0[j];
                if (XV > 1) x_val[XV > 1 ? 1 : 0][x] = R.v1[j];
                if constexpr (PRE) {
                    x_n[x] = rn;
                    r_pos[j] = a.pcount ? ((p << 16) | atomicAdd(&hist[p], 1u))   // partial rows: no merge
                                        : (0x80000000u | p);                        // bucketed after the merge
                }
                else r_pos[j] = (p << 16) | atomicAdd(&hist[p], 1u);
            }
            // ROLL: the pair's registers had their last use in the staging stores and the hist atomic above; tile nxt's
            // loads of the same pair go out here, in flight through the rest of classify, the barrier, the scan and
            // the scatter (the tile's last pair: behind the reservation, below)
            if constexpr (ROLL != 0) {
                if ((j & 1) != 0 && j != ITEMS - 1) load_pair(R, nxt, j >> 1);
            }
        }
        if constexpr (PRE) {
            __syncthreads();                        // the tile's staged (key, rel) visible to every lane
#pragma unroll
            for (int j = 0; j < ITEMS; ++j) {
                if (r_pos[j] == ~0u || !(r_pos[j] & 0x80000000u)) continue;
                const uint32_t x = (uint32_t)xof(j);
                const unsigned long long key = R.key[j];
                const uint32_t rel = x_rel[x];
                uint32_t hs = ((uint32_t)key * 0x9E3779B1u + (uint32_t)(key >> 32) * 0x85EBCA77u + rel * 0xC2B2AE3Du) >> (32 - kHtLog);
                for (int probe = 0; probe < kHt; ++probe) {
                    const uint32_t old = atomicCAS(&ht[hs], 0u, x + 1u);
                    if (old == 0u) {                // representative of its (key, slice) in this tile
                        const uint32_t p = r_pos[j] & 0xffffu;
                        r_pos[j] = (p << 16) | atomicAdd(&hist[p], 1u);
                        break;
                    }
                    const uint32_t o = old - 1u;
                    if (x_key[o] == key && x_rel[o] == rel) {   // merge into the representative
                        atomicAdd(&x_n[o], 1u);
                        if constexpr (NV > 0) atomicAdd(&x_val[0][o], R.v0[j]);
                        r_pos[j] = ~0u;
                        break;
                    }
                    hs = (hs + 1u) & (kHt - 1);
                }
            }
        }
        QMARK(0);
        __syncthreads();                                // the tile's counts are complete
        // thread p owns partition p from here: its run reservation (a returning atomic) is issued BEFORE the next tile's
        // loads (vmcnt retires in order, so waiting for the reservation does not drain the prefetch)
        const int p = tid;
        const uint32_t h = p < a.np ? hist[p] : 0u;
        const uint32_t g = h ? atomicAdd(&a.b_cnt[p * kSub + sub], h) : 0u;
        if (p < a.np) hist[p] = 0;                      // nobody else reads it again this tile: ready for the next one
        // ROLL: the tile's last pair goes out behind the reservation, in every wave: the wait for g (at gbase, behind
        // the LDS scatter) is then vmcnt(3) and leaves those three loads in flight; issued ahead of the reservation
        // they would have to land first (vmcnt retires in order). Unconditional: under `wave owns a partition` hipcc's
        // waitcnt analysis merged the paths and waited vmcnt(0) right behind the reservation.
        if constexpr (ROLL != 0) load_pair(R, nxt, ITEMS / 2 - 1);
        // exclusive scan of the counts over p = tid: wave scan, per-wave sums, each thread adds the sums of the waves
        // before its own (one barrier; the partition p's run starts at toff[p] in the tile's staging order)
        {
            uint32_t incl = h;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(incl, d);
                if (lane >= d) incl += y;
            }
            if (lane == 63) wsum[tid >> 6] = incl;
            __syncthreads();
            uint32_t woff = 0;
#pragma unroll 1
            for (int v = 0; v < (tid >> 6); ++v) woff += wsum[v];   // wave-uniform trip count, few registers
            if (p < a.np) toff[p] = woff + incl - h;
            if (tid == THREADS - 1) s_total = woff + incl;
        }
        if constexpr (ROLL == 0) load(R, nxt);          // the next tile in flight from here on (unconditional)
        if constexpr (PRE) for (int i = tid; i < kHt / 4; i += THREADS) ((uint4*)ht)[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();                                // toff and s_total complete
        QMARK(1);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {               // the LDS scatter does not need the reservation: the
            if (r_pos[j] == ~0u) continue;              // reservation's latency overlaps this loop
            const uint32_t p = r_pos[j] >> 16;
            const uint32_t sidx = toff[p] + (r_pos[j] & 0xffffu);
            s_part[sidx] = (uint16_t)p;
            s_src[sidx] = (uint16_t)xof(j);
        }
        if (p < a.np) {
            gbase[p] = g;
            // records past the sub-bucket's end (skewed keys) go to the v1 replay: one spill reservation
            // per (tile, overflowing partition) -- a per-wave reservation on the single spill counter
            // serialised ~100 K same-address device atomics per push under Zipf(1.1)
            const uint64_t end = (uint64_t)g + h;
            if (end > (uint64_t)a.capb) {
                const uint32_t ov = (uint32_t)(end - std::max<uint64_t>(g, (uint64_t)a.capb));
                atomicAdd(&a.st->ovf_n, (int32_t)ov);
                if constexpr (!PRE) sbase[p] = (uint32_t)atomicAdd(&a.st->spill_n, (int32_t)ov);
            }
        }
        __syncthreads();
        QMARK(2);
        const uint32_t total = s_total;
        // fixed trip count, every store issued (lanes without a record write the trash area): the next
        // classify then waits for its loads with an exact vmcnt instead of draining these stores
#pragma unroll
        for (int jj = 0; jj < ITEMS; ++jj) {
            const uint32_t sidx = (uint32_t)(jj * THREADS + tid);
            const bool valid = sidx < total;
            const uint32_t p = valid ? s_part[sidx] : 0u;
            const uint32_t x = valid ? s_src[sidx] : 0u;
            const uint64_t dst = (uint64_t)gbase[p] + (sidx - toff[p]);
            const bool inb = valid && dst < (uint64_t)a.capb;
            if (valid && !inb) {                // sub-bucket full (skewed keys)
                if constexpr (PRE) {            // a merged entry has no record index to replay: apply it now
                    const int32_t slot = a.rel2slot[x_rel[x]];
                    if (slot >= 0)
                        pre_apply_global(a.key_table, a.key_mask, a.seg_log, a.part_bits, a.slot_base[slot], a.stride,
                                         NV, (int64_t)x_key[x], x_n[x], NV > 0 ? x_val[0][x] : 0ull, a.st);
                } else {                        // the v1 replay takes it
                    const uint64_t first = std::max<uint64_t>(gbase[p], (uint64_t)a.capb);
                    put_idx(a.spill, (int64_t)sbase[p] + (int64_t)(dst - first), a.spill_cap, (int32_t)(t0 + x), a.st);
                }
            }
            const uint64_t o = !inb ? a.trash + (uint64_t)(jj * THREADS + tid)
                                    : bucket_base(p, sub, a.np, a.sub_major) * (uint64_t)a.capb + dst;
            a.b_key[o] = x_key[x];              // NW: packed at staging
            a.b_rel[o] = x_rel[x];
            if constexpr (PRE) a.b_n[o] = (uint16_t)x_n[x];
            if (XV > 0) a.b_val0[o] = x_val[0][x];
            if (XV > 1) a.b_val1[o] = x_val[XV > 1 ? 1 : 0][x];
        }
        QMARK(3);
        __syncthreads();
        QMARK(4);
    };
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += G) step(ra, tile, tile + G);
    if (KPROF(a.prof) && tid == 0) for (int q = 0; q < 6; ++q) a.prof[(int64_t)blockIdx.x * 8 + q] = pacc[q];
#undef QMARK
    for (int sh = 32; sh >= 1; sh >>= 1) {
        dropped += __shfl_xor(dropped, sh);
        if constexpr (NW) wide += __shfl_xor(wide, sh);
        relmax = max(relmax, (uint32_t)__shfl_xor((int)relmax, sh));
        relmin = min(relmin, (uint32_t)__shfl_xor((int)relmin, sh));
    }
    if (lane == 0) {
        if (dropped) atomicAdd(&a.st->dropped, (unsigned long long)dropped);
        if (NW && wide) atomicAdd(&a.st->wide_n, (int32_t)wide);
        if (relmin != ~0u) {
            atomicMax(&a.st->max_q, (unsigned long long)jm::ord_i64(a.q_base + (int64_t)relmax));
            atomicMin(&a.st->min_q, (unsigned long long)jm::ord_i64(a.q_base + (int64_t)relmin));
        }
    }
    if (relmin != ~0u)
        for (uint32_t r = relmin + (uint32_t)lane; r <= relmax; r += 64) {
            const int32_t slot = a.rel2slot[r];
            if (slot >= 0 && a.touched[slot] != a.epoch) a.touched[slot] = a.epoch;
        }
}

struct CombineArgs {
    const unsigned long long* b_key;
    const unsigned long long* b_val0;
    const unsigned long long* b_val1;
    const uint16_t* b_rel;
    const uint16_t* b_n;               // PRE buckets: records per entry (nullptr: one each)
    const uint32_t* b_cnt;
    int64_t capb;
    int32_t seg_log, np, sl;           // sl: LDS slice window
    int32_t sub_major;                 // bucket layout (bucket_base)
    const int32_t* rel2slot;           // [kRelCap]
    const uint8_t* relfresh;           // [kRelCap] 1: the slot still holds its identities (no record reached it yet);
                                       // 2: a stale slot (below), as fresh as 1 to the merge
    // Stale retirement (DESIGN.md §5): a slot the tumbling fire retired without storing identities still holds the
    // fired window's values. The slices of this push that sit on such slots have relfresh 2; those inside the push's
    // slice range (DevStatus min_q .. max_q of Phase P, final when this kernel starts) leave it clean: a block's merge
    // of such a slice stores every kid of its segment, and the block stores identities over its segment for the ones
    // it never merges. Stale slices outside the range are not written and stay stale (the host reads the same range).
    int32_t stale;                     // 1: some relfresh entry is 2
    int64_t q_base;                    // slice number of rel 0
    unsigned long long* key_table;
    unsigned long long* const* slot_base;
    int64_t stride;
    DevStatus* st;
    long long* prof;                   // optional per-block phase cycle counters (FWA_OPT_PROFILE)
};

__device__ __forceinline__ unsigned long long ident_of(int acc_kind) { return acc_kind == ACC_MIN_ORD ? ~0ull : 0ull; }

__device__ __forceinline__ unsigned long long carried_ord(unsigned long long raw, int kind) {
    switch (kind) {
        case FWA_MIN_I64: case FWA_MAX_I64: case FWA_MINBY_I64: case FWA_MAXBY_I64: return jm::ord_i64((int64_t)raw);
        case FWA_MIN_I32: case FWA_MAX_I32: return jm::ord_i64((int64_t)(int32_t)(uint32_t)raw);   // (load_ord's domain)
        case FWA_MIN_F32: case FWA_MAX_F32:
            return jm::ord_bits64((uint64_t)__double_as_longlong((double)__uint_as_float((uint32_t)raw)));
        default: return jm::ord_bits64(raw);
    }
}

__device__ __forceinline__ double carried_f64(unsigned long long raw, int kind) {
    return (kind == FWA_SUM_F32 || kind == FWA_AVG_F32) ? (double)__uint_as_float((uint32_t)raw)
                                                         : __longlong_as_double((long long)raw);
}

// Apply one combiner entry (slice rel, global kid g, n records, carried values) to its slice's HBM
// accumulators with device atomics (stragglers: their slice was already merged by this block).
__device__ __forceinline__ void strag_apply(const CombineArgs& a, const EngineConst& c, int rel, uint32_t g, uint32_t n,
                                            unsigned long long x0, unsigned long long x1) {
    const int32_t slot = a.rel2slot[rel];
    if (slot < 0) return;
    unsigned long long* base = a.slot_base[slot];
    atomicAdd(&base[g], (unsigned long long)n);
    for (int jj = 0; jj < c.naggs; ++jj) {
        const AggDesc d = c.agg[jj];
        if (d.acc == 0 || d.alias) continue;
        const unsigned long long raw = d.kind == FWA_COUNT_COL ? (unsigned long long)n : d.vslot == 0 ? x0 : x1;
        unsigned long long* gp = base + (int64_t)d.acc * a.stride + g;
        switch (d.acc_kind) {
            case ACC_ADD_I64: atomicAdd(gp, raw); break;
            case ACC_ADD_F64: atomicAdd((double*)gp, carried_f64(raw, d.kind)); break;
            case ACC_MIN_ORD: atomicMin(gp, carried_ord(raw, d.kind)); break;
            case ACC_MAX_ORD: atomicMax(gp, carried_ord(raw, d.kind)); break;
            default: break;
        }
    }
}

// Stale retirement: the push's slice range as relative slices [lo, hi] (hi < lo: nothing to clean).
__device__ __forceinline__ void stale_range(const CombineArgs& a, int& lo, int& hi) {
    lo = 0;
    hi = -1;
    if (!a.stale) return;
    const unsigned long long mn = a.st->min_q, mx = a.st->max_q;
    if (mn == ~0ull) return;
    lo = (int)(jm::unord_i64(mn) - a.q_base);
    hi = (int)(jm::unord_i64(mx) - a.q_base);
}

// ... and identities over kids [k0, k1) of the slot of relative slice rel, every column (k0, k1 even: 16-byte stores).
// kind_of(cc): the accumulator kind of column cc > 0.
template <int TH, class F>
__device__ __forceinline__ void stale_ident(const CombineArgs& a, int rel, int64_t k0, int64_t k1, int tid, int nacc, F&& kind_of) {
    const int32_t slot = a.rel2slot[rel];
    if (slot < 0) return;
    const int64_t n2 = (k1 - k0) / 2;
    for (int cc = 0; cc < nacc; ++cc) {
        const unsigned long long id = cc == 0 ? 0ull : ident_of(kind_of(cc));
        ulonglong2* col = (ulonglong2*)(a.slot_base[slot] + (int64_t)cc * a.stride + k0);
        for (int64_t i = tid; i < n2; i += TH) col[i] = make_ulonglong2(id, id);
    }
}

// The kids behind the partitions (np << seg_log .. stride - 1: the side slot of the INT64_MIN key and the padding) belong
// to no combiner block and are written by the v1 path only, in a later kernel: the last block restores them up front.
template <int TH, class F>
__device__ __forceinline__ void stale_side(const CombineArgs& a, int lo, int hi, int tid, int nacc, F&& kind_of) {
    for (int r = lo; r <= hi; ++r)
        if (a.relfresh[r] == 2) stale_ident<TH>(a, r, (int64_t)a.np << a.seg_log, a.stride, tid, nacc, kind_of);
}

// A block merges the slices [first lo, last lo + SL) of its window, each once and in order (no window passes), and its
// stragglers are older than the window: records of a slice below the first lo, or of one already merged. The first lo
// is the oldest slice of the block's first chunk (every wave's list starts there). So, ahead of the chunk loop, the
// stale slices below it get their identities, with a barrier ahead of any straggler's atomics (a full straggler list
// applies them at once) -- all of the range when the partition got no entry; the stale slices inside the window's path
// are stored whole by their merge, which a barrier separates from the later stragglers as ever; and the ones above the
// last window get their identities on exit.
// (lo, ident_seg, s_first, the first chunk's nrel: the bodies' locals. The conditions are uniform over the block. The
// range is read again at each use: nothing of this stays in registers across the chunk loop. WMIN: the wave's minimum
// of an unsigned value, in lane 0 at least.)
#define STALE_BELOW(WMIN) do { \
        if (a.stale) { \
            uint32_t m_ = 0x7fffffffu; \
            for (int j_ = 0; j_ < IT; ++j_) m_ = min(m_, (uint32_t)nrel[j_]);   /* (an invalid entry's -1: the largest) */ \
            m_ = WMIN(m_); \
            if (lane == 0) atomicMin(&s_first, (int)m_); \
            __syncthreads(); \
            int s_lo_, s_hi_; \
            stale_range(a, s_lo_, s_hi_); \
            const int first_ = s_first; \
            for (int r_ = s_lo_; r_ <= s_hi_ && r_ < first_; ++r_) if (a.relfresh[r_] == 2) ident_seg(r_); \
            __syncthreads(); \
        } } while (0)
#define STALE_ABOVE() do { \
        if (lo != 0x7fffffff) { \
            int s_lo_, s_hi_; \
            stale_range(a, s_lo_, s_hi_); \
            for (int r_ = max(s_lo_, lo + SL); r_ <= s_hi_; ++r_) if (a.relfresh[r_] == 2) ident_seg(r_); \
        } } while (0)
#define STALE_SIDE(NACC) do { \
        int s_lo_, s_hi_; \
        stale_range(a, s_lo_, s_hi_); \
        if (p == a.np - 1) stale_side<TH>(a, s_lo_, s_hi_, tid, NACC, kind_of); } while (0)

// Stragglers of one combiner block, kept in LDS and applied after the block's last merge.
constexpr int kStragL = 256;
struct StragL {
    uint32_t g, n;
    int32_t rel, pad;
    unsigned long long x0, x1;
};

// combine3's LDS key segment is stored swizzled: the four 16-byte quads of an 8-slot bucket are permuted by the bucket
// index's bits 2-3 (logical slot s at s ^ (((s >> 5) & 3) << 1)), so the same quad of 16 random buckets lands on 16
// distinct 16-byte bank groups (unswizzled: 4, i.e. a 4-way bank conflict on every probe read, SQ counters r05).
__device__ __forceinline__ uint32_t kswz(uint32_t s) { return s ^ (((s >> 5) & 3u) << 1); }


// ------------------------------------------------------------------------------------------------
// combine3: the Phase A combiner, restructured for latency tolerance (DESIGN.md §4, r01 clock64
// profile: the v2 combiner spent 43 % of its time in serialised flat RMWs / scalar-load waits).
//  * wave w streams sub-bucket w (64 lanes, coalesced); the next chunk's loads are issued before the
//    current chunk is combined (register double buffer);
//  * ONE barrier per chunk: each wave publishes its chunk's slice range into a double-buffered LDS
//    slot, the block range is read back after the barrier (no LDS atomics, no second barrier);
//  * aggregate descriptors are hoisted into registers once; the inner loop has no scalar loads;
//  * the slice flush reads LDS into registers, then issues every HBM load of the flush before any
//    add/store (one exposed latency per flush instead of one per slot and column), through
//    address-space-1 pointers (global_load/store, not flat).
typedef __attribute__((address_space(1))) unsigned long long g_u64;
typedef const __attribute__((address_space(1))) unsigned long long* gc_u64_ptr;

// ------------------------------------------------------------------------------------------------
// combine3, lean body (DESIGN.md §5 "Lean narrow combiner"): the narrow flagship shape -- NW 1, LAYOUT 1 (COUNT + one
// BIGINT SUM), no PRE, no MP. Same LDS accumulators, window, stragglers and errors as the general body below; what
// differs is how a chunk's entries find their slots:
//  * the partition's key segment is held in LDS as a 4-byte image: kLeanEmpty for kEmptyKey, the low word for a key
//    that fits int32, kLeanForeign for any other resident (a 64-bit key of the v1 replay: occupied, never matches).
//    partition3 sends both marker values to the v1 replay, so no entry key equals a marker. A bucket is 32 bytes:
//    two ds_read_b128, eight 32-bit compares;
//  * hashes and bucket addresses are computed before the chunk barrier; after it the home buckets of BT entries are
//    read together (one exposed LDS latency per batch) and matched with a select chain: "found, and where" only;
//  * entries not found in their home bucket set a bit in a per-lane mask; one loop per chunk takes each lane's lowest
//    missed entry through the general probe (next buckets, first empty slot in logical order, 32-bit CAS insert);
//  * a chunk whose entries are, for the whole wave, valid, found, inside the window and no stragglers issues its
//    LDS adds back to back; any other chunk runs the per-entry code of the general body.
// On exit only the slots this block filled are written to the 64-bit table (sign-extended); foreign and untouched
// slots are never rewritten.
constexpr int32_t kLeanEmpty = (int32_t)0x80000000;
constexpr int32_t kLeanForeign = (int32_t)0x80000001;
typedef int32_t lean_i4 __attribute__((ext_vector_type(4)));

// The 4-byte segment is stored swizzled like the 8-byte one: the two 16-byte quads of a 32-byte bucket are exchanged by
// the bucket index's bit 3 (logical slot s at s ^ (((s >> 6) & 1) << 2)), so the first quads of 16 random buckets fall
// on all 16 bank groups of 16 bytes of a 256-byte LDS row (unswizzled: on the 8 even ones).
__device__ __forceinline__ uint32_t kswz32(uint32_t s) { return s ^ (((s >> 6) & 1u) << 2); }

__device__ __forceinline__ int32_t lean_key_image(unsigned long long k) {
    if (k == kEmptyKey) return kLeanEmpty;
    const bool narrow = (int64_t)(int32_t)(uint32_t)k == (int64_t)k && (uint32_t)k - 0x80000000u > 1u;
    return narrow ? (int32_t)(uint32_t)k : kLeanForeign;
}

// Make the compiler have every bucket of a batch loaded HERE: one statement, so no read can sink behind another
// entry's match (see consume()).
template <int BT>
__device__ __forceinline__ void lean_pin(const lean_i4* qa, const lean_i4* qb) {
    static_assert(BT >= 1 && BT <= 4, "batch size");
    if constexpr (BT == 1) asm volatile("" : : "v"(qa[0]), "v"(qb[0]));
    else if constexpr (BT == 2) asm volatile("" : : "v"(qa[0]), "v"(qb[0]), "v"(qa[1]), "v"(qb[1]));
    else if constexpr (BT == 3) asm volatile("" : : "v"(qa[0]), "v"(qb[0]), "v"(qa[1]), "v"(qb[1]), "v"(qa[2]), "v"(qb[2]));
    else asm volatile("" : : "v"(qa[0]), "v"(qb[0]), "v"(qa[1]), "v"(qb[1]), "v"(qa[2]), "v"(qb[2]), "v"(qa[3]), "v"(qb[3]));
}

// Which of a bucket's 8 physical slots holds kk (-1: none). Eight compares into eight scalar masks, then eight selects:
// written out because the compiler chains compare and select through VCC, with a wait slot between the two every time
// (a VALU write of a scalar mask needs two wait states before a VALU read of it; here eight instructions lie between).
// The selects run from slot 7 down to slot 0, each eight instructions behind its compare: the lowest matching slot wins
// (a key is in a bucket once at most; the empty test of the general probe wants the first empty slot).
__device__ __forceinline__ int32_t lean_match(const lean_i4& qa, const lean_i4& qb, int32_t kk) {
    int32_t t = -1;
    unsigned long long m0, m1, m2, m3, m4, m5, m6, m7;
    asm("v_cmp_eq_u32_e64 %8, %16, %17\n\t"
        "v_cmp_eq_u32_e64 %7, %15, %17\n\t"
        "v_cmp_eq_u32_e64 %6, %14, %17\n\t"
        "v_cmp_eq_u32_e64 %5, %13, %17\n\t"
        "v_cmp_eq_u32_e64 %4, %12, %17\n\t"
        "v_cmp_eq_u32_e64 %3, %11, %17\n\t"
        "v_cmp_eq_u32_e64 %2, %10, %17\n\t"
        "v_cmp_eq_u32_e64 %1, %9, %17\n\t"
        "v_cndmask_b32_e64 %0, %0, 7, %8\n\t"
        "v_cndmask_b32_e64 %0, %0, 6, %7\n\t"
        "v_cndmask_b32_e64 %0, %0, 5, %6\n\t"
        "v_cndmask_b32_e64 %0, %0, 4, %5\n\t"
        "v_cndmask_b32_e64 %0, %0, 3, %4\n\t"
        "v_cndmask_b32_e64 %0, %0, 2, %3\n\t"
        "v_cndmask_b32_e64 %0, %0, 1, %2\n\t"
        "v_cndmask_b32_e64 %0, %0, 0, %1"
        : "+v"(t), "=&s"(m0), "=&s"(m1), "=&s"(m2), "=&s"(m3), "=&s"(m4), "=&s"(m5), "=&s"(m6), "=&s"(m7)
        : "v"(qa.x), "v"(qa.y), "v"(qa.z), "v"(qa.w), "v"(qb.x), "v"(qb.y), "v"(qb.z), "v"(qb.w), "v"(kk));
    return t;
}

// The home bucket's first slot: jm::mix64 of the sign-extended key, of which a segment of at most 2^24 slots needs the
// low 24 bits only. Bit for bit mix64's, with half of its 32-bit multiplies: the key's upper word is 0 or ~0, so its
// products are a select; the last product is needed to bit 55, which 24-bit multiplies give for its two upper terms.
__device__ __forceinline__ uint32_t lean_home(int32_t k, uint32_t smask) {
    constexpr uint32_t c1l = 0x1ce4e5b9u, c1h = 0xbf58476du, c2l = 0x133111ebu, c2h = 0x94d049bbu;
    const uint32_t s = (uint32_t)(k >> 31);
    const uint32_t xlo = (uint32_t)k ^ (((uint32_t)k >> 30) | (s << 2));   // x = z ^ (z >> 30); its upper word is s & ~3
    const unsigned long long p = (unsigned long long)xlo * c1l;
    const uint32_t z1lo = (uint32_t)p;
    const uint32_t z1hi = (uint32_t)(p >> 32) + xlo * c1h + (s & (0u - 4u * c1l));
    const uint32_t ylo = z1lo ^ ((z1lo >> 27) | (z1hi << 5));              // y = z1 ^ (z1 >> 27)
    const uint32_t yhi = z1hi ^ (z1hi >> 27);
    const unsigned long long q = (unsigned long long)ylo * c2l;
    const uint32_t z2lo = (uint32_t)q;
    const uint32_t z2hi = (uint32_t)(q >> 32) + __umul24(ylo, c2h) + __umul24(yhi, c2l);   // low 24 bits
    const uint32_t h = z2lo ^ ((z2lo >> 31) | (z2hi << 1));                // z2 ^ (z2 >> 31), low 25 bits
    return h & smask & ~(uint32_t)(kBucket - 1);
}

// Minimum (unsigned) or maximum (signed) over the wave's 64 lanes, as a scalar: four DPP steps reduce each row of 16
// lanes (pairs, quads, half rows, rows), the four rows meet in scalar registers. All lanes must be active.
template <bool kMax>
__device__ __forceinline__ int lean_wave_red(int v) {
    auto step = [](int x, int y) { return kMax ? max(x, y) : (int)min((uint32_t)x, (uint32_t)y); };
    v = step(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));    // quad_perm:[1,0,3,2]
    v = step(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));    // quad_perm:[2,3,0,1]
    v = step(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true));   // row_half_mirror
    v = step(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true));   // row_mirror
    return step(step(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
                step(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

template <int IT, int BT, int SL, int TH>
__device__ __forceinline__ void combine3_lean(const CombineArgs& a, const EngineConst& c) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(IT % BT == 0, "whole batches");
    static_assert(TH / kSub == 64, "one wave per sub-bucket");
    constexpr int kWaves = TH / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int p = blockIdx.x;
    const int seg = 1 << a.seg_log;
    const uint32_t smask = (uint32_t)seg - 1u;
    __shared__ StragL s_strag[kStragL];
    __shared__ int s_sn, s_first;
    // LDS, at the general body's offsets (push_v2 sizes one block for both): key image [seg] i32 (swizzled, kswz32),
    // COUNT [SL][seg] u32, SUM [SL][seg] u64, s_mm: the block's slice range of a chunk {min, max} x 3 (below), s_new
    int32_t* lkey = (int32_t*)smem;
    uint32_t* lcnt = (uint32_t*)(smem + (size_t)seg * 8);
    unsigned long long* lacc = (unsigned long long*)(smem + (size_t)seg * 8 + (size_t)SL * seg * 4);
    int* s_mm = (int*)(smem + (size_t)seg * 8 + (size_t)SL * seg * 4 + (size_t)SL * seg * 8);
    int* s_new = s_mm + 4 * kWaves;
    long long pt = clock64();
    long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PMARK(k) do { if (KPROF(a.prof)) { const long long _t = clock64(); pacc[k] += _t - pt; pt = _t; } } while (0)
    unsigned long long* gkeys = a.key_table + ((int64_t)p << a.seg_log);
    for (int i = tid; i < seg; i += TH) lkey[kswz32((uint32_t)i)] = lean_key_image(gkeys[i]);
    for (int i = tid; i < SL * seg; i += TH) { lcnt[i] = 0; lacc[i] = 0ull; }
    if (tid == 0) { *s_new = 0; s_sn = 0; s_first = 0x7fffffff; }
    if (tid < 3) { s_mm[2 * tid] = 0x7fffffff; s_mm[2 * tid + 1] = -1; }
    constexpr int64_t kChunk = (int64_t)IT * 64;
    // (the wave's own count, as a scalar: whole chunks are loaded without a bounds test per entry)
    const int my_cnt = __builtin_amdgcn_readfirstlane((int)min((int64_t)a.b_cnt[p * kSub + wv], a.capb));
    const int64_t boff = (int64_t)bucket_base(p, wv, a.np, a.sub_major) * a.capb;
    int64_t cnt = 0;
    for (int s2 = 0; s2 < kSub; ++s2) cnt = max(cnt, min((int64_t)a.b_cnt[p * kSub + s2], a.capb));
    const gc_u64_ptr bk = (const gc_u64_ptr)(a.b_key + boff);
    const __attribute__((address_space(1))) uint16_t* br = (const __attribute__((address_space(1))) uint16_t*)(a.b_rel + boff);
    int lo = 0x7fffffff;
    // stale retirement (CombineArgs): a stale slice is stored whole by its merge
    auto kind_of = [](int) { return (int)ACC_ADD_I64; };
    auto ident_seg = [&](int r) { stale_ident<TH>(a, r, (int64_t)p << a.seg_log, ((int64_t)p + 1) << a.seg_log, tid, 2, kind_of); };
    STALE_SIDE(2);
    auto flush = [&](int rel) {   // merge window slice `rel` into HBM (the general body's flush for COUNT + one ADD_I64)
        constexpr int kPer = 4096 / TH;   // seg <= 4096
        const int w = rel & (SL - 1);
        const int32_t slot = (rel >= 0 && rel < kRelCap) ? a.rel2slot[rel] : -1;
        g_u64* base = slot >= 0 ? (g_u64*)a.slot_base[slot] : nullptr;
        const int fr = (slot >= 0 && a.relfresh) ? (int)a.relfresh[rel] : 0;
        const bool fresh = fr != 0;
        // stale: every kid, the ones without a count too (a slice past the push's range, in the last window of a push of
        // fewer than SL slices, gets identities it did not need; the host keeps it stale)
        const bool all = fr == 2;
        uint32_t k[kPer];
        unsigned long long x[kPer];
        int64_t g[kPer];
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
            const int i = tid + m * TH;
            k[m] = 0; x[m] = 0ull;
            g[m] = ((int64_t)p << a.seg_log) + i;
            if (i < seg) { k[m] = lcnt[w * seg + i]; lcnt[w * seg + i] = 0; }
            if (k[m]) { x[m] = lacc[(size_t)w * seg + i]; lacc[(size_t)w * seg + i] = 0ull; }
        }
        if (!base) return;
        g_u64* col = base + a.stride;
        unsigned long long old[kPer], old1[kPer];
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
            old[m] = (k[m] && !fresh) ? base[g[m]] : 0ull;
            old1[m] = (k[m] && !fresh) ? col[g[m]] : 0ull;
        }
#pragma unroll
        for (int m = 0; m < kPer; ++m)
            if (k[m] || (all && tid + m * TH < seg)) { base[g[m]] = old[m] + k[m]; col[g[m]] = old1[m] + x[m]; }
    };
    __syncthreads();
    // register double buffer: n* = chunk in flight, the packed entries (key | value << 32) are unpacked at use
    unsigned long long nkey[IT];
    int nrel[IT];
    auto load_chunk = [&](int64_t cb) {
        if (cb + kChunk <= (int64_t)my_cnt) {   // a whole chunk: one address, the entries at constant offsets
            const gc_u64_ptr pk = bk + cb + lane;
            const __attribute__((address_space(1))) uint16_t* pr = br + cb + lane;
#pragma unroll
            for (int j = 0; j < IT; ++j) { nkey[j] = pk[j * 64]; nrel[j] = (int)pr[j * 64]; }
        } else {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                const int64_t i = cb + (int64_t)j * 64 + lane;
                const bool ok = i < (int64_t)my_cnt;
                nkey[j] = ok ? bk[i] : 0ull;
                nrel[j] = ok ? (int)br[i] : -1;
            }
        }
    };
    load_chunk(0);
#define STALE_WMIN(x) (uint32_t)lean_wave_red<false>((int)(x))
    STALE_BELOW(STALE_WMIN);
#undef STALE_WMIN
    PMARK(0);
    int it = 0;
    for (int64_t cb = 0; cb < cnt; cb += kChunk, ++it) {
        int32_t key[IT], val[IT];
        int rel[IT];
        const bool whole = cb + kChunk <= (int64_t)my_cnt;   // (wave-uniform) every entry of this wave's chunk is valid
        uint32_t rminu = 0xffffffffu;       // (an invalid entry's -1 is the largest unsigned)
        int rmax = -1;
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            key[j] = (int32_t)(uint32_t)nkey[j];
            val[j] = (int32_t)(uint32_t)(nkey[j] >> 32);
            rel[j] = nrel[j];
            rminu = min(rminu, (uint32_t)rel[j]);
            rmax = max(rmax, rel[j]);
        }
        PMARK(1);
        if (cb + kChunk < cnt) load_chunk(cb + kChunk);
        // the block's slice range of this chunk: every wave's range meets in one {min, max} pair of LDS (one lane's
        // atomics), read back after the barrier. Three pairs in turn: the pair of chunk it + 1 is reset here, after the
        // barrier of chunk it - 1 behind which its last readers (chunk it - 2) are done, before the barrier of chunk it
        // ahead of which nobody writes it.
        const int wmin = (int)min((uint32_t)lean_wave_red<false>((int)rminu), 0x7fffffffu), wmax = lean_wave_red<true>(rmax);
        int* mm = s_mm + 2 * (it % 3);
        if (lane == 0) { atomicMin(&mm[0], wmin); atomicMax(&mm[1], wmax); }
        if (tid == 0) { int* nx = s_mm + 2 * ((it + 1) % 3); nx[0] = 0x7fffffff; nx[1] = -1; }
        // hashes and home buckets before the barrier (pinned: the compiler otherwise sinks them behind it)
        uint32_t hb[IT];
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            hb[j] = lean_home(key[j], smask);
            consume(hb[j]);
        }
        PMARK(2);
        __syncthreads();
        PMARK(3);
        const int cmin = __builtin_amdgcn_readfirstlane(mm[0]), cmax = __builtin_amdgcn_readfirstlane(mm[1]);
        if (cmax < 0) continue;
        if (lo == 0x7fffffff) lo = cmin;
        if (cmax >= lo + SL) {              // slide the window up to the chunk's newest slice
            while (cmax >= lo + SL) { flush(lo); ++lo; if (KPROF(a.prof)) pacc[7] += 1000; }
            __syncthreads();
        }
        const int lo_c = lo;                // entries older than this are stragglers
        PMARK(4);
        if (KPROF(a.prof)) pacc[7] += 1;
        // fast match: the home buckets of BT entries read together, then "found, and where" per entry. Physical quads
        // (the swizzle exchanges a bucket's two quads): the logical slot is taken at the end.
        // (hb[j] becomes the entry's slot once it is found: one register for both; a missed entry keeps its bucket)
        uint32_t miss = 0;
#pragma unroll
        for (int j0 = IT - BT; j0 >= 0; j0 -= BT) {   // (descending: entry j's miss bit is shifted up to bit j)
            lean_i4 qa[BT], qb[BT];
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                qa[u] = *(const lean_i4*)&lkey[hb[j0 + u]];
                qb[u] = *(const lean_i4*)&lkey[hb[j0 + u] + 4];
            }
            lean_pin<BT>(qa, qb);
#pragma unroll
            for (int u = BT - 1; u >= 0; --u) {
                const int32_t t = lean_match(qa[u], qb[u], key[j0 + u]);
                const uint32_t b = hb[j0 + u];
                // found: the logical slot; missed (t -1): some slot of the home bucket, the bucket is its & ~7
                hb[j0 + u] = b + (((uint32_t)t ^ (b >> 4)) & 4u) + ((uint32_t)t & 3u);
                miss = __builtin_amdgcn_alignbit(miss, (uint32_t)t, 31);   // miss << 1 | t's sign
            }
        }
        // misses: each lane's lowest missed entry through the general probe, until no lane has one
        uint32_t todo = miss;
        if (!whole) {                       // (an invalid entry needs no slot; its bit stays in miss)
            uint32_t ok = 0;
#pragma unroll
            for (int j = 0; j < IT; ++j) ok |= rel[j] >= 0 ? (1u << j) : 0u;
            todo &= ok;
        }
        while (todo) {
            const int jm_ = __builtin_ctz(todo);
            todo &= todo - 1u;
            int32_t kk = key[0];
            uint32_t b = hb[0];
#pragma unroll
            for (int j = 1; j < IT; ++j) { kk = jm_ == j ? key[j] : kk; b = jm_ == j ? hb[j] : b; }
            b &= ~(uint32_t)(kBucket - 1);
            int32_t found = -1;
            for (int round = 0; round <= (seg >> 2) && found < 0; ++round) {
                const uint32_t f = ((b >> 6) & 1u) << 2;
                const lean_i4 pa = *(const lean_i4*)&lkey[b + f];          // the quads in logical order
                const lean_i4 pb = *(const lean_i4*)&lkey[b + (f ^ 4u)];
                const int32_t eq = lean_match(pa, pb, kk), em = lean_match(pa, pb, kLeanEmpty);
                if (eq >= 0) { found = (int32_t)(b + (uint32_t)eq); break; }
                if (em >= 0) {                  // absent: insert at the first empty slot (CAS vs other lanes)
                    const uint32_t sidx = b + (uint32_t)em;
                    const int32_t old = atomicCAS(&lkey[kswz32(sidx)], kLeanEmpty, kk);
                    if (old == kLeanEmpty) { found = (int32_t)sidx; atomicAdd(s_new, 1); break; }
                    if (old == kk) { found = (int32_t)sidx; break; }
                    continue;                   // lost the slot to another key: re-read this bucket
                }
                b = (b + kBucket) & smask;
            }
            if (found >= 0) miss &= ~(1u << jm_);
#pragma unroll
            for (int j = 0; j < IT; ++j) hb[j] = (jm_ == j && found >= 0) ? (uint32_t)found : hb[j];
        }
        // simple chunk (wave-uniform): every entry valid, found, in [lo_c, lo_c + SL)
        uint32_t out = 0;                   // outside the window (invalid entries too: rel -1)
#pragma unroll
        for (int j = 0; j < IT; ++j) out |= (uint32_t)(rel[j] - lo_c) & ~(uint32_t)(SL - 1);
        if (__builtin_amdgcn_ballot_w64((out | miss) != 0u) == 0ull) {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                const uint32_t at = ((uint32_t)(rel[j] & (SL - 1)) << a.seg_log) + hb[j];
                atomicAdd(&lcnt[at], 1u);
                atomicAdd(&lacc[at], (unsigned long long)(int64_t)val[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                if (rel[j] < 0 || rel[j] >= lo + SL) continue;
                if (miss & (1u << j)) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); continue; }
                const int32_t local = (int32_t)hb[j];
                const unsigned long long x0 = (unsigned long long)(int64_t)val[j];
                if (rel[j] < lo_c) {
                    // older than the window (its slice is already merged into HBM): listed in LDS and applied
                    // with device atomics after the last merge
                    if (KPROF(a.prof)) pacc[6] += 1000000;
                    const uint32_t g = (uint32_t)(((int64_t)p << a.seg_log) + local);
                    const int si = atomicAdd(&s_sn, 1);
                    if (si < kStragL) s_strag[si] = StragL{g, 1u, rel[j], 0, x0, 0ull};
                    else strag_apply(a, c, rel[j], g, 1u, x0, 0ull);
                    continue;
                }
                const int w = rel[j] & (SL - 1);
                atomicAdd(&lcnt[w * seg + local], 1u);
                atomicAdd(&lacc[(size_t)w * seg + local], x0);
            }
        }
        PMARK(5);
    }
    __syncthreads();
    if (lo != 0x7fffffff)
        for (int r = lo; r < lo + SL; ++r) flush(r);
    STALE_ABOVE();
    __syncthreads();                    // every merge of this block stored before the stragglers' atomics
    if (tid == 0 && s_sn) atomicAdd(&a.st->strag_n, s_sn);
    for (int t = tid; t < min(s_sn, kStragL); t += TH) {
        const StragL se = s_strag[t];
        strag_apply(a, c, se.rel, se.g, se.n, se.x0, se.x1);
    }
    if (*s_new) {                       // publish the slots this block filled (exclusive owner of this segment)
        for (int i = tid; i < seg; i += TH) {
            const int32_t k32 = lkey[kswz32((uint32_t)i)];
            if (k32 != kLeanEmpty && gkeys[i] == kEmptyKey) gkeys[i] = (unsigned long long)(int64_t)k32;
        }
        if (tid == 0) atomicAdd(&a.st->n_keys, (unsigned long long)*s_new);
    }
    if (KPROF(a.prof) && tid == 0) for (int q = 0; q < 8; ++q) a.prof[(int64_t)p * 8 + q] = pacc[q];
#undef PMARK
}

// LAYOUT: the accumulator columns, fixed at compile time for the common shapes so the per-record
// path has no descriptor switch (a runtime switch over 8 columns cost ~1000 scalar instructions per
// record from SGPR spills): 1 = COUNT + one ADD_I64 fed by value slot 0 (SUM/AVG over BIGINT);
// 2 = COUNT only; 0 = generic (descriptor table in LDS, one column per loop trip).
// MP: window passes (below) for chunks spanning more slices than the window; chosen per handle once a push
// saw many stragglers (small HOP/CUMULATE slices), since the passes cost registers the common case needs.
// LEAN: the lean body above (narrow COUNT + BIGINT SUM entries only) with first probes in batches of LEAN entries;
// 0: the general body.
template <int IT, int SL, int NV, int TH, int LAYOUT, int PRE = 0, int MP = 0, int NW = 0, int LEAN = 0>
__global__ void __launch_bounds__(TH, 1) combine3_kernel(CombineArgs a, const EngineConst* __restrict__ cp) {
    if constexpr (LEAN != 0) {
        static_assert(NW == 1 && LAYOUT == 1 && NV == 1 && PRE == 0 && MP == 0, "lean body: narrow COUNT + SUM entries");
        combine3_lean<IT, LEAN, SL, TH>(a, *cp);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int kWaves = TH / 64;
    constexpr int LPS = TH / kSub;     // lanes per sub-bucket (64: one wave per sub; 32: two subs per wave)
    static_assert(LPS == 32 || LPS == 64, "sub-bucket lane mapping");
    const EngineConst& c = *cp;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int sub = tid / LPS, li = tid % LPS;
    const int p = blockIdx.x;
    const int seg = 1 << a.seg_log;
    const uint32_t smask = (uint32_t)seg - 1u;
    const int nacc = LAYOUT == 1 ? 2 : (LAYOUT == 2 ? 1 : c.nacc_comb);
    __shared__ int s_desc[kMaxAggsInt + 1];   // generic layout: per column kind | vslot << 8 | input kind << 16
    __shared__ StragL s_strag[kStragL];
    __shared__ int s_sn, s_first;
    if (LAYOUT == 0 && tid == 0) {
        for (int j = 0; j < c.naggs; ++j)
            if (c.agg[j].acc > 0 && !c.agg[j].alias) s_desc[c.agg[j].acc] = c.agg[j].acc_kind | (c.agg[j].vslot << 8) | (c.agg[j].kind << 16);
    }
    // LDS: key segment [seg] (swizzled, kswz), COUNT [SL][seg] u32, the other accumulators [nacc-1][SL][seg] u64
    unsigned long long* lkey = (unsigned long long*)smem;
    uint32_t* lcnt = (uint32_t*)(smem + (size_t)seg * 8);
    unsigned long long* lacc = (unsigned long long*)(smem + (size_t)seg * 8 + (size_t)SL * seg * 4);
    int* s_mm = (int*)(smem + (size_t)seg * 8 + (size_t)SL * seg * 4 + (size_t)(nacc - 1) * SL * seg * 8);
    // s_mm: [2][kWaves] mins, [2][kWaves] maxs, s_new
    int* s_min = s_mm;
    int* s_max = s_mm + 2 * kWaves;
    int* s_new = s_mm + 4 * kWaves;
    long long pt = clock64();
    long long pacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PMARK(k) do { if (KPROF(a.prof)) { const long long _t = clock64(); pacc[k] += _t - pt; pt = _t; } } while (0)
    unsigned long long* gkeys = a.key_table + ((int64_t)p << a.seg_log);
    for (int i = tid; i < seg; i += TH) lkey[kswz((uint32_t)i)] = gkeys[i];
    for (int i = tid; i < SL * seg; i += TH) lcnt[i] = 0;
    if (tid == 0) { *s_new = 0; s_sn = 0; s_first = 0x7fffffff; }
    __syncthreads();
    for (int cc = 1; cc < nacc; ++cc) {
        const unsigned long long id = LAYOUT == 1 ? 0ull : ident_of(s_desc[cc] & 0xff);
        for (int i = tid; i < SL * seg; i += TH) lacc[(size_t)(cc - 1) * SL * seg + i] = id;
    }
    constexpr int64_t kChunk = (int64_t)IT * LPS;
    // sub-buckets: this wave's own list
    const int64_t my_cnt = min((int64_t)a.b_cnt[p * kSub + sub], a.capb);
    const int64_t boff = (int64_t)bucket_base(p, sub, a.np, a.sub_major) * a.capb;
    int64_t cnt = 0;
    for (int s2 = 0; s2 < kSub; ++s2) cnt = max(cnt, min((int64_t)a.b_cnt[p * kSub + s2], a.capb));
    const gc_u64_ptr bk = (const gc_u64_ptr)(a.b_key + boff);
    const gc_u64_ptr bv0 = a.b_val0 ? (const gc_u64_ptr)(a.b_val0 + boff) : nullptr;
    const gc_u64_ptr bv1 = a.b_val1 ? (const gc_u64_ptr)(a.b_val1 + boff) : nullptr;
    const __attribute__((address_space(1))) uint16_t* br = (const __attribute__((address_space(1))) uint16_t*)(a.b_rel + boff);
    const __attribute__((address_space(1))) uint16_t* bn = PRE ? (const __attribute__((address_space(1))) uint16_t*)(a.b_n + boff) : nullptr;
    int lo = 0x7fffffff;
    // stale retirement (CombineArgs; the host sets it for neither PRE buckets nor window passes): a stale slice is
    // stored whole by its merge
    constexpr bool kStale = !PRE && !MP;
    auto kind_of = [&](int cc) { return LAYOUT == 1 ? (int)ACC_ADD_I64 : (s_desc[cc] & 0xff); };
    auto ident_seg = [&](int r) { stale_ident<TH>(a, r, (int64_t)p << a.seg_log, ((int64_t)p + 1) << a.seg_log, tid, nacc, kind_of); };
    if constexpr (kStale) STALE_SIDE(nacc);
    auto flush = [&](int rel) {   // merge window slice `rel` into HBM; every thread owns seg/TH slots
        constexpr int kPer = 4096 / TH;   // seg <= 4096
        const int w = rel & (SL - 1);
        const int32_t slot = (rel >= 0 && rel < kRelCap) ? a.rel2slot[rel] : -1;
        g_u64* base = slot >= 0 ? (g_u64*)a.slot_base[slot] : nullptr;
        // a slot no record reached before this push holds its identities, and this block merges each of its slices
        // once (later entries of the slice straggle, applied after the last merge; the host passes no flags when Phase P
        // may have written slots itself, PRE): store without reading
        const int fr = (slot >= 0 && a.relfresh) ? (int)a.relfresh[rel] : 0;
        const bool fresh = fr != 0;
        const bool all = kStale && fr == 2;   // stale: every kid, identities where no count (the lean body's note)
        uint32_t k[kPer];
        int64_t g[kPer];
#pragma unroll
        for (int m = 0; m < kPer; ++m) {
            const int i = tid + m * TH;
            k[m] = 0;
            g[m] = ((int64_t)p << a.seg_log) + i;
            if (i < seg) { k[m] = lcnt[w * seg + i]; lcnt[w * seg + i] = 0; }
        }
        if (base) {
            unsigned long long old[kPer];
#pragma unroll
            for (int m = 0; m < kPer; ++m) old[m] = (k[m] && !fresh) ? base[g[m]] : 0ull;
#pragma unroll
            for (int m = 0; m < kPer; ++m) if (k[m] || (all && tid + m * TH < seg)) base[g[m]] = old[m] + k[m];
        }
        for (int cc = 1; cc < nacc; ++cc) {
            const int akc = LAYOUT == 1 ? ACC_ADD_I64 : (s_desc[cc] & 0xff);
            unsigned long long x[kPer], old[kPer];
            const unsigned long long id = ident_of(akc);
#pragma unroll
            for (int m = 0; m < kPer; ++m) {
                const int i = tid + m * TH;
                x[m] = id;
                if (k[m]) {
                    unsigned long long* lp = &lacc[(size_t)(cc - 1) * SL * seg + (size_t)w * seg + i];
                    x[m] = *lp;
                    *lp = id;
                }
            }
            if (!base) continue;
            g_u64* col = base + (int64_t)cc * a.stride;
#pragma unroll
            for (int m = 0; m < kPer; ++m) old[m] = (k[m] && !fresh) ? col[g[m]] : id;
#pragma unroll
            for (int m = 0; m < kPer; ++m) {
                if (!k[m]) {
                    if (all && tid + m * TH < seg) col[g[m]] = id;
                    continue;
                }
                unsigned long long r = old[m];
                switch (akc) {
                    case ACC_ADD_I64: r = old[m] + x[m]; break;
                    case ACC_ADD_F64: r = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)old[m]) + __longlong_as_double((long long)x[m])); break;
                    case ACC_MIN_ORD: r = x[m] < old[m] ? x[m] : old[m]; break;
                    case ACC_MAX_ORD: r = x[m] > old[m] ? x[m] : old[m]; break;
                    default: break;
                }
                col[g[m]] = r;
            }
        }
    };
    __syncthreads();
    // register double buffer: n* = chunk in flight, c* = chunk being combined
    unsigned long long nkey[IT], nx0[IT], nx1[IT];
    int nrel[IT];
    uint32_t nnn[IT];                   // PRE: records per entry
    auto load_chunk = [&](int64_t cb) {
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            const int64_t i = cb + (int64_t)j * LPS + li;
            const bool ok = i < my_cnt;
            int r;
            if constexpr (NW == 1) {                        // narrow entry (key | value << 32), unpacked at use
                nkey[j] = ok ? bk[i] : 0ull;
                r = ok ? (int)br[i] : -1;
            } else {
                nkey[j] = ok ? bk[i] : 0ull;
                nx0[j] = (NV > 0 && ok) ? bv0[i] : 0ull;
                r = ok ? (int)br[i] : -1;
            }
            if constexpr (NW != 2) nx1[j] = (NV > 1 && ok) ? bv1[i] : 0ull;   // NW 2: in the key word's top half
            nrel[j] = r;
            nnn[j] = PRE ? (ok ? (uint32_t)bn[i] : 0u) : 1u;
        }
    };
    load_chunk(0);
    if constexpr (kStale) {
        auto wmin = [](uint32_t x) { for (int sh = 32; sh >= 1; sh >>= 1) x = min(x, (uint32_t)__shfl_xor((int)x, sh)); return x; };
        STALE_BELOW(wmin);
    }
    PMARK(0);
    int it = 0;
    for (int64_t cb = 0; cb < cnt; cb += kChunk, ++it) {
        unsigned long long key[IT], x0[IT], x1[IT];
        int rel[IT];
        uint32_t nr[IT];
        int rmin = 0x7fffffff, rmax = -1;
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            if constexpr (NW == 1) {
                key[j] = (unsigned long long)(int64_t)(int32_t)(uint32_t)nkey[j];
                x0[j] = (unsigned long long)(int64_t)(int32_t)(uint32_t)(nkey[j] >> 32);
                x1[j] = nx1[j];
            } else if constexpr (NW == 2) {   // the 4-byte value's raw bits (carried_f64 / carried_ord read 32 of them)
                key[j] = (unsigned long long)(int64_t)(int32_t)(uint32_t)nkey[j];
                x0[j] = nx0[j];
                x1[j] = nkey[j] >> 32;
            } else {
                key[j] = nkey[j]; x0[j] = nx0[j]; x1[j] = nx1[j];
            }
            rel[j] = nrel[j]; nr[j] = nnn[j];
            if (rel[j] >= 0) { rmin = min(rmin, rel[j]); rmax = max(rmax, rel[j]); }
        }
        PMARK(1);
        if (cb + kChunk < cnt) load_chunk(cb + kChunk);
        for (int sh = 32; sh >= 1; sh >>= 1) { rmin = min(rmin, __shfl_xor(rmin, sh)); rmax = max(rmax, __shfl_xor(rmax, sh)); }
        const int buf = it & 1;
        if (lane == 0) { s_min[buf * kWaves + wv] = rmin; s_max[buf * kWaves + wv] = rmax; }
        // first probes in flight across the barrier
        uint32_t pos[IT];
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            pos[j] = (uint32_t)jm::mix64(key[j]) & smask;
        }
        PMARK(2);
        __syncthreads();
        PMARK(3);
        int cmin = 0x7fffffff, cmax = -1;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) { cmin = min(cmin, s_min[buf * kWaves + v]); cmax = max(cmax, s_max[buf * kWaves + v]); }
        if (cmax < 0) continue;
        if (lo == 0x7fffffff) lo = cmin;
        if constexpr (MP) {
            if (cmin >= lo + SL) {          // the whole chunk is past the window: merge it out, jump to cmin
                for (int r = lo; r < lo + SL; ++r) flush(r);
                if (KPROF(a.prof)) pacc[7] += 1000;
                lo = cmin;
                __syncthreads();
            }
        } else if (cmax >= lo + SL) {       // slide the window up to the chunk's newest slice
            while (cmax >= lo + SL) { flush(lo); ++lo; if (KPROF(a.prof)) pacc[7] += 1000; }
            __syncthreads();
        }
        const int lo_c = lo;                // entries older than this are stragglers
        PMARK(4);
        if (KPROF(a.prof)) pacc[7] += 1;
        // bucket probing: read the key's 8-slot home bucket (4 x ds_read_b128, issued together), compare all 8; only keys
        // displaced past their bucket (a few %) take another round. Logical slots, stored swizzled (kswz: the reads of
        // 16 lanes spread over all 16 bank groups).
        int32_t loc[IT];
#pragma unroll
        for (int j = 0; j < IT; ++j) {
            loc[j] = -2;
            if (rel[j] < 0) continue;
            const unsigned long long kk = key[j];
            uint32_t b = pos[j] & ~(uint32_t)(kBucket - 1);
            int32_t found = -1;
            for (int round = 0; round <= (seg >> 2) && found < 0; ++round) {
                const uint32_t f = ((b >> 5) & 3u) << 1;
                const ulonglong2 q0 = *(const ulonglong2*)&lkey[b + (0u ^ f)];
                const ulonglong2 q1 = *(const ulonglong2*)&lkey[b + (2u ^ f)];
                const ulonglong2 q2 = *(const ulonglong2*)&lkey[b + (4u ^ f)];
                const ulonglong2 q3 = *(const ulonglong2*)&lkey[b + (6u ^ f)];
                const unsigned long long v[8] = {q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
                uint32_t eq = 0, em = 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) { eq |= (uint32_t)(v[t] == kk) << t; em |= (uint32_t)(v[t] == kEmptyKey) << t; }
                if (eq) { found = (int32_t)(b + __builtin_ctz(eq)); break; }
                if (em) {                       // absent: insert at the first empty slot (CAS vs other lanes)
                    const uint32_t sidx = b + __builtin_ctz(em);
                    const unsigned long long old = atomicCAS(&lkey[kswz(sidx)], kEmptyKey, kk);
                    if (old == kEmptyKey) { found = (int32_t)sidx; atomicAdd(s_new, 1); break; }
                    if (old == kk) { found = (int32_t)sidx; break; }
                    continue;                   // lost the slot to another key: re-read this bucket
                }
                b = (b + kBucket) & smask;
            }
            loc[j] = found;
        }
        // window passes (MP): a chunk can span more slices than the LDS window holds (HOP/CUMULATE 1 s slices:
        // a sub-bucket's 256-entry chunk covers seconds of event time); its entries stay in registers and are
        // added window by window, merging out between passes only the slices the next pass needs (the window
        // ends at the chunk's newest slice, so the next chunk's older entries still find it)
        int from = lo_c;                    // entries below this were added by an earlier pass (or straggle)
        for (int pass = 0;; ++pass) {
#pragma unroll
            for (int j = 0; j < IT; ++j) {
                if (rel[j] < 0 || rel[j] >= lo + SL) continue;
                const int32_t local = loc[j];
                if (local < 0) { if (pass == 0) { a.st->key_full = 1; raise_error(a.st, FWA_E_OOM); } continue; }
                if (rel[j] < from) {
                    if (pass > 0) continue;     // added in an earlier pass
                    // older than the window (its slice is already merged into HBM): listed in LDS and applied
                    // with device atomics after the last merge (this block owns the kid; a list shared by all
                    // blocks serialised them on one counter)
                    if (KPROF(a.prof)) pacc[6] += 1000000;
                    const uint32_t g = (uint32_t)(((int64_t)p << a.seg_log) + local);
                    const int si = atomicAdd(&s_sn, 1);
                    if (si < kStragL) s_strag[si] = StragL{g, PRE ? nr[j] : 1u, rel[j], 0, x0[j], x1[j]};
                    else strag_apply(a, c, rel[j], g, PRE ? nr[j] : 1u, x0[j], x1[j]);
                    continue;
                }
                const int w = rel[j] & (SL - 1);
                atomicAdd(&lcnt[w * seg + local], PRE ? nr[j] : 1u);
                if constexpr (LAYOUT == 1) {
                    atomicAdd(&lacc[(size_t)w * seg + local], x0[j]);
                } else if constexpr (LAYOUT == 0) {
                    for (int cc = 1; cc < nacc; ++cc) {
                        const int d = s_desc[cc];
                        unsigned long long* lp = &lacc[(size_t)(cc - 1) * SL * seg + (size_t)w * seg + local];
                        const int ik = d >> 16;
                        const unsigned long long raw = ik == FWA_COUNT_COL ? 1ull   // non-NULL counter (NULL rows take the v1 path)
                                                     : (NV > 1 && ((d >> 8) & 0xff) != 0) ? x1[j] : x0[j];
                        switch (d & 0xff) {
                            case ACC_ADD_I64: atomicAdd(lp, raw); break;
                            case ACC_ADD_F64: atomicAdd((double*)lp, carried_f64(raw, ik)); break;
                            case ACC_MIN_ORD: atomicMin(lp, carried_ord(raw, ik)); break;
                            case ACC_MAX_ORD: atomicMax(lp, carried_ord(raw, ik)); break;
                            default: break;
                        }
                    }
                }
            }
            if (!MP || cmax < lo + SL) break;
            __syncthreads();                // the window's adds done before it is merged out
            from = lo + SL;
            const int nl = min(lo + SL, cmax - SL + 1);
            while (lo < nl) { flush(lo); ++lo; if (KPROF(a.prof)) pacc[7] += 1000; }
            __syncthreads();                // merged and cleared before the next pass adds
        }
        PMARK(5);
    }
    __syncthreads();
    if (lo != 0x7fffffff)
        for (int r = lo; r < lo + SL; ++r) flush(r);
    if constexpr (kStale) STALE_ABOVE();
    __syncthreads();                    // every merge of this block stored before the stragglers' atomics
    if (tid == 0 && s_sn) atomicAdd(&a.st->strag_n, s_sn);
    for (int t = tid; t < min(s_sn, kStragL); t += TH) {
        const StragL se = s_strag[t];
        strag_apply(a, c, se.rel, se.g, se.n, se.x0, se.x1);
    }
    if (*s_new) {                       // publish newly inserted keys (exclusive owner of this segment)
        for (int i = tid; i < seg; i += TH) gkeys[i] = lkey[kswz((uint32_t)i)];
        if (tid == 0) atomicAdd(&a.st->n_keys, (unsigned long long)*s_new);
    }
    if (KPROF(a.prof) && tid == 0) for (int q = 0; q < 8; ++q) a.prof[(int64_t)p * 8 + q] = pacc[q];
#undef PMARK
}
