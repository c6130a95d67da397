// COUNT / SUM / AVG(DISTINCT col) over Table windows (include/flink_amd.h, FWA_COUNT_DISTINCT, FWA_AGG_DISTINCT) --
// included by engine.hip.
//
// Reference: the planner expands COUNT(DISTINCT c) into a distinct view (a MapView<value, bitmap> per (key, slice) in
// the accumulator, DistinctInfo / AggsHandlerCodeGenerator.addReusableDistinctAccumulators) and counts a value the first
// time the view sees it; NULL values are never added (Count1AggFunction over the distinct filter).
//
// Design: a tumbling window is one slice, so COUNT(DISTINCT c) of a (key, window) is the SUM(BIGINT) of a 0/1 column
// "this record is the first one of its (key, window, value)". fwa_create rewrites COUNT_DISTINCT(c) in place into
// SUM_I64(m) over a marked column m that only the engine writes (dist_plan, the sibling of dec_plan), and every push
// first runs distinct_mark_kernel over the batch: it inserts (key, value, slice, column) into one device-resident
// open-addressing set per handle and writes mark[i] = 1 iff this insert created the entry. Phase P / A, the fire
// kernels, record lists and snapshots then see an ordinary 64-bit sum. A window of several slices (HOP, CUMULATE,
// SESSION) needs the union of per-slice sets at the fire, which is not a sum: HOP and CUMULATE take it there under
// FWA_CFG_DISTINCT_RANGE (range mode, below), Table SESSION windows of a fixed gap under FWA_CFG_DISTINCT_SESSION
// (session mode, below); DataStream handles, reductions and PREHASHED keys are refused.
//
// The set. One 32-byte aligned entry per slot, three 64-bit words used (the fourth pads the entry to one 32-byte
// sector, so a probe is one aligned vector load):
//   word 0  key   (a zero key is stored as 1 with tag bit 3 set)
//   word 1  value (a zero value is stored as 1 with tag bit 4 set)
//   word 2  tag = q << 6 | 1 << 5 | value-was-zero << 4 | key-was-zero << 3 | marked column (3 bits)
// EMPTY = 0 for every word; bit 5 keeps a tag from being 0. The slice number q keeps 58 bits: |q| <= 2^63 / size, so
// windows of 64 ms and more can never alias (smaller ones are refused at fwa_create).
// Insert: words are claimed in order with atomicCAS(word, EMPTY, mine) and never change afterwards. At each word a
// CAS that returns EMPTY or my own word goes on to the next word of the same slot; any other value moves to the next
// slot (linear probing from a 64-bit mix of the three words). The lane whose tag CAS returned EMPTY created the entry;
// a lane that finds its own tag is a duplicate. Equal entries walk the same slots and meet the same immutable words,
// so exactly one lane reports "new" and an entry never lands in two slots; nothing spins or waits for another lane.
// A plain 32-byte load precedes the CASes: duplicates (the common case) cost no atomic; a stale load can only show
// EMPTY where a word is set by now, which falls through to the CAS.
// Capacity is decided on the host before each launch: bound = an upper bound of occupied slots (previous bound +
// records x marked columns) stays <= slots / 2, so a launch cannot fill the table. The marking pass also counts the
// entries it created (one atomic per wave); the count comes back with the push and replaces the "+ records" of that
// push, so pushes of mostly known values do not inflate the bound. When the bound would not fit,
// distinct_count_kernel counts the entries of windows that have not fired (one atomic per block) and the table is rebuilt
// at 2 x (live + this batch) slots (rounded up to a power of two): into a new allocation when the size changes
// (distinct_rebuild_kernel re-inserts the live entries), in place when it does not (distinct_extract_kernel moves the
// live entries to a side buffer and clears every slot in the same pass, distinct_insert_side_kernel puts them back: no
// allocation of the table's size in the steady state). The bound becomes the exact count. Firing a window costs
// nothing: its entries are garbage the next rebuild drops, so the set holds live entries + one batch (x <= 4 for the
// load factor and the rounding).
//
// Range mode (FWA_CFG_DISTINCT_RANGE on a Table HOP or CUMULATE handle). A hop window is a range of slices and the
// carried window sums add and subtract whole slices, so a per-slice additive mark cannot count it: a value present in
// slices 1 and 3 is the "first" of each slice but must count once in [1, 3], once in [2, 5] and once in [0, 1] -- no
// fixed 0/1 per (value, slice) gives all three, the union has to be taken per window. So the count moves from the push
// to the fire, and the set changes the meaning of its slice field only:
//   word 2  tag's slice field = the block number B = q >> 6 (arithmetic), q the slice number of the ingest directory
//   word 3  occupancy bitmap: bit q & 63 is set iff the value occurred for the key in slice q
// One entry per (key, value, column, block of 64 slices). B needs six bits fewer than q, so the 64 ms limit does not
// apply. The push runs distinct_mark_range_kernel (upsert, then atomicOr of the bit only when a plain load does not
// show it: duplicates stay atomic-free) and writes no marked column; dist_plan rewrites COUNT_DISTINCT(c) into COUNT(*)
// (a BIGINT that is never NULL and needs no value column), so the handle keeps its ingest and its fire, and every
// firing step of fwa_advance_watermark then calls dist_range_count before it retires slices:
//   dist_rows_index_kernel   zeroes the distinct columns of the step's rows and indexes the rows by (key, window end) in
//                            a u32 open-addressing table (plan-owned scratch)
//   dist_range_count_kernel  scans the set; an entry whose bits meet a fired window's slice range counts 1 for that
//                            window iff no earlier block of the window holds the same (key, value, column) with bits in
//                            the range (a read-only probe per earlier block: at most ceil(N / 64) for N slices), so
//                            each value is counted by exactly one of its entries; the count goes to the row by atomicAdd
// A live entry without a row is a broken invariant (accepted record => COUNT(*) > 0 => a row): the step fails.
// Rebuilds carry word 3 (the live cut is the block of q_min: a block is live while its highest slice is); the snapshot
// section keeps its layout, one entry per set bit, and restore folds them back.
//
// Session mode (FWA_CFG_DISTINCT_SESSION on a Table SESSION handle: fixed gap g, no allowed lateness). The "slice" of a
// record is its cell floor(local ts / g) (DESIGN.md section 2 has the argument): two accepted records of a key in one cell
// are less than g apart and so in one session, two in-flight sessions of a key are more than g apart and so never share
// a cell, and the session [s, e) holds exactly the key's accepted records of the cells [floor(s / g), floor((e - g) / g)].
// The entry is the one of range mode with the cell in place of the slice (tag field = cell >> 6, word 3 = cell bitmap;
// an entry is live iff its bitmap is non-zero). Two things differ from range mode, and both are needed for exactness:
//   * the marking pass runs BEHIND the ingest and skips the records the ingest dropped (a dropped record may share its
//     cell with an accepted one of another session: g = 10, watermark 20, 10 is dropped, 12 is accepted as [12, 22)).
//     dist_plan makes the internal configuration collect the dropped indices on the device; dist_drop_mask_kernel
//     scatters them into a byte mask and distinct_mark_session_kernel reads it.
//   * a fired session's bits are cleared at its fire (g = 10: [0, 10) fires at watermark 9, then 5 is accepted as the
//     new session [5, 15) in the same cell 0). dist_session_count: dist_sess_index_kernel enters every fired row once per
//     64-cell block of its range in a (key, block) multimap, dist_sess_count_kernel<S> counts as the range count does
//     (first block of the row's range that holds the value), dist_sess_clear_kernel -- a launch of its own, the count
//     reads other entries' bits -- drops the bits inside each fired row's range. An entry that meets no fired row
//     belongs to a session in flight.
//
// SUM / AVG(DISTINCT col) (FWA_AGG_DISTINCT on SUM_I64 / SUM_F64 / AVG_I64 / AVG_F64). The entry's word 1 already is the
// value, so the sum rides on the count. TUMBLE: distinct_mark_kernel<true> also writes w = mark ? value : 0 per summed
// column (bits 0: the identity of the BIGINT and of the DOUBLE sum), dist_plan rewrites the aggregate in place into
// SUM_I64(w) / SUM_F64(w), and the distinct count SUM_I64(m) -- the caller's COUNT_DISTINCT or a hidden aggregate behind
// the caller's -- decides NULL and divides AVG. Range mode: dist_range_count_kernel<true> adds the decoded value and 1
// to two plan-owned per-row columns where it counts an entry. Either way dist_finish_kernel writes the caller-visible
// value and NULL flag into plan-owned columns at fill_out (never in place: fill_out may run twice over the same rows).

struct DistWin { int64_t q_lo, q_hi, end; };   // a fired window: its slice range and its end as the fire emits it
struct DistMarkHold {                      // session mode: what the marking pass behind the ingest reads
    const int64_t* keys = nullptr;
    const int64_t* ts = nullptr;
    const int64_t* src[FWA_MAX_AGGS] = {};
    const uint8_t* nul[FWA_MAX_AGGS] = {};
    int64_t n = 0;                         // 0: nothing held
};

struct DistinctPlan {
    fwa_config ucfg;                       // the caller's configuration (fwa_get_config)
    int32_t nd = 0;                        // marked columns (one per distinct source column)
    int32_t src[FWA_MAX_AGGS] = {};        // marked column d: the caller's value column
    int32_t mcol[FWA_MAX_AGGS] = {};       // ... and the internal value-column index of its 0/1 column
    int64_t mask = 0;                      // bit j: the caller's aggregate j is a distinct one (snapshot header)
    int64_t cmask = 0;                     // ... and of those, the COUNT_DISTINCT ones
    // SUM / AVG(DISTINCT) (FWA_AGG_DISTINCT): the sum beside the count, finished into plan-owned columns (dist_finish)
    int32_t ns = 0;                        // summed source columns
    int32_t sidx[FWA_MAX_AGGS] = {};       // marked column d: its ordinal among the summed ones, -1: only counted
    int32_t sf64[FWA_MAX_AGGS] = {};       // ... its values are DOUBLE bits (else BIGINT)
    int32_t wcol[FWA_MAX_AGGS] = {};       // ... TUMBLE: the internal value-column index of w = mark ? value : 0
    int32_t fkind[FWA_MAX_AGGS] = {};      // caller's aggregate j: FWA_SUM_I64 / SUM_F64 / AVG_I64 / AVG_F64 when it
                                           // carries FWA_AGG_DISTINCT, else 0
    int32_t fd[FWA_MAX_AGGS] = {};         // ... its marked column
    int32_t fsum[FWA_MAX_AGGS] = {};       // ... TUMBLE: the internal aggregate summing w
    int32_t fcnt[FWA_MAX_AGGS] = {};       // ... TUMBLE: the internal aggregate summing m (the distinct count)
    unsigned long long* d_fout[FWA_MAX_AGGS] = {};   // finished results and NULL flags per such aggregate, [fout_cap]
    uint8_t* d_fnull[FWA_MAX_AGGS] = {};
    int64_t fout_cap = 0;
    unsigned long long* d_rsum = nullptr;  // range mode: per-row sums [ns][rs_cap], then per-row distinct counts [ns][rs_cap]
    int64_t rs_cap = 0;
    unsigned long long* d_tab = nullptr;   // the set, [slots][4]
    int64_t slots = 0, first_slots = 0;    // first_slots: FWA_OPT_DISTINCT_SLOTS (0: sized from the first push)
    int64_t bound = 0;                     // upper bound of occupied slots
    int64_t live = 0, rebuilds = 0;        // entries counted at the last rebuild; rebuilds so far
    unsigned long long* d_mark = nullptr;  // marked columns, [nd][mark_cap], then the summed columns w, [ns][mark_cap]
    int64_t mark_cap = 0;
    char* d_stage = nullptr;               // host pushes: every input column, staged once
    size_t stage_bytes = 0;
    unsigned long long* d_ctr = nullptr;   // [0] entries counted / created, [1] inserts that found no slot,
    unsigned long long* h_ctr = nullptr;   // [2] entries the last marking pass created (h_ctr[2]: its pinned landing),
                                           // [3] range mode: counted entries whose (key, window) has no row
    unsigned int* d_bcnt = nullptr;        // table scans: live entries per block [kDistScanGrid], then (8-byte aligned)
    unsigned long long* d_bpre = nullptr;  // ... their exclusive prefix [kDistScanGrid]
    unsigned long long* d_side = nullptr;  // in-place rebuild: the live entries, [3][side_cap] (range mode: [4][side_cap])
    int64_t side_cap = 0;
    hipEvent_t ev[3] = {};                 // marking pass begin / end (timed), its created-count copy
    bool timing = false;                   // ev[0..1] hold a marking pass not yet added to ingest_ms
    int64_t last_add = 0;                  // the last marking pass's share of `bound`, until its exact count replaces it
    // range mode (FWA_CFG_DISTINCT_RANGE, HOP / CUMULATE): word 3 is a slice bitmap, counts are taken at the fire
    bool range = false;
    // session mode (FWA_CFG_DISTINCT_SESSION): range is set too (same entry), the tag's field is cell >> 6
    bool sess = false;
    int64_t gap = 0;                       // the session gap = the cell width
    uint8_t* d_dmask = nullptr;            // the push's dropped records as a byte mask, [dmask_cap]
    int64_t dmask_cap = 0;
    int64_t* d_rblk = nullptr;             // the block each slot of d_rtab was entered under, [rtab_cap]
    int64_t rblk_cap = 0;
    DistMarkHold hold;                     // the push's columns, kept from dist_mark to the pass behind the ingest
    unsigned int* d_rtab = nullptr;        // the step's rows by (key, window end), session mode: by (key, block), once per
                                           // block of the row's cell range: row + 1 per slot, [rtab_cap]
    int64_t rtab_cap = 0;
    DistWin* d_wins = nullptr;             // the step's windows, [wins_cap]
    int64_t wins_cap = 0;
    hipEvent_t rev[3] = {};                // row-index pass begin, count pass begin / end (session mode: the clear's end)
    double index_ms = 0.0, count_ms = 0.0; // their device time so far (also part of fire_ms)
    int64_t count_steps = 0;               // firing steps counted
};

namespace {

const char* const kDistNoPartials = "partial accumulators of COUNT(DISTINCT): a distinct count is not mergeable without "
                                    "shipping the sets";
constexpr int64_t kDistMinSlots = 1 << 12;
constexpr int64_t kDistMinSize = 64;       // ms: the tag keeps 58 bits of the slice number

__device__ __forceinline__ uint64_t dist_hash(uint64_t k, uint64_t v, uint64_t t) {
    return jm::mix64(k ^ jm::mix64(v ^ jm::mix64(t)));
}

__host__ __device__ __forceinline__ uint64_t dist_tag(int64_t q, uint64_t key, uint64_t val, int d) {
    return ((uint64_t)q << 6) | 32ull | (val == 0 ? 16ull : 0ull) | (key == 0 ? 8ull : 0ull) | (uint64_t)(d & 7);
}
__host__ __device__ __forceinline__ int64_t dist_tag_q(uint64_t tag) { return (int64_t)tag >> 6; }
// Session mode: the cell of a local timestamp, floor(t / g) with g > 0 (local time may be negative).
__host__ __device__ __forceinline__ int64_t dist_cell(int64_t t, int64_t g) {
    const int64_t q = t / g;
    return (t < 0 && q * g != t) ? q - 1 : q;
}

// 1: this call created the entry, 0: it was there, -1: no slot (the host's bound makes that impossible); *slot: where
__device__ __forceinline__ int dist_upsert(unsigned long long* tab, uint64_t smask, uint64_t k, uint64_t v, uint64_t t,
                                           uint64_t* slot) {
    uint64_t i = dist_hash(k, v, t) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe, i = (i + 1) & smask) {
        unsigned long long* s = tab + 4 * i;
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(s);
        unsigned long long c = kv.x;
        if (c == 0ull) { c = atomicCAS(s, 0ull, (unsigned long long)k); if (c == 0ull) c = k; }
        if (c != k) continue;
        c = kv.y;
        if (c == 0ull) { c = atomicCAS(s + 1, 0ull, (unsigned long long)v); if (c == 0ull) c = v; }
        if (c != v) continue;
        c = s[2];
        *slot = i;
        if (c == 0ull) { c = atomicCAS(s + 2, 0ull, (unsigned long long)t); if (c == 0ull) return 1; }
        if (c == t) return 0;
    }
    return -1;
}
__device__ __forceinline__ int dist_insert(unsigned long long* tab, uint64_t smask, uint64_t k, uint64_t v, uint64_t t) {
    uint64_t slot;
    return dist_upsert(tab, smask, k, v, t, &slot);
}

// Range mode: set `bits` in the bitmap of the slot dist_upsert returned; a plain load first, so a bit that is there
// costs no atomic (a stale load can only miss a bit, which falls through to the atomicOr).
__device__ __forceinline__ void dist_or_bits(unsigned long long* tab, uint64_t slot, unsigned long long bits) {
    unsigned long long* w = tab + 4 * slot + 3;
    if ((*w & bits) != bits) atomicOr(w, bits);
}

// Read-only probe: the slot of (k, v, t) or -1. It may stop at a slot whose key word is 0: words never change between
// rebuilds, every insert of an earlier launch ran to its end, and no insert runs beside the caller.
__device__ __forceinline__ int64_t dist_find(const unsigned long long* tab, uint64_t smask, uint64_t k, uint64_t v, uint64_t t) {
    uint64_t i = dist_hash(k, v, t) & smask;
    for (uint64_t probe = 0; probe <= smask; ++probe, i = (i + 1) & smask) {
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(tab + 4 * i);
        if (kv.x == 0ull) return -1;
        if (kv.x == k && kv.y == v && tab[4 * i + 2] == t) return (int64_t)i;
    }
    return -1;
}

// The bits of block B that lie in the slice range [q_lo, q_hi] (the two must intersect).
__device__ __forceinline__ unsigned long long dist_block_mask(int64_t q_lo, int64_t q_hi, int64_t B) {
    const int64_t b0 = (int64_t)((uint64_t)B << 6);
    const int lo = q_lo > b0 ? (int)(q_lo - b0) : 0;
    const int hi = q_hi < b0 + 63 ? (int)(q_hi - b0) : 63;
    return (~0ull >> (63 - hi)) & (~0ull << lo);
}

struct DistMarkArgs {
    const int64_t* keys;
    const int64_t* ts;
    const int64_t* src[FWA_MAX_AGGS];      // source value column of marked column d (8-byte values, compared by bits)
    const uint8_t* nul[FWA_MAX_AGGS];      // its NULL flags (nullptr: none)
    unsigned long long* mark[FWA_MAX_AGGS];
    unsigned long long* wsum[FWA_MAX_AGGS]; // SUM / AVG(DISTINCT): w = mark ? value : 0 (nullptr: column d is only counted)
    int32_t nd;
    int64_t n;
    int64_t q_min;                         // first slice whose window has not fired at the handle's watermark
    unsigned long long* tab;
    uint64_t smask;                        // slots - 1
    unsigned long long* ctr;
    const uint8_t* dmask;                  // session mode: 1 where the ingest dropped the record
    int64_t gap;                           // ... and the cell width
};

// One thread per record: the slice number as the ingest kernels compute it, then one set insert per marked column.
// S: some column is also summed -- its first occurrences carry their value into w (bits 0 are the identity of both the
// BIGINT and the DOUBLE sum, +0.0); the count-only instantiation has neither the store nor the pointer loads.
template <bool S>
__global__ void __launch_bounds__(256) distinct_mark_kernel(DistMarkArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    unsigned int created = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = (uint64_t)a.keys[i];
        const int64_t q = sp_slice(c, assign_ts(c, a.ts[i]));
        for (int d = 0; d < a.nd; ++d) {
            unsigned long long m = 0ull, w = 0ull;
            if (q >= a.q_min && !(a.nul[d] && a.nul[d][i])) {
                const uint64_t v = (uint64_t)a.src[d][i];
                const int r = dist_insert(a.tab, a.smask, key ? key : 1ull, v ? v : 1ull, dist_tag(q, key, v, d));
                if (r < 0) atomicAdd(a.ctr + 1, 1ull);
                m = r > 0 ? 1ull : 0ull;
                if (S) w = r > 0 ? v : 0ull;
                created += r > 0 ? 1u : 0u;
            }
            a.mark[d][i] = m;
            if (S) { if (a.wsum[d]) a.wsum[d][i] = w; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) created += __shfl_down(created, o);    // the whole wave is back here
    if ((threadIdx.x & 63) == 0 && created) atomicAdd(a.ctr + 2, (unsigned long long)created);
}

// Range mode, one thread per record: upsert (key, value, block of q, column) and set bit q & 63 of its bitmap. No marked
// column is written (a.mark is unused).
// The q >= q_min filter is garbage control only. A record it skips is one the ingest drops: every window containing its
// slice has fired, so its bit lies in no window that fires again and is never read. The opposite error -- skipping a
// record the ingest accepts -- would lose a value, and cannot happen: q_min comes from accept_threshold at the handle's
// watermark (dist_qmin), the function and the watermark the ingest directory's thresholds come from, and "unknown"
// (LONG_MIN) filters nothing.
__global__ void __launch_bounds__(256) distinct_mark_range_kernel(DistMarkArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    unsigned int created = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = sp_slice(c, assign_ts(c, a.ts[i]));
        if (q < a.q_min) continue;
        const uint64_t key = (uint64_t)a.keys[i];
        const unsigned long long bit = 1ull << (q & 63);
        for (int d = 0; d < a.nd; ++d) {
            if (a.nul[d] && a.nul[d][i]) continue;
            const uint64_t v = (uint64_t)a.src[d][i];
            uint64_t slot = 0;
            const int r = dist_upsert(a.tab, a.smask, key ? key : 1ull, v ? v : 1ull, dist_tag(q >> 6, key, v, d), &slot);
            if (r < 0) { atomicAdd(a.ctr + 1, 1ull); continue; }
            dist_or_bits(a.tab, slot, bit);
            created += r > 0 ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) created += __shfl_down(created, o);    // the whole wave is back here
    if ((threadIdx.x & 63) == 0 && created) atomicAdd(a.ctr + 2, (unsigned long long)created);
}

// Session mode: the dropped-record indices of the push just ingested (list[0 .. *n), any order) as a byte mask over the
// batch (zeroed ahead of the launch). *n is read on the device: the host never copies the list for this.
__global__ void __launch_bounds__(256) dist_drop_mask_kernel(const int32_t* list, const unsigned long long* n, int64_t cap,
                                                            uint8_t* mask) {
    const int64_t m = (int64_t)*n < cap ? (int64_t)*n : cap;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = list[i];
        if (r >= 0 && r < cap) mask[r] = 1;
    }
}

// Session mode, one thread per record, behind the ingest: a record the ingest dropped sets no bit (its cell may hold an
// accepted record of another session); otherwise upsert (key, value, block of the cell, column) and set bit cell & 63.
// The cell comes from the local timestamp the session paths use (assign_ts).
__global__ void __launch_bounds__(256) distinct_mark_session_kernel(DistMarkArgs a, const EngineConst* __restrict__ cp) {
    const EngineConst& c = *cp;
    unsigned int created = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        if (a.dmask[i]) continue;
        const int64_t q = dist_cell(assign_ts(c, a.ts[i]), a.gap);
        const uint64_t key = (uint64_t)a.keys[i];
        const unsigned long long bit = 1ull << (q & 63);
        for (int d = 0; d < a.nd; ++d) {
            if (a.nul[d] && a.nul[d][i]) continue;
            const uint64_t v = (uint64_t)a.src[d][i];
            uint64_t slot = 0;
            const int r = dist_upsert(a.tab, a.smask, key ? key : 1ull, v ? v : 1ull, dist_tag(q >> 6, key, v, d), &slot);
            if (r < 0) { atomicAdd(a.ctr + 1, 1ull); continue; }
            dist_or_bits(a.tab, slot, bit);
            created += r > 0 ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) created += __shfl_down(created, o);    // the whole wave is back here
    if ((threadIdx.x & 63) == 0 && created) atomicAdd(a.ctr + 2, (unsigned long long)created);
}

// The scans of the table give block b the slots [b * chunk, (b + 1) * chunk): the count pass leaves each block's live
// count, from which the extract pass knows where the block's entries go without a shared cursor (one atomic on one
// word per wave and iteration capped both passes at the rate of that word: ~50 ms for 2^28 slots).
constexpr int kDistScanGrid = 4096;
__device__ __forceinline__ void dist_block_range(int64_t slots, int64_t* lo, int64_t* hi) {
    const int64_t chunk = (((slots + gridDim.x - 1) / gridDim.x) + 255) & ~(int64_t)255;
    *lo = (int64_t)blockIdx.x * chunk;
    *hi = *lo + chunk < slots ? *lo + chunk : slots;
}

// Entries of windows that have not fired: per block into bcnt[], and their sum with one atomic per block.
// R: word 3 is a bitmap and an entry without bits is dead (session mode clears the bits of fired sessions; in range
// mode every entry has a bit).
template <bool R>
__global__ void __launch_bounds__(256) distinct_count_kernel(const unsigned long long* tab, int64_t slots, int64_t q_min,
                                                            unsigned long long* ctr, unsigned int* bcnt) {
    __shared__ unsigned int tot;
    if (threadIdx.x == 0) tot = 0;
    __syncthreads();
    int64_t lo, hi;
    dist_block_range(slots, &lo, &hi);
    unsigned int mine = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const unsigned long long t = tab[4 * i + 2];
        mine += (t != 0ull && dist_tag_q(t) >= q_min && (!R || tab[4 * i + 3] != 0ull)) ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&tot, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        bcnt[blockIdx.x] = tot;
        if (tot) atomicAdd(ctr, (unsigned long long)tot);
    }
}

// Exclusive prefix of the nb block counts (one wave: 64 runs of consecutive blocks).
__global__ void __launch_bounds__(64) distinct_prefix_kernel(const unsigned int* bcnt, int nb, unsigned long long* bpre) {
    const int lane = threadIdx.x, per = (nb + 63) / 64;
    const int lo = lane * per, hi = lo + per < nb ? lo + per : nb;
    unsigned long long sum = 0;
    for (int j = lo; j < hi; ++j) sum += bcnt[j];
    unsigned long long incl = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    unsigned long long run = incl - sum;
    for (int j = lo; j < hi; ++j) { bpre[j] = run; run += bcnt[j]; }
}

// Rebuild into a new table: the entries of unfired windows re-inserted; ctr[0] receives the entries created there (the
// exact live count), one atomic per wave. q_min is the live cut in the tag's unit (range mode, R: blocks, and the
// bitmap moves with its entry).
template <bool R>
__global__ void __launch_bounds__(256) distinct_rebuild_kernel(const unsigned long long* tab, int64_t slots, int64_t q_min,
                                                              unsigned long long* ntab, uint64_t nsmask,
                                                              unsigned long long* ctr) {
    unsigned int made = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(tab + 4 * i);
        const unsigned long long t = tab[4 * i + 2];
        const unsigned long long bits = R ? tab[4 * i + 3] : 1ull;
        if (t != 0ull && dist_tag_q(t) >= q_min && bits != 0ull) {
            uint64_t slot = 0;
            const int r = dist_upsert(ntab, nsmask, kv.x, kv.y, t, &slot);
            if (r < 0) atomicAdd(ctr + 1, 1ull);
            else if (R) dist_or_bits(ntab, slot, bits);
            made += r > 0 ? 1u : 0u;
        }
    }
    for (int o = 32; o > 0; o >>= 1) made += __shfl_down(made, o);
    if ((threadIdx.x & 63) == 0 && made) atomicAdd(ctr, (unsigned long long)made);
}

// In-place rebuild, first half: block b's entries of unfired windows move to side[3][cap] from bpre[b] on (an LDS
// cursor orders them inside the block) and every slot is cleared in the same pass (each thread owns its slot: nothing
// inserts meanwhile). ctr[0] receives the entries moved. Range mode (R): side[4][cap], the bitmap as the fourth word.
template <bool R>
__global__ void __launch_bounds__(256) distinct_extract_kernel(unsigned long long* tab, int64_t slots, int64_t q_min,
                                                              unsigned long long* side, int64_t cap,
                                                              const unsigned long long* bpre, unsigned long long* ctr) {
    __shared__ unsigned int cur;
    if (threadIdx.x == 0) cur = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t base = (int64_t)bpre[blockIdx.x];
    int64_t lo, hi;
    dist_block_range(slots, &lo, &hi);
    for (int64_t i0 = lo; i0 < hi; i0 += 256) {           // (uniform per block: every lane takes every iteration)
        const int64_t i = i0 + threadIdx.x;
        ulonglong2 kv = make_ulonglong2(0ull, 0ull);
        unsigned long long t = 0ull, bits = 0ull;
        if (i < hi) {
            kv = *reinterpret_cast<const ulonglong2*>(tab + 4 * i);
            t = tab[4 * i + 2];
            if (R) bits = tab[4 * i + 3];
            if (kv.x | kv.y | t) {
                *reinterpret_cast<ulonglong2*>(tab + 4 * i) = make_ulonglong2(0ull, 0ull);
                tab[4 * i + 2] = 0ull;
                if (R) tab[4 * i + 3] = 0ull;
            }
        }
        const bool livee = t != 0ull && dist_tag_q(t) >= q_min && (!R || bits != 0ull);
        const unsigned long long b = __ballot(livee);
        if (!b) continue;                                  // (wave-uniform)
        unsigned int off = 0;
        if (lane == 0) off = atomicAdd(&cur, (unsigned int)__popcll(b));
        off = __shfl(off, 0);
        if (livee) {
            const int64_t pos = base + off + __popcll(b & ((1ull << lane) - 1ull));
            if (pos < cap) {
                side[pos] = kv.x; side[cap + pos] = kv.y; side[2 * cap + pos] = t;
                if (R) side[3 * cap + pos] = bits;
            }
            else atomicAdd(ctr + 1, 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && cur) atomicAdd(ctr, (unsigned long long)cur);
}

// Restore and the in-place rebuild's second half: entries given as their three stored words (w[3][n]), inserted
// without marking. Range mode (R): w[4][n], the fourth word ORed into the entry's bitmap (restore folds one bit each).
template <bool R>
__global__ void __launch_bounds__(256) distinct_insert_side_kernel(const unsigned long long* w, int64_t stride, int64_t n,
                                                                  unsigned long long* tab, uint64_t smask,
                                                                  unsigned long long* ctr) {
    unsigned int made = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t slot = 0;
        const int r = dist_upsert(tab, smask, w[i], w[stride + i], w[2 * stride + i], &slot);
        if (r < 0) atomicAdd(ctr + 1, 1ull);
        else if (R) dist_or_bits(tab, slot, w[3 * stride + i]);
        made += r > 0 ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) made += __shfl_down(made, o);
    if ((threadIdx.x & 63) == 0 && made) atomicAdd(ctr, (unsigned long long)made);
}

// ---- range mode: the count of a firing step ----

struct DistRangeArgs {
    const unsigned long long* tab;
    int64_t slots;
    uint64_t smask;
    const DistWin* wins;
    int32_t nw;
    int32_t na;                            // distinct aggregates
    const int64_t* o_key;
    const int64_t* o_end;
    int64_t row0, nrows;                   // the step's rows: [row0, row0 + nrows)
    unsigned int* rtab;
    uint32_t rmask;                        // row-table slots - 1
    unsigned long long* o_agg[FWA_MAX_AGGS];   // output column of distinct aggregate a
    int32_t agg_d[FWA_MAX_AGGS];               // ... and the ordinal of its source column
    int32_t ns;                                // summed source columns (SUM / AVG(DISTINCT))
    int32_t sum_d[FWA_MAX_AGGS];               // ... their ordinals among the source columns
    int32_t sum_f64[FWA_MAX_AGGS];             // ... DOUBLE bits (else BIGINT)
    unsigned long long* r_sum[FWA_MAX_AGGS];   // ... per-row sum of the window's distinct values (plan-owned)
    unsigned long long* r_cnt[FWA_MAX_AGGS];   // ... and their number
    unsigned long long* ctr;
    // session mode (rows by (key, block) in rtab, a multimap)
    const int64_t* o_start;
    int64_t* rblk;                             // the block slot h of rtab was entered under
    int64_t gap;
    unsigned long long* tabw;                  // the set, for the clear
};

__device__ __forceinline__ uint32_t dist_row_hash(int64_t key, int64_t end) {
    return (uint32_t)jm::mix64((uint64_t)key ^ jm::mix64((uint64_t)end));
}

// One thread per emitted row: its distinct columns start from 0 (the fire wrote COUNT(*) there) and the row enters the
// row table under (key, window end), which is unique within a step.
__global__ void __launch_bounds__(256) dist_rows_index_kernel(DistRangeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrows) return;
    const int64_t row = a.row0 + i;
    for (int j = 0; j < a.na; ++j) a.o_agg[j][row] = 0ull;
    for (int s = 0; s < a.ns; ++s) { a.r_sum[s][row] = 0ull; a.r_cnt[s][row] = 0ull; }   // (0: +0.0 as well)
    uint32_t h = dist_row_hash(a.o_key[row], a.o_end[row]) & a.rmask;
    for (uint32_t probe = 0; probe <= a.rmask; ++probe, h = (h + 1) & a.rmask)
        if (atomicCAS(a.rtab + h, 0u, (unsigned int)(i + 1)) == 0u) return;
}

// Row of (key, end) relative to row0, or -1. Equality reads the row's own columns.
__device__ __forceinline__ int64_t dist_row_find(const DistRangeArgs& a, int64_t key, int64_t end) {
    uint32_t h = dist_row_hash(key, end) & a.rmask;
    for (uint32_t probe = 0; probe <= a.rmask; ++probe, h = (h + 1) & a.rmask) {
        const unsigned int r = a.rtab[h];
        if (r == 0u) return -1;
        const int64_t row = a.row0 + (int64_t)r - 1;
        if (a.o_key[row] == key && a.o_end[row] == end) return row;
    }
    return -1;
}

// One thread per slot of the set (block ranges as dist_block_range; the entry read as two aligned 16-byte loads). A
// live entry (key, value, B, d, bits) is tried against the step's windows, staged in LDS kDistWinLds at a time (the
// common step fires one window): with m = bits & the window's range inside block B non-zero, it is the window's first
// block of its (key, value, d) iff no earlier block B' in [q_lo >> 6, B) holds an entry with bits in the range -- one
// read-only probe per earlier block, none for a window inside one block. Only the first block counts: +1 on the row of
// (key, window end) for every aggregate over column d. Entries without a row are counted in ctr[3] (one atomic per wave).
// S: some column is also summed -- where the entry counts, its decoded value (a stored 1 with tag bit 4 is 0) is added
// to the row's sum of column d (u64 add: BIGINT wraps by itself; DOUBLE: a double atomic add) and 1 to the row's
// distinct count of d, which the finish step needs even without a COUNT_DISTINCT of the caller's.
constexpr int kDistWinLds = 128;
template <bool S>
__global__ void __launch_bounds__(256) dist_range_count_kernel(DistRangeArgs a) {
    __shared__ DistWin s_win[kDistWinLds];
    int64_t lo, hi;
    dist_block_range(a.slots, &lo, &hi);
    unsigned int miss = 0;
    for (int w0 = 0; w0 < a.nw; w0 += kDistWinLds) {       // (uniform per block)
        const int cn = a.nw - w0 < kDistWinLds ? a.nw - w0 : kDistWinLds;
        __syncthreads();
        for (int w = threadIdx.x; w < cn; w += 256) s_win[w] = a.wins[w0 + w];
        __syncthreads();
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            const ulonglong2 tb = *reinterpret_cast<const ulonglong2*>(a.tab + 4 * i + 2);
            if (tb.x == 0ull || tb.y == 0ull) continue;
            const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(a.tab + 4 * i);
            const int64_t B = dist_tag_q(tb.x);
            const int64_t b0 = (int64_t)((uint64_t)B << 6);
            for (int w = 0; w < cn; ++w) {
                const int64_t q_lo = s_win[w].q_lo, q_hi = s_win[w].q_hi;
                if (q_hi < b0 || q_lo > b0 + 63) continue;
                if (!(tb.y & dist_block_mask(q_lo, q_hi, B))) continue;
                bool first = true;
                for (int64_t Bp = q_lo >> 6; first && Bp < B; ++Bp) {
                    const int64_t s = dist_find(a.tab, a.smask, kv.x, kv.y, (tb.x & 63ull) | ((uint64_t)Bp << 6));
                    if (s >= 0 && (a.tab[4 * s + 3] & dist_block_mask(q_lo, q_hi, Bp))) first = false;
                }
                if (!first) continue;
                const int64_t row = dist_row_find(a, (tb.x & 8ull) ? 0 : (int64_t)kv.x, s_win[w].end);
                if (row < 0) { ++miss; continue; }
                const int d = (int)(tb.x & 7ull);
                for (int j = 0; j < a.na; ++j) if (a.agg_d[j] == d) atomicAdd(a.o_agg[j] + row, 1ull);
                if (S) {
                    const unsigned long long v = (tb.x & 16ull) ? 0ull : kv.y;
                    for (int s = 0; s < a.ns; ++s) {
                        if (a.sum_d[s] != d) continue;
                        if (a.sum_f64[s]) atomicAdd(reinterpret_cast<double*>(a.r_sum[s] + row), __longlong_as_double((long long)v));
                        else atomicAdd(a.r_sum[s] + row, v);
                        atomicAdd(a.r_cnt[s] + row, 1ull);
                    }
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) miss += __shfl_down(miss, o);          // the whole wave is back here
    if ((threadIdx.x & 63) == 0 && miss) atomicAdd(a.ctr + 3, (unsigned long long)miss);
}

// ---- session mode: the count of a firing step, and the clear behind it ----

// The cell range of a fired session [start, end): its records lie in [start, end - gap].
__device__ __forceinline__ void dist_sess_range(const DistRangeArgs& a, int64_t row, int64_t* c_lo, int64_t* c_hi) {
    *c_lo = dist_cell(a.o_start[row], a.gap);
    *c_hi = dist_cell(jm::wsub(a.o_end[row], a.gap), a.gap);
    if (*c_hi < *c_lo) *c_hi = *c_lo;
}

// Sizing pre-pass, one thread per fired row: the 64-cell blocks the step's rows touch, summed into ctr[3] (one atomic
// per wave). The row table is a multimap with one slot per (row, block), so its size cannot come from nrows alone.
__global__ void __launch_bounds__(256) dist_sess_blocks_kernel(DistRangeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long nb = 0;
    if (i < a.nrows) {
        int64_t c_lo, c_hi;
        dist_sess_range(a, a.row0 + i, &c_lo, &c_hi);
        nb = (unsigned long long)((c_hi >> 6) - (c_lo >> 6) + 1);
    }
    for (int o = 32; o > 0; o >>= 1) nb += __shfl_down(nb, o);
    if ((threadIdx.x & 63) == 0 && nb) atomicAdd(a.ctr + 3, nb);
}

// Row index, one thread per fired row: its distinct columns and per-row sums start from 0, and the row enters the row
// table once per block of its cell range under (key, block); the slot keeps the block, so a lookup of (key, B) meets a
// row of many blocks once. Several fired sessions of one key may share a block: all of them stay in the chain.
__global__ void __launch_bounds__(256) dist_sess_index_kernel(DistRangeArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nrows) return;
    const int64_t row = a.row0 + i;
    for (int j = 0; j < a.na; ++j) a.o_agg[j][row] = 0ull;
    for (int s = 0; s < a.ns; ++s) { a.r_sum[s][row] = 0ull; a.r_cnt[s][row] = 0ull; }   // (0: +0.0 as well)
    int64_t c_lo, c_hi;
    dist_sess_range(a, row, &c_lo, &c_hi);
    const int64_t key = a.o_key[row];
    for (int64_t B = c_lo >> 6; B <= (c_hi >> 6); ++B) {
        uint32_t h = dist_row_hash(key, B) & a.rmask;
        for (uint32_t probe = 0; probe <= a.rmask; ++probe, h = (h + 1) & a.rmask)
            if (atomicCAS(a.rtab + h, 0u, (unsigned int)(i + 1)) == 0u) { a.rblk[h] = B; break; }
    }
}

// The bits of entry (key, B) that lie in fired rows, visited one row at a time: f(row, mask of the row's range in B).
// Slots are final here (the index kernel is an earlier launch), so the walk may stop at an empty one.
template <typename F>
__device__ __forceinline__ void dist_sess_rows_of(const DistRangeArgs& a, int64_t key, int64_t B, F f) {
    uint32_t h = dist_row_hash(key, B) & a.rmask;
    for (uint32_t probe = 0; probe <= a.rmask; ++probe, h = (h + 1) & a.rmask) {
        const unsigned int r = a.rtab[h];
        if (r == 0u) return;
        if (a.rblk[h] != B) continue;
        const int64_t row = a.row0 + (int64_t)r - 1;
        if (a.o_key[row] != key) continue;
        int64_t c_lo, c_hi;
        dist_sess_range(a, row, &c_lo, &c_hi);
        f(row, c_lo, c_hi, dist_block_mask(c_lo, c_hi, B));
    }
}

// One thread per slot of the set. A live entry (key, value, B, d, bits) whose bits meet the cell range of a fired row
// of (key, B) counts for that row iff no earlier block of the row's range holds the same (key, value, d) with bits in
// the range (read-only probes, at most the session's block count). An entry that meets no row belongs to a session in
// flight. S: as dist_range_count_kernel, the decoded value also goes to the row's sum and 1 to the row's count.
template <bool S>
__global__ void __launch_bounds__(256) dist_sess_count_kernel(DistRangeArgs a) {
    int64_t lo, hi;
    dist_block_range(a.slots, &lo, &hi);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const ulonglong2 tb = *reinterpret_cast<const ulonglong2*>(a.tab + 4 * i + 2);
        if (tb.x == 0ull || tb.y == 0ull) continue;
        const ulonglong2 kv = *reinterpret_cast<const ulonglong2*>(a.tab + 4 * i);
        const int64_t B = dist_tag_q(tb.x);
        const int d = (int)(tb.x & 7ull);
        dist_sess_rows_of(a, (tb.x & 8ull) ? 0 : (int64_t)kv.x, B,
                          [&](int64_t row, int64_t c_lo, int64_t c_hi, unsigned long long m) {
            if (!(tb.y & m)) return;
            for (int64_t Bp = c_lo >> 6; Bp < B; ++Bp) {
                const int64_t s = dist_find(a.tab, a.smask, kv.x, kv.y, (tb.x & 63ull) | ((uint64_t)Bp << 6));
                if (s >= 0 && (a.tab[4 * s + 3] & dist_block_mask(c_lo, c_hi, Bp))) return;
            }
            for (int j = 0; j < a.na; ++j) if (a.agg_d[j] == d) atomicAdd(a.o_agg[j] + row, 1ull);
            if (S) {
                const unsigned long long v = (tb.x & 16ull) ? 0ull : kv.y;
                for (int s = 0; s < a.ns; ++s) {
                    if (a.sum_d[s] != d) continue;
                    if (a.sum_f64[s]) atomicAdd(reinterpret_cast<double*>(a.r_sum[s] + row), __longlong_as_double((long long)v));
                    else atomicAdd(a.r_sum[s] + row, v);
                    atomicAdd(a.r_cnt[s] + row, 1ull);
                }
            }
        });
    }
}

// The clear, a launch behind the count (which reads other entries' bits): every entry drops the bits inside the cell
// range of each fired row of its (key, block). One thread owns each slot and no marking pass runs beside it: plain
// stores. An entry left without bits is dead; the next rebuild drops it.
__global__ void __launch_bounds__(256) dist_sess_clear_kernel(DistRangeArgs a) {
    int64_t lo, hi;
    dist_block_range(a.slots, &lo, &hi);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const ulonglong2 tb = *reinterpret_cast<const ulonglong2*>(a.tab + 4 * i + 2);
        if (tb.x == 0ull || tb.y == 0ull) continue;
        const unsigned long long k = a.tab[4 * i];
        unsigned long long bits = tb.y;
        dist_sess_rows_of(a, (tb.x & 8ull) ? 0 : (int64_t)k, dist_tag_q(tb.x),
                          [&](int64_t, int64_t, int64_t, unsigned long long m) { bits &= ~m; });
        if (bits != tb.y) a.tabw[4 * i + 3] = bits;
    }
}

// ---- SUM / AVG(DISTINCT): the finish of the fired rows ----

struct DistFinDesc {
    const unsigned long long* sum;         // per row: the sum of the window's distinct values (BIGINT or DOUBLE bits)
    const unsigned long long* cnt;         // ... and their number
    unsigned long long* out;               // the caller-visible column (plan-owned: the inputs stay as fired)
    uint8_t* nul;
    int32_t kind;                          // FWA_SUM_I64 / SUM_F64 / AVG_I64 / AVG_F64
};
struct DistFinArgs {
    DistFinDesc a[FWA_MAX_AGGS];
    int32_t na;
    int64_t n;
};

// One thread per (row, aggregate): SQL NULL without a non-NULL value; AVG(BIGINT) divides like Java's long division
// (truncating; the divisor is a positive count), AVG(DOUBLE) by the count as a double.
__global__ void __launch_bounds__(256) dist_finish_kernel(DistFinArgs f) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.n) return;
    const DistFinDesc& d = f.a[blockIdx.y];
    const unsigned long long c = d.cnt[i];
    unsigned long long r = c ? d.sum[i] : 0ull;
    if (c && d.kind == FWA_AVG_I64) r = (unsigned long long)((long long)r / (long long)c);
    else if (c && d.kind == FWA_AVG_F64)
        r = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)r) / (double)(long long)c);
    d.out[i] = r;
    d.nul[i] = c ? 0 : 1;
}

// ---- host ----

// FWA_AGG_DISTINCT on a kind (SUM / AVG(DISTINCT col)); dist_plan refuses the bit on every kind it does not belong to
bool dist_is_sum(int kind) { return kind > 0 && (kind & FWA_AGG_DISTINCT) != 0; }
bool dist_is_kind(int kind) { return kind == FWA_COUNT_DISTINCT || dist_is_sum(kind); }

bool has_distinct(const fwa_config* c) {
    for (int j = 0; j < c->num_aggs && j < FWA_MAX_AGGS; ++j) if (dist_is_kind(c->aggs[j].kind)) return true;
    return false;
}

// The internal configuration of a handle with distinct aggregates. COUNT_DISTINCT(c) is rewritten in place into
// SUM_I64 of the marked column m of c (same position, same result type). SUM / AVG(DISTINCT c) (FWA_AGG_DISTINCT) is
// rewritten in place into SUM_I64 / SUM_F64 of a second engine-written column w = mark ? value : 0 (the two forms over
// one column share that accumulator) and finished at the fire from it and from the distinct count SUM_I64(m): the
// caller's own COUNT_DISTINCT(c), or a hidden aggregate appended behind the caller's, so caller positions never move.
// Range mode rewrites every distinct aggregate into a COUNT(*) placeholder. 0 or an fwa_status with *why set.
int dist_plan(const fwa_config* u, DistinctPlan* P, fwa_config* icfg, std::string* why) {
    P->ucfg = *u;
    *icfg = *u;
    if (u->num_aggs < 0 || u->num_aggs > FWA_MAX_AGGS) return FWA_E_ARG;
    int base[FWA_MAX_AGGS] = {};                              // the kind without the modifier bit
    int vtype[FWA_MAX_COLS] = {};                             // summed source column: 1 BIGINT, 2 DOUBLE
    for (int j = 0; j < u->num_aggs; ++j) {
        const fwa_agg_spec& s = u->aggs[j];
        base[j] = dist_is_sum(s.kind) ? (s.kind & ~FWA_AGG_DISTINCT) : s.kind;
        if (base[j] < 0 || base[j] >= FWA_AGG_KIND_COUNT) return FWA_E_ARG;
        if (base[j] != FWA_COUNT && (s.col < 0 || s.col >= FWA_MAX_COLS)) return FWA_E_ARG;
        if (!dist_is_sum(s.kind)) continue;
        const bool i64 = base[j] == FWA_SUM_I64 || base[j] == FWA_AVG_I64;
        const bool f64 = base[j] == FWA_SUM_F64 || base[j] == FWA_AVG_F64;
        if (!i64 && !f64) {
            const bool named = base[j] == FWA_SUM_F32 || base[j] == FWA_AVG_F32 || base[j] == FWA_SUM_I32 ||
                               (base[j] >= FWA_SUM_DEC && base[j] <= FWA_AVG_DEC128);
            *why = named ? "FWA_AGG_DISTINCT: FLOAT, INT and DECIMAL distinct sums are not supported (SUM / AVG(DISTINCT) "
                           "over BIGINT and DOUBLE only)"
                         : "FWA_AGG_DISTINCT: a modifier of FWA_SUM_I64, FWA_SUM_F64, FWA_AVG_I64 and FWA_AVG_F64 only "
                           "(MIN / MAX(DISTINCT) are plain MIN / MAX, COUNT(DISTINCT) is FWA_COUNT_DISTINCT)";
            return FWA_E_ARG;
        }
        if (vtype[s.col] && vtype[s.col] != (i64 ? 1 : 2)) {
            *why = "FWA_AGG_DISTINCT: BIGINT and DOUBLE distinct aggregates over one value column";
            return FWA_E_ARG;
        }
        vtype[s.col] = i64 ? 1 : 2;
    }
    auto no = [&](const char* m) { *why = std::string("COUNT(DISTINCT): ") + m; return FWA_E_UNSUPPORTED; };
    const bool hop = u->window_kind == FWA_SLIDE || u->window_kind == FWA_CUMULATE;
    if (hop && !(u->flags & FWA_CFG_DISTINCT_RANGE))
        return no("SLIDE / CUMULATE windows need FWA_CFG_DISTINCT_RANGE (a window of several slices needs the union of "
                  "their sets, which is not additive: the flag takes the count from the set at every fire)");
    const bool sess = u->window_kind == FWA_SESSION && (u->flags & FWA_CFG_DISTINCT_SESSION);
    if (u->window_kind != FWA_TUMBLE && !hop && !sess)
        return no("only TUMBLE windows, and SLIDE / CUMULATE under FWA_CFG_DISTINCT_RANGE (a window of several slices "
                  "needs the union of their sets, which is not additive); a Table SESSION window of a fixed gap takes "
                  "it under FWA_CFG_DISTINCT_SESSION");
    if (u->semantics != FWA_SEM_TABLE) return no("a Table aggregate (FWA_SEM_TABLE)");
    if (u->flags & FWA_CFG_REDUCE) return no("not a DataStream reduction");
    if (u->key_kind == FWA_KEY_PREHASHED)
        return no("PREHASHED keys are not supported (the set keeps no hash per entry to place it in a key group)");
    if (sess && u->allowed_lateness_ms > 0)
        return no("SESSION windows with allowed lateness are not supported (the cell bitmap is exact only when a "
                  "session's fire and its cleanup coincide)");
    if (sess && (u->flags & FWA_CFG_DYNAMIC_GAP))
        return no("SESSION windows with a per-record gap are not supported (the cells need one fixed gap)");
    // the marked column of aggregate j's source column (created on first use), and what SUM / AVG(DISTINCT) adds to it
    auto column_of = [&](int j) {
        const fwa_agg_spec& s = u->aggs[j];
        int d = -1;
        for (int i = 0; i < P->nd; ++i) if (P->src[i] == s.col) d = i;
        if (d < 0) { d = P->nd++; P->src[d] = s.col; P->sidx[d] = -1; }
        P->mask |= (int64_t)1 << j;
        if (!dist_is_sum(s.kind)) { P->cmask |= (int64_t)1 << j; return d; }
        if (P->sidx[d] < 0) { P->sidx[d] = P->ns++; P->sf64[d] = vtype[s.col] == 2; }
        P->fkind[j] = base[j];
        P->fd[j] = d;
        return d;
    };
    if (hop || sess) {
        // session mode: the same rewrite, so the handle keeps every session route; the marking pass runs behind the
        // ingest and needs its dropped-record indices on the device, which the internal configuration collects (the
        // caller's own flags decide what fwa_late_records and fwa_get_config answer)
        if (sess) {
            P->sess = true;
            P->gap = u->gap_ms;
            icfg->flags |= FWA_CFG_LATE_INDICES;
        }
        // range mode: a distinct aggregate -> COUNT(*), a BIGINT that is never NULL, shares column 0 and reads no value
        // column, so nothing is remapped and the handle keeps the two-phase ingest and the carried HOP sums; the fire
        // overwrites the column from the set (dist_range_count), sums go to plan-owned columns
        P->range = true;
        bool read[FWA_MAX_COLS] = {};
        for (int j = 0; j < u->num_aggs; ++j)
            if (u->aggs[j].kind != FWA_COUNT && !dist_is_kind(u->aggs[j].kind)) read[u->aggs[j].col] = true;
        for (int j = 0; j < u->num_aggs; ++j) {
            const fwa_agg_spec& s = u->aggs[j];
            if (!dist_is_kind(s.kind)) continue;
            column_of(j);
            icfg->aggs[j].kind = FWA_COUNT;
            icfg->aggs[j].col = 0;
            if (!read[s.col]) icfg->nullable_cols &= ~(1 << s.col);   // nothing else reads its NULL flags
        }
        return FWA_OK;
    }
    if (u->size_ms > 0 && u->size_ms < kDistMinSize) return no("windows shorter than 64 ms are not supported");
    // value-column indices: a source column that only distinct aggregates read hands its index to its marked column;
    // otherwise the marked column takes an index nothing else uses, and so does every summed column w
    bool used[FWA_MAX_COLS] = {}, isrc[FWA_MAX_COLS] = {};
    for (int j = 0; j < u->num_aggs; ++j) {
        const fwa_agg_spec& s = u->aggs[j];
        if (dist_is_kind(s.kind)) isrc[s.col] = true;
        else if (s.kind != FWA_COUNT) used[s.col] = true;     // COUNT(col) reads the column's NULL flags
    }
    int mof[FWA_MAX_COLS], wof[FWA_MAX_COLS];
    for (int c = 0; c < FWA_MAX_COLS; ++c) mof[c] = wof[c] = -1;
    for (int c = 0; c < FWA_MAX_COLS; ++c) if (isrc[c] && !used[c]) mof[c] = c;
    for (int c = 0; c < FWA_MAX_COLS; ++c) {
        if (!isrc[c] || mof[c] >= 0) continue;
        for (int m = 0; m < FWA_MAX_COLS && mof[c] < 0; ++m) {
            if (used[m] || isrc[m]) continue;
            mof[c] = m;
            used[m] = true;
        }
        if (mof[c] < 0) return no("no free value column for the marked column (FWA_MAX_COLS)");
    }
    for (int c = 0; c < FWA_MAX_COLS; ++c) {
        if (!vtype[c]) continue;
        for (int m = 0; m < FWA_MAX_COLS && wof[c] < 0; ++m) {
            if (used[m] || isrc[m]) continue;
            wof[c] = m;
            used[m] = true;
        }
        if (wof[c] < 0) return no("no free value column for the summed column of SUM / AVG(DISTINCT) (FWA_MAX_COLS)");
    }
    int cnt_of[FWA_MAX_AGGS];                                 // marked column d: the internal aggregate SUM_I64(m)
    for (int d = 0; d < FWA_MAX_AGGS; ++d) cnt_of[d] = -1;
    for (int j = 0; j < u->num_aggs; ++j) {
        const fwa_agg_spec& s = u->aggs[j];
        if (!dist_is_kind(s.kind)) continue;
        const int d = column_of(j);
        P->mcol[d] = mof[s.col];
        icfg->nullable_cols &= ~(1 << P->mcol[d]);            // the marked column holds no NULLs
        if (!dist_is_sum(s.kind)) {
            icfg->aggs[j].kind = FWA_SUM_I64;
            icfg->aggs[j].col = P->mcol[d];
            if (cnt_of[d] < 0) cnt_of[d] = j;
            continue;
        }
        P->wcol[d] = wof[s.col];
        icfg->nullable_cols &= ~(1 << P->wcol[d]);            // nor does w: a NULL or repeated value is the identity
        icfg->aggs[j].kind = P->sf64[d] ? FWA_SUM_F64 : FWA_SUM_I64;
        icfg->aggs[j].col = P->wcol[d];
        P->fsum[j] = j;
    }
    for (int d = 0; d < P->nd; ++d) {                         // the hidden counters, behind the caller's aggregates
        if (P->sidx[d] < 0 || cnt_of[d] >= 0) continue;
        if (icfg->num_aggs >= FWA_MAX_AGGS)
            return no("SUM / AVG(DISTINCT) needs one more aggregate for the hidden distinct count of its column, and "
                      "none of the FWA_MAX_AGGS is left");
        cnt_of[d] = icfg->num_aggs;
        icfg->aggs[icfg->num_aggs].kind = FWA_SUM_I64;
        icfg->aggs[icfg->num_aggs].col = P->mcol[d];
        icfg->num_aggs++;
    }
    for (int j = 0; j < u->num_aggs; ++j) if (P->fkind[j]) P->fcnt[j] = cnt_of[P->fd[j]];
    return FWA_OK;
}

void dist_free(DistinctPlan* P) {
    if (!P) return;
    for (void* p : {(void*)P->d_tab, (void*)P->d_mark, (void*)P->d_stage, (void*)P->d_ctr, (void*)P->d_side, (void*)P->d_bcnt,
                    (void*)P->d_bpre, (void*)P->d_rtab, (void*)P->d_wins, (void*)P->d_rsum, (void*)P->d_dmask,
                    (void*)P->d_rblk})
        if (p) (void)hipFree(p);
    for (int j = 0; j < FWA_MAX_AGGS; ++j) {
        if (P->d_fout[j]) (void)hipFree(P->d_fout[j]);
        if (P->d_fnull[j]) (void)hipFree(P->d_fnull[j]);
    }
    if (P->h_ctr) (void)hipHostFree(P->h_ctr);
    for (hipEvent_t ev : P->ev) if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : P->rev) if (ev) (void)hipEventDestroy(ev);
    delete P;
}

// First slice whose window has not fired at the handle's watermark (every lower slice drops its records), or
// LONG_MIN_J when that is not known cheaply: skipping lower slices only keeps garbage out of the set.
int64_t dist_qmin(const fwa_engine* e) {
    if (e->wm == LONG_MIN_J || (e->dist && e->dist->sess)) return LONG_MIN_J;   // (session mode: live = has bits)
    auto fired = [&](int64_t q) {
        int64_t thr;
        bool always;
        accept_threshold(e, q, &thr, &always);
        return !always && e->wm >= thr;
    };
    const int64_t lw = e->tz.empty() ? e->wm : jm::tz_to_local(e->tz.data(), (int)(e->tz.size() / 2), e->wm);
    int64_t q = slice_q(e, lw);
    if (e->dist && e->dist->range) {
        // a window of many slices: "fired" only ever turns off as q grows (the last window's end does not decrease), so
        // the first unfired slice of (q - slices per window - 66, q + 2] comes from a bisection; outside that: unknown
        const int64_t back = e->size / e->g + 66;
        if (q > LONG_MAX_J - 4 || q < LONG_MIN_J + back + 4) return LONG_MIN_J;
        int64_t lo = q - back, hi = q + 2;                    // fired(lo), !fired(hi)
        if (!fired(lo) || fired(hi)) return LONG_MIN_J;
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (fired(mid)) lo = mid; else hi = mid;
        }
        return hi;
    }
    if (q > LONG_MAX_J - 2 || q < LONG_MIN_J + 70) return LONG_MIN_J;
    q += 1;
    for (int step = 0; step < 64; ++step, --q) if (fired(q - 1)) return q;
    return LONG_MIN_J;
}

int dist_counters(fwa_engine* e) {
    DistinctPlan* P = e->dist;
    if (P->d_ctr) return FWA_OK;
    HIPCHK(e, hipMalloc(&P->d_ctr, 32));
    HIPCHK(e, hipHostMalloc((void**)&P->h_ctr, 32));
    memset(P->h_ctr, 0, 32);
    HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 32, e->stream));
    HIPCHK(e, hipMalloc(&P->d_bcnt, sizeof(unsigned int) * kDistScanGrid));
    HIPCHK(e, hipMalloc(&P->d_bpre, sizeof(unsigned long long) * kDistScanGrid));
    for (hipEvent_t& ev : P->ev) HIPCHK(e, hipEventCreate(&ev));
    if (P->range) for (hipEvent_t& ev : P->rev) HIPCHK(e, hipEventCreate(&ev));
    return FWA_OK;
}

// The live cut in the unit of the tag's slice field: q_min itself, or its block in range mode (a block is live while
// its highest slice is).
int64_t dist_cut(const DistinctPlan* P, int64_t q_min) { return P->range && q_min != LONG_MIN_J ? q_min >> 6 : q_min; }

// Read ctr[0] (and check ctr[1]) after the work enqueued so far; synchronises.
int dist_read_counter(fwa_engine* e, int64_t* out) {
    DistinctPlan* P = e->dist;
    HIPCHK(e, hipMemcpyAsync(P->h_ctr, P->d_ctr, 16, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (P->h_ctr[1]) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) set overflowed its bound");
    *out = (int64_t)P->h_ctr[0];
    return FWA_OK;
}

int64_t dist_pow2(int64_t x) {
    int64_t p = 64;
    while (p < x) p <<= 1;
    return p;
}

// The entries of windows that have not fired at the handle's watermark (and, per scan block, in d_bcnt); synchronises.
int dist_count_live(fwa_engine* e, int64_t q_min, int grid, int64_t* livee) {
    DistinctPlan* P = e->dist;
    HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 8, e->stream));
    if (P->range) distinct_count_kernel<true><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, P->d_ctr, P->d_bcnt);
    else distinct_count_kernel<false><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, P->d_ctr, P->d_bcnt);
    HIPCHK(e, hipGetLastError());
    return dist_read_counter(e, livee);
}

// In-place rebuild after dist_count_live: the live entries through the side buffer (which keeps them, [3][side_cap],
// for the snapshot to read), every other slot cleared.
int dist_compact(fwa_engine* e, int64_t q_min, int grid, int64_t livee) {
    DistinctPlan* P = e->dist;
    if (livee > P->side_cap) {
        if (P->d_side) HIPCHK(e, hipFree(P->d_side));
        P->d_side = nullptr;
        P->side_cap = 0;
        const int64_t cap = std::max<int64_t>(livee + livee / 4, 1 << 12);
        HIPCHK(e, hipMalloc(&P->d_side, (P->range ? 32 : 24) * (size_t)cap));
        P->side_cap = cap;
    }
    int64_t taken = 0, moved = 0;
    HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 8, e->stream));
    distinct_prefix_kernel<<<1, 64, 0, e->stream>>>(P->d_bcnt, grid, P->d_bpre);
    HIPCHK(e, hipGetLastError());
    if (P->range)
        distinct_extract_kernel<true><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, P->d_side, P->side_cap,
                                                                   P->d_bpre, P->d_ctr);
    else
        distinct_extract_kernel<false><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, P->d_side, P->side_cap,
                                                                    P->d_bpre, P->d_ctr);
    HIPCHK(e, hipGetLastError());
    if (int rc = dist_read_counter(e, &taken)) return rc;
    if (taken != livee) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) rebuild lost entries");
    if (taken > 0) {
        HIPCHK(e, hipMemsetAsync(P->d_ctr, 0, 8, e->stream));
        if (P->range)
            distinct_insert_side_kernel<true><<<grid_for(taken, 4096), 256, 0, e->stream>>>(
                P->d_side, P->side_cap, taken, P->d_tab, (uint64_t)P->slots - 1, P->d_ctr);
        else
            distinct_insert_side_kernel<false><<<grid_for(taken, 4096), 256, 0, e->stream>>>(
                P->d_side, P->side_cap, taken, P->d_tab, (uint64_t)P->slots - 1, P->d_ctr);
        HIPCHK(e, hipGetLastError());
        if (int rc = dist_read_counter(e, &moved)) return rc;
        if (moved != livee) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) rebuild lost entries");
    }
    P->live = livee;
    P->rebuilds++;
    return FWA_OK;
}

// Make room for `add` more inserts: bound + add <= slots / 2, rebuilding the table from its live entries otherwise.
int dist_reserve(fwa_engine* e, int64_t add) {
    DistinctPlan* P = e->dist;
    if (int rc = dist_counters(e)) return rc;
    if (!P->d_tab) {
        P->slots = P->first_slots > 0 ? P->first_slots : dist_pow2(std::max<int64_t>(2 * add, kDistMinSlots));
        HIPCHK(e, hipMalloc(&P->d_tab, 32 * (size_t)P->slots));
        HIPCHK(e, hipMemsetAsync(P->d_tab, 0, 32 * (size_t)P->slots, e->stream));
        P->bound = 0;
    }
    if (P->last_add) {   // the last marking pass's exact count (its copy was enqueued behind it) replaces its estimate
        HIPCHK(e, hipEventSynchronize(P->ev[2]));
        const int64_t made = (int64_t)P->h_ctr[2];
        if (made >= 0 && made <= P->last_add) P->bound -= P->last_add - made;
        P->last_add = 0;
    }
    if (P->bound + add <= P->slots / 2) { P->bound += add; return FWA_OK; }
    const int64_t q_min = dist_cut(P, dist_qmin(e));          // (range mode: the cut is a block number)
    const int grid = grid_for(P->slots, kDistScanGrid);
    int64_t livee = 0;
    if (int rc = dist_count_live(e, q_min, grid, &livee)) return rc;
    const int64_t nslots = dist_pow2(std::max<int64_t>(2 * (livee + add), 64));
    if (nslots == P->slots) {   // same size: in place, through the side buffer
        if (int rc = dist_compact(e, q_min, grid, livee)) return rc;
        P->bound = livee + add;
        return FWA_OK;
    }
    unsigned long long* ntab = nullptr;
    HIPCHK(e, hipMalloc(&ntab, 32 * (size_t)nslots));
    hipError_t r = hipMemsetAsync(ntab, 0, 32 * (size_t)nslots, e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(P->d_ctr, 0, 8, e->stream);
    if (r == hipSuccess) {
        if (P->range)
            distinct_rebuild_kernel<true><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, ntab,
                                                                       (uint64_t)nslots - 1, P->d_ctr);
        else
            distinct_rebuild_kernel<false><<<grid, 256, 0, e->stream>>>(P->d_tab, P->slots, q_min, ntab,
                                                                        (uint64_t)nslots - 1, P->d_ctr);
        r = hipGetLastError();
    }
    int64_t moved = 0;
    int rc = r == hipSuccess ? dist_read_counter(e, &moved) : fail(e, FWA_E_DEVICE, hipGetErrorString(r));
    if (rc || moved != livee) {
        (void)hipFree(ntab);
        return rc ? rc : fail(e, FWA_E_STATE, "COUNT(DISTINCT) rebuild lost entries");
    }
    HIPCHK(e, hipFree(P->d_tab));
    P->d_tab = ntab;
    P->slots = nslots;
    P->live = moved;
    P->bound = moved + add;
    P->rebuilds++;
    return FWA_OK;
}

// The marking pass's device time, once its events completed, goes to ingest_ms (like the index column of reductions).
void dist_collect_timing(fwa_engine* e) {
    DistinctPlan* P = e->dist;
    if (!P || !P->timing || hipEventQuery(P->ev[1]) != hipSuccess) return;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, P->ev[0], P->ev[1]) == hipSuccess) e->ingest_ms += ms;
    P->timing = false;
}

size_t dist_in_width(int kind) { return is_dec_kind(kind) ? (size_t)dec_width(kind) : type_size(kind); }

// Mark the batch. On return *keys / *ts, vals[] and nulls[] are device pointers laid out for the internal
// configuration (the marked columns at their indices); host inputs are staged once, here.
int dist_mark(fwa_engine* e, const int64_t** keys, const int64_t** ts, const void* const* val_cols,
              const uint8_t* const* null_cols, int64_t n, bool device, const void** vals, const uint8_t** nulls) {
    DistinctPlan* P = e->dist;
    const fwa_config& u = P->ucfg;
    dist_collect_timing(e);
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
    if (!P->range && n > P->mark_cap) {
        if (P->d_mark) HIPCHK(e, hipFree(P->d_mark));
        P->d_mark = nullptr;
        P->mark_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 1 << 16);
        HIPCHK(e, hipMalloc(&P->d_mark, sizeof(unsigned long long) * (size_t)cap * (size_t)(P->nd + P->ns)));
        P->mark_cap = cap;
    }
    if (int rc = dist_reserve(e, n * P->nd)) return rc;
    DistMarkArgs a;
    memset(&a, 0, sizeof(a));
    a.keys = *keys;
    a.ts = *ts;
    a.nd = P->nd;
    a.n = n;
    a.q_min = dist_qmin(e);
    a.tab = P->d_tab;
    a.smask = (uint64_t)P->slots - 1;
    a.ctr = P->d_ctr;
    for (int d = 0; d < P->nd; ++d) {
        a.src[d] = (const int64_t*)vals[P->src[d]];
        a.nul[d] = nulls[P->src[d]];
        a.mark[d] = P->range ? nullptr : P->d_mark + (size_t)d * (size_t)P->mark_cap;
        a.wsum[d] = P->range || P->sidx[d] < 0 ? nullptr : P->d_mark + (size_t)(P->nd + P->sidx[d]) * (size_t)P->mark_cap;
    }
    if (P->sess) {   // the pass runs behind the ingest (dist_mark_session): the room is reserved, the columns are held
        P->hold.keys = a.keys;
        P->hold.ts = a.ts;
        for (int d = 0; d < P->nd; ++d) { P->hold.src[d] = a.src[d]; P->hold.nul[d] = a.nul[d]; }
        P->hold.n = n;
    }
    if (!P->sess) {
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 2, 0, 8, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[0], e->stream));
    if (P->range) distinct_mark_range_kernel<<<grid_for(n, 1 << 16), 256, 0, e->stream>>>(a, e->d_ec);
    else if (P->ns) distinct_mark_kernel<true><<<grid_for(n, 1 << 16), 256, 0, e->stream>>>(a, e->d_ec);
    else distinct_mark_kernel<false><<<grid_for(n, 1 << 16), 256, 0, e->stream>>>(a, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->ev[1], e->stream));
    P->timing = true;
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 2, P->d_ctr + 2, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[2], e->stream));
    P->last_add = n * P->nd;
    }
    // the internal layout: a source column that only distinct aggregates read is not passed on (its index may now hold
    // its marked column, or a DECIMAL piece); NULL flags only where the internal configuration still declares them
    for (int d = 0; d < P->nd; ++d) {
        bool other = false;
        for (int j = 0; j < u.num_aggs; ++j)
            other |= u.aggs[j].kind != FWA_COUNT && !dist_is_kind(u.aggs[j].kind) && u.aggs[j].col == P->src[d];
        if (!other) vals[P->src[d]] = nullptr;
    }
    for (int d = 0; d < P->nd && !P->range; ++d) {
        vals[P->mcol[d]] = a.mark[d];
        if (a.wsum[d]) vals[P->wcol[d]] = a.wsum[d];
    }
    for (int c = 0; c < FWA_MAX_COLS; ++c) if (!((e->cfg.nullable_cols >> c) & 1)) nulls[c] = nullptr;
    return FWA_OK;
}

// Session mode: the marking pass of the push the ingest just settled (ok) -- or nothing, with the reserved room given
// back, when the ingest refused the push. The set's bound was checked by dist_mark ahead of the ingest; the created
// count comes back here, inside the call (the pass reads the caller's columns, so the call waits for it).
int dist_mark_session(fwa_engine* e, bool ok) {
    DistinctPlan* P = e->dist;
    const int64_t n = P->hold.n;
    if (n <= 0) return FWA_OK;
    P->hold.n = 0;
    const int64_t add = n * P->nd;
    if (!ok) { P->bound -= std::min(P->bound, add); return FWA_OK; }
    if (!e->d_dropidx || e->dropidx_cap < n) return fail(e, FWA_E_STATE, "COUNT(DISTINCT): the push kept no dropped-record list");
    if (n > P->dmask_cap) {
        if (P->d_dmask) HIPCHK(e, hipFree(P->d_dmask));
        P->d_dmask = nullptr;
        P->dmask_cap = 0;
        const int64_t cap = std::max<int64_t>(n, 1 << 16);
        HIPCHK(e, hipMalloc(&P->d_dmask, (size_t)cap));
        P->dmask_cap = cap;
    }
    DistMarkArgs a;
    memset(&a, 0, sizeof(a));
    a.keys = P->hold.keys;
    a.ts = P->hold.ts;
    a.nd = P->nd;
    a.n = n;
    a.tab = P->d_tab;
    a.smask = (uint64_t)P->slots - 1;
    a.ctr = P->d_ctr;
    a.dmask = P->d_dmask;
    a.gap = P->gap;
    for (int d = 0; d < P->nd; ++d) { a.src[d] = P->hold.src[d]; a.nul[d] = P->hold.nul[d]; }
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 1, 0, 16, e->stream));
    HIPCHK(e, hipMemsetAsync(P->d_dmask, 0, (size_t)n, e->stream));
    HIPCHK(e, hipEventRecord(P->ev[0], e->stream));
    dist_drop_mask_kernel<<<grid_for(n, 1 << 10), 256, 0, e->stream>>>(e->d_dropidx, &e->d_st->drop_n, n, P->d_dmask);
    HIPCHK(e, hipGetLastError());
    distinct_mark_session_kernel<<<grid_for(n, 1 << 16), 256, 0, e->stream>>>(a, e->d_ec);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->ev[1], e->stream));
    P->timing = true;
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 1, P->d_ctr + 1, 16, hipMemcpyDeviceToHost, e->stream));
    if (int rc = stream_sync(e)) return rc;
    if (P->h_ctr[1]) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) set overflowed its bound");
    const int64_t made = (int64_t)P->h_ctr[2];
    if (made >= 0 && made <= add) P->bound -= add - made;
    dist_collect_timing(e);
    return FWA_OK;
}

// What the fire-time passes of range and session mode share: the set, the step's rows, the output column of every
// COUNT_DISTINCT aggregate and the plan-owned per-row sums (grown here) of every summed column.
int dist_fire_args(fwa_engine* e, int64_t row0, int64_t nrows, DistRangeArgs* ap) {
    DistinctPlan* P = e->dist;
    DistRangeArgs& a = *ap;
    if (P->ns && row0 + nrows > P->rs_cap) {
        if (P->d_rsum) HIPCHK(e, hipFree(P->d_rsum));
        P->d_rsum = nullptr;
        P->rs_cap = 0;
        const int64_t cap = std::max<int64_t>(row0 + nrows + nrows / 4, 1 << 12);
        HIPCHK(e, hipMalloc(&P->d_rsum, 16 * (size_t)cap * (size_t)P->ns));
        P->rs_cap = cap;
    }
    a.tab = P->d_tab;
    a.slots = P->slots;
    a.smask = (uint64_t)P->slots - 1;
    a.o_key = e->o_key;
    a.o_end = e->o_end;
    a.row0 = row0;
    a.nrows = nrows;
    a.ctr = P->d_ctr;
    for (int j = 0; j < P->ucfg.num_aggs; ++j) {
        if (!((P->cmask >> j) & 1)) continue;
        const int oj = e->dec ? e->dec->umap[j] : j;       // (a DECIMAL plan renumbers the internal aggregates)
        if (oj < 0) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) aggregate has no output column");
        for (int d = 0; d < P->nd; ++d) if (P->src[d] == P->ucfg.aggs[j].col) a.agg_d[a.na] = d;
        a.o_agg[a.na++] = (unsigned long long*)e->o_agg[oj];
    }
    for (int d = 0; d < P->nd; ++d) {
        if (P->sidx[d] < 0) continue;
        const int s = P->sidx[d];
        a.sum_d[s] = d;
        a.sum_f64[s] = P->sf64[d];
        a.r_sum[s] = P->d_rsum + (size_t)s * (size_t)P->rs_cap;
        a.r_cnt[s] = P->d_rsum + (size_t)(P->ns + s) * (size_t)P->rs_cap;
    }
    a.ns = P->ns;
    return FWA_OK;
}

// Range mode: the distinct columns of the rows [row0, row0 + nrows) that a watermark step just fired for `wins`
// ((end, start) as fwa_advance_watermark collects them; both fire paths emit these bounds unchanged). Enqueued on the
// handle's stream behind the fire and ahead of anything a later push sets; synchronises before the rows are read.
int dist_range_count(fwa_engine* e, const std::set<std::pair<int64_t, int64_t>>& wins, int64_t row0, int64_t nrows) {
    DistinctPlan* P = e->dist;
    if (nrows <= 0 || wins.empty()) return FWA_OK;
    if (nrows >= (int64_t)1 << 31) return fail(e, FWA_E_STATE, "COUNT(DISTINCT): too many rows in one firing step");
    if (int rc = dist_counters(e)) return rc;
    std::vector<DistWin> hw;
    hw.reserve(wins.size());
    for (auto& w : wins) hw.push_back({slice_q(e, w.second), slice_q(e, jm::wsub(w.first, 1)), w.first});
    if ((int64_t)hw.size() > P->wins_cap) {
        if (P->d_wins) HIPCHK(e, hipFree(P->d_wins));
        P->d_wins = nullptr;
        P->wins_cap = 0;
        const int64_t cap = std::max<int64_t>(2 * (int64_t)hw.size(), 64);
        HIPCHK(e, hipMalloc(&P->d_wins, sizeof(DistWin) * (size_t)cap));
        P->wins_cap = cap;
    }
    const int64_t rcap = dist_pow2(2 * nrows);
    if (rcap > P->rtab_cap) {
        if (P->d_rtab) HIPCHK(e, hipFree(P->d_rtab));
        P->d_rtab = nullptr;
        P->rtab_cap = 0;
        HIPCHK(e, hipMalloc(&P->d_rtab, sizeof(unsigned int) * (size_t)rcap));
        P->rtab_cap = rcap;
    }
    if (int rc = upload(e, P->d_wins, hw.data(), sizeof(DistWin) * hw.size())) return rc;
    DistRangeArgs a;
    memset(&a, 0, sizeof(a));
    a.wins = P->d_wins;
    a.nw = (int32_t)hw.size();
    a.rtab = P->d_rtab;
    a.rmask = (uint32_t)(rcap - 1);
    if (int rc = dist_fire_args(e, row0, nrows, &a)) return rc;
    HIPCHK(e, hipMemsetAsync(P->d_rtab, 0, sizeof(unsigned int) * (size_t)rcap, e->stream));
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 3, 0, 8, e->stream));
    HIPCHK(e, hipEventRecord(P->rev[0], e->stream));
    dist_rows_index_kernel<<<grid_for(nrows, (int64_t)1 << 23), 256, 0, e->stream>>>(a);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->rev[1], e->stream));
    if (P->d_tab) {   // (no table: nothing but NULLs was ever pushed, every count stays 0)
        if (P->ns) dist_range_count_kernel<true><<<grid_for(P->slots, kDistScanGrid), 256, 0, e->stream>>>(a);
        else dist_range_count_kernel<false><<<grid_for(P->slots, kDistScanGrid), 256, 0, e->stream>>>(a);
        HIPCHK(e, hipGetLastError());
    }
    HIPCHK(e, hipEventRecord(P->rev[2], e->stream));
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 3, P->d_ctr + 3, 8, hipMemcpyDeviceToHost, e->stream));
    if (int rc = stream_sync(e)) return rc;
    if (P->h_ctr[3]) return fail(e, FWA_E_STATE, "COUNT(DISTINCT): a counted value's (key, window) has no fired row");
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms0, P->rev[0], P->rev[1]));
    HIPCHK(e, hipEventElapsedTime(&ms1, P->rev[1], P->rev[2]));
    P->index_ms += ms0;
    P->count_ms += ms1;
    P->count_steps++;
    e->fire_ms += ms0 + ms1;
    return FWA_OK;
}

// Session mode: the distinct columns of the rows [0, nrows) that fire_sessions just emitted (o_start / o_end are local
// times), then the clear of their bits. On the handle's stream behind the fire, before the rows are handed out and
// before any later push; synchronises. A step that fired nothing launches nothing.
int dist_session_count(fwa_engine* e, int64_t nrows) {
    DistinctPlan* P = e->dist;
    if (nrows <= 0) return FWA_OK;
    if (nrows >= (int64_t)1 << 31) return fail(e, FWA_E_STATE, "COUNT(DISTINCT): too many rows in one firing step");
    if (int rc = dist_counters(e)) return rc;
    DistRangeArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = dist_fire_args(e, 0, nrows, &a)) return rc;
    a.o_start = e->o_start;
    a.gap = P->gap;
    a.tabw = P->d_tab;
    const unsigned rgrid = (unsigned)((nrows + 255) / 256);
    // the multimap's size: the blocks the rows touch, summed on the device
    HIPCHK(e, hipMemsetAsync(P->d_ctr + 3, 0, 8, e->stream));
    HIPCHK(e, hipEventRecord(P->rev[0], e->stream));
    dist_sess_blocks_kernel<<<rgrid, 256, 0, e->stream>>>(a);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(P->h_ctr + 3, P->d_ctr + 3, 8, hipMemcpyDeviceToHost, e->stream));
    if (int rc = stream_sync(e)) return rc;
    const int64_t nblk = (int64_t)P->h_ctr[3];
    if (nblk < nrows || nblk >= (int64_t)1 << 30)
        return fail(e, FWA_E_STATE, "COUNT(DISTINCT): the fired sessions span too many 64-cell blocks for one step");
    const int64_t rcap = dist_pow2(2 * nblk);
    if (rcap > P->rtab_cap) {
        if (P->d_rtab) HIPCHK(e, hipFree(P->d_rtab));
        if (P->d_rblk) HIPCHK(e, hipFree(P->d_rblk));
        P->d_rtab = nullptr;
        P->d_rblk = nullptr;
        P->rtab_cap = 0;
        HIPCHK(e, hipMalloc(&P->d_rtab, sizeof(unsigned int) * (size_t)rcap));
        HIPCHK(e, hipMalloc(&P->d_rblk, sizeof(int64_t) * (size_t)rcap));
        P->rtab_cap = rcap;
    }
    a.rtab = P->d_rtab;
    a.rblk = P->d_rblk;
    a.rmask = (uint32_t)(rcap - 1);
    HIPCHK(e, hipMemsetAsync(P->d_rtab, 0, sizeof(unsigned int) * (size_t)rcap, e->stream));
    dist_sess_index_kernel<<<rgrid, 256, 0, e->stream>>>(a);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipEventRecord(P->rev[1], e->stream));
    if (P->d_tab) {   // (no table: nothing but NULLs was ever pushed, every count stays 0)
        const int grid = grid_for(P->slots, kDistScanGrid);
        if (P->ns) dist_sess_count_kernel<true><<<grid, 256, 0, e->stream>>>(a);
        else dist_sess_count_kernel<false><<<grid, 256, 0, e->stream>>>(a);
        HIPCHK(e, hipGetLastError());
        dist_sess_clear_kernel<<<grid, 256, 0, e->stream>>>(a);
        HIPCHK(e, hipGetLastError());
    }
    HIPCHK(e, hipEventRecord(P->rev[2], e->stream));
    if (int rc = stream_sync(e)) return rc;
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms0, P->rev[0], P->rev[1]));
    HIPCHK(e, hipEventElapsedTime(&ms1, P->rev[1], P->rev[2]));
    P->index_ms += ms0;
    P->count_ms += ms1;
    P->count_steps++;
    e->fire_ms += ms0 + ms1;
    return FWA_OK;
}

// SUM / AVG(DISTINCT): the caller-visible columns of the nrows fired rows into P->d_fout / d_fnull, from the internal
// sums as fired (TUMBLE: the accumulators of w and m; range mode: the per-row columns of the step's count pass). The
// inputs are left as they are, so fill_out may run again over the same rows. Synchronises.
int dist_finish(fwa_engine* e, int64_t nrows) {
    DistinctPlan* P = e->dist;
    if (!P->ns) return FWA_OK;
    if (nrows > P->fout_cap || !P->fout_cap) {
        const int64_t cap = std::max<int64_t>(nrows + nrows / 4, 1 << 12);
        for (int j = 0; j < P->ucfg.num_aggs; ++j) {
            if (!P->fkind[j]) continue;
            if (P->d_fout[j]) HIPCHK(e, hipFree(P->d_fout[j]));
            if (P->d_fnull[j]) HIPCHK(e, hipFree(P->d_fnull[j]));
            P->d_fout[j] = nullptr;
            P->d_fnull[j] = nullptr;
            HIPCHK(e, hipMalloc(&P->d_fout[j], 8 * (size_t)cap));
            HIPCHK(e, hipMalloc(&P->d_fnull[j], (size_t)cap));
        }
        P->fout_cap = cap;
    }
    if (nrows == 0) return FWA_OK;
    if (P->range && nrows > P->rs_cap) return fail(e, FWA_E_STATE, "SUM(DISTINCT): fired rows without a count pass");
    DistFinArgs f;
    memset(&f, 0, sizeof(f));
    f.n = nrows;
    for (int j = 0; j < P->ucfg.num_aggs; ++j) {
        if (!P->fkind[j]) continue;
        DistFinDesc& d = f.a[f.na++];
        if (P->range) {
            const int s = P->sidx[P->fd[j]];
            d.sum = P->d_rsum + (size_t)s * (size_t)P->rs_cap;
            d.cnt = P->d_rsum + (size_t)(P->ns + s) * (size_t)P->rs_cap;
        } else {                                           // (a DECIMAL plan renumbers the internal aggregates)
            const int is = e->dec ? e->dec->umap[P->fsum[j]] : P->fsum[j];
            const int ic = e->dec ? e->dec->umap[P->fcnt[j]] : P->fcnt[j];
            if (is < 0 || ic < 0) return fail(e, FWA_E_STATE, "SUM(DISTINCT) aggregate has no output column");
            d.sum = (const unsigned long long*)e->o_agg[is];
            d.cnt = (const unsigned long long*)e->o_agg[ic];
        }
        d.out = P->d_fout[j];
        d.nul = P->d_fnull[j];
        d.kind = P->fkind[j];
    }
    dist_finish_kernel<<<dim3((unsigned)((nrows + 255) / 256), (unsigned)f.na), 256, 0, e->stream>>>(f);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return FWA_OK;
}

// ---- engine snapshot / restore: the set's live entries as a section behind the FWASNAP1 body ----
// off[max_parallelism + 1], then key[m], value[m], slice_start[m], column[m] (the marked column's ordinal: the
// distinct source columns in first-use order), bucketed by key group like the body.
int dist_snapshot_section(fwa_engine* e, std::vector<int64_t>* sec, int64_t* m_out) {
    DistinctPlan* P = e->dist;
    const int maxp = e->cfg.max_parallelism;
    // the live entries come out of an in-place rebuild (its side buffer keeps them): the copy to the host and the
    // host's memory are bounded by the live count, not by the table
    int64_t m = 0;
    std::vector<unsigned long long> w;
    std::vector<int64_t> qs;                              // range mode: the slice number of entry i
    if (P->d_tab) {
        if (int rc = dist_counters(e)) return rc;
        const int64_t q_live = dist_qmin(e);
        const int64_t q_min = dist_cut(P, q_live);
        const int grid = grid_for(P->slots, kDistScanGrid);
        if (int rc = dist_count_live(e, q_min, grid, &m)) return rc;
        if (int rc = dist_compact(e, q_min, grid, m)) return rc;
        P->bound = m;                                     // exact now: the pending estimate of the last push is void
        P->last_add = 0;
        const int nw = P->range ? 4 : 3;
        w.resize((size_t)nw * (size_t)m);
        for (int c = 0; c < nw && m > 0; ++c)
            HIPCHK(e, hipMemcpy(w.data() + (size_t)c * m, P->d_side + (size_t)c * P->side_cap, 8 * (size_t)m,
                                hipMemcpyDeviceToHost));
        if (P->range) {
            // one section entry per set bit of a live block, its slice's number in qs[]; the bits of slices under
            // q_live belong to fired windows only and stay behind
            std::vector<unsigned long long> x[3];
            const int64_t mb = m;
            for (int64_t i = 0; i < mb; ++i) {
                const int64_t b0 = (int64_t)((uint64_t)dist_tag_q(w[2 * mb + i]) << 6);
                for (unsigned long long bits = w[3 * mb + i]; bits; bits &= bits - 1) {
                    const int64_t q = b0 + __builtin_ctzll(bits);
                    if (q < q_live) continue;
                    for (int c = 0; c < 3; ++c) x[c].push_back(w[(size_t)c * mb + i]);
                    qs.push_back(q);
                }
            }
            m = (int64_t)qs.size();
            w.resize(3 * (size_t)m);
            for (int c = 0; c < 3 && m > 0; ++c) memcpy(w.data() + (size_t)c * m, x[c].data(), 8 * (size_t)m);
        }
    }
    std::vector<int32_t> kg((size_t)m);
    std::vector<int64_t> off((size_t)maxp + 1, 0);
    for (int64_t i = 0; i < m; ++i) {
        const uint64_t t = w[2 * m + i];
        const int64_t key = (t & 8) ? 0 : (int64_t)w[i];
        kg[i] = jm::key_group_of(key, e->cfg.key_kind, 0, maxp);
        if (kg[i] < 0) return fail(e, FWA_E_STATE, "COUNT(DISTINCT) set holds a key outside every key group");
        off[kg[i] + 1]++;
    }
    for (int g = 0; g < maxp; ++g) off[g + 1] += off[g];
    sec->assign((size_t)maxp + 1 + 4 * (size_t)m, 0);
    memcpy(sec->data(), off.data(), 8 * ((size_t)maxp + 1));
    int64_t* body = sec->data() + maxp + 1;
    std::vector<int64_t> cur(off.begin(), off.end() - 1);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t d = cur[kg[i]]++;
        const uint64_t t = w[2 * m + i];
        body[d] = (t & 8) ? 0 : (int64_t)w[i];
        body[m + d] = (t & 16) ? 0 : (int64_t)w[m + i];
        body[2 * m + d] = P->sess ? (int64_t)((uint64_t)qs[i] * (uint64_t)P->gap)   // the cell's start, local time
                                  : slice_start(e, P->range ? qs[i] : dist_tag_q(t));
        body[3 * m + d] = (int64_t)(t & 7);
    }
    *m_out = m;
    return FWA_OK;
}

// Insert the entries of this handle's key groups from one blob's section (no marking).
int dist_restore_section(fwa_engine* e, const int64_t* sec, int64_t m) {
    DistinctPlan* P = e->dist;
    const int maxp = e->cfg.max_parallelism;
    const int64_t lo = sec[e->cfg.kg_start], hi = sec[e->cfg.kg_end + 1];
    if (lo < 0 || hi < lo || hi > m) return fail(e, FWA_E_ARG, "corrupt COUNT(DISTINCT) key-group offsets");
    const int64_t n = hi - lo;
    if (n == 0) return FWA_OK;
    const int64_t* body = sec + maxp + 1;
    const size_t nw = P->range ? 4 : 3;                   // range mode: block tag + the slice's bit, folded by the insert
    std::vector<unsigned long long> w(nw * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = (uint64_t)body[lo + i], val = (uint64_t)body[m + lo + i];
        const int64_t d = body[3 * m + lo + i];
        if (d < 0 || d >= P->nd) return fail(e, FWA_E_ARG, "corrupt COUNT(DISTINCT) entry");
        const int64_t q = P->sess ? dist_cell(body[2 * m + lo + i], P->gap) : slice_q(e, body[2 * m + lo + i]);
        w[i] = key ? key : 1ull;
        w[n + i] = val ? val : 1ull;
        w[2 * n + i] = dist_tag(P->range ? q >> 6 : q, key, val, (int)d);
        if (P->range) w[3 * n + i] = 1ull << (q & 63);
    }
    if (int rc = dist_reserve(e, n)) return rc;
    unsigned long long* dw = nullptr;
    HIPCHK(e, hipMalloc(&dw, 8 * nw * (size_t)n));
    hipError_t r = hipMemcpyAsync(dw, w.data(), 8 * nw * (size_t)n, hipMemcpyHostToDevice, e->stream);
    if (r == hipSuccess) {
        if (P->range)
            distinct_insert_side_kernel<true><<<grid_for(n), 256, 0, e->stream>>>(dw, n, n, P->d_tab,
                                                                                  (uint64_t)P->slots - 1, P->d_ctr);
        else
            distinct_insert_side_kernel<false><<<grid_for(n), 256, 0, e->stream>>>(dw, n, n, P->d_tab,
                                                                                   (uint64_t)P->slots - 1, P->d_ctr);
        r = hipGetLastError();
    }
    const hipError_t rs = hipStreamSynchronize(e->stream);
    (void)hipFree(dw);
    if (r != hipSuccess || rs != hipSuccess) return fail(e, FWA_E_DEVICE, "COUNT(DISTINCT) restore failed");
    return FWA_OK;
}

}  // namespace
