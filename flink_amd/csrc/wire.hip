// wire.hip -- GPU decoder of Flink's network wire format behind include/flink_amd_wire.h.
//
// Input: the data-buffer payloads of one channel, concatenated (an element may span buffers, as in
// SpillingAdaptiveSpanningRecordDeserializer.java:88-131). Each element is a 4-byte big-endian length L
// followed by L bytes: the StreamElementSerializer tag and body (StreamElementSerializer.java:158-211,
// framed by RecordWriter.serializeRecord :145-157). Element boundaries are a sequential chain, so the decoder
// splits the bytes into 4 KiB chunks and runs three steps, all on the GPU:
//
//   scan    : per chunk, for EVERY candidate entry offset e in [0, S) (S = longest element + 4, so the first
//             element starting in a chunk is always one of them) walk the chain through the chunk in LDS and
//             record where it leaves (entry offset into the next chunk), END (stream ends / partial element)
//             or CORRUPT (tag / length mismatch), plus the records and events it passed: a map e -> exit.
//   compose : the maps of 64 consecutive chunks are composed in LDS (function composition is associative),
//             level by level, until one map covers the stream; its value at e = 0 is the whole call's count.
//   resolve : back down the levels, every chunk learns its true entry offset and the global record / event
//             index of its first element; chunks past the END are marked dead.
//   decode  : per chunk, one lane walks the true chain in LDS to list the element starts, then the wave
//             decodes the elements in parallel into SoA columns (key, ts, value columns, NULL flags) and an
//             event list (watermark / status / latency marker / record attributes) with record positions.
//
// Rows with STRING fields (FWA_FIELD_STRING) make records of varying length: the kernels are instantiated a second
// time (VAR) in which a record header is valid when its length is in range and equals the row's own size int, the
// walk falls back to listed scalar steps when consecutive elements differ in size, and the decode pass writes, per
// STRING field, the length, NULL flag and input byte offset of every record's value. fwa_wire_strings_of turns those
// into Arrow-style offsets (device scan) and bytes (gather from the still-resident wire bytes) on demand. The
// fixed-length instantiation is the code as it was.
//
// Rows with non-compact DECIMAL fields (FWA_FIELD_DECIMAL) vary in length too (16 reserved bytes per non-NULL one, or
// per field in the writeDecimal(null) form) and take the VAR scan; their decode pass is a third instantiation (DEC),
// in which the record's lane checks each DECIMAL column's slot against the row, assembles the big-endian bytes in LDS
// and stores the sign-extended 128-bit value with one 16-byte store. Schemas without one run the kernels they ran.
//
// TUPLE values with java.lang.String fields (FWA_FIELD_JSTRING: StringSerializer -> StringValue.writeString, len + 1 as
// a varint, then every UTF-16 code unit as a varint of 1..3 bytes; null is 00) vary in length as well and are a third
// instantiation (JS) of scan and decode: a record header is valid on its length alone (a weak filter, and a sound one:
// see element_at), and the decode pass walks the fields with a running cursor, checks each String's canonical form and
// writes the same per-record length / NULL flag / byte offset arrays as the STRING path, so fwa_wire_strings_of serves
// both. A value is handed on as its char bytes as they stand on the wire. fwa_jstring_hash is String.hashCode() over
// those bytes. The two instantiations above are the code as it was.
//
// HBM traffic: the wire bytes are read twice (scan, decode), the maps are S x 4 B per 4 KiB chunk, the
// columns are written once. Bound: HBM (wire decoder).
//
// The sender side (fwa_wire_encode: fired rows written as channel bytes) is wire_encode.inc, included at the end.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flink_amd_wire.h"

namespace {

constexpr int kChunk = 4096;            // bytes per chunk
constexpr int kMaxStep = 253;           // S limit: entry offsets < S must fit a byte next to two status codes
constexpr uint32_t kMaxBody = kMaxStep - 4;   // longest element body (the length prefix's value)
constexpr int kNone = 9;                // scan: no candidate at this lane (past S, or already settled)
constexpr uint32_t kNxtEnd = 0xFE;      // chain ends inside the chunk (stream end or partial element)
constexpr uint32_t kNxtCorrupt = 0xFF;  // chain hits a malformed element
constexpr uint32_t kDead = 0xFF;        // resolve: chunk lies after the stream's END (nothing to decode)
constexpr int kLdsBudget = 60 * 1024;   // compose / resolve LDS per block
constexpr int64_t kPersistBlocks = 256 * 24;   // scan / decode: persistent single-wave blocks (24 per CU)

// Per-schema constants (kernel argument, copied by value).
struct WireConst {
    int32_t body[6];                   // element body length per tag (the 4-byte length prefix must equal it)
    int32_t step;                      // S
    int32_t format, arity;
    int32_t ftype[FWA_WIRE_MAX_FIELDS];
    int32_t foff[FWA_WIRE_MAX_FIELDS]; // TUPLE: offset of the field in the value; ROWDATA: offset of its slot in the row
    int32_t key_field, ts_field, num_cols;
    int32_t col_field[FWA_MAX_COLS];
    int32_t row_size, nullbits;        // ROWDATA: BinaryRowData size (fixed part only) and null-bit-set width
    int32_t nstr;                      // STRING fields (> 0: records vary in length, the VAR kernels run)
    int32_t str_field[FWA_WIRE_MAX_FIELDS];
    int32_t ndecf, ndec;               // DECIMAL fields (> 0: VAR as well) and how many of them are value columns
};

struct WireStatus {
    int32_t error;                     // first fwa_status raised by the decode kernel
    int32_t err_tag;
    int64_t err_pos;                   // byte offset of the offending element
    int64_t consumed;                  // bytes of whole elements (written by the END chunk)
};

// The staged chunk in LDS, read through aligned 32-bit words (two ds_read_b32 + a funnel shift per unaligned
// 4-byte field instead of four byte reads); the buffer carries 8 bytes of padding past the last staged byte.
struct Lds {
    const uint32_t* w;
    __device__ __forceinline__ uint32_t u32le(int p) const {
        const int i = p >> 2, sh = (p & 3) * 8;
        return (uint32_t)((((uint64_t)w[i + 1] << 32) | w[i]) >> sh);
    }
    __device__ __forceinline__ uint32_t byte(int p) const { return (w[p >> 2] >> ((p & 3) * 8)) & 0xFF; }
    __device__ __forceinline__ uint32_t be32(int p) const { return __builtin_bswap32(u32le(p)); }
    __device__ __forceinline__ uint64_t le64(int p) const {
        const int i = p >> 2, sh = (p & 3) * 8;
        const uint32_t a = w[i], b = w[i + 1], c = w[i + 2];
        const uint32_t lo = (uint32_t)((((uint64_t)b << 32) | a) >> sh);
        const uint32_t hi = (uint32_t)((((uint64_t)c << 32) | b) >> sh);
        return ((uint64_t)hi << 32) | lo;
    }
    __device__ __forceinline__ uint64_t be64(int p) const { return __builtin_bswap64(le64(p)); }
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
constexpr int kBufWords = (kChunk + kMaxStep + 3 + 8 + 3) / 4;

// Copy bytes [0, lim) of src (a chunk start: 4 KiB-aligned offset into the input) into LDS.
__device__ __forceinline__ void stage_chunk(uint32_t* words, const uint8_t* __restrict__ src, int lim, bool aligned) {
    uint8_t* buf = reinterpret_cast<uint8_t*>(words);
    int done = 0;
    if (aligned) {
        const int n16 = lim >> 4;
        for (int i = threadIdx.x; i < n16; i += blockDim.x)
            reinterpret_cast<u32x4*>(buf)[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src) + i);
        done = n16 << 4;
    }
    for (int i = done + threadIdx.x; i < lim; i += blockDim.x) buf[i] = src[i];
}

// The chain step shared by scan and decode: classify the element starting at p (rem = bytes left in the stream
// from the chunk start). Returns 0: a whole element of length 4 + *len; 1: END; 2: CORRUPT. The expected body
// lengths are selected from uniform values (no per-lane indexed load of the kernel argument).
//
// VAR (rows with STRING fields): body[0] / body[1] are the shortest record bodies (fixed part only). A record header
// is accepted when its length is at least that, the row's size int equals the length minus the header (a 32-bit
// equality, which keeps false candidates as rare as the exact length does for fixed rows), the element is within the
// 249-byte ceiling (else 3: TOO LONG) and the RowKind byte is INSERT (else 4, *tag = 256 + RowKind). The order of
// these checks is part of the format the tests' reference decoder restates.
//
// JS (TUPLE values with JSTRING fields; with VAR): a tuple has no size int to cross-check, so a record header is
// accepted on its length alone: at least body[0] / body[1] (tag, [timestamp], the fixed fields, one byte per JSTRING
// field), at most the ceiling (else 3), the element inside the stream (else 1). The filter is weak -- any four bytes
// that read as 2..249 in front of a 00 / 01 pass it -- and that is sound: a false candidate only costs the scan a walk
// whose map entry nobody composes with, because every entry is the exact exit of the chain from that offset and the
// composition follows the one chain that starts at byte 0 of the call.
template <bool VAR, bool JS = false>
__device__ __forceinline__ int element_at(const Lds& b, int p, int rem, const WireConst& w, uint32_t* len,
                                          int* tag) {
    if (p + 5 > rem) return 1;
    const uint32_t l = b.be32(p);
    const int t = (int)b.byte(p + 4);
    *tag = t;
    const int32_t want = t == 0 ? w.body[0] : t == 1 ? w.body[1] : t == 2 ? w.body[2] : t == 3 ? w.body[3]
                       : t == 4 ? w.body[4] : t == 5 ? w.body[5] : -1;
    if constexpr (JS) {
        if (t <= 1) {
            if (l < (uint32_t)want) return 2;
            if (l > kMaxBody) return 3;
            if (p + 4 + (int)l > rem) return 1;
            *len = l;
            return 0;
        }
    } else if constexpr (VAR) {
        if (t <= 1) {
            const int hdr = t == 0 ? 13 : 5;                       // tag, [timestamp], size int
            if (l < (uint32_t)want) return 2;
            if (p + 4 + hdr > rem) return 1;                       // the size int is not here yet
            if (b.be32(p + hdr) != l - (uint32_t)hdr) return 2;
            if (l > kMaxBody) return 3;
            if (p + 4 + (int)l > rem) return 1;
            const int kind = (int)b.byte(p + 4 + hdr);
            if (kind != 0) { *tag = 256 + kind; return 4; }
            *len = l;
            return 0;
        }
    }
    if (l != (uint32_t)want) return 2;
    if (p + 4 + (int)l > rem) return 1;
    *len = l;
    return 0;
}

// Wave-cooperative walk of the element chain from p through the chunk. Element boundaries are a sequential
// chain, but almost every element has the length of the one before it (a channel carries one record type), so
// the wave SPECULATES: lane i checks the header at p + i * R (R = the last element's size); the longest prefix of
// lanes whose header is a whole element of size R is exactly the next stretch of the chain (each check confirms
// the previous lane's boundary), one ballot per 64 elements. The first lane that fails is resolved by one scalar
// step (another element kind / END / CORRUPT), which also sets the new R. visit(pos, tag, rec_before, evt_rank)
// runs on the lane owning each element. Returns 0 (left the chunk: *stop >= kChunk), 1 END, 2 CORRUPT (VAR: 3, 4).
//
// VAR: rows whose strings are all inline have one size and the speculation runs as above. When it misses twice in
// a row (k = 0: sizes alternate), the wave lists up to 64 elements by uniform scalar steps, lane i keeping the i-th,
// and the lanes visit them in parallel; it goes back to speculating after a list whose elements all had one size.
template <bool VAR, bool JS = false, class F>
__device__ __forceinline__ int wave_walk(const Lds& b, int p, int remi, const WireConst& w, uint32_t* nrec,
                                         uint32_t* nevt, int* stop, int* badtag, F&& visit) {
    const int lane = threadIdx.x & 63;
    const uint64_t below = (1ull << lane) - 1;
    uint32_t nr = 0, ne = 0;
    int R = 0;
    int miss = 0;
    for (;;) {
        if (p >= kChunk) { *nrec = nr; *nevt = ne; *stop = p; return 0; }
        if (R > 0) {
            const int pos = p + lane * R;
            uint32_t len = 0;
            int tag = 0;
            const bool ok = pos < kChunk && element_at<VAR, JS>(b, pos, remi, w, &len, &tag) == 0 && (int)len + 4 == R;
            const uint64_t m = __ballot(ok);
            const int k = ~m == 0 ? 64 : __builtin_ctzll(~m);
            const bool mine = lane < k;
            const uint64_t rm = __ballot(mine && tag <= 1), em = __ballot(mine && tag > 1);
            if (mine) visit(pos, tag, nr + (uint32_t)__popcll(rm & below), ne + (uint32_t)__popcll(em & below));
            nr += (uint32_t)__popcll(rm);
            ne += (uint32_t)__popcll(em);
            p += k * R;
            if (k == 64 || p >= kChunk) continue;
            if constexpr (VAR) miss = k == 0 ? miss + 1 : 0;
        }
        if constexpr (VAR) {
            if (miss >= 2) {
                // The uniform steps read nothing but the length prefixes (every lane executes them, so they are kept
                // to a load and an add); lane i then checks element i in full, and the longest prefix of valid elements
                // is the chain: a length prefix is only followed after its own element proved valid.
                int cnt = 0, mypos = p, q = p;
                while (cnt < 64 && q < kChunk) {
                    const uint32_t l = b.be32(q);                   // (stale bytes past the stream's end fail the check)
                    if (lane == cnt) mypos = q;
                    ++cnt;
                    if (l > kMaxBody) break;                        // its lane settles it; nothing is listed behind it
                    q += 4 + (int)l;
                }
                uint32_t len = 0;
                int tag = 0;
                const bool ok = lane < cnt && element_at<VAR, JS>(b, mypos, remi, w, &len, &tag) == 0;
                const uint64_t m = __ballot(ok);
                const int k = ~m == 0 ? 64 : __builtin_ctzll(~m);   // <= cnt
                const bool mine = lane < k;
                const uint64_t rm = __ballot(mine && tag <= 1), em = __ballot(mine && tag > 1);
                if (mine) visit(mypos, tag, nr + (uint32_t)__popcll(rm & below), ne + (uint32_t)__popcll(em & below));
                nr += (uint32_t)__popcll(rm);
                ne += (uint32_t)__popcll(em);
                const int sz0 = __shfl((int)len, 0, 64);
                const bool same = k >= 2 && __ballot(mine && (int)len != sz0) == 0;
                if (k == cnt) p = q;                                // every listed element is valid: q is the next start
                else p = __shfl(mypos, k, 64);                      // the first invalid one: the scalar step below names it
                if (same) { R = 4 + sz0; miss = 0; }
                else R = 0;
                if (k == cnt) continue;
            }
        }
        uint32_t len = 0;                                          // scalar step at p (uniform)
        int tag = 0;
        const int st = element_at<VAR, JS>(b, p, remi, w, &len, &tag);
        if (st) { *nrec = nr; *nevt = ne; *stop = p; *badtag = tag; return st; }
        if (lane == 0) visit(p, tag, nr, ne);
        if (tag <= 1) ++nr; else ++ne;
        R = 4 + (int)len;
        p += R;
    }
}

// Next-chunk prefetch in registers: while the wave walks chunk c, the 16-byte loads of its next chunk are in
// flight (they land in LDS after the walk). Chunks reaching the stream end and unaligned inputs are staged byte-wise.
struct Prefetch {
    static constexpr int kVec = 5;                     // 16-byte loads per lane: 320 x 16 B >= kChunk + kMaxStep + 3
    u32x4 r[kVec];
    bool ok = false;
    __device__ __forceinline__ void issue(const uint8_t* __restrict__ in, int64_t nbytes, int64_t c, int nvec,
                                          bool aligned) {
        const int64_t cs = c * kChunk;
        ok = aligned && cs + (int64_t)nvec * 16 <= nbytes;
        if (!ok) return;
        const u32x4* src = reinterpret_cast<const u32x4*>(in + cs);
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int i = threadIdx.x + 64 * k;
            if (i < nvec) r[k] = __builtin_nontemporal_load(src + i);
        }
    }
    __device__ __forceinline__ void land(uint32_t* buf, int nvec) const {
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const int i = threadIdx.x + 64 * k;
            if (i < nvec) reinterpret_cast<u32x4*>(buf)[i] = r[k];
        }
    }
};
static_assert(Prefetch::kVec * 64 * 16 >= kChunk + kMaxStep + 3, "prefetch covers a chunk and its halo");

// Stage chunk c from the prefetch (or byte-wise), then put chunk `next` in flight. Returns the bytes left.
__device__ __forceinline__ int stage_pf(uint32_t* buf, const uint8_t* __restrict__ in, int64_t nbytes, int64_t nchunks,
                                        int64_t c, int64_t next, const WireConst& w, bool aligned, Prefetch& pf) {
    const int nvec = (kChunk + w.step + 15) / 16;
    const int64_t cs = c * kChunk;
    const int64_t rem = nbytes - cs;
    __syncthreads();                                              // previous chunk fully read
    if (pf.ok) pf.land(buf, nvec);
    else {
        const int lim = (int)std::min<int64_t>(rem, kChunk + w.step);
        if (lim > 0) stage_chunk(buf, in + cs, lim, aligned);
    }
    __syncthreads();
    if (next < nchunks) pf.issue(in, nbytes, next, nvec, aligned);
    else pf.ok = false;
    return (int)std::min<int64_t>(rem, 1 << 30);                  // bytes left, clamped (chains stop within C + S)
}

// ---- scan: persistent 64-lane blocks, one chunk at a time. Candidates whose first header is already invalid
// (nearly all of them on real data) are settled in one lane-parallel check; each surviving candidate is walked
// by the whole wave.
//
// VAR: several candidates in [0, S) are starts of the same chain (one per element that begins there). The walk of the
// first one leaves, at every element start below S, the records / events before it (vis[]); the map entries of those
// later candidates are the walk's exit and its totals minus that rank, and they are not walked again. ----
constexpr uint32_t kVisMark = 1u << 31, kVisDone = 1u << 30;
template <bool VAR, bool JS = false>
__global__ __launch_bounds__(64) void wire_scan_kernel(const uint8_t* __restrict__ in, int64_t nbytes,
                                                        int64_t nchunks, WireConst w, bool aligned,
                                                        uint32_t* __restrict__ map0) {
    __shared__ uint32_t buf[kBufWords];
    __shared__ uint32_t vis[VAR ? 256 : 1];
    const Lds b{buf};
    const int lane = threadIdx.x;
    Prefetch pf;
    if ((int64_t)blockIdx.x < nchunks) pf.issue(in, nbytes, blockIdx.x, (kChunk + w.step + 15) / 16, aligned);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        if constexpr (VAR)
            for (int i = lane; i < 256; i += 64) vis[i] = 0;      // (the barriers of stage_pf order this)
        const int remi = stage_pf(buf, in, nbytes, nchunks, c, c + gridDim.x, w, aligned, pf);
        for (int e0 = 0; e0 < w.step; e0 += 64) {
            const int e = e0 + lane;
            uint32_t len = 0;
            int tag = 0;
            int first = e < w.step ? element_at<VAR, JS>(b, e, remi, w, &len, &tag) : kNone;
            if constexpr (VAR)
                if (first == 0 && (vis[e] & kVisDone)) first = kNone;  // settled by an earlier candidate's walk
            if (first >= 1 && first < kNone) map0[c * w.step + e] = first == 1 ? kNxtEnd : kNxtCorrupt;
            uint64_t alive = __ballot(first == 0);
            while (alive) {
                const int j = __builtin_ctzll(alive);
                alive &= alive - 1;
                uint32_t nrec = 0, nevt = 0;
                int stop = 0, bt = 0;
                if constexpr (VAR) {
                    const int S = w.step;
                    const int r = wave_walk<VAR, JS>(b, e0 + j, remi, w, &nrec, &nevt, &stop, &bt,
                                                 [&](int pos, int, uint32_t rb, uint32_t eb) {
                                                     if (pos < S) vis[pos] = kVisMark | rb | (eb << 12);
                                                 });
                    const uint32_t nx = r == 0 ? (uint32_t)(stop - kChunk) : r == 1 ? kNxtEnd : kNxtCorrupt;
                    __syncthreads();
                    for (int pos = lane; pos < S; pos += 64) {
                        const uint32_t v = vis[pos];
                        if (!(v & kVisMark)) continue;
                        map0[c * S + pos] = nx | ((nrec - (v & 0xFFF)) << 8) | ((nevt - ((v >> 12) & 0xFFF)) << 20);
                        vis[pos] = kVisDone;
                    }
                    __syncthreads();
                    alive &= ~__ballot(e < S && (vis[e] & kVisDone));
                } else {
                    const int r = wave_walk<VAR>(b, e0 + j, remi, w, &nrec, &nevt, &stop, &bt, [](int, int, uint32_t, uint32_t) {});
                    const uint32_t nx = r == 0 ? (uint32_t)(stop - kChunk) : r == 1 ? kNxtEnd : kNxtCorrupt;
                    if (lane == 0) map0[c * w.step + e0 + j] = nx | (nrec << 8) | (nevt << 20);   // <= 683 elements per chunk
                }
            }
        }
    }
}

// Level maps: SoA (next u8, nrec u32, nevt u32) per (item, entry offset). Level 0 is the packed scan map.
struct LevelMap {
    const uint32_t* packed;            // level 0
    const uint8_t* nxt;
    const uint32_t* nrec;
    const uint32_t* nevt;
};

__device__ __forceinline__ void load_children(const LevelMap& m, int64_t first, int nch, int S, uint8_t* s_nxt,
                                              uint32_t* s_nrec, uint32_t* s_nevt) {
    const int64_t base = first * S;
    for (int i = threadIdx.x; i < nch * S; i += blockDim.x) {
        if (m.packed) {
            const uint32_t v = m.packed[base + i];
            s_nxt[i] = (uint8_t)(v & 0xFF);
            s_nrec[i] = (v >> 8) & 0xFFF;
            s_nevt[i] = v >> 20;
        } else {
            s_nxt[i] = m.nxt[base + i];
            s_nrec[i] = m.nrec[base + i];
            s_nevt[i] = m.nevt[base + i];
        }
    }
}

// ---- compose: parent map = composition of its (up to `fan`) children's maps ----
__global__ __launch_bounds__(256) void wire_compose_kernel(LevelMap child, int64_t nitems, int S, int fan,
                                                            uint8_t* __restrict__ p_nxt, uint32_t* __restrict__ p_nrec,
                                                            uint32_t* __restrict__ p_nevt) {
    extern __shared__ uint32_t lds[];
    uint32_t* s_nrec = lds;
    uint32_t* s_nevt = s_nrec + fan * S;
    uint8_t* s_nxt = reinterpret_cast<uint8_t*>(s_nevt + fan * S);
    const int64_t first = (int64_t)blockIdx.x * fan;
    const int nch = (int)std::min<int64_t>(fan, nitems - first);
    load_children(child, first, nch, S, s_nxt, s_nrec, s_nevt);
    __syncthreads();
    for (int e = threadIdx.x; e < S; e += blockDim.x) {
        uint32_t cur = (uint32_t)e, nrec = 0, nevt = 0;
        for (int k = 0; k < nch; ++k) {
            const int i = k * S + (int)cur;
            nrec += s_nrec[i];
            nevt += s_nevt[i];
            cur = s_nxt[i];
            if (cur >= kNxtEnd) break;
        }
        const int64_t o = (int64_t)blockIdx.x * S + e;
        p_nxt[o] = (uint8_t)cur;
        p_nrec[o] = nrec;
        p_nevt[o] = nevt;
    }
}

// ---- resolve: a parent's entry offset and first record / event index -> each child's ----
__global__ __launch_bounds__(256) void wire_resolve_kernel(LevelMap child, int64_t nitems, int S, int fan,
                                                            const uint8_t* __restrict__ p_ent,
                                                            const uint64_t* __restrict__ p_rec,
                                                            const uint64_t* __restrict__ p_evt,
                                                            uint8_t* __restrict__ c_ent, uint64_t* __restrict__ c_rec,
                                                            uint64_t* __restrict__ c_evt) {
    extern __shared__ uint32_t lds[];
    uint32_t* s_nrec = lds;
    uint32_t* s_nevt = s_nrec + fan * S;
    uint8_t* s_nxt = reinterpret_cast<uint8_t*>(s_nevt + fan * S);
    const int64_t first = (int64_t)blockIdx.x * fan;
    const int nch = (int)std::min<int64_t>(fan, nitems - first);
    load_children(child, first, nch, S, s_nxt, s_nrec, s_nevt);
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t cur = p_ent[blockIdx.x];
    uint64_t rb = p_rec[blockIdx.x], eb = p_evt[blockIdx.x];
    for (int k = 0; k < nch; ++k) {
        c_ent[first + k] = (uint8_t)cur;
        c_rec[first + k] = rb;
        c_evt[first + k] = eb;
        if (cur == kDead) continue;
        const int i = k * S + (int)cur;
        rb += s_nrec[i];
        eb += s_nevt[i];
        cur = s_nxt[i] >= kNxtEnd ? kDead : s_nxt[i];
    }
}

struct DecodeOut {
    int64_t* key;
    int64_t* ts;
    void* col[FWA_MAX_COLS];
    uint8_t* col_null[FWA_MAX_COLS];
    uint8_t* key_null;
    int64_t* evt_pos;
    int32_t* evt_tag;
    int64_t* evt_val;
    int64_t evt_cap;
    WireStatus* st;
    // STRING field k of record g, at [k * str_stride + g]: value length, input byte offset of its first byte
    // (an inline value points into its slot), NULL flag
    int32_t* str_len;
    int64_t* str_src;
    uint8_t* str_null;
    int64_t str_stride;
};

constexpr int kErrTooLong = 512;       // WireStatus.err_tag of an element over the ceiling (>= 256: RowKind + 256)
constexpr int kErrSlot = 513;          // ... of a STRING slot pointing outside its row
constexpr int kErrDecSlot = 514;       // ... of a DECIMAL slot: bytes outside the row's variable-length part, 0 or > 16 of them
constexpr int kErrJstr = 515;          // ... of a TUPLE value whose field walk does not end at the element's end

__device__ void raise_err(WireStatus* st, int code, int tag, int64_t pos) {
    if (atomicCAS(&st->error, 0, code) == 0) {
        st->err_tag = tag;
        st->err_pos = pos;
    }
}

// Field f of a record whose value starts at q (TUPLE) / whose row starts at q (ROWDATA), as 64 bits
// (INT sign-extended, FLOAT as its 32 bits in the low word, DOUBLE bits).
__device__ __forceinline__ uint64_t read_field(const Lds& b, int q, int f, const WireConst& w) {
    const int t = w.ftype[f];
    const int at = q + w.foff[f];
    if (w.format == FWA_WIRE_TUPLE) {
        if (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) return b.be64(at);
        const uint32_t v = b.be32(at);
        return t == FWA_FIELD_INT ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v;
    }
    if (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) return b.le64(at);
    const uint32_t v = b.u32le(at);
    return t == FWA_FIELD_INT ? (uint64_t)(int64_t)(int32_t)v : (uint64_t)v;
}

__device__ __forceinline__ bool field_null(const Lds& b, int row, int f) {   // BinarySegmentUtils.bitGet
    const int bit = f + 8;                                                  // (BinaryRowData header: 8 bits)
    return (b.byte(row + (bit >> 3)) >> (bit & 7)) & 1;
}

// ---- decode: persistent 64-lane blocks; the chunk's true chain is walked from its resolved entry and every
// element is decoded by the lane that confirmed it. VAR: element_at has already checked the row's size int and
// RowKind; every STRING slot is checked against the row here, before anything reads the value's bytes.
// DEC (with VAR): the schema has DECIMAL value columns; their slots are checked the same way, then the 1..16 big-endian
// bytes (inside the row, so inside the staged chunk and its halo) are read from LDS by the record's lane ----
//
// JS (with VAR): TUPLE values with JSTRING fields (StringSerializer -> StringValue.writeString, flink-core/.../types/
// StringValue.java:  len + 1 as a varint of 7-bit groups, low group first, then every UTF-16 code unit coded the same
// way, 1..3 bytes). Nothing has a fixed offset, so the record's lane walks the fields in order from the element's bytes
// in LDS with a running cursor: fixed fields big-endian at the cursor, a JSTRING as its length varint and then `len`
// chars, each checked for the canonical form (at most three groups, a last group that is not zero behind a
// continuation, a third group <= 3). A char ends at its first byte below 0x80, so skipping n chars is counting n such
// bytes. No byte at or past the element's end is read, and the cursor must stand exactly there after the last field.
template <bool VAR, bool DEC = false, bool JS = false>
__global__ __launch_bounds__(64) void wire_decode_kernel(const uint8_t* __restrict__ in, int64_t nbytes, int64_t nchunks,
                                                          WireConst w, bool aligned, const uint8_t* __restrict__ c_ent,
                                                          const uint64_t* __restrict__ c_rec,
                                                          const uint64_t* __restrict__ c_evt, DecodeOut o) {
    __shared__ uint32_t buf[kBufWords];
    const Lds b{buf};
    Prefetch pf;
    if ((int64_t)blockIdx.x < nchunks) pf.issue(in, nbytes, blockIdx.x, (kChunk + w.step + 15) / 16, aligned);
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const uint32_t ent = c_ent[c];
        const int64_t cs = c * kChunk;
        const int remi = stage_pf(buf, in, nbytes, nchunks, c, c + gridDim.x, w, aligned, pf);
        if (ent == kDead) continue;
        const uint64_t rb = c_rec[c], eb = c_evt[c];
        auto visit = [&](int p, int tag, uint32_t rbefore, uint32_t erank) {
            int q = p + 5;
            if (tag <= 1) {
                const int64_t g = (int64_t)(rb + rbefore);
                int64_t ts = (int64_t)0x8000000000000000LL;          // StreamRecord without timestamp
                if (tag == FWA_TAG_REC_WITH_TIMESTAMP) { ts = (int64_t)b.be64(q); q += 8; }
                bool knull = false;
                if constexpr (JS) {
                    const int end = p + 4 + (int)b.be32(p);          // <= p + 253, inside the staged bytes (element_at)
                    bool bad = false;
                    int k = 0;
                    for (int f = 0; f < w.arity && !bad; ++f) {
                        const int t = w.ftype[f];
                        if (t != FWA_FIELD_JSTRING) {
                            const int nb = (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) ? 8 : 4;
                            if (q + nb > end) { bad = true; break; }
                            uint64_t v;
                            if (nb == 8) v = b.be64(q);
                            else { const uint32_t x = b.be32(q); v = t == FWA_FIELD_INT ? (uint64_t)(int64_t)(int32_t)x : (uint64_t)x; }
                            q += nb;
                            if (f == w.ts_field) ts = (int64_t)v;
                            for (int j = 0; j < w.num_cols; ++j) {
                                if (w.col_field[j] != f) continue;
                                if (t == FWA_FIELD_FLOAT) reinterpret_cast<uint32_t*>(o.col[j])[g] = (uint32_t)v;
                                else reinterpret_cast<uint64_t*>(o.col[j])[g] = v;
                            }
                            continue;
                        }
                        // StringValue.readString: the length varint (an int: at most 5 groups), 0 = null, else len + 1
                        uint64_t lv = 0;
                        int sh = 0, first = -1;
                        for (;;) {
                            if (q >= end || sh > 28) { bad = true; break; }
                            const uint32_t c = b.byte(q++);
                            if (first < 0) first = (int)c;
                            lv |= (uint64_t)(c & 0x7f) << sh;
                            sh += 7;
                            if (c < 0x80) break;
                        }
                        if (bad) break;
                        const bool isnull = first == 0;
                        if (!isnull && lv == 0) { bad = true; break; }    // 80 00: a length of -1 to the reference reader
                        const int64_t nch = isnull ? 0 : (int64_t)lv - 1;
                        if (nch > end - q) { bad = true; break; }         // every char has at least one byte
                        const int v0 = q;
                        int run = 0;                                      // continuation bytes of the char under the cursor
                        for (int64_t left = nch; left > 0;) {
                            if (run == 0 && left >= 4 && q + 4 <= end) {      // four one-byte chars (ASCII text) at once
                                if (!(b.u32le(q) & 0x80808080u)) { q += 4; left -= 4; continue; }
                            }
                            if (q >= end) { bad = true; break; }
                            const uint32_t c = b.byte(q++);
                            if (c >= 0x80) {
                                if (++run >= 3) { bad = true; break; }    // a fourth group
                                continue;
                            }
                            if ((run > 0 && c == 0) || (run == 2 && c > 3)) { bad = true; break; }
                            run = 0;
                            --left;
                        }
                        if (bad) break;
                        const int64_t at = k * o.str_stride + g;
                        o.str_len[at] = q - v0;
                        o.str_src[at] = cs + v0;
                        o.str_null[at] = isnull;
                        ++k;
                    }
                    if (bad || q != end) { raise_err(o.st, FWA_E_CORRUPT, kErrJstr, cs + p); return; }
                    o.ts[g] = ts;
                    return;
                }
                if constexpr (VAR) {
                    const int size = (int)b.be32(q);                 // == L - header, <= 249 (element_at)
                    q += 4;
                    if (w.ts_field >= 0 && field_null(b, q, w.ts_field)) { raise_err(o.st, FWA_E_ARG, tag, cs + p); return; }
                    for (int j = 0; j < w.num_cols; ++j) o.col_null[j][g] = field_null(b, q, w.col_field[j]);
                    if (w.key_field >= 0) {
                        knull = field_null(b, q, w.key_field);
                        o.key_null[g] = knull;
                        o.key[g] = knull ? 0 : (int64_t)read_field(b, q, w.key_field, w);
                    }
                    for (int k = 0; k < w.nstr; ++k) {
                        const int f = w.str_field[k];
                        const uint64_t slot = b.le64(q + w.foff[f]);
                        const bool isnull = field_null(b, q, f);
                        int64_t src = cs + q + w.foff[f];
                        uint32_t len = 0;
                        if (!isnull) {
                            if (slot >> 63) {                        // inline: length in the top byte, bytes below it
                                len = (uint32_t)(slot >> 56) & 0x7f;
                                if (len > 7) { raise_err(o.st, FWA_E_CORRUPT, kErrSlot, cs + p); len = 0; }
                            } else {                                 // offset << 32 | length, inside the row
                                const uint64_t off = slot >> 32, ln = slot & 0xffffffffull;
                                if (off < (uint64_t)w.row_size || off + ln > (uint64_t)size) raise_err(o.st, FWA_E_CORRUPT, kErrSlot, cs + p);
                                else { len = (uint32_t)ln; src = cs + q + (int64_t)off; }
                            }
                        }
                        const int64_t at = k * o.str_stride + g;
                        o.str_len[at] = (int32_t)len;
                        o.str_src[at] = src;
                        o.str_null[at] = isnull;
                    }
                } else if (w.format == FWA_WIRE_ROWDATA) {
                    if ((int32_t)b.be32(q) != w.row_size) { raise_err(o.st, FWA_E_UNSUPPORTED, tag, cs + p); return; }
                    q += 4;                                          // row bytes start; byte 0 = RowKind
                    if (b.byte(q) != 0) { raise_err(o.st, FWA_E_UNSUPPORTED, 256 + (int)b.byte(q), cs + p); return; }
                    knull = field_null(b, q, w.key_field);
                    if (w.ts_field >= 0 && field_null(b, q, w.ts_field)) { raise_err(o.st, FWA_E_ARG, tag, cs + p); return; }
                    for (int j = 0; j < w.num_cols; ++j) o.col_null[j][g] = field_null(b, q, w.col_field[j]);
                    o.key_null[g] = knull;
                }
                if constexpr (!VAR) o.key[g] = knull ? 0 : (int64_t)read_field(b, q, w.key_field, w);
                o.ts[g] =w.ts_field >= 0 ? (int64_t)read_field(b, q, w.ts_field, w) : ts;
                for (int j = 0; j < w.num_cols; ++j) {
                    const int f = w.col_field[j];
                    if constexpr (DEC) {
                        if (w.ftype[f] == FWA_FIELD_DECIMAL) {
                            // BinarySegmentUtils.readDecimalData: new BigInteger(the slot's `len` bytes). The reader
                            // asks neither for the minimal length nor for 16 bytes inside the row; a NULL field's slot
                            // is not looked at (setNullAt leaves 0, writeDecimal(null) leaves cursor << 32)
                            uint64_t lo = 0, hi = 0;
                            if (!field_null(b, q, f)) {
                                const uint64_t slot = b.le64(q + w.foff[f]);
                                const uint64_t off = slot >> 32, ln = slot & 0xffffffffull;
                                const uint64_t size = (uint64_t)b.be32(q - 4);      // the row's size int (<= 249)
                                if (off < (uint64_t)w.row_size || off + ln > size || ln < 1 || ln > 16)
                                    raise_err(o.st, FWA_E_CORRUPT, kErrDecSlot, cs + p);
                                else {
                                    const int at = q + (int)off;
                                    lo = hi = (b.byte(at) & 0x80) ? ~0ull : 0ull;   // sign extension from the first byte
                                    for (int i = 0; i < (int)ln; ++i) {
                                        hi = (hi << 8) | (lo >> 56);
                                        lo = (lo << 8) | b.byte(at + i);
                                    }
                                }
                            }
                            const u64x2 v128 = {lo, hi};
                            reinterpret_cast<u64x2*>(o.col[j])[g] = v128;
                            continue;
                        }
                    }
                    const uint64_t v = read_field(b, q, f, w);
                    if (w.ftype[f] == FWA_FIELD_FLOAT) reinterpret_cast<uint32_t*>(o.col[j])[g] = (uint32_t)v;
                    else reinterpret_cast<uint64_t*>(o.col[j])[g] = v;
                }
            } else {
                const int64_t g = (int64_t)(eb + erank);
                if (g >= o.evt_cap) return;                          // host grows the list and decodes again
                int64_t v[4] = {0, 0, 0, 0};
                if (tag == FWA_TAG_WATERMARK) v[0] = (int64_t)b.be64(q);
                else if (tag == FWA_TAG_STREAM_STATUS) v[0] = (int32_t)b.be32(q);
                else if (tag == FWA_TAG_LATENCY_MARKER) {
                    v[0] = (int64_t)b.be64(q);
                    v[1] = (int64_t)b.be64(q + 8);
                    v[2] = (int64_t)b.be64(q + 16);
                    v[3] = (int32_t)b.be32(q + 24);
                } else v[0] = b.byte(q) != 0;                        // RECORD_ATTRIBUTES: readBoolean
                o.evt_pos[g] = (int64_t)(rb + rbefore);
                o.evt_tag[g] = tag;
                for (int k = 0; k < 4; ++k) o.evt_val[4 * g + k] = v[k];
            }
        };
        uint32_t nrec = 0, nevt = 0;
        int stop = 0, bt = 0;
        const int r = wave_walk<VAR, JS>(b, (int)ent, remi, w, &nrec, &nevt, &stop, &bt, visit);
        if (threadIdx.x == 0) {
            if (r == 1) o.st->consumed = cs + stop;
            else if (r == 2) raise_err(o.st, FWA_E_CORRUPT, bt, cs + stop);
            else if (r == 3) raise_err(o.st, FWA_E_UNSUPPORTED, kErrTooLong, cs + stop);
            else if (r == 4) raise_err(o.st, FWA_E_UNSUPPORTED, bt, cs + stop);
        }
    }
}

// ---- string extraction (fwa_wire_strings_of): offsets = exclusive scan of the lengths (hipcub), then this gather.
// Values average tens of bytes, so a wave takes 64 consecutive strings, whose output bytes are one contiguous
// run, and copies that run byte-parallel: consecutive lanes write consecutive output bytes (coalesced) and find
// their string by a binary search over the wave's 65 offsets in LDS; the reads stay within the few KiB of wire
// bytes the 64 records came from. ----
constexpr int kGatherWaves = 4;
__global__ __launch_bounds__(64 * kGatherWaves) void wire_gather_kernel(const uint8_t* __restrict__ in,
                                                                        const int64_t* __restrict__ src,
                                                                        const int32_t* __restrict__ off, int64_t n,
                                                                        uint8_t* __restrict__ out) {
    __shared__ int32_t s_off[kGatherWaves][65];
    __shared__ int64_t s_src[kGatherWaves][64];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t bb = (int64_t)blockIdx.x * (64 * kGatherWaves); bb < n; bb += (int64_t)gridDim.x * (64 * kGatherWaves)) {
        const int64_t base = bb + wv * 64;
        const int m = (int)std::min<int64_t>(64, n - base);         // strings of this wave (<= 0: none)
        __syncthreads();                                            // the previous round's reads are done
        if (lane < m) { s_off[wv][lane] = off[base + lane]; s_src[wv][lane] = src[base + lane]; }
        if (lane == 0 && m > 0) s_off[wv][m] = off[base + m];
        __syncthreads();
        if (m <= 0) continue;
        const int32_t o0 = s_off[wv][0], total = s_off[wv][m] - o0;
        for (int32_t j = lane; j < total; j += 64) {
            const int32_t t = o0 + j;
            int lo = 0, hi = m;                                     // last string with off <= t (skips empty ones)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[wv][mid] <= t) lo = mid; else hi = mid;
            }
            out[t] = in[s_src[wv][lo] + (t - s_off[wv][lo])];
        }
    }
}

// 64-bit total of the lengths (inputs of 2 GiB and more, where the int32 offsets could wrap)
__global__ __launch_bounds__(256) void wire_len_sum_kernel(const int32_t* __restrict__ len, int64_t n,
                                                            unsigned long long* __restrict__ total) {
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        s += (unsigned long long)(uint32_t)len[i];
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
}

// ---- String.hashCode() of values in the canonical char-byte form (fwa_jstring_hash). Keys are short, so a lane takes
// a value and a wave 64 consecutive ones, whose bytes are one contiguous run of the Arrow bytes. The run is brought into
// LDS a tile at a time, coalesced: 16-byte loads for the aligned middle, byte loads for the ragged head and tail (the
// tile keeps the run's 16-byte phase), so no lane issues strided byte loads to HBM. Each lane then reads the part of
// its value that lies in the tile from LDS and carries (hash, char under assembly) to the next tile; a value of any
// length is hashed that way, and a run of 64 five-byte keys is one tile.
// h = 31 * h + c per code unit; a code unit's 7-bit groups arrive low group first and it ends at a byte below 0x80. ----
constexpr int kHashTile = 4096;
__global__ __launch_bounds__(64) void wire_jstring_hash_kernel(const int32_t* __restrict__ off, const uint8_t* __restrict__ bytes,
                                                                const uint8_t* __restrict__ nulls, int64_t n,
                                                                int32_t* __restrict__ out) {
    __shared__ u32x4 tile[kHashTile / 16 + 1];
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(tile);
    uint8_t* tw = reinterpret_cast<uint8_t*>(tile);
    const int lane = threadIdx.x;
    const int64_t nwaves = (n + 63) / 64;
    for (int64_t wv = blockIdx.x; wv < nwaves; wv += gridDim.x) {
        const int64_t base = wv * 64;
        const int m = (int)std::min<int64_t>(64, n - base);
        const int64_t g = base + lane;
        const int64_t r0 = off[base], r1 = off[base + m];          // the wave's run of bytes
        const bool live = lane < m && !(nulls && nulls[g]);
        const int64_t s = lane < m ? off[g] : r1, e = lane < m ? off[g + 1] : r1;
        uint32_t h = 0, ch = 0;
        int sh = 0;
        for (int64_t t0 = r0; t0 < r1;) {
            const uint8_t* __restrict__ src = bytes + t0;
            const int skew = (int)(reinterpret_cast<uintptr_t>(src) & 15);
            const int len = (int)std::min<int64_t>(r1 - t0, kHashTile - skew);
            __syncthreads();                                          // the previous tile has been read
            const int head = std::min(len, (16 - skew) & 15);
            for (int j = lane; j < head; j += 64) tw[skew + j] = src[j];
            const int nfull = (len - head) >> 4, v0 = (skew + head) >> 4;
            const u32x4* __restrict__ sv = reinterpret_cast<const u32x4*>(src + head);
            for (int i = lane; i < nfull; i += 64) tile[v0 + i] = sv[i];
            for (int j = head + (nfull << 4) + lane; j < len; j += 64) tw[skew + j] = src[j];
            __syncthreads();
            if (live) {
                const int a = (int)(std::max<int64_t>(s, t0) - t0), z = (int)(std::min<int64_t>(e, t0 + len) - t0);
                for (int j = a; j < z; ++j) {
                    const uint32_t c = tb[skew + j];
                    ch |= (c & 0x7f) << sh;
                    sh += 7;
                    if (c < 0x80) { h = 31u * h + (ch & 0xffffu); ch = 0; sh = 0; }
                    else if (sh > 14) sh = 14;                        // (not canonical: keep the shift defined)
                }
            }
            t0 += len;
        }
        if (lane < m) out[g] = live ? (int32_t)h : 0;
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// host side

struct fwa_wire_decoder {
    fwa_wire_schema sc;
    WireConst w;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // input staging (host inputs)
    uint8_t* d_in = nullptr;
    int64_t in_cap = 0;
    // level maps
    uint32_t* map0 = nullptr;
    int64_t map0_cap = 0;                  // entries
    uint8_t* lv_nxt = nullptr;             // all levels >= 1, concatenated
    uint32_t* lv_nrec = nullptr;
    uint32_t* lv_nevt = nullptr;
    int64_t lv_cap = 0;                    // entries
    uint8_t* ent = nullptr;                // per item of every level (concatenated): entry offset / dead
    uint64_t* rec = nullptr;
    uint64_t* evt = nullptr;
    int64_t ent_cap = 0;
    // outputs
    int64_t* key = nullptr;
    int64_t* ts = nullptr;
    void* col[FWA_MAX_COLS] = {};
    uint8_t* col_null[FWA_MAX_COLS] = {};
    uint8_t* key_null = nullptr;
    int64_t out_cap = 0;
    // STRING fields: per-record pass outputs and the extraction's outputs, [nstr][out_cap + 1]
    int32_t* str_len = nullptr;
    int64_t* str_src = nullptr;
    uint8_t* str_null = nullptr;
    int32_t* str_off = nullptr;
    uint8_t* str_bytes[FWA_WIRE_MAX_FIELDS] = {};
    int64_t str_bytes_cap[FWA_WIRE_MAX_FIELDS] = {};
    int64_t str_total[FWA_WIRE_MAX_FIELDS] = {};
    bool str_done[FWA_WIRE_MAX_FIELDS] = {};      // extracted since the last decode
    bool str_valid = false;                       // a decode succeeded and its input is taken to be resident
    const uint8_t* last_in = nullptr;             // device bytes of the last decode (staging buffer or the caller's)
    int64_t last_nbytes = 0, last_nrec = 0;
    void* scan_tmp = nullptr;
    size_t scan_tmp_cap = 0;
    unsigned long long* d_total = nullptr;
    int64_t* d_evt_pos = nullptr;
    int32_t* d_evt_tag = nullptr;
    int64_t* d_evt_val = nullptr;
    int64_t evt_cap = 0;
    std::vector<int64_t> h_evt_pos, h_evt_val;
    std::vector<int32_t> h_evt_tag;
    WireStatus* d_st = nullptr;
    WireStatus* h_st = nullptr;            // pinned
    uint32_t* h_root = nullptr;            // pinned: root nrec / nevt / nxt
    hipEvent_t ev[4] = {};
    fwa_wire_stats stats = {};
};

namespace {

int fail(fwa_wire_decoder* d, int code, const std::string& m) {
    if (d) d->err = m;
    return code;
}

#define WCK(call)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(d, e_ == hipErrorOutOfMemory ? FWA_E_OOM : FWA_E_DEVICE,                  \
                        std::string(#call ": ") + hipGetErrorString(e_));                          \
    } while (0)

template <class T>
int grow(fwa_wire_decoder* d, T** p, int64_t* cap, int64_t need, int64_t elem = sizeof(T)) {
    if (need <= *cap) return 0;
    int64_t n = std::max<int64_t>(need, *cap + *cap / 2);
    if (*p) WCK(hipFree(*p));
    *p = nullptr;
    WCK(hipMalloc((void**)p, std::max<int64_t>(n, 1) * elem));
    *cap = n;
    return 0;
}

int field_bytes(int t) { return (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) ? 8 : 4; }

int compose_fan(int S) {
    const int per = S * 9;                 // nrec + nevt + nxt per entry
    return std::max(2, std::min(64, kLdsBudget / per));
}

int grow_outputs(fwa_wire_decoder* d, int64_t n) {
    if (n <= d->out_cap) return 0;
    const int64_t cap = std::max<int64_t>(n, d->out_cap + d->out_cap / 2);
    auto re = [&](void** p, int64_t elem) -> int {
        if (*p) WCK(hipFree(*p));
        *p = nullptr;
        WCK(hipMalloc(p, std::max<int64_t>(cap, 1) * elem));
        return 0;
    };
    int rc;
    if ((rc = re((void**)&d->key, 8)) || (rc = re((void**)&d->ts, 8))) return rc;
    for (int j = 0; j < d->w.num_cols; ++j) {
        const int ft = d->w.ftype[d->w.col_field[j]];
        if ((rc = re(&d->col[j], ft == FWA_FIELD_FLOAT ? 4 : ft == FWA_FIELD_DECIMAL ? 16 : 8))) return rc;
        if (d->w.format == FWA_WIRE_ROWDATA && (rc = re((void**)&d->col_null[j], 1))) return rc;
    }
    if (d->w.format == FWA_WIRE_ROWDATA && (rc = re((void**)&d->key_null, 1))) return rc;
    if (d->w.nstr > 0) {
        const int64_t per = (int64_t)d->w.nstr * (cap + 1);
        auto rs = [&](void** p, int64_t elem) -> int {
            if (*p) WCK(hipFree(*p));
            *p = nullptr;
            WCK(hipMalloc(p, per * elem));
            return 0;
        };
        if ((rc = rs((void**)&d->str_len, 4)) || (rc = rs((void**)&d->str_src, 8)) || (rc = rs((void**)&d->str_null, 1)) ||
            (rc = rs((void**)&d->str_off, 4)))
            return rc;
    }
    d->out_cap = cap;
    return 0;
}

int grow_events(fwa_wire_decoder* d, int64_t n) {
    if (n <= d->evt_cap) return 0;
    const int64_t cap = std::max<int64_t>(n, 2 * d->evt_cap);
    int64_t c1 = 0, c2 = 0, c3 = 0;
    if (d->d_evt_pos) WCK(hipFree(d->d_evt_pos));
    if (d->d_evt_tag) WCK(hipFree(d->d_evt_tag));
    if (d->d_evt_val) WCK(hipFree(d->d_evt_val));
    d->d_evt_pos = nullptr; d->d_evt_tag = nullptr; d->d_evt_val = nullptr;
    int rc;
    if ((rc = grow(d, &d->d_evt_pos, &c1, cap)) || (rc = grow(d, &d->d_evt_tag, &c2, cap)) ||
        (rc = grow(d, &d->d_evt_val, &c3, 4 * cap)))
        return rc;
    d->evt_cap = cap;
    return 0;
}

}  // namespace

extern "C" {

int fwa_wire_create(const fwa_wire_schema* s, fwa_wire_decoder** out) {
    if (!s || !out) return FWA_E_ARG;
    *out = nullptr;
    fwa_wire_decoder* d = new fwa_wire_decoder();
    d->sc = *s;
    WireConst& w = d->w;
    memset(&w, 0, sizeof(w));
    auto bad = [&](int code, const char* m) { d->err = m; int c = code; fwa_wire_destroy(d); return c; };
    if (s->format != FWA_WIRE_TUPLE && s->format != FWA_WIRE_ROWDATA) return bad(FWA_E_ARG, "unknown wire format");
    if (s->arity < 1 || s->arity > FWA_WIRE_MAX_FIELDS) return bad(FWA_E_ARG, "arity out of range");
    if (s->num_cols < 0 || s->num_cols > FWA_MAX_COLS) return bad(FWA_E_ARG, "num_cols out of range");
    w.format = s->format;
    w.arity = s->arity;
    int off = 0, njs = 0;
    w.nullbits = ((s->arity + 63 + 8) / 64) * 8;                  // BinaryRowData.calculateBitSetWidthInBytes
    for (int f = 0; f < s->arity; ++f) {
        const int t = s->field[f];
        if (t < FWA_FIELD_LONG || (t > FWA_FIELD_STRING && t != FWA_FIELD_DECIMAL && t != FWA_FIELD_JSTRING))
            return bad(FWA_E_UNSUPPORTED, "unsupported field type");
        if (t == FWA_FIELD_JSTRING) {
            if (s->format != FWA_WIRE_TUPLE)
                return bad(FWA_E_UNSUPPORTED, "JSTRING fields (StringSerializer) are decoded in TUPLE values only: a row's "
                                              "CHAR / VARCHAR / STRING field is FWA_FIELD_STRING");
            w.str_field[w.nstr++] = f;
            ++njs;
        }
        if (t == FWA_FIELD_DECIMAL) {
            if (s->format != FWA_WIRE_ROWDATA)
                return bad(FWA_E_UNSUPPORTED, "DECIMAL fields are decoded in ROWDATA rows only: a Tuple's BigDecSerializer is "
                                              "another format");
            ++w.ndecf;
        }
        if (t == FWA_FIELD_STRING) {
            if (s->format != FWA_WIRE_ROWDATA)
                return bad(FWA_E_UNSUPPORTED, "STRING fields are decoded in ROWDATA rows only: a Tuple's StringSerializer writes "
                                              "varint-prefixed UTF-16 code units, and DataStream String keys are PREHASHED");
            w.str_field[w.nstr++] = f;
        }
        w.ftype[f] = t;
        if (s->format == FWA_WIRE_TUPLE) { w.foff[f] = off; off += t == FWA_FIELD_JSTRING ? 1 : field_bytes(t); }
        else w.foff[f] = w.nullbits + 8 * f;                      // (JSTRING schemas: the shortest value; foff is not used)
    }
    if (njs > 0 && s->key_field != -1)
        return bad(FWA_E_ARG, "a schema with JSTRING fields has key_field -1: the key is built from the string (fwa_keydict_encode, "
                              "fwa_jstring_hash)");
    auto integral = [&](int f) { return f >= 0 && f < s->arity && (w.ftype[f] == FWA_FIELD_LONG || w.ftype[f] == FWA_FIELD_INT); };
    if (!(s->key_field == -1 && w.nstr > 0) && !integral(s->key_field))
        return bad(FWA_E_ARG, "key_field must be a LONG or INT field (or -1 in a schema with STRING fields)");
    if (s->ts_field != -1 && !integral(s->ts_field)) return bad(FWA_E_ARG, "ts_field must be -1 or a LONG/INT field");
    w.key_field = s->key_field;
    w.ts_field = s->ts_field;
    w.num_cols = s->num_cols;
    for (int j = 0; j < s->num_cols; ++j) {
        if (s->col_field[j] < 0 || s->col_field[j] >= s->arity) return bad(FWA_E_ARG, "col_field out of range");
        if (w.ftype[s->col_field[j]] == FWA_FIELD_STRING) return bad(FWA_E_ARG, "a STRING field cannot be a value column");
        if (w.ftype[s->col_field[j]] == FWA_FIELD_JSTRING) return bad(FWA_E_ARG, "a JSTRING field cannot be a value column");
        if (w.ftype[s->col_field[j]] == FWA_FIELD_DECIMAL) ++w.ndec;
        w.col_field[j] = s->col_field[j];
    }
    int value_len;
    if (s->format == FWA_WIRE_TUPLE) value_len = off;
    else { w.row_size = w.nullbits + 8 * s->arity; value_len = 4 + w.row_size; }
    w.body[FWA_TAG_REC_WITH_TIMESTAMP] = 1 + 8 + value_len;
    w.body[FWA_TAG_REC_WITHOUT_TIMESTAMP] = 1 + value_len;
    w.body[FWA_TAG_WATERMARK] = 1 + 8;
    w.body[FWA_TAG_LATENCY_MARKER] = 1 + 8 + 8 + 8 + 4;
    w.body[FWA_TAG_STREAM_STATUS] = 1 + 4;
    w.body[FWA_TAG_RECORD_ATTRIBUTES] = 1 + 1;
    int mx = 0;
    for (int t = 0; t < 6; ++t) mx = std::max(mx, w.body[t]);
    w.step = 4 + mx;
    if (w.step > kMaxStep) return bad(FWA_E_UNSUPPORTED, "elements longer than 249 bytes");
    if (w.nstr + w.ndecf > 0) w.step = kMaxStep;                  // records up to the ceiling; body[0..1] are the shortest
    d->device = s->device;
    hipError_t e;
    if ((e = hipSetDevice(d->device)) != hipSuccess || (e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc((void**)&d->d_st, sizeof(WireStatus))) != hipSuccess ||
        (e = hipMalloc((void**)&d->d_total, 8)) != hipSuccess ||
        (e = hipHostMalloc((void**)&d->h_st, sizeof(WireStatus))) != hipSuccess ||
        (e = hipHostMalloc((void**)&d->h_root, 4 * sizeof(uint32_t))) != hipSuccess)
        return bad(FWA_E_DEVICE, hipGetErrorString(e));
    for (auto& x : d->ev)
        if ((e = hipEventCreate(&x)) != hipSuccess) return bad(FWA_E_DEVICE, hipGetErrorString(e));
    const int64_t hint = s->max_bytes > 0 ? s->max_bytes : (64ll << 20);
    int rc;
    if ((rc = grow_outputs(d, hint / (4 + std::min(w.body[0], w.body[1]))) ) || (rc = grow_events(d, 1 << 14))) {
        int c = rc;
        fwa_wire_destroy(d);
        return c;
    }
    *out = d;
    return FWA_OK;
}

void fwa_wire_destroy(fwa_wire_decoder* d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    void* ps[] = {d->d_in, d->map0, d->lv_nxt, d->lv_nrec, d->lv_nevt, d->ent, d->rec, d->evt, d->key, d->ts,
                  d->key_null, d->d_evt_pos, d->d_evt_tag, d->d_evt_val, d->d_st, d->str_len, d->str_src, d->str_null,
                  d->str_off, d->scan_tmp, d->d_total};
    for (void* p : ps) if (p) (void)hipFree(p);
    for (int j = 0; j < FWA_MAX_COLS; ++j) {
        if (d->col[j]) (void)hipFree(d->col[j]);
        if (d->col_null[j]) (void)hipFree(d->col_null[j]);
    }
    for (auto p : d->str_bytes) if (p) (void)hipFree(p);
    if (d->h_st) (void)hipHostFree(d->h_st);
    if (d->h_root) (void)hipHostFree(d->h_root);
    for (auto& x : d->ev) if (x) (void)hipEventDestroy(x);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

const char* fwa_wire_last_error(const fwa_wire_decoder* d) { return d ? d->err.c_str() : "null decoder"; }

int fwa_wire_get_stats(fwa_wire_decoder* d, fwa_wire_stats* out) {
    if (!d || !out) return FWA_E_ARG;
    *out = d->stats;
    return FWA_OK;
}

int fwa_wire_decode(fwa_wire_decoder* d, const uint8_t* bytes, int64_t nbytes, int32_t flags, fwa_wire_batch* out) {
    if (!d || !out || nbytes < 0 || (nbytes > 0 && !bytes)) return fail(d, FWA_E_ARG, "bad arguments");
    memset(out, 0, sizeof(*out));
    d->str_valid = false;
    WCK(hipSetDevice(d->device));
    const WireConst& w = d->w;
    const int S = w.step;
    const uint8_t* in = bytes;
    if (!(flags & FWA_WIRE_DEVICE_BYTES) && nbytes > 0) {
        int rc = grow(d, &d->d_in, &d->in_cap, nbytes);
        if (rc) return rc;
        WCK(hipMemcpyAsync(d->d_in, bytes, nbytes, hipMemcpyHostToDevice, d->stream));
        in = d->d_in;
    }
    const bool aligned = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    const int64_t nchunks = nbytes / kChunk + 1;                  // the last chunk always holds the stream end
    // level sizes
    const int fan = compose_fan(S);
    std::vector<int64_t> n_items{nchunks};
    while (n_items.back() > 1) n_items.push_back((n_items.back() + fan - 1) / fan);
    const int L = (int)n_items.size();                            // levels 0..L-1, level L-1 has 1 item
    std::vector<int64_t> lv_off(L, 0), it_off(L, 0);              // level l >= 1 map offset; item offset (all levels)
    int64_t lv_total = 0, it_total = 0;
    for (int l = 0; l < L; ++l) {
        it_off[l] = it_total;
        it_total += n_items[l] + 1;
        if (l >= 1) { lv_off[l] = lv_total; lv_total += n_items[l] * S; }
    }
    int rc;
    if ((rc = grow(d, &d->map0, &d->map0_cap, nchunks * S))) return rc;
    if (lv_total > d->lv_cap) {                                   // the three level arrays share one capacity
        for (void* p : {(void*)d->lv_nxt, (void*)d->lv_nrec, (void*)d->lv_nevt}) if (p) WCK(hipFree(p));
        d->lv_nxt = nullptr; d->lv_nrec = nullptr; d->lv_nevt = nullptr;
        const int64_t cap = std::max<int64_t>(lv_total, d->lv_cap + d->lv_cap / 2);
        WCK(hipMalloc((void**)&d->lv_nxt, cap));
        WCK(hipMalloc((void**)&d->lv_nrec, cap * 4));
        WCK(hipMalloc((void**)&d->lv_nevt, cap * 4));
        d->lv_cap = cap;
    }
    if (it_total > d->ent_cap) {                                  // per-item entry / bases, all levels
        for (void* p : {(void*)d->ent, (void*)d->rec, (void*)d->evt}) if (p) WCK(hipFree(p));
        d->ent = nullptr; d->rec = nullptr; d->evt = nullptr;
        const int64_t cap = std::max<int64_t>(it_total, d->ent_cap + d->ent_cap / 2);
        WCK(hipMalloc((void**)&d->ent, cap));
        WCK(hipMalloc((void**)&d->rec, cap * 8));
        WCK(hipMalloc((void**)&d->evt, cap * 8));
        d->ent_cap = cap;
    }
    // worst case records: every element a record of the shorter record kind
    if ((rc = grow_outputs(d, nbytes / (4 + std::min(w.body[0], w.body[1])) + 1))) return rc;

    hipStream_t st = d->stream;
    WCK(hipMemsetAsync(d->d_st, 0, sizeof(WireStatus), st));
    WCK(hipEventRecord(d->ev[0], st));
    const unsigned grid = (unsigned)std::min<int64_t>(nchunks, kPersistBlocks);
    const bool var = w.nstr + w.ndecf > 0;
    const bool js = var && w.format == FWA_WIRE_TUPLE;           // JSTRING fields: the only variable-length TUPLE values
    if (js) hipLaunchKernelGGL((wire_scan_kernel<true, true>), dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w, aligned, d->map0);
    else if (var) hipLaunchKernelGGL(wire_scan_kernel<true>, dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w, aligned, d->map0);
    else hipLaunchKernelGGL(wire_scan_kernel<false>, dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w, aligned, d->map0);
    WCK(hipGetLastError());
    WCK(hipEventRecord(d->ev[1], st));
    auto level_map = [&](int l) {
        LevelMap m{};
        if (l == 0) m.packed = d->map0;
        else { m.nxt = d->lv_nxt + lv_off[l]; m.nrec = d->lv_nrec + lv_off[l]; m.nevt = d->lv_nevt + lv_off[l]; }
        return m;
    };
    const int tpb = S <= 64 ? 64 : (S <= 128 ? 128 : 256);
    const size_t lds = (size_t)fan * S * 9 + 16;
    for (int l = 0; l + 1 < L; ++l) {
        hipLaunchKernelGGL(wire_compose_kernel, dim3((unsigned)n_items[l + 1]), dim3(tpb), lds, st, level_map(l),
                           n_items[l], S, fan, d->lv_nxt + lv_off[l + 1], d->lv_nrec + lv_off[l + 1],
                           d->lv_nevt + lv_off[l + 1]);
        WCK(hipGetLastError());
    }
    // root: entry 0, first record / event 0
    const int64_t root = it_off[L - 1];
    WCK(hipMemsetAsync(d->ent + root, 0, 1, st));
    WCK(hipMemsetAsync(d->rec + root, 0, 8, st));
    WCK(hipMemsetAsync(d->evt + root, 0, 8, st));
    for (int l = L - 2; l >= 0; --l) {
        hipLaunchKernelGGL(wire_resolve_kernel, dim3((unsigned)n_items[l + 1]), dim3(tpb), lds, st, level_map(l),
                           n_items[l], S, fan, d->ent + it_off[l + 1], d->rec + it_off[l + 1], d->evt + it_off[l + 1],
                           d->ent + it_off[l], d->rec + it_off[l], d->evt + it_off[l]);
        WCK(hipGetLastError());
    }
    // totals of the whole call = the root map at entry 0
    if (L == 1) {
        WCK(hipMemcpyAsync(d->h_root, d->map0, 4, hipMemcpyDeviceToHost, st));
    } else {
        WCK(hipMemcpyAsync(d->h_root + 1, d->lv_nrec + lv_off[L - 1], 4, hipMemcpyDeviceToHost, st));
        WCK(hipMemcpyAsync(d->h_root + 2, d->lv_nevt + lv_off[L - 1], 4, hipMemcpyDeviceToHost, st));
    }
    DecodeOut o{};
    o.key = d->key;
    o.ts = d->ts;
    for (int j = 0; j < FWA_MAX_COLS; ++j) { o.col[j] = d->col[j]; o.col_null[j] = d->col_null[j]; }
    o.key_null = d->key_null;
    o.st = d->d_st;
    o.str_len = d->str_len;
    o.str_src = d->str_src;
    o.str_null = d->str_null;
    o.str_stride = d->out_cap + 1;
    for (int pass = 0; pass < 2; ++pass) {
        o.evt_pos = d->d_evt_pos;
        o.evt_tag = d->d_evt_tag;
        o.evt_val = d->d_evt_val;
        o.evt_cap = d->evt_cap;
        if (js) hipLaunchKernelGGL((wire_decode_kernel<true, false, true>), dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w,
                                   aligned, d->ent, d->rec, d->evt, o);
        else if (w.ndec > 0) hipLaunchKernelGGL((wire_decode_kernel<true, true>), dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w,
                                           aligned, d->ent, d->rec, d->evt, o);
        else if (var) hipLaunchKernelGGL(wire_decode_kernel<true>, dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w, aligned,
                                         d->ent, d->rec, d->evt, o);
        else hipLaunchKernelGGL(wire_decode_kernel<false>, dim3(grid), dim3(64), 0, st, in, nbytes, nchunks, w, aligned,
                                d->ent, d->rec, d->evt, o);
        WCK(hipGetLastError());
        WCK(hipEventRecord(d->ev[2], st));
        WCK(hipMemcpyAsync(d->h_st, d->d_st, sizeof(WireStatus), hipMemcpyDeviceToHost, st));
        WCK(hipStreamSynchronize(st));
        int64_t nrec, nevt;
        if (L == 1) { nrec = (d->h_root[0] >> 8) & 0xFFF; nevt = d->h_root[0] >> 20; }
        else { nrec = d->h_root[1]; nevt = d->h_root[2]; }
        if (nevt > d->evt_cap && pass == 0) {                     // more events than the list holds: grow, decode again
            if ((rc = grow_events(d, nevt))) return rc;
            WCK(hipMemsetAsync(d->d_st, 0, sizeof(WireStatus), st));
            continue;
        }
        float ms_scan = 0, ms_all = 0;
        (void)hipEventElapsedTime(&ms_scan, d->ev[0], d->ev[1]);
        (void)hipEventElapsedTime(&ms_all, d->ev[0], d->ev[2]);
        d->stats.calls++;
        d->stats.bytes_in += nbytes;
        d->stats.scan_ms += ms_scan;
        d->stats.decode_ms += ms_all;
        const WireStatus& hs = *d->h_st;
        if (hs.error) {
            char m[256];
            if (hs.error == FWA_E_CORRUPT && hs.err_tag < 256) snprintf(m, sizeof m, "Corrupt stream, found tag: %d (element at byte %lld)", hs.err_tag, (long long)hs.err_pos);
            else if (hs.error == FWA_E_ARG) snprintf(m, sizeof m, "NULL rowtime field in the row at byte %lld", (long long)hs.err_pos);
            else if (hs.err_tag == kErrSlot) snprintf(m, sizeof m, "Corrupt stream: a STRING slot points outside its row (record at byte %lld)", (long long)hs.err_pos);
            else if (hs.err_tag == kErrDecSlot) snprintf(m, sizeof m, "Corrupt stream: a DECIMAL slot names bytes outside its row, none or more than 16 (record at byte %lld)", (long long)hs.err_pos);
            else if (hs.err_tag == kErrJstr) snprintf(m, sizeof m, "Corrupt stream: the fields of a TUPLE value do not end at its element's end, or a String is not in StringValue's canonical form (record at byte %lld)", (long long)hs.err_pos);
            else if (hs.err_tag == kErrTooLong) snprintf(m, sizeof m, "element longer than the %d-byte limit at byte %lld", (int)kMaxBody, (long long)hs.err_pos);
            else if (hs.err_tag >= 256) snprintf(m, sizeof m, "RowKind %d at byte %lld: window aggregation consumes insert-only rows", hs.err_tag - 256, (long long)hs.err_pos);
            else snprintf(m, sizeof m, "row size differs from the schema's fixed-length row at byte %lld", (long long)hs.err_pos);
            return fail(d, hs.error, m);
        }
        d->stats.records_out += nrec;
        if (nevt > 0) {
            d->h_evt_pos.resize(nevt);
            d->h_evt_tag.resize(nevt);
            d->h_evt_val.resize(4 * nevt);
            WCK(hipMemcpy(d->h_evt_pos.data(), d->d_evt_pos, nevt * 8, hipMemcpyDeviceToHost));
            WCK(hipMemcpy(d->h_evt_tag.data(), d->d_evt_tag, nevt * 4, hipMemcpyDeviceToHost));
            WCK(hipMemcpy(d->h_evt_val.data(), d->d_evt_val, nevt * 32, hipMemcpyDeviceToHost));
        }
        out->n_records = nrec;
        out->n_events = nevt;
        out->consumed = hs.consumed;
        out->key = w.key_field >= 0 ? d->key : nullptr;
        out->ts = d->ts;
        for (int j = 0; j < w.num_cols; ++j) { out->col[j] = d->col[j]; out->col_null[j] = d->col_null[j]; }
        out->key_null = w.key_field >= 0 ? d->key_null : nullptr;
        if (var) {
            d->str_valid = true;
            d->last_in = in;
            d->last_nbytes = nbytes;
            d->last_nrec = nrec;
            for (auto& x : d->str_done) x = false;
        }
        out->evt_pos = nevt ? d->h_evt_pos.data() : nullptr;
        out->evt_tag = nevt ? d->h_evt_tag.data() : nullptr;
        out->evt_val = nevt ? d->h_evt_val.data() : nullptr;
        return FWA_OK;
    }
    return fail(d, FWA_E_STATE, "event list did not settle");
}

int fwa_wire_strings_of(fwa_wire_decoder* d, int32_t field, fwa_wire_strings* out) {
    if (!d || !out) return fail(d, FWA_E_ARG, "bad arguments");
    memset(out, 0, sizeof(*out));
    const WireConst& w = d->w;
    int k = -1;
    for (int i = 0; i < w.nstr; ++i) if (w.str_field[i] == field) k = i;
    if (k < 0) return fail(d, FWA_E_ARG, "not a STRING / JSTRING field of the schema");
    if (!d->str_valid) return fail(d, FWA_E_STATE, "no decoded batch: strings follow a successful fwa_wire_decode");
    const int64_t n = d->last_nrec, stride = d->out_cap + 1;
    const int32_t* len = d->str_len + k * stride;
    int32_t* off = d->str_off + k * stride;
    if (!d->str_done[k]) {
        WCK(hipSetDevice(d->device));
        hipStream_t st = d->stream;
        if (d->last_nbytes >= (1ll << 31)) {                      // only then can the values reach 2^31 bytes
            unsigned long long total = 0;
            WCK(hipMemsetAsync(d->d_total, 0, 8, st));
            hipLaunchKernelGGL(wire_len_sum_kernel, dim3(1024), dim3(256), 0, st, len, n, d->d_total);
            WCK(hipGetLastError());
            WCK(hipMemcpyAsync(&total, d->d_total, 8, hipMemcpyDeviceToHost, st));
            WCK(hipStreamSynchronize(st));
            if (total >= (1ull << 31)) return fail(d, FWA_E_UNSUPPORTED, "the field's values of one decode reach 2^31 bytes (int32 offsets)");
        }
        size_t tb = 0;                                            // n + 1 items: offsets[n] = the total (len[n] is not used)
        WCK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, len, off, (int)(n + 1), st));
        if (tb > d->scan_tmp_cap) {
            if (d->scan_tmp) WCK(hipFree(d->scan_tmp));
            d->scan_tmp = nullptr;
            d->scan_tmp_cap = 0;
            WCK(hipMalloc(&d->scan_tmp, tb));
            d->scan_tmp_cap = tb;
        }
        WCK(hipcub::DeviceScan::ExclusiveSum(d->scan_tmp, tb, len, off, (int)(n + 1), st));
        int32_t total = 0;
        WCK(hipMemcpyAsync(&total, off + n, 4, hipMemcpyDeviceToHost, st));
        WCK(hipStreamSynchronize(st));
        int rc = grow(d, &d->str_bytes[k], &d->str_bytes_cap[k], std::max<int64_t>(total, 1));
        if (rc) return rc;
        if (total > 0) {
            const unsigned grid = (unsigned)std::min<int64_t>((n + 64 * kGatherWaves - 1) / (64 * kGatherWaves), 256 * 16);
            hipLaunchKernelGGL(wire_gather_kernel, dim3(grid), dim3(64 * kGatherWaves), 0, st, d->last_in, d->str_src + k * stride,
                               off, n, d->str_bytes[k]);
            WCK(hipGetLastError());
            WCK(hipStreamSynchronize(st));
        }
        d->str_total[k] = total;
        d->str_done[k] = true;
    }
    out->offsets = off;
    out->bytes = d->str_bytes[k];
    out->null = d->str_null + k * stride;
    out->total_bytes = d->str_total[k];
    return FWA_OK;
}

int fwa_jstring_hash(const int32_t* offsets, const uint8_t* bytes, const uint8_t* nulls, int64_t n, int32_t* out,
                     int32_t device) {
    if (n < 0 || n >= (1ll << 31) || (n > 0 && (!offsets || !out))) return FWA_E_ARG;
    if (n == 0) return FWA_OK;
    if (hipSetDevice(device) != hipSuccess) return FWA_E_DEVICE;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 63) / 64, 256 * 32);
    hipLaunchKernelGGL(wire_jstring_hash_kernel, dim3(grid), dim3(64), 0, 0, offsets, bytes, nulls, n, out);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return FWA_E_DEVICE;
    return FWA_OK;
}

}  // extern "C"

#include "wire_encode.inc"
