// wire_encode.inc -- the sender side of include/flink_amd_wire.h (fwa_wire_encode), included at the end of wire.hip.
//
// The rows of one watermark step (fwa_out's SoA columns, and the decoded key dictionary columns of a Table job) become
// the channel bytes RecordWriter would have produced: be32 L | tag | [be64 ts] | value per row, then the step's
// non-record elements. Two sets of kernels:
//
//   fixed-length schemas: every element has E bytes and element i starts at i * E. E is rarely a multiple of 4 (37, 45,
//     57), so a lane storing its own element would scatter unaligned byte stores over HBM. Instead a wave takes a tile of
//     64 rows -- 64 * E bytes, a multiple of 16 whatever E is, so every tile starts 16-byte aligned and only the last one
//     has a ragged tail -- reads its columns coalesced (lane r reads row r of each column), assembles the 64 elements in
//     LDS, and streams the tile's contiguous bytes to HBM with 16-byte stores, consecutive lanes writing consecutive
//     vectors. In LDS an element's fields straddle words that the neighbouring rows' elements share, so the buffer is
//     zeroed and every field is OR-ed into its (up to three) aligned words with ds_or_b32: no lane reads a word another
//     lane is assembling. Each output byte is written once.
//
//   schemas with STRING fields (VAR): a size pass (fixed part + the 8-rounded lengths of the values longer than 7
//     bytes), an exclusive scan to 64-bit element offsets (hipcub), and the write pass: a wave per 64 rows, whose bytes
//     [off[base], off[base + m]) are again one contiguous run. It is staged in LDS at the run's own 16-byte phase when it
//     fits kEncTile (head and tail bytes of the run are stored byte-wise by this tile, the aligned middle with 16-byte
//     stores). In a staged tile the row's lane also brings its values in: unaligned 8-byte loads (the 64 values of a field
//     are one contiguous run of the Arrow bytes, so the wave's loads share their cache lines) OR-ed into LDS like any
//     field. A run too long for LDS (one 70 000-byte value is enough) is written directly: the fixed parts with byte
//     stores, the values byte-parallel like wire_gather_kernel's -- consecutive lanes take consecutive source bytes and
//     find their row by a binary search over the wave's 65 offsets.
//
//   schemas with DECIMAL fields (DEC) take the same three passes, instantiated a second time: a non-NULL DECIMAL result
//     adds 16 bytes to its element (AbstractBinaryWriter.writeDecimal :164-196), and the row's lane writes them through
//     the sink in both the staged and the direct path -- the minimal big-endian bytes of the 128-bit value (BigInteger.
//     toByteArray: bitLength / 8 + 1 of them, from the count of leading sign bits), zeros up to 16, slot = cursor << 32 |
//     length. A NULL result is setNullAt (RowDataSerializer.toBinaryRow :196-212): the bit, a zero slot, nothing reserved.
//     Schemas without a DECIMAL field run the instantiations they ran.
//
//   TUPLE values with JSTRING fields (JS) are a third instantiation of the three passes. A String field is the varint of
//     its code-unit count + 1 and then the key dictionary's char bytes verbatim (the canonical form: the count is the
//     number of bytes below 0x80, counted eight bytes at a time), and the fields behind it follow unaligned, so the row's
//     lane walks the fields with a running position instead of the schema's offsets. Staged tiles take the bytes
//     through the sink like a STRING's; in the direct path the wave goes field by field -- the lanes write their fixed
//     fields and length prefixes, then the field's values are copied byte-parallel as above.
//
// The trailing events (a handful) are laid out on the host and copied behind the rows on the encoder's stream.
// HBM traffic: every column read once, every output byte written once; VAR adds 16 B per row of sizes / offsets.

namespace {

enum EncClass { kEncI64 = 0, kEncI32 = 1, kEncF64 = 2, kEncF32 = 3, kEncStr = 4, kEncDec = 5 };
constexpr int kEncTile = 12 * 1024;          // VAR: LDS bytes of a staged tile (per single-wave block)
constexpr int64_t kEncBlocks = 256 * 16;     // persistent single-wave blocks

struct EncConst {
    int32_t format, arity, with_ts;
    int32_t efix;                            // element bytes, length prefix included, fixed part only
    int32_t hdr;                             // prefix + tag + [timestamp]: where the value starts (5 or 13)
    int32_t row_size, nullbits;              // ROWDATA: fixed part of the row, width of its null-bit set
    int32_t nstr;                            // STRING fields (> 0: elements vary in size)
    int32_t ftype[FWA_WIRE_MAX_FIELDS];      // wire type
    int32_t scls[FWA_WIRE_MAX_FIELDS];       // EncClass of the source column
    int32_t adj[FWA_WIRE_MAX_FIELDS];        // added to an int64 source (WIN_TIME: -1)
    int32_t foff[FWA_WIRE_MAX_FIELDS];       // offset of the field (TUPLE) / its slot (ROWDATA) in the element
    int32_t ndec;                            // DECIMAL fields (> 0: elements vary in size too); behind the members above,
                                             // so that those keep their places in the kernel argument
    int32_t njs;                             // JSTRING fields of a TUPLE value (> 0: elements vary in size; efix counts
                                             // none of their bytes and foff is not used)
};

struct EncCols {
    const void* col[FWA_WIRE_MAX_FIELDS];
    const uint8_t* nul[FWA_WIRE_MAX_FIELDS];
    const int32_t* soff[FWA_WIRE_MAX_FIELDS];    // STRING: Arrow offsets / bytes
    const uint8_t* sbytes[FWA_WIRE_MAX_FIELDS];
    const int64_t* win_end;                      // record timestamps (with_ts)
};

// The wire bits of field f of row g in the low bytes (INT / FLOAT: 32 bits, upper half zero).
__device__ __forceinline__ uint64_t enc_load(const EncConst& c, const EncCols& k, int f, int64_t g) {
    const int cls = c.scls[f];
    uint64_t v;
    if (cls == kEncI64) v = (uint64_t)(reinterpret_cast<const int64_t*>(k.col[f])[g] + c.adj[f]);
    else if (cls == kEncF64) v = reinterpret_cast<const uint64_t*>(k.col[f])[g];
    else if (cls == kEncI32) v = (uint64_t)(int64_t)reinterpret_cast<const int32_t*>(k.col[f])[g];
    else v = reinterpret_cast<const uint32_t*>(k.col[f])[g];
    const int t = c.ftype[f];
    return (t == FWA_FIELD_INT || t == FWA_FIELD_FLOAT) ? (v & 0xffffffffull) : v;
}

// An element under assembly in zeroed LDS: bytes are OR-ed into their aligned words (neighbouring elements share words).
struct EncLdsSink {
    uint32_t* w;
    int base;                                // byte position of the element in the buffer
    // v holds nbytes (1..8) bytes, little-endian, the rest zero
    __device__ __forceinline__ void put(int pos, uint64_t v, int nbytes) const {
        const int p = base + pos, i = p >> 2, b = p & 3, sh = b * 8;
        const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
        atomicOr(&w[i], lo << sh);
        if (b + nbytes > 4) atomicOr(&w[i + 1], sh ? (lo >> (32 - sh)) | (hi << sh) : hi);
        if (b + nbytes > 8) atomicOr(&w[i + 2], hi >> (32 - sh));             // (b > 0 here)
    }
    __device__ __forceinline__ void zero(int64_t, int) const {}               // the buffer is zeroed
};

// The same straight to HBM (tiles too long for LDS): byte stores, every byte of the element exactly once.
struct EncGlobalSink {
    uint8_t* p;                              // the element's first byte
    __device__ __forceinline__ void put(int pos, uint64_t v, int nbytes) const {
        for (int b = 0; b < nbytes; ++b) p[pos + b] = (uint8_t)(v >> (8 * b));
    }
    __device__ __forceinline__ void zero(int64_t pos, int n) const {
        for (int b = 0; b < n; ++b) p[pos + b] = 0;
    }
};

// nb (0..8) bytes of a STRING value at p, little-endian. whole: the 8 bytes at p lie inside the column's bytes, so one
// unaligned 8-byte load serves; the last values of a column are read byte by byte instead of past its end.
__device__ __forceinline__ uint64_t enc_str_bytes(const uint8_t* __restrict__ p, int nb, bool whole) {
    uint64_t v = 0;
    if (whole) {
        __builtin_memcpy(&v, p, 8);
        if (nb < 8) v &= (1ull << (8 * nb)) - 1;
    } else
        for (int b = 0; b < nb; ++b) v |= (uint64_t)p[b] << (8 * b);
    return v;
}

// Code units of a value in the canonical char-byte form: its bytes below 0x80.
__device__ __forceinline__ int64_t enc_js_chars(const uint8_t* __restrict__ p, int64_t len, int64_t so, int64_t end) {
    int64_t cnt = 0;
    for (int64_t o = 0; o < len; o += 8) {
        const int nb = (int)std::min<int64_t>(8, len - o);
        const uint64_t v = enc_str_bytes(p + o, nb, so + o + 8 <= end);
        cnt += nb - __builtin_popcountll(v & 0x8080808080808080ull);
    }
    return cnt;
}

// StringValue.writeString's length prefix: x in 7-bit groups, low group first, as little-endian bytes; *nb = 1..5.
__device__ __forceinline__ uint64_t enc_varint(uint64_t x, int* nb) {
    uint64_t v = 0;
    int i = 0;
    for (;; ++i) {
        const uint64_t grp = x & 0x7f;
        x >>= 7;
        v |= (grp | (x ? 0x80ull : 0ull)) << (8 * i);
        if (!x) break;
    }
    *nb = i + 1;
    return v;
}

__device__ __forceinline__ int enc_varint_len(uint64_t x) { return x < (1ull << 7) ? 1 : x < (1ull << 14) ? 2 : x < (1ull << 21) ? 3 : x < (1ull << 28) ? 4 : 5; }

// Row g's element (esize: its bytes, prefix included). COPY: with the bytes of its STRING values, 8 at a time through
// the sink; otherwise those are left to the caller's copy pass. n: the rows of the call (the columns' end).
// DEC: the schema has DECIMAL fields; their 16 reserved bytes always go through the sink.
template <bool VAR, bool COPY, bool DEC, bool JS = false, class Sink>
__device__ __forceinline__ void enc_element(const EncConst& c, const EncCols& k, int64_t g, int64_t esize, const Sink& s,
                                            int64_t n = 0) {
    const uint32_t L = (uint32_t)(esize - 4);
    s.put(0, (uint64_t)__builtin_bswap32(L) | ((uint64_t)(c.with_ts ? FWA_TAG_REC_WITH_TIMESTAMP : FWA_TAG_REC_WITHOUT_TIMESTAMP) << 32), 5);
    if (c.with_ts) s.put(5, __builtin_bswap64((uint64_t)(k.win_end[g] - 1)), 8);
    if (c.format == FWA_WIRE_TUPLE) {
        if constexpr (JS) {                                       // (staged tiles only: COPY)
            int pos = c.hdr;
            for (int f = 0; f < c.arity; ++f) {
                const int t = c.ftype[f];
                if (t == FWA_FIELD_JSTRING) {
                    const int64_t so = k.soff[f][g];
                    const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - so);
                    const int64_t end = (int64_t)k.soff[f][n];
                    const uint8_t* __restrict__ src = k.sbytes[f] + so;
                    int nb;
                    const uint64_t lv = enc_varint((uint64_t)enc_js_chars(src, len, so, end) + 1, &nb);
                    s.put(pos, lv, nb);
                    pos += nb;
                    for (int64_t o = 0; o < len; o += 8)
                        s.put(pos + (int)o, enc_str_bytes(src + o, (int)std::min<int64_t>(8, len - o), so + o + 8 <= end),
                              (int)std::min<int64_t>(8, len - o));
                    pos += (int)len;
                    continue;
                }
                const uint64_t v = enc_load(c, k, f, g);
                if (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) { s.put(pos, __builtin_bswap64(v), 8); pos += 8; }
                else { s.put(pos, __builtin_bswap32((uint32_t)v), 4); pos += 4; }
            }
            return;
        }
        for (int f = 0; f < c.arity; ++f) {
            const uint64_t v = enc_load(c, k, f, g);
            const int t = c.ftype[f];
            if (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) s.put(c.foff[f], __builtin_bswap64(v), 8);
            else s.put(c.foff[f], __builtin_bswap32((uint32_t)v), 4);
        }
        return;
    }
    const int row = c.hdr + 4;
    s.put(c.hdr, __builtin_bswap32((uint32_t)(esize - row)), 4);
    uint64_t nullbits = 0;                                        // byte 0: RowKind INSERT
    int64_t cursor = c.row_size;
    for (int f = 0; f < c.arity; ++f) {
        const bool isnull = k.nul[f] && k.nul[f][g];
        uint64_t slot = 0;
        if (isnull) nullbits |= 1ull << (f + 8);                  // setNullAt: the bit, and a zero slot
        else if (VAR && c.ftype[f] == FWA_FIELD_STRING) {
            const int64_t so = k.soff[f][g];
            const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - so);   // (offsets never decrease)
            const int64_t end = COPY ? (int64_t)k.soff[f][n] : 0;  // the column's bytes end here
            const uint8_t* __restrict__ src = k.sbytes[f] + so;
            if (len <= 7) {                                       // inline: 0x80 | length on top of the bytes
                slot = (0x80ull | (uint64_t)len) << 56;
                if constexpr (COPY) s.put(c.foff[f], slot | enc_str_bytes(src, (int)len, so + 8 <= end), 8);
                else s.put(c.foff[f] + (int)len, slot >> (8 * len), 8 - (int)len);   // bytes [0, len): the copy pass
                continue;
            }
            slot = ((uint64_t)cursor << 32) | (uint64_t)len;
            const int64_t r8 = (len + 7) & ~7ll;
            if constexpr (COPY)
                for (int64_t o = 0; o < len; o += 8)
                    s.put((int)(row + cursor + o), enc_str_bytes(src + o, (int)std::min<int64_t>(8, len - o), so + o + 8 <= end),
                          (int)std::min<int64_t>(8, len - o));
            s.zero(row + cursor + len, (int)(r8 - len));
            cursor += r8;
        } else if (DEC && c.ftype[f] == FWA_FIELD_DECIMAL) {
            const uint64_t* __restrict__ v = reinterpret_cast<const uint64_t*>(k.col[f]) + 2 * g;   // low, high
            const uint64_t lo = v[0], hi = v[1];
            const uint64_t sx = (uint64_t)((int64_t)hi >> 63);     // BigInteger.bitLength: the bits below the sign bits
            const uint64_t xh = hi ^ sx, xl = lo ^ sx;
            const int bits = xh ? 128 - __builtin_clzll(xh) : xl ? 64 - __builtin_clzll(xl) : 0;
            const int len = bits / 8 + 1;                          // toByteArray: 1..16 bytes
            const int sh = 128 - 8 * len;                          // the value's top `len` bytes, zeros behind them
            const uint64_t top = sh >= 64 ? lo << (sh - 64) : sh ? (hi << sh) | (lo >> (64 - sh)) : hi;
            const uint64_t low = sh >= 64 ? 0 : lo << sh;
            slot = ((uint64_t)cursor << 32) | (uint64_t)len;
            s.put((int)(row + cursor), __builtin_bswap64(top), 8);
            s.put((int)(row + cursor) + 8, __builtin_bswap64(low), 8);
            cursor += 16;
        } else slot = enc_load(c, k, f, g);
        s.put(c.foff[f], slot, 8);
    }
    s.put(row, nullbits, c.nullbits);
}

// ---- fixed-length schemas: one wave per tile of 64 rows, assembled in LDS, streamed out in 16-byte vectors ----
__global__ __launch_bounds__(64) void wire_enc_fixed_kernel(EncConst c, EncCols k, int64_t n, uint8_t* __restrict__ out) {
    extern __shared__ u32x4 enc_buf[];                            // 64 * efix + 32 bytes
    uint32_t* w = reinterpret_cast<uint32_t*>(enc_buf);
    const int lane = threadIdx.x;
    const int64_t ntiles = (n + 63) / 64;
    const int full = 64 * c.efix;                                 // bytes of a whole tile, a multiple of 64
    const u32x4 z = {0, 0, 0, 0};
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * 64;
        const int m = (int)std::min<int64_t>(64, n - base);
        const int bytes = m * c.efix;
        const int nz = (bytes + 15) / 16 + 1;                     // one vector past the end: put() may OR a zero there
        __syncthreads();                                          // the previous tile has been streamed out
        for (int i = lane; i < nz; i += 64) enc_buf[i] = z;
        __syncthreads();
        if (lane < m) enc_element<false, false, false>(c, k, base + lane, c.efix, EncLdsSink{w, lane * c.efix});
        __syncthreads();
        uint8_t* dst = out + tile * (int64_t)full;                // 16-byte aligned (out is, full is a multiple of 16)
        const int nfull = bytes >> 4;
        for (int i = lane; i < nfull; i += 64) reinterpret_cast<u32x4*>(dst)[i] = enc_buf[i];
        const uint8_t* bb = reinterpret_cast<const uint8_t*>(w);
        for (int b = (nfull << 4) + lane; b < bytes; b += 64) dst[b] = bb[b];   // the last tile's ragged tail
    }
}

// ---- VAR: element sizes ----
template <bool DEC, bool JS = false>
__global__ __launch_bounds__(256) void wire_enc_size_kernel(EncConst c, EncCols k, int64_t n, int64_t* __restrict__ size) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= n; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = 0;
        if (g < n) {
            s = c.efix;
            for (int f = 0; f < c.arity; ++f) {
                if constexpr (JS) {
                    if (c.ftype[f] != FWA_FIELD_JSTRING) continue;
                    const int64_t so = k.soff[f][g];
                    const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - so);
                    s += enc_varint_len((uint64_t)enc_js_chars(k.sbytes[f] + so, len, so, (int64_t)k.soff[f][n]) + 1) + len;
                    continue;
                }
                if (DEC && c.ftype[f] == FWA_FIELD_DECIMAL) {
                    if (!(k.nul[f] && k.nul[f][g])) s += 16;
                    continue;
                }
                if (c.ftype[f] != FWA_FIELD_STRING || (k.nul[f] && k.nul[f][g])) continue;
                const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - k.soff[f][g]);   // (offsets never decrease)
                if (len > 7) s += (len + 7) & ~7ll;
            }
        }
        size[g] = s;                                              // size[n] = 0: the scan's last item is the total
    }
}

// ---- VAR: the write pass ----
template <bool DEC, bool JS = false>
__global__ __launch_bounds__(64) void wire_enc_var_kernel(EncConst c, EncCols k, int64_t n, const int64_t* __restrict__ eoff,
                                                           uint8_t* __restrict__ out) {
    __shared__ u32x4 buf[(kEncTile + 48) / 16];
    __shared__ int32_t s_so[65];                                  // the current STRING field: Arrow offsets of the wave's rows
    __shared__ int64_t s_dst[64];                                 // where each row's value goes (-1: NULL, nothing)
    uint32_t* w = reinterpret_cast<uint32_t*>(buf);
    uint8_t* wb = reinterpret_cast<uint8_t*>(buf);
    const int lane = threadIdx.x;
    const int64_t ntiles = (n + 63) / 64;
    const int row = c.hdr + 4;
    const u32x4 z = {0, 0, 0, 0};
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t base = tile * 64;
        const int m = (int)std::min<int64_t>(64, n - base);
        const int64_t b0 = eoff[base], b1 = eoff[base + m];
        const int64_t tb = b1 - b0;
        const int skew = (int)(b0 & 15);                          // the run keeps its 16-byte phase in LDS
        const bool staged = tb + skew <= kEncTile;
        const int64_t g = base + lane;
        const int64_t es = lane < m ? eoff[g] : b1;
        const int64_t esize = lane < m ? eoff[g + 1] - es : 0;
        // position of this lane's element: in the buffer (staged) or in the output (direct)
        const int64_t epos = staged ? skew + (es - b0) : es;
        __syncthreads();                                          // the previous tile has been streamed out
        if (staged) {
            const int nz = (int)((skew + tb + 15) >> 4) + 1;
            for (int i = lane; i < nz; i += 64) buf[i] = z;
            __syncthreads();
            if (lane < m) enc_element<true, true, DEC, JS>(c, k, g, esize, EncLdsSink{w, (int)epos}, n);
        } else if constexpr (JS) {
            // a run longer than the LDS tile, TUPLE values: field by field, the lanes write their fixed fields and length
            // prefixes at their running positions, then the wave copies the field's values byte-parallel
            const EncGlobalSink gs{out + es};
            int64_t pos = c.hdr;
            if (lane < m) {
                gs.put(0, (uint64_t)__builtin_bswap32((uint32_t)(esize - 4)) |
                              ((uint64_t)(c.with_ts ? FWA_TAG_REC_WITH_TIMESTAMP : FWA_TAG_REC_WITHOUT_TIMESTAMP) << 32), 5);
                if (c.with_ts) gs.put(5, __builtin_bswap64((uint64_t)(k.win_end[g] - 1)), 8);
            }
            for (int f = 0; f < c.arity; ++f) {
                const int t = c.ftype[f];
                if (t != FWA_FIELD_JSTRING) {
                    if (lane < m) {
                        const uint64_t v = enc_load(c, k, f, g);
                        if (t == FWA_FIELD_LONG || t == FWA_FIELD_DOUBLE) { gs.put((int)pos, __builtin_bswap64(v), 8); pos += 8; }
                        else { gs.put((int)pos, __builtin_bswap32((uint32_t)v), 4); pos += 4; }
                    }
                    continue;
                }
                __syncthreads();                                  // the last field's offsets have been read
                if (lane < m) {
                    const int32_t so = k.soff[f][g];
                    const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - so);
                    int nb;
                    const uint64_t lv = enc_varint((uint64_t)enc_js_chars(k.sbytes[f] + so, len, so, (int64_t)k.soff[f][n]) + 1, &nb);
                    gs.put((int)pos, lv, nb);
                    pos += nb;
                    s_so[lane] = so;
                    s_dst[lane] = es + pos;
                    pos += len;
                }
                if (lane == 0) s_so[m] = k.soff[f][base + m];
                __syncthreads();
                const int32_t o0 = s_so[0], total = s_so[m] - o0;
                const uint8_t* __restrict__ src = k.sbytes[f];
                for (int32_t j = lane; j < total; j += 64) {
                    const int32_t tt = o0 + j;
                    int lo = 0, hi = m;                           // last row with offset <= tt (skips empty values)
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_so[mid] <= tt) lo = mid; else hi = mid;
                    }
                    out[s_dst[lo] + (tt - s_so[lo])] = src[tt];
                }
            }
        } else {
            // a run longer than the LDS tile: everything but the values' bytes by the row's lane, then those bytes field by
            // field (their variable-length parts follow in field order, the 16 bytes of a DECIMAL, already written, among
            // them), byte-parallel over the wave
            if (lane < m) enc_element<true, false, DEC>(c, k, g, esize, EncGlobalSink{out + es});
            int64_t cursor = c.row_size;
            for (int f = 0; f < c.arity; ++f) {
                if (DEC && c.ftype[f] == FWA_FIELD_DECIMAL) {
                    if (lane < m && !(k.nul[f] && k.nul[f][g])) cursor += 16;
                    continue;
                }
                if (c.ftype[f] != FWA_FIELD_STRING) continue;
                __syncthreads();                                  // the last field's offsets have been read
                if (lane < m) {
                    const int32_t so = k.soff[f][g];
                    const int64_t len = std::max<int64_t>(0, (int64_t)k.soff[f][g + 1] - so);
                    int64_t d = -1;
                    if (!(k.nul[f] && k.nul[f][g])) {
                        if (len <= 7) d = epos + c.foff[f];
                        else { d = epos + row + cursor; cursor += (len + 7) & ~7ll; }
                    }
                    s_so[lane] = so;
                    s_dst[lane] = d;
                }
                if (lane == 0) s_so[m] = k.soff[f][base + m];
                __syncthreads();
                const int32_t o0 = s_so[0], total = s_so[m] - o0;
                const uint8_t* __restrict__ src = k.sbytes[f];
                for (int32_t j = lane; j < total; j += 64) {
                    const int32_t t = o0 + j;
                    int lo = 0, hi = m;                           // last row with offset <= t (skips empty values)
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_so[mid] <= t) lo = mid; else hi = mid;
                    }
                    const int64_t d = s_dst[lo];
                    if (d >= 0) out[d + (t - s_so[lo])] = src[t];
                }
            }
        }
        __syncthreads();
        if (!staged) continue;
        // stream [b0, b1): the head up to the first 16-byte boundary and the tail byte-wise, the middle in vectors
        const int head = (int)std::min<int64_t>(tb, (16 - skew) & 15);
        for (int b = lane; b < head; b += 64) out[b0 + b] = wb[skew + b];
        const int nfull = (int)((tb - head) >> 4);
        const int v0 = (skew + head) >> 4;
        u32x4* dst = reinterpret_cast<u32x4*>(out + b0 + head);
        for (int i = lane; i < nfull; i += 64) dst[i] = buf[v0 + i];
        for (int64_t b = head + ((int64_t)nfull << 4) + lane; b < tb; b += 64) out[b0 + b] = wb[skew + b];
    }
}

thread_local std::string g_enc_create_err;

}  // namespace

struct fwa_wire_encoder {
    fwa_wire_out_schema sc;
    EncConst c;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    uint8_t* d_out = nullptr;
    int64_t out_cap = 0;
    uint8_t* h_out = nullptr;                // pinned, FWA_WIRE_HOST_BYTES
    int64_t h_cap = 0;
    uint8_t* d_stage = nullptr;              // host rows
    int64_t stage_cap = 0;
    int64_t* d_size = nullptr;               // VAR: [n + 1] sizes, offsets
    int64_t* d_off = nullptr;
    int64_t row_cap = 0;
    void* scan_tmp = nullptr;
    size_t scan_tmp_cap = 0;
    uint8_t* h_evt = nullptr;                // pinned: the events' bytes, and the scan's total
    int64_t h_evt_cap = 0;
    int64_t* h_total = nullptr;              // pinned
    hipEvent_t ev[5] = {};
    fwa_wire_enc_stats stats = {};
};

namespace {

int efail(fwa_wire_encoder* e, int code, const std::string& m) {
    if (e) e->err = m;
    return code;
}

#define ECK(call)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return efail(e, e_ == hipErrorOutOfMemory ? FWA_E_OOM : FWA_E_DEVICE,                 \
                         std::string(#call ": ") + hipGetErrorString(e_));                         \
    } while (0)

template <class T>
int egrow(fwa_wire_encoder* e, T** p, int64_t* cap, int64_t need, bool pinned = false) {
    if (need <= *cap) return 0;
    const int64_t n = std::max<int64_t>(need, *cap + *cap / 2);
    if (*p) ECK(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    *cap = 0;
    if (pinned) ECK(hipHostMalloc((void**)p, n * sizeof(T)));
    else ECK(hipMalloc((void**)p, n * sizeof(T)));
    *cap = n;
    return 0;
}

// Result column class of an aggregate kind (enum fwa_agg_kind); -1 unknown. *raw: FIRST_* / SEL_* bits.
int agg_class(int kind, bool* raw) {
    *raw = false;
    switch (kind & ~FWA_AGG_DISTINCT) {
        case 0: case 1: case 4: case 5: case 10: case 13: case 23: case 24: case 33: return kEncI64;
        case 2: case 6: case 7: case 11: case 29: case 30: return kEncF32;
        case 3: case 8: case 9: case 12: case 27: case 28: return kEncF64;
        case 18: case 19: case 20: case 25: case 26: return kEncI32;
        case 21: case 31: *raw = true; return kEncI64;
        case 22: case 32: *raw = true; return kEncI32;
        case 14: case 15: case 16: case 17: return kEncDec;       // 16 bytes per row: DECIMAL(38, s)
        default: return -1;
    }
}

int class_bytes(int cls) { return cls == kEncDec ? 16 : (cls == kEncI64 || cls == kEncF64) ? 8 : 4; }

int event_bytes(const fwa_wire_event& ev, uint8_t* p) {          // StreamElementSerializer.serialize :169-184
    auto be = [&](uint8_t* q, uint64_t v, int nb) { for (int b = 0; b < nb; ++b) q[b] = (uint8_t)(v >> (8 * (nb - 1 - b))); };
    int body;
    p[4] = (uint8_t)ev.tag;
    switch (ev.tag) {
        case FWA_TAG_WATERMARK: be(p + 5, (uint64_t)ev.val[0], 8); body = 9; break;
        case FWA_TAG_STREAM_STATUS: be(p + 5, (uint64_t)ev.val[0], 4); body = 5; break;
        case FWA_TAG_LATENCY_MARKER:
            be(p + 5, (uint64_t)ev.val[0], 8); be(p + 13, (uint64_t)ev.val[1], 8); be(p + 21, (uint64_t)ev.val[2], 8);
            be(p + 29, (uint64_t)ev.val[3], 4); body = 29; break;
        case FWA_TAG_RECORD_ATTRIBUTES: p[5] = ev.val[0] != 0; body = 2; break;
        default: return -1;
    }
    be(p, (uint64_t)body, 4);
    return 4 + body;
}

}  // namespace

extern "C" {

int fwa_wire_enc_create(const fwa_wire_out_schema* s, fwa_wire_encoder** out) {
    if (!s || !out) { g_enc_create_err = "null schema or result pointer"; return FWA_E_ARG; }
    *out = nullptr;
    g_enc_create_err.clear();
    auto bad = [&](int code, const std::string& m) { g_enc_create_err = m; return code; };
    if (s->format != FWA_WIRE_TUPLE && s->format != FWA_WIRE_ROWDATA) return bad(FWA_E_ARG, "unknown wire format");
    if (s->arity < 1 || s->arity > FWA_WIRE_MAX_FIELDS)
        return bad(FWA_E_ARG, "arity " + std::to_string(s->arity) + " out of range (1.." + std::to_string(FWA_WIRE_MAX_FIELDS) + ")");
    if (s->record_ts != FWA_REC_TS_NONE && s->record_ts != FWA_REC_TS_WIN_TIME) return bad(FWA_E_ARG, "unknown record_ts");
    EncConst c;
    memset(&c, 0, sizeof(c));
    c.format = s->format;
    c.arity = s->arity;
    c.with_ts = s->record_ts == FWA_REC_TS_WIN_TIME;
    c.hdr = c.with_ts ? 13 : 5;
    c.nullbits = ((s->arity + 63 + 8) / 64) * 8;                  // BinaryRowData.calculateBitSetWidthInBytes
    c.row_size = c.nullbits + 8 * s->arity;
    static const char* tname[] = {"LONG", "DOUBLE", "FLOAT", "INT", "STRING", "?", "DECIMAL", "?", "JSTRING"};
    static const char* cname[] = {"an int64", "an int32", "a double", "a float", "a STRING", "a DECIMAL"};
    int off = c.hdr;
    for (int f = 0; f < s->arity; ++f) {
        const int t = s->field[f];
        const std::string at = "field " + std::to_string(f) + ": ";
        if (t < FWA_FIELD_LONG || (t > FWA_FIELD_STRING && t != FWA_FIELD_DECIMAL && t != FWA_FIELD_JSTRING))
            return bad(FWA_E_ARG, at + "unknown field type");
        if (t == FWA_FIELD_JSTRING && s->format != FWA_WIRE_TUPLE)
            return bad(FWA_E_ARG, at + "JSTRING fields (StringSerializer) are written in TUPLE values only: a row's CHAR / "
                                       "VARCHAR / STRING field is STRING");
        if (t == FWA_FIELD_DECIMAL && s->format != FWA_WIRE_ROWDATA)
            return bad(FWA_E_ARG, at + "DECIMAL fields are written in ROWDATA rows only (a Tuple's BigDecSerializer is another "
                                       "format)");
        if (t == FWA_FIELD_STRING && s->format != FWA_WIRE_ROWDATA)
            return bad(FWA_E_ARG, at + "STRING fields are written in ROWDATA rows only (a Tuple's StringSerializer writes "
                                       "varint-prefixed UTF-16 code units)");
        int cls;
        bool raw = false;
        switch (s->src[f]) {
            case FWA_SRC_KEY: case FWA_SRC_WIN_START: case FWA_SRC_WIN_END: case FWA_SRC_WIN_TIME: cls = kEncI64; break;
            case FWA_SRC_KEYCOL:
                if (s->src_index[f] < 0 || s->src_index[f] >= FWA_KEYDICT_MAX_ARITY) return bad(FWA_E_ARG, at + "KEYCOL index out of range");
                switch (s->src_kind[f]) {
                    case FWA_KEY_FIELD_BIGINT: cls = kEncI64; break;
                    case FWA_KEY_FIELD_INT: cls = kEncI32; break;
                    case FWA_KEY_FIELD_DOUBLE: cls = kEncF64; break;
                    case FWA_KEY_FIELD_STRING: cls = kEncStr; break;
                    default: return bad(FWA_E_ARG, at + "unknown key field type");
                }
                break;
            case FWA_SRC_AGG:
                if (s->src_index[f] < 0 || s->src_index[f] >= FWA_MAX_AGGS) return bad(FWA_E_ARG, at + "AGG index out of range");
                cls = agg_class(s->src_kind[f], &raw);
                if (cls == kEncDec && t != FWA_FIELD_DECIMAL)
                    return bad(FWA_E_UNSUPPORTED, at + "a DECIMAL aggregate result is written as FWA_FIELD_DECIMAL only: the "
                                                       "reference row carries a non-compact DecimalData, DECIMAL(38, s)");
                if (cls < 0) return bad(FWA_E_ARG, at + "unknown aggregate kind");
                break;
            default: return bad(FWA_E_ARG, at + "unknown source");
        }
        bool ok;
        switch (cls) {
            case kEncI64: ok = t == FWA_FIELD_LONG || t == FWA_FIELD_INT || (raw && t == FWA_FIELD_DOUBLE); break;
            case kEncI32: ok = t == FWA_FIELD_INT || t == FWA_FIELD_LONG || (raw && t == FWA_FIELD_FLOAT); break;
            case kEncF64: ok = t == FWA_FIELD_DOUBLE; break;
            case kEncF32: ok = t == FWA_FIELD_FLOAT; break;
            case kEncDec: ok = t == FWA_FIELD_DECIMAL; break;
            default: ok = t == FWA_FIELD_STRING || t == FWA_FIELD_JSTRING; break;   // (each in its own format, above)
        }
        if (!ok) return bad(FWA_E_ARG, at + cname[cls] + " source cannot be written as " + tname[t]);
        c.ftype[f] = t;
        c.scls[f] = cls;
        c.adj[f] = s->src[f] == FWA_SRC_WIN_TIME ? -1 : 0;
        if (t == FWA_FIELD_STRING) ++c.nstr;
        if (t == FWA_FIELD_DECIMAL) ++c.ndec;
        if (t == FWA_FIELD_JSTRING) ++c.njs;
        if (s->format == FWA_WIRE_TUPLE) { c.foff[f] = off; off += t == FWA_FIELD_JSTRING ? 0 : field_bytes(t); }
        else c.foff[f] = c.hdr + 4 + c.nullbits + 8 * f;
    }
    c.efix = s->format == FWA_WIRE_TUPLE ? off : c.hdr + 4 + c.row_size;
    fwa_wire_encoder* e = new fwa_wire_encoder();
    e->sc = *s;
    e->c = c;
    e->device = s->device;
    auto dead = [&](int code, const std::string& m) { fwa_wire_enc_destroy(e); return bad(code, m); };
    hipError_t he;
    if ((he = hipSetDevice(e->device)) != hipSuccess || (he = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess ||
        (he = hipHostMalloc((void**)&e->h_total, 8)) != hipSuccess)
        return dead(FWA_E_DEVICE, hipGetErrorString(he));
    for (auto& x : e->ev)
        if ((he = hipEventCreate(&x)) != hipSuccess) return dead(FWA_E_DEVICE, hipGetErrorString(he));
    const int64_t hint = s->max_bytes > 0 ? s->max_bytes : (64ll << 20);
    int rc;
    if ((rc = egrow(e, &e->d_out, &e->out_cap, hint)) || (rc = egrow(e, &e->h_evt, &e->h_evt_cap, 4096, true)))
        return dead(rc, e->err);
    *out = e;
    return FWA_OK;
}

void fwa_wire_enc_destroy(fwa_wire_encoder* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    void* ps[] = {e->d_out, e->d_stage, e->d_size, e->d_off, e->scan_tmp};
    for (void* p : ps) if (p) (void)hipFree(p);
    if (e->h_out) (void)hipHostFree(e->h_out);
    if (e->h_evt) (void)hipHostFree(e->h_evt);
    if (e->h_total) (void)hipHostFree(e->h_total);
    for (auto& x : e->ev) if (x) (void)hipEventDestroy(x);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* fwa_wire_enc_last_error(const fwa_wire_encoder* e) { return e ? e->err.c_str() : g_enc_create_err.c_str(); }

int fwa_wire_enc_get_stats(fwa_wire_encoder* e, fwa_wire_enc_stats* out) {
    if (!e || !out) return FWA_E_ARG;
    *out = e->stats;
    return FWA_OK;
}

int fwa_wire_encode(fwa_wire_encoder* e, const fwa_out* rows, const fwa_wire_keycols* kc, const fwa_wire_event* events,
                    int32_t n_events, int32_t flags, fwa_wire_bytes* out) {
    if (!e) return FWA_E_ARG;
    if (!rows || !out || rows->n_rows < 0 || n_events < 0 || (n_events > 0 && !events)) return efail(e, FWA_E_ARG, "bad arguments");
    memset(out, 0, sizeof(*out));
    const EncConst& c = e->c;
    const fwa_wire_out_schema& s = e->sc;
    const int64_t n = rows->n_rows;
    if (n >= (1ll << 31) - 1) return efail(e, FWA_E_UNSUPPORTED, "2^31 rows or more in one call");
    // the events' bytes
    if (int rc = egrow(e, &e->h_evt, &e->h_evt_cap, (int64_t)n_events * 33 + 1, true)) return rc;
    int64_t evt_bytes = 0;
    for (int i = 0; i < n_events; ++i) {
        const int nb = event_bytes(events[i], e->h_evt + evt_bytes);
        if (nb < 0) return efail(e, FWA_E_ARG, "event " + std::to_string(i) + ": tag " + std::to_string(events[i].tag) + " is not a non-record element (2..5)");
        evt_bytes += nb;
    }
    ECK(hipSetDevice(e->device));
    hipStream_t st = e->stream;
    // the columns each field reads
    EncCols k;
    memset(&k, 0, sizeof(k));
    struct Stage { const void** slot; const void* host; int64_t bytes; };
    std::vector<Stage> stage;
    const bool host_rows = !rows->on_device;
    auto need = [&](const void** slot, const void* p, int64_t bytes) {   // a fwa_out column: staged when the rows are host memory
        *slot = p;
        if (host_rows && n > 0 && p) stage.push_back({slot, p, bytes});
    };
    for (int f = 0; f < c.arity; ++f) {
        const std::string at = "field " + std::to_string(f) + ": ";
        const int j = s.src_index[f];
        switch (s.src[f]) {
            case FWA_SRC_KEY: need(&k.col[f], rows->key, n * 8); break;
            case FWA_SRC_WIN_START: need(&k.col[f], rows->win_start, n * 8); break;
            case FWA_SRC_WIN_END: case FWA_SRC_WIN_TIME: need(&k.col[f], rows->win_end, n * 8); break;
            case FWA_SRC_AGG:
                if (j >= rows->num_aggs) return efail(e, FWA_E_ARG, at + "aggregate " + std::to_string(j) + " is not in the rows");
                need(&k.col[f], rows->agg[j], n * class_bytes(c.scls[f]));
                need((const void**)&k.nul[f], rows->agg_null[j], n);
                break;
            default:                                              // FWA_SRC_KEYCOL: device pointers
                if (!kc) return efail(e, FWA_E_ARG, at + "a KEYCOL source needs the key columns (keycols is NULL)");
                if (j >= kc->n_cols) return efail(e, FWA_E_ARG, at + "key column " + std::to_string(j) + " is not in keycols");
                k.nul[f] = kc->null[j];
                if (c.scls[f] == kEncStr) {
                    k.soff[f] = kc->str[j].offsets;
                    k.sbytes[f] = kc->str[j].bytes;
                    k.col[f] = k.soff[f];
                } else k.col[f] = kc->col[j];
        }
        if (n > 0 && !k.col[f]) return efail(e, FWA_E_ARG, at + "the source column is a NULL pointer");
        if (c.format == FWA_WIRE_TUPLE && k.nul[f])
            return efail(e, FWA_E_ARG, at + "a nullable source in a TUPLE value: TupleSerializer cannot write null fields");
    }
    if (c.with_ts) {
        need((const void**)&k.win_end, rows->win_end, n * 8);
        if (n > 0 && !k.win_end) return efail(e, FWA_E_ARG, "record timestamps need win_end");
    }
    if (!stage.empty()) {
        int64_t total = 0;
        for (auto& x : stage) total += (x.bytes + 15) & ~15ll;
        if (int rc = egrow(e, &e->d_stage, &e->stage_cap, total)) return rc;
        int64_t at = 0;
        for (auto& x : stage) {
            ECK(hipMemcpyAsync(e->d_stage + at, x.host, x.bytes, hipMemcpyHostToDevice, st));
            *x.slot = e->d_stage + at;
            at += (x.bytes + 15) & ~15ll;
        }
    }
    const bool var = c.nstr + c.ndec + c.njs > 0;
    const bool dec = c.ndec > 0, js = c.njs > 0;
    int64_t rows_bytes = n * c.efix;
    float ms_size = 0, ms_scan = 0, ms_write = 0;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 63) / 64, kEncBlocks);
    if (var && n > 0) {
        if (n + 1 > e->row_cap) {
            int64_t c1 = 0, c2 = 0;
            if (e->d_size) ECK(hipFree(e->d_size));
            if (e->d_off) ECK(hipFree(e->d_off));
            e->d_size = nullptr; e->d_off = nullptr; e->row_cap = 0;
            const int64_t cap = std::max<int64_t>(n + 1, e->row_cap + e->row_cap / 2);
            int rc;
            if ((rc = egrow(e, &e->d_size, &c1, cap)) || (rc = egrow(e, &e->d_off, &c2, cap))) return rc;
            e->row_cap = cap;
        }
        ECK(hipEventRecord(e->ev[0], st));
        const dim3 sgrid((unsigned)std::min<int64_t>((n + 256) / 256, 4096));
        if (js) hipLaunchKernelGGL((wire_enc_size_kernel<false, true>), sgrid, dim3(256), 0, st, c, k, n, e->d_size);
        else if (dec) hipLaunchKernelGGL(wire_enc_size_kernel<true>, sgrid, dim3(256), 0, st, c, k, n, e->d_size);
        else hipLaunchKernelGGL(wire_enc_size_kernel<false>, sgrid, dim3(256), 0, st, c, k, n, e->d_size);
        ECK(hipGetLastError());
        ECK(hipEventRecord(e->ev[1], st));
        size_t tb = 0;
        ECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, e->d_size, e->d_off, (int)(n + 1), st));
        if (tb > e->scan_tmp_cap) {
            if (e->scan_tmp) ECK(hipFree(e->scan_tmp));
            e->scan_tmp = nullptr;
            e->scan_tmp_cap = 0;
            ECK(hipMalloc(&e->scan_tmp, tb));
            e->scan_tmp_cap = tb;
        }
        ECK(hipcub::DeviceScan::ExclusiveSum(e->scan_tmp, tb, e->d_size, e->d_off, (int)(n + 1), st));
        ECK(hipEventRecord(e->ev[2], st));
        ECK(hipMemcpyAsync(e->h_total, e->d_off + n, 8, hipMemcpyDeviceToHost, st));
        ECK(hipStreamSynchronize(st));
        rows_bytes = *e->h_total;
        (void)hipEventElapsedTime(&ms_size, e->ev[0], e->ev[1]);
        (void)hipEventElapsedTime(&ms_scan, e->ev[1], e->ev[2]);
    }
    const int64_t nbytes = rows_bytes + evt_bytes;
    if (int rc = egrow(e, &e->d_out, &e->out_cap, nbytes + 16)) return rc;
    if (n > 0) {
        ECK(hipEventRecord(e->ev[3], st));
        if (js) hipLaunchKernelGGL((wire_enc_var_kernel<false, true>), dim3(grid), dim3(64), 0, st, c, k, n, e->d_off, e->d_out);
        else if (dec) hipLaunchKernelGGL(wire_enc_var_kernel<true>, dim3(grid), dim3(64), 0, st, c, k, n, e->d_off, e->d_out);
        else if (var) hipLaunchKernelGGL(wire_enc_var_kernel<false>, dim3(grid), dim3(64), 0, st, c, k, n, e->d_off, e->d_out);
        else hipLaunchKernelGGL(wire_enc_fixed_kernel, dim3(grid), dim3(64), (size_t)(64 * c.efix + 32), st, c, k, n, e->d_out);
        ECK(hipGetLastError());
        ECK(hipEventRecord(e->ev[4], st));
    }
    if (evt_bytes > 0) ECK(hipMemcpyAsync(e->d_out + rows_bytes, e->h_evt, evt_bytes, hipMemcpyHostToDevice, st));
    if ((flags & FWA_WIRE_HOST_BYTES) && nbytes > 0) {
        if (int rc = egrow(e, &e->h_out, &e->h_cap, nbytes, true)) return rc;
        ECK(hipMemcpyAsync(e->h_out, e->d_out, nbytes, hipMemcpyDeviceToHost, st));
    }
    ECK(hipStreamSynchronize(st));
    if (n > 0) (void)hipEventElapsedTime(&ms_write, e->ev[3], e->ev[4]);
    e->stats.calls++;
    e->stats.rows_in += n;
    e->stats.bytes_out += nbytes;
    e->stats.size_ms += ms_size;
    e->stats.scan_ms += ms_scan;
    e->stats.encode_ms += ms_size + ms_scan + ms_write;
    out->dev = e->d_out;
    out->host = (flags & FWA_WIRE_HOST_BYTES) && nbytes > 0 ? e->h_out : nullptr;
    out->nbytes = nbytes;
    return FWA_OK;
}

}  // extern "C"
