// Which partition3_kernel / combine3_kernel instantiation a two-phase push runs (ingest.inc; DESIGN.md section 4).
// Shared by engine.hip (ingest_host.inc: the launch tables), tools/regprobe.hip (the register / spill report) and
// tests/test_ingest_launch_cpu.py, which compiles this file with the host compiler alone: plain C++, no HIP.
//
//   V2Shape            what the choice depends on, filled by plan_v2 (ingest_host.inc)
//   v2_shape_valid     the invariants among its fields
//   p3_key / c3_key    shape -> template arguments (and Phase P's grid)
//   FWA_P3_INSTANCES / FWA_C3_INSTANCES   one row per instantiation: every tuple the key functions return for a valid
//                      shape and no other (the CPU test enumerates the shapes and compares both ways). A new variant is
//                      a branch in a key function plus its rows here; launch, probe and spill check follow.

// entries per lane and chunk of a combiner with window passes (-DFWA_MP_IT=4 for tools/regprobe.sh: DESIGN.md section 4)
#ifndef FWA_MP_IT
#define FWA_MP_IT 2
#endif

struct V2Shape {
    int nv;          // carried value columns: 0, 1, 2
    int vw;          // bit v: value column v (v < nv) is 8 bytes wide
    int layout;      // combiner accumulators: 0 general, 1 COUNT + one BIGINT sum over value column 0, 2 COUNT alone
    bool pre;        // Phase P merges equal (key, slice) records of a tile (skewed keys, partial rows)
    bool mp;         // combiner window passes
    int kgm;         // key groups: 0 all owned, 1 checked per record, 2 checked with supplied hashes (PREHASHED)
    bool w16;        // key, timestamp and value column 0 aligned for paired 16-byte loads
    bool narrow;     // narrow entries, COUNT + SUM(BIGINT)
    bool narrow2;    // narrow entries, an 8-byte beside a 4-byte value column
    bool roll;       // rolling issue of the next tile's loads (FWA_OPT_INGEST_VARIANT bit 10 clear)
    bool old_body;   // the general combiner body on narrow entries (FWA_OPT_INGEST_VARIANT bit 1 set)
};

// What create_engine and plan_v2 can produce. (nv, layout): layout 2 is a handle without accumulators past COUNT, so
// without value columns; layout 1 is one such accumulator fed by the one value column.
inline bool v2_shape_valid(const V2Shape& s) {
    if (s.nv < 0 || s.nv > 2 || s.vw < 0 || s.vw >= (1 << s.nv) || s.kgm < 0 || s.kgm > 2) return false;
    if (!(s.nv == 0 ? s.layout == 0 || s.layout == 2 : s.nv == 1 ? s.layout == 0 || s.layout == 1 : s.layout == 0)) return false;
    if (s.pre && !((s.layout == 2 && s.nv == 0) || (s.layout == 1 && s.nv == 1 && (s.vw & 1)))) return false;
    if (s.narrow && !(s.layout == 1 && s.nv == 1 && (s.vw & 1) && s.w16 && !s.pre)) return false;
    if (s.narrow2 && !(s.layout == 0 && s.nv == 2 && s.vw == 1 && s.kgm == 0 && !s.pre)) return false;
    if (s.w16 && s.kgm != 0) return false;
    return true;
}

// partition3_kernel<NV, ITEMS, 1024, VW, KG, PRE, W16, NW, ROLL> on a grid of clamp(ceil(n / tile), 1, max_grid) blocks
struct P3Key {
    int nv, items, vw, kg, pre, w16, nw, roll;
    int tile, max_grid;
};
// combine3_kernel<IT, 2, NV, 1024, LAYOUT, PRE, MP, NW, LEAN> on one block per partition
struct C3Key {
    int it, nv, layout, pre, mp, nw, lean;
};

inline bool same_kernel(const P3Key& a, const P3Key& b) {
    return a.nv == b.nv && a.items == b.items && a.vw == b.vw && a.kg == b.kg && a.pre == b.pre && a.w16 == b.w16 &&
           a.nw == b.nw && a.roll == b.roll;
}
inline bool same_kernel(const C3Key& a, const C3Key& b) {
    return a.it == b.it && a.nv == b.nv && a.layout == b.layout && a.pre == b.pre && a.mp == b.mp && a.nw == b.nw &&
           a.lean == b.lean;
}

// Phase P. Items per lane: 8 / 6 / 4 with 0 / 1 / 2 value columns; supplied key hashes are one column more per tile, and
// two items fewer keep the kernel free of VGPR spills. The grid still counts tiles of the full item count then, so such
// a push runs fewer blocks over more tiles each. A value column the kernel does not carry counts as 8 bytes wide in VW.
inline P3Key p3_key(const V2Shape& s) {
    const int items0 = s.nv == 2 ? 4 : (s.nv == 1 ? 6 : 8), cut = s.kgm == 2 ? 2 : 0, tile = items0 * 1024;
    const int vw1 = (s.vw & 1) ? 3 : 2;
    if (s.pre) return {s.nv, 4, 3, s.kgm, 1, 0, 0, 0, 4096, 256};
    if (s.nv == 0) return {0, 8 - cut, 3, s.kgm, 0, 0, 0, 0, tile, 256};
    if (s.narrow) return {1, 6, 3, 0, 0, 1, 1, s.roll ? 1 : 0, tile, 256};
    if (s.narrow2) return {2, 4, 1, 0, 0, 0, 2, 0, tile, 256};
    if (s.nv == 1 && s.w16) return {1, 6, vw1, 0, 0, 1, 0, 0, tile, 256};
    if (s.nv == 1) return {1, 6 - cut, vw1, s.kgm, 0, 0, 0, 0, tile, 256};
    return {2, 4 - cut, s.vw, s.kgm, 0, 0, 0, 0, tile, 256};
}

// Phase A. Entries per lane and chunk: the largest counts whose kernels keep every value in registers at 1024 threads
// (a VGPR spill is not harmless here, DESIGN.md section 4 "Skewed keys"; tests/test_abi.py checks the code object): 4, 3
// with two carried value columns, 6 for narrow entries (the lean body too: 8 spill), FWA_MP_IT with window passes.
inline C3Key c3_key(const V2Shape& s) {
    const int mp = s.mp ? 1 : 0;
    if (s.narrow) {   // the lean body (4-byte key image in LDS, batched first probes, misses deferred) unless A/B'd away
        if (s.mp) return {FWA_MP_IT, 1, 1, 0, 1, 1, 0};
        return {6, 1, 1, 0, 0, 1, s.old_body ? 0 : 3};
    }
    if (s.narrow2) return {s.mp ? FWA_MP_IT : 4, 2, 0, 0, mp, 2, 0};
    const int it = s.mp ? FWA_MP_IT : (s.nv == 2 ? 3 : 4);
    if (s.pre && s.layout == 1) return {it, 1, 1, 1, mp, 0, 0};
    if (s.pre) return {it, 0, 2, 1, mp, 0, 0};
    return {it, s.nv, s.layout, 0, mp, 0, 0};
}

// X(NV, ITEMS, VW, KG, PRE, W16, NW, ROLL)
#define FWA_P3_INSTANCES(X)                                                                                  \
    /* PRE (skew merge, partial rows) */                                                                     \
    X(0, 4, 3, 0, 1, 0, 0, 0) X(0, 4, 3, 1, 1, 0, 0, 0) X(0, 4, 3, 2, 1, 0, 0, 0)                            \
    X(1, 4, 3, 0, 1, 0, 0, 0) X(1, 4, 3, 1, 1, 0, 0, 0) X(1, 4, 3, 2, 1, 0, 0, 0)                            \
    /* no value column */                                                                                    \
    X(0, 8, 3, 0, 0, 0, 0, 0) X(0, 8, 3, 1, 0, 0, 0, 0) X(0, 6, 3, 2, 0, 0, 0, 0)                            \
    /* narrow entries: COUNT + SUM(BIGINT) burst / rolling loads; 8-byte beside 4-byte column */             \
    X(1, 6, 3, 0, 0, 1, 1, 0) X(1, 6, 3, 0, 0, 1, 1, 1) X(2, 4, 1, 0, 0, 0, 2, 0)                            \
    /* one value column: paired loads, then by key-group mode */                                             \
    X(1, 6, 2, 0, 0, 1, 0, 0) X(1, 6, 3, 0, 0, 1, 0, 0)                                                      \
    X(1, 6, 2, 0, 0, 0, 0, 0) X(1, 6, 2, 1, 0, 0, 0, 0) X(1, 4, 2, 2, 0, 0, 0, 0)                            \
    X(1, 6, 3, 0, 0, 0, 0, 0) X(1, 6, 3, 1, 0, 0, 0, 0) X(1, 4, 3, 2, 0, 0, 0, 0)                            \
    /* two value columns, by widths */                                                                       \
    X(2, 4, 0, 0, 0, 0, 0, 0) X(2, 4, 0, 1, 0, 0, 0, 0) X(2, 2, 0, 2, 0, 0, 0, 0)                            \
    X(2, 4, 1, 0, 0, 0, 0, 0) X(2, 4, 1, 1, 0, 0, 0, 0) X(2, 2, 1, 2, 0, 0, 0, 0)                            \
    X(2, 4, 2, 0, 0, 0, 0, 0) X(2, 4, 2, 1, 0, 0, 0, 0) X(2, 2, 2, 2, 0, 0, 0, 0)                            \
    X(2, 4, 3, 0, 0, 0, 0, 0) X(2, 4, 3, 1, 0, 0, 0, 0) X(2, 2, 3, 2, 0, 0, 0, 0)

// X(IT, NV, LAYOUT, PRE, MP, NW, LEAN)
#define FWA_C3_INSTANCES(X)                                                                                  \
    /* narrow entries: window passes, general body (A/B), lean body; the two-column kind */                  \
    X(FWA_MP_IT, 1, 1, 0, 1, 1, 0) X(6, 1, 1, 0, 0, 1, 0) X(6, 1, 1, 0, 0, 1, 3)                             \
    X(FWA_MP_IT, 2, 0, 0, 1, 2, 0) X(4, 2, 0, 0, 0, 2, 0)                                                    \
    /* PRE buckets */                                                                                        \
    X(4, 1, 1, 1, 0, 0, 0) X(FWA_MP_IT, 1, 1, 1, 1, 0, 0)                                                    \
    X(4, 0, 2, 1, 0, 0, 0) X(FWA_MP_IT, 0, 2, 1, 1, 0, 0)                                                    \
    /* each (value columns, layout) a handle can have */                                                     \
    X(4, 0, 0, 0, 0, 0, 0) X(FWA_MP_IT, 0, 0, 0, 1, 0, 0)                                                    \
    X(4, 0, 2, 0, 0, 0, 0) X(FWA_MP_IT, 0, 2, 0, 1, 0, 0)                                                    \
    X(4, 1, 0, 0, 0, 0, 0) X(FWA_MP_IT, 1, 0, 0, 1, 0, 0)                                                    \
    X(4, 1, 1, 0, 0, 0, 0) X(FWA_MP_IT, 1, 1, 0, 1, 0, 0)                                                    \
    X(3, 2, 0, 0, 0, 0, 0) X(FWA_MP_IT, 2, 0, 0, 1, 0, 0)
