"""The two-phase ingest's launch table (flink_amd/csrc/ingest_launch.inc) without a GPU: a stand-alone C++17 program,
compiled with the host compiler, includes the file as the engine and tools/regprobe.hip do.

It enumerates every V2Shape over the full ranges of its fields, keeps the ones v2_shape_valid accepts (plan_v2 checks
the same function on every push), and prints the partition3 / combine3 template tuples they map to, next to the rows of
FWA_P3_INSTANCES / FWA_C3_INSTANCES. The two sets must be equal both ways: every reachable tuple is instantiated, and
nothing is instantiated (compiled, linked, spill-checked) that no push can launch. A second mode maps hand-written
shapes, which are checked against the table in DESIGN.md section 4."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP_IT = 2                          # FWA_MP_IT's default

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>
#include "ingest_launch.inc"

typedef std::tuple<int, int, int, int, int, int, int, int> T8;
static void put(const char* tag, const T8& t, int n) {
    const int v[8] = {std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t), std::get<4>(t), std::get<5>(t),
                      std::get<6>(t), std::get<7>(t)};
    printf("%s", tag);
    for (int i = 0; i < n; ++i) printf(" %d", v[i]);
    printf("\n");
}
static T8 tp(const P3Key& k) { return T8(k.nv, k.items, k.vw, k.kg, k.pre, k.w16, k.nw, k.roll); }
static T8 tc(const C3Key& k) { return T8(k.it, k.nv, k.layout, k.pre, k.mp, k.nw, k.lean, 0); }

int main(int argc, char** argv) {
    if (argc > 1) {   // nv vw layout pre mp kgm w16 narrow narrow2 roll old_body -> valid, p3 key + grid numbers, c3 key
        for (int i = 1; i < argc; ++i) {
            int f[11];
            char* p = argv[i];
            for (int j = 0; j < 11; ++j) f[j] = (int)strtol(p, &p, 10);
            const V2Shape s = {f[0], f[1], f[2], f[3] != 0, f[4] != 0, f[5], f[6] != 0, f[7] != 0, f[8] != 0, f[9] != 0, f[10] != 0};
            const P3Key a = p3_key(s);
            const C3Key b = c3_key(s);
            printf("%d | %d %d %d %d %d %d %d %d | %d %d | %d %d %d %d %d %d %d\n", v2_shape_valid(s) ? 1 : 0, a.nv, a.items,
                   a.vw, a.kg, a.pre, a.w16, a.nw, a.roll, a.tile, a.max_grid, b.it, b.nv, b.layout, b.pre, b.mp, b.nw, b.lean);
        }
        return 0;
    }
    std::set<T8> p3, c3;
    long valid = 0;
    // one step past every field's range, so that the range checks of v2_shape_valid are exercised too
    for (int nv = -1; nv <= 3; ++nv) for (int vw = -1; vw <= 4; ++vw) for (int layout = -1; layout <= 3; ++layout)
    for (int kgm = -1; kgm <= 3; ++kgm) for (int bits = 0; bits < 128; ++bits) {
        const V2Shape s = {nv, vw, layout, (bits & 1) != 0, (bits & 2) != 0, kgm, (bits & 4) != 0, (bits & 8) != 0,
                           (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0};
        if (!v2_shape_valid(s)) continue;
        ++valid;
        p3.insert(tp(p3_key(s)));
        c3.insert(tc(c3_key(s)));
    }
    printf("VALID %ld\n", valid);
    for (const T8& t : p3) put("P3 reach", t, 8);
    for (const T8& t : c3) put("C3 reach", t, 7);
#define ROW_P3(NV, IT, VW, KG, PRE, W16, NW, ROLL) put("P3 row", T8(NV, IT, VW, KG, PRE, W16, NW, ROLL), 8);
#define ROW_C3(IT, NV, LY, PRE, MP, NW, LEAN) put("C3 row", T8(IT, NV, LY, PRE, MP, NW, LEAN, 0), 7);
    FWA_P3_INSTANCES(ROW_P3)
    FWA_C3_INSTANCES(ROW_C3)
    return 0;
}
'''


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    d = tmp_path_factory.mktemp("ingest_launch")
    src, exe = str(d / "planner.cpp"), str(d / "planner")
    open(src, "w").write(SRC)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "flink_amd", "csrc"), src,
                           "-o", exe])
    return exe


def lines(out, tag):
    return [tuple(int(x) for x in ln[len(tag):].split()) for ln in out.splitlines() if ln.startswith(tag)]


def test_every_reachable_tuple_has_a_row_and_every_row_is_reachable(planner):
    out = subprocess.check_output([planner], text=True)
    assert lines(out, "VALID")[0][0] > 100
    for kind, width in (("P3", 8), ("C3", 7)):
        reach, rows = lines(out, kind + " reach"), lines(out, kind + " row")
        assert all(len(t) == width for t in reach + rows)
        assert len(set(rows)) == len(rows), "%s: a tuple is listed twice" % kind
        assert set(reach) - set(rows) == set(), "%s: reachable, not instantiated" % kind
        assert set(rows) - set(reach) == set(), "%s: instantiated, not reachable" % kind
    assert len(lines(out, "P3 row")) == 32 and len(lines(out, "C3 row")) == 19


def shape(nv=0, vw=0, layout=0, pre=0, mp=0, kgm=0, w16=0, narrow=0, narrow2=0, roll=1, old_body=0):
    return (nv, vw, layout, pre, mp, kgm, w16, narrow, narrow2, roll, old_body)


# shape -> partition tuple (NV, ITEMS, VW, KG, PRE, W16, NW, ROLL), records per grid block, combine tuple
# (IT, NV, LAYOUT, PRE, MP, NW, LEAN); written from the tables in DESIGN.md section 4, not from the code
SPEC = [
    # partition row 1: PRE, tile 4096 whatever the handle
    (shape(nv=0, layout=2, pre=1), (0, 4, 3, 0, 1, 0, 0, 0), 4096, (4, 0, 2, 1, 0, 0, 0)),
    (shape(nv=1, vw=1, layout=1, pre=1, kgm=2, mp=1), (1, 4, 3, 2, 1, 0, 0, 0), 4096, (MP_IT, 1, 1, 1, 1, 0, 0)),
    (shape(nv=0, layout=2, pre=1, mp=1, kgm=1), (0, 4, 3, 1, 1, 0, 0, 0), 4096, (MP_IT, 0, 2, 1, 1, 0, 0)),
    # row 2: no value column; PREHASHED: two items fewer, the grid still by 8 x 1024
    (shape(nv=0, layout=2, w16=1), (0, 8, 3, 0, 0, 0, 0, 0), 8192, (4, 0, 2, 0, 0, 0, 0)),
    (shape(nv=0, layout=0, kgm=2), (0, 6, 3, 2, 0, 0, 0, 0), 8192, (4, 0, 0, 0, 0, 0, 0)),
    # row 3: narrow, rolling and burst loads; lean body, general body (variant bit 1), window passes
    (shape(nv=1, vw=1, layout=1, w16=1, narrow=1, roll=1), (1, 6, 3, 0, 0, 1, 1, 1), 6144, (6, 1, 1, 0, 0, 1, 3)),
    (shape(nv=1, vw=1, layout=1, w16=1, narrow=1, roll=0, old_body=1), (1, 6, 3, 0, 0, 1, 1, 0), 6144, (6, 1, 1, 0, 0, 1, 0)),
    (shape(nv=1, vw=1, layout=1, w16=1, narrow=1, mp=1, old_body=1), (1, 6, 3, 0, 0, 1, 1, 1), 6144, (MP_IT, 1, 1, 0, 1, 1, 0)),
    # row 4: narrow2 (roll and old_body do not reach it)
    (shape(nv=2, vw=1, layout=0, narrow2=1, roll=1, old_body=1), (2, 4, 1, 0, 0, 0, 2, 0), 4096, (4, 2, 0, 0, 0, 2, 0)),
    (shape(nv=2, vw=1, layout=0, narrow2=1, mp=1), (2, 4, 1, 0, 0, 0, 2, 0), 4096, (MP_IT, 2, 0, 0, 1, 2, 0)),
    # row 5: one value column, paired loads; 4-byte column: VW 2
    (shape(nv=1, vw=0, layout=1, w16=1), (1, 6, 2, 0, 0, 1, 0, 0), 6144, (4, 1, 1, 0, 0, 0, 0)),
    (shape(nv=1, vw=1, layout=0, w16=1, roll=0), (1, 6, 3, 0, 0, 1, 0, 0), 6144, (4, 1, 0, 0, 0, 0, 0)),
    # row 6: one value column, one record per load
    (shape(nv=1, vw=1, layout=1, kgm=1), (1, 6, 3, 1, 0, 0, 0, 0), 6144, (4, 1, 1, 0, 0, 0, 0)),
    (shape(nv=1, vw=0, layout=0, kgm=2, mp=1), (1, 4, 2, 2, 0, 0, 0, 0), 6144, (MP_IT, 1, 0, 0, 1, 0, 0)),
    # row 7: two value columns; three entries per lane in the combiner
    (shape(nv=2, vw=3, layout=0, w16=1), (2, 4, 3, 0, 0, 0, 0, 0), 4096, (3, 2, 0, 0, 0, 0, 0)),
    (shape(nv=2, vw=1, layout=0, kgm=2), (2, 2, 1, 2, 0, 0, 0, 0), 4096, (3, 2, 0, 0, 0, 0, 0)),
    (shape(nv=2, vw=2, layout=0, kgm=1, mp=1), (2, 4, 2, 1, 0, 0, 0, 0), 4096, (MP_IT, 2, 0, 0, 1, 0, 0)),
]

# what neither create_engine nor plan_v2 produces
INVALID = [
    shape(nv=1, vw=1, layout=2),                       # COUNT alone carries no value
    shape(nv=0, vw=0, layout=1),                       # COUNT + SUM(BIGINT) adds the carried value
    shape(nv=2, vw=3, layout=1),                       # two value columns feed at least two accumulators
    shape(nv=0, vw=1, layout=2),                       # a width without its column
    shape(nv=2, vw=3, layout=0, pre=1),                # PRE: COUNT, or COUNT + SUM(BIGINT) over an 8-byte column
    shape(nv=1, vw=0, layout=1, pre=1),
    shape(nv=1, vw=1, layout=1, w16=1, kgm=1),         # paired loads only when every key group is owned
    shape(nv=1, vw=1, layout=1, narrow=1),             # narrow needs the paired loads
    shape(nv=1, vw=1, layout=1, w16=1, narrow=1, pre=1),
    shape(nv=2, vw=1, layout=0, narrow2=1, kgm=1),
    shape(nv=2, vw=3, layout=0, narrow2=1),
]


def test_spec_table(planner):
    args = [" ".join(map(str, s)) for s, _, _, _ in SPEC] + [" ".join(map(str, s)) for s in INVALID]
    out = subprocess.check_output([planner] + args, text=True).splitlines()
    assert len(out) == len(SPEC) + len(INVALID)
    for (s, p3, tile, c3), ln in zip(SPEC, out):
        valid, got_p3, grid, got_c3 = [tuple(int(x) for x in part.split()) for part in ln.split("|")]
        assert valid == (1,), s
        assert got_p3 == p3, s
        assert grid == (tile, 256), s
        assert got_c3 == c3, s
    for s, ln in zip(INVALID, out[len(SPEC):]):
        assert ln.split("|")[0].strip() == "0", s


def test_gpu_cases_cover_exactly_the_rows(planner):
    """tests/test_ingest_launch_gpu.py names the row each of its cases launches: together they are the two lists."""
    from test_ingest_launch_gpu import CASES
    out = subprocess.check_output([planner], text=True)
    assert {c["p3"] for c in CASES.values()} == set(lines(out, "P3 row"))
    assert {c["c3"] for c in CASES.values()} == set(lines(out, "C3 row"))


def test_gpu_cases_fire_rows_in_the_oracle():
    """Every GPU case's inputs give the oracle rows to fire: all windows of about 3 000 keys over 4 slices."""
    import test_ingest_launch_gpu as G
    for name in G.CASES:
        rows = G.reference(name)
        assert len(rows["key"]) > G.KEYS, name
        assert rows["agg0"].any(), name
