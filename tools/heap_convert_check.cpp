// heap_convert_check.cpp -- the host conversion of flink_amd/csrc/heap_snapshot.cpp (Flink heap key-group bytes <->
// FWASNAP1 words) as a stand-alone program, so that it can run under the host sanitizers without a GPU: the engine and
// the key dictionary are stubs that keep the FWASNAP1 words / the key strings in host memory.
//   g++ -std=c++17 -O0 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/heap_convert_check.cpp \
//       flink_amd/csrc/heap_snapshot.cpp -o heap_convert_check && ./heap_convert_check <key-group section file>
// The section file is the key-group section of the reference's reduce checkpoint (tests/test_heap_convert_cpu.py cuts
// it out of tests/golden/flink_snapshots/ with tests/heap_reader.py and runs this program). Checked:
//  1. String-keyed TUMBLE reduction: the section restores, is written again with the same length and contents prefix,
//     and that body restores to the same words;
//  2. every truncation and every single-byte damage of the section is refused or taken, never a bad access;
//  3. hand-made session blobs of reductions over each field type: written and restored to the same words.
// Exit status 0 and a last line "OK" when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "../include/flink_amd.h"
#include "../flink_amd/csrc/dec_view.h"

struct fwa_engine { fwa_config c; int64_t key_pos = -1; int64_t nh = 0; std::string err; std::vector<int64_t> blob; int restores = 0; };
struct fwa_keydict { std::vector<std::string> strs; std::map<std::string, int64_t> idx; };

int fwa_keydict_host_strings(fwa_keydict* d, std::vector<std::string>* strs) { *strs = d->strs; return 0; }
int fwa_keydict_encode_host_str(fwa_keydict* d, const uint64_t*, const uint64_t*, const std::vector<std::string>& strs, int64_t n, int64_t* ids) {
    for (int64_t i = 0; i < n; ++i) {
        auto it = d->idx.find(strs[(size_t)i]);
        if (it == d->idx.end()) { it = d->idx.emplace(strs[(size_t)i], (int64_t)d->strs.size()).first; d->strs.push_back(strs[(size_t)i]); }
        ids[i] = it->second | (int64_t)(7ull << 48);     // top bits: a group that means nothing here
    }
    return 0;
}
extern "C" {
int fwa_get_config(const fwa_engine* e, fwa_config* out) { *out = e->c; return 0; }
int fwa_set_error(fwa_engine* e, int code, const char* msg) { e->err = msg; return code; }
int fwa_get_option(const fwa_engine* e, int32_t opt, int64_t* v) { if (opt != FWA_OPT_HEAP_KEY_POS) return FWA_E_ARG; *v = e->key_pos; return 0; }
int fwa_dec_view(const fwa_engine*, FwaDecView* v) { v->active = 0; return 0; }
void fwa_blob_free(fwa_blob* b) { free(b->data); b->data = nullptr; b->size = 0; }
int fwa_snapshot(fwa_engine* e, fwa_blob* out) {
    std::vector<int64_t> w = e->blob;
    if (w.empty()) {
        w.assign(32 + e->c.max_parallelism + 1, 0);
        w[0] = 0x3150414E53415746ll; w[1] = 1; w[2] = e->c.window_kind; w[3] = e->c.semantics; w[4] = e->c.size_ms; w[5] = e->c.slide_ms;
        w[6] = e->c.offset_ms; w[7] = e->c.gap_ms; w[8] = e->c.allowed_lateness_ms; w[9] = e->c.max_parallelism; w[10] = e->c.key_kind;
        w[11] = e->c.num_aggs;
        for (int j = 0; j < e->c.num_aggs; ++j) w[12 + j] = e->c.aggs[j].kind;
        w[20] = INT64_MIN; w[25] = e->nh;
    }
    out->size = (int64_t)w.size() * 8;
    out->data = malloc((size_t)out->size);
    memcpy(out->data, w.data(), (size_t)out->size);
    return 0;
}
int fwa_restore(fwa_engine* e, const void* const* blobs, const int64_t* sizes, int32_t n) {
    if (n != 1) return FWA_E_ARG;
    e->blob.assign((const int64_t*)blobs[0], (const int64_t*)blobs[0] + sizes[0] / 8);
    e->restores++;
    return 0;
}
int fwa_keydict_host_rows(fwa_keydict* d, int32_t* arity, int32_t* types, std::vector<uint64_t>* slots, std::vector<uint64_t>* nulls) {
    *arity = 1; types[0] = FWA_KEY_FIELD_STRING; slots->assign(d->strs.size(), 0); nulls->assign(d->strs.size(), 0); return 0;
}
int fwa_keydict_encode_host(fwa_keydict*, const uint64_t*, const uint64_t*, int64_t, int64_t*) { return FWA_E_ARG; }
}

static std::vector<uint8_t> slurp(const char* p) {
    FILE* f = fopen(p, "rb"); std::vector<uint8_t> b; int c;
    while (f && (c = fgetc(f)) != EOF) b.push_back((uint8_t)c);
    if (f) fclose(f);
    return b;
}
static fwa_engine mk(int wk, int kk, int kind, int maxp, int key_pos, int nh) {
    fwa_engine e; memset(&e.c, 0, sizeof(e.c));
    e.c.abi_version = FWA_ABI_VERSION; e.c.window_kind = wk; e.c.semantics = FWA_SEM_DATASTREAM; e.c.size_ms = wk == FWA_SESSION ? 0 : 3000;
    e.c.gap_ms = wk == FWA_SESSION ? 500 : 0; e.c.key_kind = kk; e.c.max_parallelism = maxp; e.c.kg_start = 0; e.c.kg_end = maxp - 1;
    e.c.num_aggs = 1; e.c.aggs[0].kind = kind; e.c.aggs[0].col = 0; e.c.flags = FWA_CFG_REDUCE; e.key_pos = key_pos; e.nh = nh;
    return e;
}
static int restore1(fwa_engine& e, fwa_keydict* d, const std::vector<uint8_t>& b, int64_t wm) {
    const void* p = b.data(); int64_t n = (int64_t)b.size();
    return d ? fwa_restore_heap_keys(&e, d, &p, &n, &wm, 1) : fwa_restore_heap(&e, &p, &n, &wm, 1);
}
int main(int argc, char** argv) {
    if (argc < 2) { puts("usage: heap_convert_check <key-group section file>"); return 2; }
    std::vector<uint8_t> fx = slurp(argv[1]);
    if (fx.empty()) { puts("empty or unreadable section file"); return 2; }
    // 1. the fixture: restore, write again, restore that -- the same FWASNAP1 words both times, the same byte count
    fwa_keydict d1, d2;
    fwa_engine a = mk(FWA_TUMBLE, FWA_KEY_PREHASHED, FWA_SUM_I32, 1, 0, 1);
    int rc = restore1(a, &d1, fx, 1999);
    printf("fixture restore rc=%d entries=%lld keys=%zu\n", rc, a.blob.size() > 21 ? (long long)a.blob[21] : -1, d1.strs.size());
    if (rc) { puts(a.err.c_str()); return 1; }
    fwa_blob out{nullptr, 0}; int64_t off[1], wm = 0;
    rc = fwa_snapshot_heap_keys(&a, &d1, &out, off, &wm);
    printf("fixture snapshot rc=%d bytes=%lld (fixture %zu) wm=%lld prefix_equal=%d\n", rc, (long long)out.size, fx.size(), (long long)wm,
           out.size >= 100 && !memcmp(out.data, fx.data(), 100));
    if (rc || out.size != (int64_t)fx.size()) return 1;
    std::vector<uint8_t> again((uint8_t*)out.data, (uint8_t*)out.data + out.size);
    fwa_blob_free(&out);
    fwa_engine b = mk(FWA_TUMBLE, FWA_KEY_PREHASHED, FWA_SUM_I32, 1, 0, 1);
    rc = restore1(b, &d2, again, 1999);
    printf("round trip rc=%d same_words=%d\n", rc, a.blob == b.blob);
    if (rc || a.blob != b.blob) return 1;
    // 2. every truncation and every single-byte damage of the fixture: an error or a restore, never a bad access
    int errs = 0, oks = 0;
    for (size_t L = 0; L < fx.size(); ++L) {
        std::vector<uint8_t> t(fx.begin(), fx.begin() + (long)L);
        fwa_engine e = mk(FWA_TUMBLE, FWA_KEY_PREHASHED, FWA_SUM_I32, 1, 0, 1); fwa_keydict d;
        (restore1(e, &d, t, 0) ? errs : oks)++;
    }
    for (size_t i = 0; i < fx.size(); ++i)
        for (int v : {0x00, 0x7f, 0x80, 0xff}) {
            std::vector<uint8_t> t = fx; t[i] = (uint8_t)v;
            fwa_engine e = mk(FWA_TUMBLE, FWA_KEY_PREHASHED, FWA_SUM_I32, 1, 0, 1); fwa_keydict d;
            (restore1(e, &d, t, 0) ? errs : oks)++;
        }
    printf("damaged bodies: %d refused, %d taken\n", errs, oks);
    // 3. a hand-made session blob (MIN_F32, Long keys, 4 key groups): write, restore, the same words but COUNT(*) = 1
    for (int kind : {FWA_MIN_F32, FWA_SUM_I32, FWA_MAXBY_F64, FWA_SUM_F32, FWA_MAX_I64}) {
        fwa_engine s = mk(FWA_SESSION, FWA_KEY_JAVA_LONG, kind, 4, 1, 0);
        const int maxp = 4, n = 5, ncols = 5;
        std::vector<int64_t> w(32 + maxp + 1 + n * ncols, 0);
        fwa_blob h{nullptr, 0}; fwa_snapshot(&s, &h); memcpy(w.data(), h.data, 32 * 8); fwa_blob_free(&h);
        w[20] = 100; w[21] = n; w[22] = 0; w[23] = maxp - 1;
        int64_t* koff = w.data() + 32; int64_t* col = koff + maxp + 1;
        // keys chosen by their key groups is the engine's business; here every entry sits where the body says
        const int64_t kgs[n] = {0, 0, 1, 3, 3};
        for (int g = 0, i = 0; g <= maxp; ++g) { while (i < n && kgs[i] < g) ++i; koff[g] = g == maxp ? n : i; }
        for (int i = 0; i < n; ++i) {
            col[i] = 1000 + i; col[n + i] = 10 * i; col[2 * n + i] = 1; col[4 * n + i] = 10 * i + 700;
            float f = 1.5f * (float)(i - 2); double dd = (double)f; uint64_t bits; memcpy(&bits, &dd, 8);
            uint64_t word;
            switch (kind) {
                case FWA_SUM_I32: word = (uint64_t)(int64_t)(i - 2); break;
                case FWA_SUM_F32: word = bits; break;
                case FWA_MAX_I64: word = (uint64_t)(int64_t)(i - 2) ^ 0x8000000000000000ull; break;
                default: word = (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull); break;
            }
            col[3 * n + i] = (int64_t)word;
        }
        s.blob = w;
        fwa_blob o2{nullptr, 0}; int64_t offs[4], wm2 = 0;
        rc = fwa_snapshot_heap(&s, &o2, offs, &wm2);
        if (rc) { printf("session snapshot rc=%d %s\n", rc, s.err.c_str()); return 1; }
        std::vector<uint8_t> body((uint8_t*)o2.data, (uint8_t*)o2.data + o2.size);
        fwa_blob_free(&o2);
        fwa_engine r = mk(FWA_SESSION, FWA_KEY_JAVA_LONG, kind, 4, 1, 0);
        rc = restore1(r, nullptr, body, wm2);
        printf("session kind %d: %zu bytes, restore rc=%d same_words=%d\n", kind, body.size(), rc, r.blob == w);
        if (rc || r.blob != w) { puts(r.err.c_str()); return 1; }
    }
    puts("OK");
    return 0;
}
