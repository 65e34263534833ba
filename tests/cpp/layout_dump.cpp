// layout_dump -- runs the host-only layout planner (csrc/alll_layout.cpp, linked directly) the
// way alll_create does and writes what it planned as raw records; tests/test_layout.py builds
// this under the address and undefined-behaviour sanitizers and checks the records.
//   layout_dump <instance> <out> <world> <rank> <n_threads> <flags> <stream_batch> <n_cu> [set_starts...]
// instance: u64 n_vars, u64 n_clauses, u64 offsets[n_clauses + 1], u32 literals[offsets[n_clauses]]
// out: records {u32 name length, name, u32 element size, u64 count, data}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alll_layout.h"

using namespace alll;

static FILE* g_out;

static void rec(const char* name, const void* p, uint32_t esize, uint64_t count) {
    const uint32_t nl = (uint32_t)strlen(name);
    fwrite(&nl, 4, 1, g_out);
    fwrite(name, 1, nl, g_out);
    fwrite(&esize, 4, 1, g_out);
    fwrite(&count, 8, 1, g_out);
    if (count) fwrite(p, esize, count, g_out);
}
static void num(const char* name, uint64_t v) { rec(name, &v, 8, 1); }
template <typename T>
static void vec(const char* name, const std::vector<T>& v) { rec(name, v.data(), sizeof(T), v.size()); }

int main(int argc, char** argv) {
    if (argc < 9) { fprintf(stderr, "usage: layout_dump instance out world rank n_threads flags stream_batch n_cu [starts]\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!f || !g_out) { perror("open"); return 2; }
    uint64_t hdr[2];
    if (fread(hdr, 8, 2, f) != 2) return 2;
    std::vector<uint64_t> offs(hdr[1] + 1);
    if (fread(offs.data(), 8, offs.size(), f) != offs.size()) return 2;
    // (the literal count comes from the file's size: a test may hand over bad offsets)
    const long at = ftell(f);
    fseek(f, 0, SEEK_END);
    std::vector<uint32_t> lits((size_t)(ftell(f) - at) / 4);
    fseek(f, at, SEEK_SET);
    if (!lits.empty() && fread(lits.data(), 4, lits.size(), f) != lits.size()) return 2;
    fclose(f);

    alll_problem prob{};
    prob.n_vars = (uint32_t)hdr[0];
    prob.n_clauses = hdr[1];
    prob.offsets = offs.data();
    prob.literals = lits.data();
    alll_options opt{};
    opt.seed = 1;
    opt.device = -1;
    opt.world = atoi(argv[3]);
    opt.rank = atoi(argv[4]);
    opt.n_threads = atoi(argv[5]);
    opt.flags = strtoull(argv[6], nullptr, 0);
    opt.stream_batch = strtoull(argv[7], nullptr, 0);
    const uint32_t n_cu = (uint32_t)atoi(argv[8]);
    std::vector<uint64_t> starts;
    for (int i = 9; i < argc; ++i) starts.push_back(strtoull(argv[i], nullptr, 0));
    if (!starts.empty()) opt.set_starts = starts.data();

    const Knobs kn = read_knobs();
    Layout l;
    int rc = plan_instance(prob, opt, kn, l);
    if (!rc) rc = plan_buckets(prob, opt, kn, n_cu, l);
    if (!rc) {
        flag_hot(prob, l);
        if (l.fixed_k > 0) {
            order_fixed(prob, kn, l);
            transpose_fixed(prob, l);
            window_bases(prob, l);
        } else if (l.ragged) {
            rc = order_ragged(prob, kn, l);
        }
    }
    num("rc", (uint64_t)rc);
    rec("err", l.err.data(), 1, l.err.size());
    if (!rc) {
        num("width", (uint64_t)(int64_t)l.width); num("fixed_k", l.fixed_k); num("ragged", l.ragged);
        num("rr_T", l.b.rr_T); num("srr_T", l.b.srr_T); num("n_words", l.b.n_words); num("win_words", l.b.win_words);
        num("n_tiles", l.b.n_tiles); num("own_begin", l.b.own_begin); num("own_end", l.b.own_end);
        num("stream_pinv", l.b.stream_pinv); num("n_hot", l.cv.n_hot); num("fp", l.fp); num("fp_inc", l.b.fp_inc);
        num("vmix_mul", l.b.vmix_mul); num("vmix_mask", l.b.vmix_mask); num("vmix_inv", l.b.vmix_inv); num("vrange", l.vrange);
        num("bkt_width", l.b.bkt_width); num("bkt_magic", l.b.bkt_magic); num("n_bkt", l.b.n_bkt); num("bkt_span", l.b.bkt_span);
        num("skewed", l.skewed); num("bucketed", l.bucketed); num("run_tiles", l.b.run_tiles); num("n_runs", l.b.n_runs);
        num("bucket_min_u", l.bucket_min_u); num("windows", l.windows); num("lit_mask", l.cv.lit_mask);
        num("id_shift", l.cv.id_shift); num("id_bits", l.cv.id_bits); num("lits_nt", l.cv.lits_nt); num("t_chunk0", l.t_chunk0);
        num("fp_ep_cap", l.b.fp_ep_cap); num("fp_ep_cap_min", FP_EP_CAP_MIN); num("fp_g_max", FP_G_MAX); num("epoch0", l.epoch0);
        vec("rr_sets", l.rr_sets); vec("is_hot", l.is_hot); vec("fp_soff", l.fp_soff); vec("fp_breg", l.fp_breg);
        vec("run_t0", l.run_t0); vec("flagged", l.flagged); vec("perm", l.perm); vec("lits_t", l.lits_t);
        vec("win_base", l.win_base); vec("rg_off", l.rg_off);
    }
    fclose(g_out);
    return 0;
}
