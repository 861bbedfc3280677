// Stage driver of the pass-major form of the range-ranked route (kernels/pass_major.inc.hip) for
// tests/test_gpu_pm_stages.py: host code only.  It runs the form's launches one stage at a time -- no context, no
// 128 Ki-read threshold --, every device buffer at exactly the size api/solve_head.inc.hip gives its counterpart with a
// guard band on either side, and hands every buffer a stage may write back to the host for tests/pm_stage_compare.py to
// hold against the host model (tests/pass_major_model.py).
//
//   pm_stage_driver <case.json> <case.bin> <dump.json> <dump.bin>
//
// case.json  {"n", "n_contigs", "ltot", "wish" (-1 global grid, +1 aligned), "ell_reg" (0: no filter), "stop_after"
//            ("A".."D"), "n_quota"} -- flat, integers and one string
// case.bin   little-endian, in this order: starts u32[n], ends u32[n], contig lengths u64[n_contigs], read offsets
//            u64[n_contigs + 1], quota vectors u32[n_quota][ltot] (one value per global position)
// dump.bin   the buffers, appended stage by stage; dump.json says where: "entries" [{stage, name, dtype, count,
//            offset}], "derived" (shift, grid, sizes), "violations" [{stage, buffer, side, offset}] -- guard bytes that
//            changed --, "inputs_changed" [names], "hip_error", "refused".
// Stages: A the producer; B row sums and tables; C bucket offsets; D0, D1, ... the walk, once per quota vector.
// Exit status: 0 fine, 2 case refused, 3 a HIP error or a guard violation (nothing more is launched after either),
// 4 bad usage or files.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "qmcp_kernels.h"

namespace {

constexpr size_t kGuard = 4096;      // bytes on either side of every buffer
constexpr uint8_t kCanary = 0xA5;

struct Buf {
    std::string name;
    size_t bytes = 0;
    char* base = nullptr;            // the allocation: guard | payload | guard
    bool input = false;
    std::vector<uint8_t> orig;       // an input's content
    template <class T> T* p() const { return reinterpret_cast<T*>(base + kGuard); }
};

struct Entry { std::string stage, name, dtype; size_t count, offset; };
struct Violation { std::string stage, buffer, side; size_t offset; };

std::vector<Buf*> g_bufs;
std::vector<Entry> g_entries;
std::vector<Violation> g_violations;
std::vector<std::string> g_inputs_changed;
std::string g_hip_error, g_refused, g_derived;
FILE* g_bin = nullptr;
size_t g_bin_at = 0;

bool hip_ok(hipError_t e, const char* what, const std::string& stage) {
    if (e == hipSuccess) return true;
    if (g_hip_error.empty()) g_hip_error = "stage " + stage + ": " + what + ": " + hipGetErrorString(e);
    return false;
}
#define CHK(expr) do { if (!hip_ok((expr), #expr, stage)) return false; } while (0)

bool alloc(Buf& b, const char* name, size_t bytes, int fill /* payload byte */, const void* content, const std::string& stage) {
    b.name = name;
    b.bytes = bytes;
    CHK(hipMalloc((void**)&b.base, bytes + 2 * kGuard));
    CHK(hipMemset(b.base, kCanary, bytes + 2 * kGuard));
    if (content != nullptr) {
        b.input = true;
        b.orig.assign((const uint8_t*)content, (const uint8_t*)content + bytes);
        if (bytes) CHK(hipMemcpy(b.base + kGuard, content, bytes, hipMemcpyHostToDevice));
    } else if (fill != kCanary && bytes) {
        CHK(hipMemset(b.base + kGuard, fill, bytes));
    }
    g_bufs.push_back(&b);
    return true;
}

// every guard band of every buffer: the first byte that is not the canary is a violation
bool check_guards(const std::string& stage) {
    std::vector<uint8_t> g(kGuard);
    for (const Buf* b : g_bufs) {
        for (int side = 0; side < 2; ++side) {
            CHK(hipMemcpy(g.data(), side ? b->base + kGuard + b->bytes : b->base, kGuard, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < kGuard; ++i)
                if (g[i] != kCanary) { g_violations.push_back({stage, b->name, side ? "high" : "low", i}); break; }
        }
    }
    return true;
}

bool check_inputs(const std::string& stage) {
    std::vector<uint8_t> h;
    for (const Buf* b : g_bufs) {
        if (!b->input || b->bytes == 0) continue;
        h.resize(b->bytes);
        CHK(hipMemcpy(h.data(), b->base + kGuard, b->bytes, hipMemcpyDeviceToHost));
        if (std::memcmp(h.data(), b->orig.data(), b->bytes) != 0) g_inputs_changed.push_back(b->name);
    }
    return true;
}

bool dump(const std::string& stage, const Buf& b, const char* dtype, size_t elem, std::vector<uint8_t>* keep = nullptr) {
    std::vector<uint8_t> h(b.bytes);
    if (b.bytes) CHK(hipMemcpy(h.data(), b.base + kGuard, b.bytes, hipMemcpyDeviceToHost));
    if (b.bytes && std::fwrite(h.data(), 1, b.bytes, g_bin) != b.bytes) { g_hip_error = "stage " + stage + ": short write of the dump"; return false; }
    g_entries.push_back({stage, b.name, dtype, b.bytes / elem, g_bin_at});
    g_bin_at += b.bytes;
    if (keep) keep->swap(h);
    return true;
}

long long jint(const std::string& text, const char* key) {
    const size_t at = text.find(std::string("\"") + key + "\"");
    if (at == std::string::npos) { std::fprintf(stderr, "case: no key %s\n", key); std::exit(4); }
    return std::strtoll(text.c_str() + text.find(':', at) + 1, nullptr, 10);
}
std::string jstr(const std::string& text, const char* key) {
    const size_t at = text.find(std::string("\"") + key + "\"");
    if (at == std::string::npos) { std::fprintf(stderr, "case: no key %s\n", key); std::exit(4); }
    const size_t q0 = text.find('"', text.find(':', at) + 1);
    return text.substr(q0 + 1, text.find('"', q0 + 1) - q0 - 1);
}

void write_manifest(const char* path) {
    FILE* f = std::fopen(path, "w");
    if (!f) return;
    auto esc = [](const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o; };
    std::fprintf(f, "{\n \"derived\": {%s},\n \"entries\": [", g_derived.c_str());
    for (size_t i = 0; i < g_entries.size(); ++i)
        std::fprintf(f, "%s\n  {\"stage\": \"%s\", \"name\": \"%s\", \"dtype\": \"%s\", \"count\": %zu, \"offset\": %zu}", i ? "," : "",
                     g_entries[i].stage.c_str(), g_entries[i].name.c_str(), g_entries[i].dtype.c_str(), g_entries[i].count, g_entries[i].offset);
    std::fprintf(f, "\n ],\n \"violations\": [");
    for (size_t i = 0; i < g_violations.size(); ++i)
        std::fprintf(f, "%s\n  {\"stage\": \"%s\", \"buffer\": \"%s\", \"side\": \"%s\", \"offset\": %zu}", i ? "," : "",
                     g_violations[i].stage.c_str(), g_violations[i].buffer.c_str(), g_violations[i].side.c_str(), g_violations[i].offset);
    std::fprintf(f, "\n ],\n \"inputs_changed\": [");
    for (size_t i = 0; i < g_inputs_changed.size(); ++i) std::fprintf(f, "%s\"%s\"", i ? ", " : "", g_inputs_changed[i].c_str());
    std::fprintf(f, "],\n \"hip_error\": %s,\n \"refused\": %s\n}\n",
                 g_hip_error.empty() ? "null" : ("\"" + esc(g_hip_error) + "\"").c_str(),
                 g_refused.empty() ? "null" : ("\"" + esc(g_refused) + "\"").c_str());
    std::fclose(f);
}

struct Case {
    uint32_t n = 0, n_contigs = 0, ltot = 0, ell_reg = 0, n_quota = 0;
    int wish = 0;
    char stop_after = 'D';
    std::vector<uint32_t> starts, ends, quota;
    std::vector<uint64_t> lengths, roff, poff;
};

// -> false after a HIP error or a guard violation: nothing more is launched
bool run(const Case& cs) {
    std::string stage = "setup";
    const uint32_t n = cs.n, ltot = cs.ltot, n_contigs = cs.n_contigs;
    // what enqueue_head derives
    const uint32_t shift = qmcp::range_shift_for(ltot);
    if (qmcp::range_path_two_level(ltot)) { g_refused = "two partition levels"; return true; }
    const qmcp::PmGridPlan grid = qmcp::pm_grid_plan(cs.roff.data(), cs.poff.data(), n_contigs, shift, qmcp::pm_pass(), cs.wish);
    const uint32_t n_ranges = grid.n_ranges;
    if (grid.words.empty()) { g_refused = "no grid tables"; return true; }
    if ((uint64_t)qmcp::pm_slots(n, n_ranges) >= (1ull << 31)) { g_refused = "pm_slots >= 2^31"; return true; }
    const uint32_t pitch = qmcp::pm_pitch(n);
    const size_t slots = qmcp::pm_slots(n, n_ranges);
    const bool filter = cs.ell_reg != 0u;
    const uint32_t exc_cap = std::max(qmcp::pm_exc_slots(n), qmcp::prepare_exc_slots(n));
    const size_t scratch_bytes = qmcp::pm_rank_scratch_bytes(shift, n_ranges, n);
    const bool by_records = qmcp::pm_rank_scratch_by_records(shift, n_ranges, n);
    {
        std::ostringstream d;
        d << "\"shift\": " << shift << ", \"n_ranges\": " << n_ranges << ", \"aligned\": " << grid.aligned << ", \"pitch\": " << pitch
          << ", \"stride\": " << qmcp::pm_stride(n_ranges) << ", \"slots\": " << slots << ", \"pass\": " << qmcp::pm_pass()
          << ", \"exc_cap\": " << (filter ? exc_cap : 0u) << ", \"scratch_bytes\": " << scratch_bytes
          << ", \"by_records\": " << (by_records ? 1 : 0) << ", \"work_words\": " << qmcp::pm_work_words();
        g_derived = d.str();
    }

    Buf starts, ends, roff, poff, gridw, keys16, idx16, cnt_tab, lst_tab, desc, work, range_start, max_load, stats, boff, selend, scalars,
        mask, scratch, exc;
    if (!alloc(starts, "starts", (size_t)n * 4, 0, cs.starts.data(), stage)) return false;
    if (!alloc(ends, "ends", (size_t)n * 4, 0, cs.ends.data(), stage)) return false;
    if (!alloc(roff, "roff", (size_t)(n_contigs + 1) * 8, 0, cs.roff.data(), stage)) return false;
    if (!alloc(poff, "poff", (size_t)(n_contigs + 1) * 8, 0, cs.poff.data(), stage)) return false;
    if (!alloc(gridw, "grid", grid.words.size() * 4, 0, grid.words.data(), stage)) return false;
    if (!alloc(keys16, "keys16", slots * 2, kCanary, nullptr, stage)) return false;
    if (!alloc(idx16, "idx16", slots * 2, kCanary, nullptr, stage)) return false;
    if (!alloc(cnt_tab, "cnt_tab", ((size_t)256 * pitch + 4) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(lst_tab, "lst_tab", (size_t)256 * pitch * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(desc, "desc", slots / 64 * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(work, "work", (size_t)qmcp::pm_work_words() * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(range_start, "range_start", 257 * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(max_load, "max_load", 2 * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(stats, "stats", 12 * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(boff, "boff", ((size_t)ltot + 1) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(selend, "selend", ((size_t)ltot + 8) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(scalars, "scalars", 64, 0xFF, nullptr, stage)) return false;
    if (!alloc(mask, "mask", (size_t)((n + 63u) / 64u) * 8, 0xFF, nullptr, stage)) return false;
    if (!alloc(scratch, "scratch", scratch_bytes, kCanary, nullptr, stage)) return false;
    if (filter && !alloc(exc, "exc", qmcp::nu_exc_bytes(exc_cap), kCanary, nullptr, stage)) return false;
    uint32_t* const d_exc = filter ? exc.p<uint32_t>() : nullptr;
    uint32_t* const d_exc_cnt = filter ? qmcp::nu_exc_counts(d_exc, exc_cap) : nullptr;

    hipStream_t st;
    CHK(hipStreamCreate(&st));
    if (!dump("in", gridw, "u32", 4)) return false;
    auto end_stage = [&]() -> bool {
        if (!check_guards(stage)) return false;
        return g_violations.empty();
    };

    stage = "A";
    {
        const uint32_t init[8] = {0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the statistics' initial values
        CHK(hipMemcpyAsync(stats.p<uint32_t>(), init, sizeof(init), hipMemcpyHostToDevice, st));
        qmcp::launch_pm_prepare_sort(st, starts.p<uint32_t>(), ends.p<uint32_t>(), n, roff.p<uint64_t>(), poff.p<uint64_t>(), n_contigs,
                                     shift, n_ranges, gridw.p<uint32_t>(), keys16.p<uint16_t>(), idx16.p<uint16_t>(),
                                     cnt_tab.p<uint32_t>(), lst_tab.p<uint32_t>(), stats.p<uint32_t>(), mask.p<unsigned long long>(),
                                     cs.ell_reg, d_exc, filter ? exc_cap : 0u, d_exc_cnt);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, keys16, "u16", 2) || !dump(stage, idx16, "u16", 2) || !dump(stage, cnt_tab, "u32", 4) ||
            !dump(stage, lst_tab, "u32", 4) || !dump(stage, stats, "u32", 4) || !dump(stage, mask, "u64", 8))
            return false;
        if (filter && !dump(stage, exc, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'A') return check_inputs(stage);

    stage = "B";
    {
        qmcp::launch_pm_row_sums(st, cnt_tab.p<uint32_t>(), lst_tab.p<uint32_t>(), n, work.p<uint32_t>());
        CHK(hipGetLastError());
        qmcp::launch_pm_tables(st, cnt_tab.p<uint32_t>(), lst_tab.p<uint32_t>(), n, n_ranges, desc.p<uint32_t>(), work.p<uint32_t>(),
                               range_start.p<uint32_t>(), max_load.p<uint32_t>(), scalars.p<uint32_t>());
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, cnt_tab, "u32", 4) || !dump(stage, desc, "u32", 4) || !dump(stage, work, "u32", 4) ||
            !dump(stage, range_start, "u32", 4) || !dump(stage, max_load, "u32", 4) || !dump(stage, scalars, "u32", 4))
            return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'B') return check_inputs(stage);

    stage = "C";
    std::vector<uint8_t> h_boff;
    {
        qmcp::launch_pm_offsets(st, keys16.p<uint16_t>(), desc.p<uint32_t>(), cnt_tab.p<uint32_t>(), n, range_start.p<uint32_t>(), shift,
                                n_ranges, gridw.p<uint32_t>(), ltot, boff.p<uint32_t>(), stats.p<uint32_t>() + 3);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, boff, "u32", 4, &h_boff) || !dump(stage, stats, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'C') return check_inputs(stage);

    const uint32_t* const hb = reinterpret_cast<const uint32_t*>(h_boff.data());
    std::vector<uint32_t> h_selend((size_t)ltot + 8, 0u);
    for (uint32_t k = 0; k < cs.n_quota; ++k) {
        stage = "D" + std::to_string(k);
        const uint32_t* const S = cs.quota.data() + (size_t)k * ltot;
        for (uint32_t p = 0; p < ltot; ++p) h_selend[p] = hb[p] + S[p];  // selend = boff (as the device wrote it) + S_k
        CHK(hipMemcpyAsync(selend.p<uint32_t>(), h_selend.data(), h_selend.size() * 4, hipMemcpyHostToDevice, st));
        if (k != 0) {  // (the first vector relies on what stages A and B cleared)
            CHK(hipMemsetAsync(mask.p<char>(), 0, mask.bytes, st));
            CHK(hipMemsetAsync(scalars.p<char>(), 0, scalars.bytes, st));
        }
        qmcp::launch_pm_walk(st, keys16.p<uint16_t>(), idx16.p<uint16_t>(), desc.p<uint32_t>(), cnt_tab.p<uint32_t>(), n,
                             range_start.p<uint32_t>(), shift, n_ranges, gridw.p<uint32_t>(), boff.p<uint32_t>(), selend.p<uint32_t>(),
                             mask.p<unsigned long long>(), scalars.p<unsigned long long>(), scratch.p<void>(), by_records);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, mask, "u64", 8) || !dump(stage, scalars, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    // what the walk only reads
    stage = "end";
    if (!dump(stage, keys16, "u16", 2) || !dump(stage, idx16, "u16", 2) || !dump(stage, cnt_tab, "u32", 4) || !dump(stage, desc, "u32", 4) ||
        !dump(stage, boff, "u32", 4))
        return false;
    return check_inputs(stage);
}

template <class T> bool read_some(std::ifstream& in, std::vector<T>& v, size_t count) {
    v.resize(count);
    if (count) in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    return (bool)in;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s case.json case.bin dump.json dump.bin\n", argv[0]); return 4; }
    std::string text;
    {
        std::ifstream f(argv[1]);
        std::stringstream ss;
        ss << f.rdbuf();
        text = ss.str();
        if (!f || text.empty()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 4; }
    }
    Case cs;
    cs.n = (uint32_t)jint(text, "n");
    cs.n_contigs = (uint32_t)jint(text, "n_contigs");
    cs.ltot = (uint32_t)jint(text, "ltot");
    cs.wish = (int)jint(text, "wish");
    cs.ell_reg = (uint32_t)jint(text, "ell_reg");
    cs.n_quota = (uint32_t)jint(text, "n_quota");
    cs.stop_after = jstr(text, "stop_after").c_str()[0];
    if (cs.n == 0 || cs.n_contigs == 0 || cs.stop_after < 'A' || cs.stop_after > 'D') { std::fprintf(stderr, "bad case\n"); return 4; }
    {
        std::ifstream in(argv[2], std::ios::binary);
        if (!in || !read_some(in, cs.starts, cs.n) || !read_some(in, cs.ends, cs.n) || !read_some(in, cs.lengths, cs.n_contigs) ||
            !read_some(in, cs.roff, (size_t)cs.n_contigs + 1) || !read_some(in, cs.quota, (size_t)cs.n_quota * cs.ltot)) {
            std::fprintf(stderr, "cannot read %s\n", argv[2]);
            return 4;
        }
    }
    cs.poff.assign((size_t)cs.n_contigs + 1, 0);
    for (uint32_t c = 0; c < cs.n_contigs; ++c) cs.poff[c + 1] = cs.poff[c] + cs.lengths[c];
    if (cs.poff[cs.n_contigs] != cs.ltot || cs.roff[cs.n_contigs] != cs.n || cs.roff[0] != 0) { std::fprintf(stderr, "inconsistent case\n"); return 4; }
    g_bin = std::fopen(argv[4], "wb");
    if (!g_bin) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 4; }
    const bool went_on = run(cs);
    std::fclose(g_bin);
    write_manifest(argv[3]);
    if (!g_hip_error.empty()) std::fprintf(stderr, "HIP error: %s\n", g_hip_error.c_str());
    for (const Violation& v : g_violations)
        std::fprintf(stderr, "guard violation: stage %s buffer %s side %s offset %zu\n", v.stage.c_str(), v.buffer.c_str(), v.side.c_str(), v.offset);
    if (!g_refused.empty()) return 2;
    return went_on && g_hip_error.empty() && g_violations.empty() && g_inputs_changed.empty() ? 0 : 3;
}
