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
// dump files and exit status: stage_driver_common.h (shared with rm_stage_driver.hip); "derived": shift, grid, sizes.
// Stages: A the producer; B row sums and tables; C bucket offsets; D0, D1, ... the walk, once per quota vector.
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
#include "stage_driver_common.h"  // buffers with guard bands, their checks, the dump and its manifest, the case readers

namespace {
using namespace stage_common;

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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s case.json case.bin dump.json dump.bin\n", argv[0]); return 4; }
    const std::string text = read_text(argv[1]);
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
    return finish(run(cs), argv[3]);
}
