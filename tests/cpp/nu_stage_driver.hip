// Stage driver of the near-uniform route (kernels/near_uniform.inc.hip and the sweeps it runs under nadj) for
// tests/test_gpu_nu_stages.py: host code only.  It runs the route's launches one stage at a time through the launch_*
// functions of qmcp_kernels.h -- no context, no gates of the host's (plan_near_uniform, the tenth-of-the-reads limit) --,
// every device buffer with a guard band on either side and a canary payload where a kernel is to write, and hands every
// buffer a stage may write back to the host for tests/nu_stage_compare.py to hold against the host model
// (tests/nu_stage_model.py).  The exception list is an INPUT here, already in the product's layout (the producers that
// write it have their own stage tests), so a case can shape groups and the overflow region as it likes.
//
//   nu_stage_driver <case.json> <case.bin> <dump.json> <dump.bin>
//
// case.json  {"n" (reads in all: sizes the list and the mask), "n_contigs", "ltot", "ell", "M", "n_groups", "n_over",
//            "suspects_cap" (may be left out: 65 536), "rounds_max", "form" ("ev" | "gen" | "gen_cuts")} -- flat, integers
//            and one string
// case.bin   little-endian, in this order: starts u32[n], ends u32[n] (every read, as the public entry takes them: only
//            stage "0" reads them), contig lengths u64[n_contigs], boff u32[ltot + 1] (prefix counts of the
//            regular reads' starts), cnt u32[n_groups] (filled slots per group, <= 128), then gs, ge, idx u32[sum cnt]
//            each (the groups' filled slots, group after group), then gs, ge, idx u32[n_over] each (the overflow region)
// dump files and exit status: stage_driver_common.h.  A launch function that returns false: "refused", status 2.
// Stages: "0" the route's two looks at the spans, launch_nu_count_span (reads of span ell) and launch_span_mode_share
// (reads sampled, reads in the fullest of 512 span bins, its span): four words, "span_stats"; "S" launch_nu_setup; "cuts"
// (gen_cuts) launch_sweep_segments; per round r = 1, 2, ... the host loop of near_uniform_tail without speculation:
// "r.sweep", the sweep of the case's form under nadj, and "r.round", launch_nu_round (then sweep_from, marks and dirty
// change places); rounds go on until one applies nothing, a flag is set or rounds_max is reached; "mark" (only after a
// round that applied nothing) launch_nu_mark_selected on a zeroed mask.  "derived" says how it ended: rounds, flags, settled.
// Forms: ev -- pack, chain, expand with nadj, sweep_from and the checkpoint buffer, selend_prev null; gen -- whole
// contigs, selend_prev and the dirty cells on; gen_cuts -- the exact stretch table once, then gen under it with the
// round before's marks from round 2 on.  seg_fine is always null: the speculative tiers live in speculative_sweep inside
// the API and stay with the large tests (tests/test_gpu_near_uniform.py).
// The list's buffer is large (the overflow region): of pick and key the groups' slots and the used part of the overflow
// region are dumped; any other slot that lost its canary -- and any change to the list's inputs -- is a violation.
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
#include "solve_words.h"
#include "stage_driver_common.h"
#include "sweep_plan.h"

namespace {
using namespace stage_common;

struct Case {
    uint32_t n = 0, n_contigs = 0, ltot = 0, ell = 0, M = 0, n_groups = 0, n_over = 0, suspects_cap = 0, rounds_max = 0;
    std::string form;
    std::vector<uint64_t> lengths, poff;
    std::vector<uint32_t> starts, ends, boff, cnt, gs, ge, idx, ogs, oge, oidx;
};
constexpr uint32_t kGroup = 128, kCanary32 = 0xA5A5A5A5u;

bool dump_host(const std::string& stage, const char* name, const char* dtype, size_t elem, const void* p, size_t count) {
    if (count && std::fwrite(p, elem, count, g_bin) != count) { g_hip_error = "stage " + stage + ": short write of the dump"; return false; }
    g_entries.push_back({stage, name, dtype, count, g_bin_at});
    g_bin_at += count * elem;
    return true;
}

// -> false after a HIP error or a guard violation: nothing more is launched
bool run(const Case& cs) {
    std::string stage = "setup";
    const uint32_t n_contigs = cs.n_contigs, ltot = cs.ltot, ell = cs.ell, M = cs.M;
    const uint32_t cap = std::max(qmcp::pm_exc_slots(cs.n), qmcp::prepare_exc_slots(cs.n));
    const uint32_t over = qmcp::nu_overflow_slots(), gcap = cap - over, groups_all = gcap / kGroup;
    if (cs.n_groups > groups_all || cs.n_over > over) { g_refused = "the list does not hold the case's groups"; return true; }
    const bool ev = cs.form == "ev", cuts = cs.form == "gen_cuts";
    uint32_t n_exc = cs.n_over;
    for (uint32_t c : cs.cnt) n_exc += c;
    const uint32_t windows = cuts ? qmcp::sweep_segment_windows(ltot, ell, n_contigs) : 0u;
    if (cuts && windows == 0) { g_refused = "no windows for cut points at this size"; return true; }
    const uint32_t n_cand = n_contigs + windows;
    const uint32_t wg_max = qmcp::sweep_ev_workgroups_max(n_contigs);
    const uint32_t cells_words = (uint32_t)(qmcp::nu_cells_bytes() / 4);  // kNuMaxCells + 3
    uint32_t shift = 8;
    while (((uint64_t)ltot >> shift) + 1 > (1u << 17)) ++shift;
    const uint32_t n_cells = (uint32_t)(((uint64_t)ltot >> shift) + 1);
    const size_t seg_words = qmcp::sweep_segment_words(n_contigs, qmcp::kMaxSweepWindows);

    // the list: canary everywhere, the inputs' slots filled, the counts' region zeroed as the producers' host code does
    const size_t exc_words = qmcp::nu_exc_bytes(cap) / 4;
    std::vector<uint32_t> h_exc(exc_words, kCanary32), h_now(exc_words);
    std::vector<uint32_t> valid;  // the filled slots, in the dense order
    {
        size_t at = 0;
        for (uint32_t g = 0; g < cs.n_groups; ++g)
            for (uint32_t k = 0; k < cs.cnt[g]; ++k, ++at) {
                const size_t i = (size_t)g * kGroup + k;
                h_exc[i] = cs.gs[at]; h_exc[cap + i] = cs.ge[at]; h_exc[2 * (size_t)cap + i] = cs.idx[at];
                valid.push_back((uint32_t)i);
            }
        for (uint32_t k = 0; k < cs.n_over; ++k) {
            const size_t i = (size_t)gcap + k;
            h_exc[i] = cs.ogs[k]; h_exc[cap + i] = cs.oge[k]; h_exc[2 * (size_t)cap + i] = cs.oidx[k];
            valid.push_back((uint32_t)i);
        }
        for (size_t g = 0; g < (size_t)cap / kGroup + 4; ++g) h_exc[6 * (size_t)cap + g] = g < cs.n_groups ? cs.cnt[g] : 0u;
    }
    std::vector<uint8_t> is_valid(cap, 0);
    for (uint32_t i : valid) is_valid[i] = 1;
    uint32_t h_stats[12] = {0};
    h_stats[qmcp::words::kExceptions] = n_exc;
    h_stats[qmcp::words::kOverflowEntries] = cs.n_over;
    {
        std::ostringstream d;
        d << "\"cap\": " << cap << ", \"n_exc\": " << n_exc << ", \"windows\": " << windows << ", \"n_cells\": " << n_cells
          << ", \"shift\": " << shift;
        g_derived = d.str();
    }

    Buf starts, ends, span_stats, boff, poff, stats, exc, ce, spine, nadj, state, viol_key, viol_idx, from0, from1, sus, marks0, marks1,
        dirty0, dirty1, prev, selend, sev, pk, lastns, ckpt, scalars, segs, mask;
    if (!alloc(starts, "starts", (size_t)cs.n * 4, 0, cs.starts.data(), stage)) return false;
    if (!alloc(ends, "ends", (size_t)cs.n * 4, 0, cs.ends.data(), stage)) return false;
    if (!alloc(span_stats, "span_stats", 4 * 4, 0, nullptr, stage)) return false;
    if (!alloc(boff, "boff", ((size_t)ltot + 1) * 4, 0, cs.boff.data(), stage)) return false;
    if (!alloc(poff, "poff", ((size_t)n_contigs + 1) * 8, 0, cs.poff.data(), stage)) return false;
    if (!alloc(stats, "stats", sizeof(h_stats), 0, h_stats, stage)) return false;
    if (!alloc(exc, "exc", exc_words * 4, kCanary, nullptr, stage)) return false;
    CHK(hipMemcpy(exc.p<uint32_t>(), h_exc.data(), exc_words * 4, hipMemcpyHostToDevice));
    if (!alloc(ce, "ce", ((size_t)ltot + 3) * 4, kCanary, nullptr, stage)) return false;
    const uint32_t scanned = std::max(std::max(ltot + 2, cells_words), groups_all + 1);  // the longest of the route's scans
    if (!alloc(spine, "spine", (size_t)(qmcp::scan_spine_entries(scanned) + 1) * 4 + 16, kCanary, nullptr, stage)) return false;
    if (!alloc(nadj, "nadj", ((size_t)ltot + 1) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(state, "state", 64, 0, nullptr, stage)) return false;
    if (!alloc(viol_key, "viol_key", (size_t)n_contigs * 8, kCanary, nullptr, stage)) return false;
    if (!alloc(viol_idx, "viol_idx", (size_t)n_contigs * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(from0, "sweep_from0", (size_t)n_contigs * 4, 0, nullptr, stage)) return false;
    if (!alloc(from1, "sweep_from1", (size_t)n_contigs * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(sus, "suspects", qmcp::nu_suspect_bytes(cs.suspects_cap), kCanary, nullptr, stage)) return false;
    if (!alloc(marks0, "marks0", (size_t)n_cand * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(marks1, "marks1", (size_t)n_cand * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(dirty0, "dirty0", qmcp::nu_cells_bytes(), ev ? kCanary : 0, nullptr, stage)) return false;
    if (!alloc(dirty1, "dirty1", qmcp::nu_cells_bytes(), ev ? kCanary : 0, nullptr, stage)) return false;
    if (!alloc(prev, "selend_prev", ((size_t)ltot + 8) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(selend, "selend", ((size_t)ltot + 8) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(scalars, "scalars", qmcp::words::kScalarsBytes, 0, nullptr, stage)) return false;
    if (!alloc(mask, "mask", (size_t)((cs.n + 63u) / 64u) * 8, 0, nullptr, stage)) return false;
    if (ev) {
        if (!alloc(sev, "sev", ((size_t)ltot + 8) * 4, kCanary, nullptr, stage)) return false;
        if (!alloc(pk, "pk", qmcp::sweep_ev_pack_bytes(ltot, ell, wg_max), kCanary, nullptr, stage)) return false;
        if (!alloc(lastns, "lastns", qmcp::sweep_ev_last_bytes(ltot, ell, wg_max), kCanary, nullptr, stage)) return false;
        if (!alloc(ckpt, "ckpt", qmcp::sweep_ev_ckpt_bytes(ltot, ell, wg_max), kCanary, nullptr, stage)) return false;
    }
    if (cuts && !alloc(segs, "segs", seg_words * 4, kCanary, nullptr, stage)) return false;
    uint32_t* const d_iters = qmcp::words::sweep_iters(scalars.p<char>());
    Buf* sweep_from[2] = {&from0, &from1};
    Buf* marks[2] = {&marks0, &marks1};
    Buf* dirty[2] = {&dirty0, &dirty1};

    hipStream_t st;
    CHK(hipStreamCreate(&st));
    // the list after a stage: what is dumped of it, and everything else of it held against what it must still be
    auto dump_list = [&]() -> bool {
        CHK(hipMemcpy(h_now.data(), exc.p<uint32_t>(), exc_words * 4, hipMemcpyDeviceToHost));
        const uint32_t* pick = h_now.data() + 3 * (size_t)cap;
        const uint64_t* key = reinterpret_cast<const uint64_t*>(h_now.data() + 4 * (size_t)cap);
        const uint32_t* goff = h_now.data() + 6 * (size_t)cap + cap / kGroup + 4;
        const uint32_t* dense = goff + cap / kGroup + 4;
        const size_t gslots = (size_t)cs.n_groups * kGroup;
        if (!dump_host(stage, "pick", "u32", 4, pick, gslots) || !dump_host(stage, "pick_over", "u32", 4, pick + gcap, cs.n_over) ||
            !dump_host(stage, "key", "u64", 8, key, gslots) || !dump_host(stage, "key_over", "u64", 8, key + gcap, cs.n_over) ||
            !dump_host(stage, "goff", "u32", 4, goff, (size_t)cs.n_groups + 1) || !dump_host(stage, "goff_total", "u32", 4, goff + groups_all, 1) ||
            !dump_host(stage, "dense", "u32", 4, dense, n_exc))
            return false;
        auto violation = [&](const char* what, size_t i) { g_violations.push_back({stage, std::string("exc.") + what, "slot", i}); return true; };
        bool bad = false;
        for (size_t i = 0; i < (size_t)cap && !bad; ++i)
            if (!is_valid[i] && pick[i] != kCanary32) bad = violation("pick", i);
        bad = false;
        for (size_t i = 0; i < (size_t)cap && !bad; ++i)
            if (!is_valid[i] && key[i] != 0xA5A5A5A5A5A5A5A5ull) bad = violation("key", i);
        bad = false;
        for (size_t i = n_exc; i < (size_t)cap + 8 && !bad; ++i)  // (the rest of the filled slots' indices, and the buffer's tail)
            if (dense[i] != kCanary32) bad = violation("dense", i);
        bad = false;
        for (size_t g = (size_t)groups_all + 1; g < (size_t)cap / kGroup + 4 && !bad; ++g)
            if (goff[g] != kCanary32) bad = violation("goff", g);
        // the producer's part: starts, ends, indices and the groups' counts
        if (std::memcmp(h_now.data(), h_exc.data(), 3 * (size_t)cap * 4) != 0 ||
            std::memcmp(h_now.data() + 6 * (size_t)cap, h_exc.data() + 6 * (size_t)cap, ((size_t)cap / kGroup + 4) * 4) != 0)
            g_inputs_changed.push_back("exc");
        return true;
    };
    auto end_stage = [&]() -> bool {  // guards and read-only inputs, after every stage
        if (!check_guards(stage) || !check_inputs(stage)) return false;
        return g_violations.empty() && g_inputs_changed.empty();
    };
    // the cells' buffers are sized for 2^17 + 1 cells whatever the genome: the case's cells are dumped, the rest must keep
    // what it held
    std::vector<uint32_t> h_words;
    auto rest_keeps = [&](const Buf& b, size_t from, size_t upto, uint32_t value) {
        for (size_t i = from; i < upto; ++i)
            if (h_words[i] != value) { g_violations.push_back({stage, b.name, "rest", i}); return; }
    };
    auto dump_cells = [&](const Buf& b, uint32_t rest) -> bool {
        h_words.resize(b.bytes / 4);
        CHK(hipMemcpy(h_words.data(), b.p<uint32_t>(), b.bytes, hipMemcpyDeviceToHost));
        rest_keeps(b, (size_t)n_cells + 1, h_words.size(), rest);
        return dump_host(stage, b.name.c_str(), "u32", 4, h_words.data(), (size_t)n_cells + 1);
    };
    auto dump_suspects = [&]() -> bool {  // the four lists whole, then the cells' counts and starts
        h_words.resize(sus.bytes / 4);
        CHK(hipMemcpy(h_words.data(), sus.p<uint32_t>(), sus.bytes, hipMemcpyDeviceToHost));
        const size_t lists = 5 * (size_t)cs.suspects_cap;
        rest_keeps(sus, lists + n_cells + 1, lists + cells_words, kCanary32);
        rest_keeps(sus, lists + cells_words + n_cells + 2, h_words.size(), kCanary32);
        return dump_host(stage, "lists", "u32", 4, h_words.data(), lists) &&
               dump_host(stage, "bins_count", "u32", 4, h_words.data() + lists, (size_t)n_cells + 1) &&
               dump_host(stage, "bins_start", "u32", 4, h_words.data() + lists + cells_words, (size_t)n_cells + 2);
    };
    auto dump_common = [&]() -> bool {
        return dump(stage, ce, "u32", 4) && dump(stage, nadj, "u32", 4) && dump(stage, state, "u32", 4) && dump(stage, selend, "u32", 4) &&
               dump_suspects() && dump(stage, viol_key, "u64", 8) && dump(stage, viol_idx, "u32", 4) &&
               dump(stage, from0, "u32", 4) && dump(stage, from1, "u32", 4) && dump(stage, marks0, "u32", 4) && dump(stage, marks1, "u32", 4) &&
               dump_cells(dirty0, ev ? kCanary32 : 0u) && dump_cells(dirty1, ev ? kCanary32 : 0u) && dump(stage, prev, "u32", 4) &&
               (!cuts || dump(stage, segs, "u32", 4)) && dump(stage, mask, "u64", 8) && dump(stage, scalars, "u32", 4) && dump_list();
    };

    stage = "0";
    qmcp::launch_nu_count_span(st, starts.p<uint32_t>(), ends.p<uint32_t>(), cs.n, ell, span_stats.p<uint32_t>());
    qmcp::launch_span_mode_share(st, starts.p<uint32_t>(), ends.p<uint32_t>(), cs.n, span_stats.p<uint32_t>() + 1);
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(st));
    if (!dump(stage, span_stats, "u32", 4) || !end_stage()) return false;

    stage = "S";
    qmcp::launch_nu_setup(st, exc.p<uint32_t>(), cap, n_exc, stats.p<uint32_t>() + qmcp::words::kOverflowEntries, boff.p<uint32_t>(), ltot, ell,
                          M, ce.p<uint32_t>(), spine.p<uint32_t>(), nadj.p<int32_t>(), state.p<uint32_t>());
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(st));
    if (!dump_common() || !end_stage()) return false;

    qmcp::SweepAxis ax{st, boff.p<uint32_t>(), poff.p<uint64_t>(), n_contigs, ltot};
    if (cuts) {
        stage = "cuts";
        ax = qmcp::launch_sweep_segments(ax, nullptr, ell, M, windows, segs.p<uint32_t>(), ce.p<uint32_t>());
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump_common() || !end_stage()) return false;
    }

    uint32_t rounds = 0, h_state[16] = {0};
    bool settled = false;
    while (rounds < cs.rounds_max && !settled) {
        ++rounds;
        stage = std::to_string(rounds) + ".sweep";
        bool ok;
        if (ev) {
            ok = qmcp::launch_sweep_ev_pack(ax, ell, M, pk.p<uint32_t>(), nadj.p<int32_t>(), sweep_from[0]->p<uint32_t>());
            if (ok) CHK(hipGetLastError());
            ok = ok && qmcp::launch_sweep_ev_chain(ax, ell, M, pk.p<uint32_t>(), sev.p<uint32_t>(), lastns.p<uint32_t>(), d_iters,
                                                   nadj.p<int32_t>(), ckpt.p<uint32_t>(), sweep_from[0]->p<uint32_t>());
            if (ok) CHK(hipGetLastError());
            ok = ok && qmcp::launch_sweep_ev_expand(ax, ell, M, sev.p<uint32_t>(), lastns.p<uint32_t>(), selend.p<uint32_t>(),
                                                    sweep_from[0]->p<uint32_t>());
        } else {
            ok = qmcp::launch_sweep_uniform_gen(ax, ell, M, selend.p<uint32_t>(), d_iters, nullptr,
                                                (ax.seg != nullptr && rounds > 1) ? marks[0]->p<uint32_t>() : nullptr, nadj.p<int32_t>());
        }
        if (!ok) { g_refused = "stage " + stage + ": the sweep does not take this span and cap"; return true; }
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump_common() || !end_stage()) return false;

        stage = std::to_string(rounds) + ".round";
        qmcp::launch_nu_round(st, exc.p<uint32_t>(), cap, n_exc, stats.p<uint32_t>() + qmcp::words::kOverflowEntries, rounds == 1,
                              boff.p<uint32_t>(), selend.p<uint32_t>(), nadj.p<int32_t>(), ce.p<uint32_t>(), poff.p<uint64_t>(), n_contigs, ell, M,
                              sus.p<uint2>(), cs.suspects_cap, state.p<uint32_t>(), viol_key.p<unsigned long long>(), viol_idx.p<uint32_t>(),
                              sweep_from[0]->p<uint32_t>(), sweep_from[1]->p<uint32_t>(), ltot, spine.p<uint32_t>(),
                              !ev ? ax.seg : nullptr, ax.n_seg_max, marks[1]->p<uint32_t>(), !ev ? prev.p<uint32_t>() : nullptr,
                              dirty[0]->p<uint32_t>(), dirty[1]->p<uint32_t>(), nullptr, nullptr);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        std::swap(sweep_from[0], sweep_from[1]);
        std::swap(marks[0], marks[1]);
        std::swap(dirty[0], dirty[1]);
        if (!dump_common() || !end_stage()) return false;
        CHK(hipMemcpy(h_state, state.p<uint32_t>(), sizeof(h_state), hipMemcpyDeviceToHost));
        if (h_state[2] != 0) break;
        settled = h_state[1] == 0;
    }
    {
        std::ostringstream d;
        d << g_derived << ", \"rounds\": " << rounds << ", \"flags\": " << h_state[2] << ", \"settled\": " << (settled ? 1 : 0)
          << ", \"selected\": " << h_state[3];
        g_derived = d.str();
    }
    if (!settled) { (void)hipStreamDestroy(st); return true; }

    stage = "mark";
    qmcp::launch_nu_mark_selected(st, exc.p<uint32_t>(), cap, n_exc, stats.p<uint32_t>() + qmcp::words::kOverflowEntries,
                                  mask.p<unsigned long long>(), scalars.p<unsigned long long>());
    CHK(hipGetLastError());
    CHK(hipStreamSynchronize(st));
    const bool ok = dump_common() && end_stage();
    (void)hipStreamDestroy(st);
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s case.json case.bin dump.json dump.bin\n", argv[0]); return 4; }
    const std::string text = read_text(argv[1]);
    Case cs;
    cs.n = (uint32_t)jint(text, "n");
    cs.n_contigs = (uint32_t)jint(text, "n_contigs");
    cs.ltot = (uint32_t)jint(text, "ltot");
    cs.ell = (uint32_t)jint(text, "ell");
    cs.M = (uint32_t)jint(text, "M");
    cs.n_groups = (uint32_t)jint(text, "n_groups");
    cs.n_over = (uint32_t)jint(text, "n_over");
    cs.suspects_cap = text.find("\"suspects_cap\"") != std::string::npos ? (uint32_t)jint(text, "suspects_cap") : 65536u;
    cs.rounds_max = (uint32_t)jint(text, "rounds_max");
    cs.form = jstr(text, "form");
    if (cs.n == 0 || cs.n_contigs == 0 || cs.n_contigs >= 256 || cs.ltot == 0 || cs.ell < 2 || cs.M == 0 || cs.suspects_cap == 0 ||
        cs.rounds_max == 0 || (cs.form != "ev" && cs.form != "gen" && cs.form != "gen_cuts")) {
        std::fprintf(stderr, "bad case\n");
        return 4;
    }
    {
        std::ifstream in(argv[2], std::ios::binary);
        bool ok = in && read_some(in, cs.starts, cs.n) && read_some(in, cs.ends, cs.n) && read_some(in, cs.lengths, cs.n_contigs) &&
                  read_some(in, cs.boff, (size_t)cs.ltot + 1) && read_some(in, cs.cnt, cs.n_groups);
        size_t slots = 0;
        for (uint32_t c : cs.cnt) { slots += c; ok = ok && c <= kGroup; }
        ok = ok && read_some(in, cs.gs, slots) && read_some(in, cs.ge, slots) && read_some(in, cs.idx, slots) &&
             read_some(in, cs.ogs, cs.n_over) && read_some(in, cs.oge, cs.n_over) && read_some(in, cs.oidx, cs.n_over);
        if (!ok) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 4; }
    }
    cs.poff.assign((size_t)cs.n_contigs + 1, 0);
    for (uint32_t c = 0; c < cs.n_contigs; ++c) cs.poff[c + 1] = cs.poff[c] + cs.lengths[c];
    // every exception inside the axis, start <= end, shorter than the span, its index a read's: what the kernels rely on
    auto inside = [&](const std::vector<uint32_t>& s, const std::vector<uint32_t>& e, const std::vector<uint32_t>& x) {
        for (size_t i = 0; i < s.size(); ++i)
            if (s[i] > e[i] || e[i] >= cs.ltot || e[i] - s[i] + 1 >= cs.ell || x[i] >= cs.n) return false;
        return true;
    };
    if (cs.poff[cs.n_contigs] != cs.ltot || cs.boff[0] != 0 || !inside(cs.gs, cs.ge, cs.idx) || !inside(cs.ogs, cs.oge, cs.oidx)) {
        std::fprintf(stderr, "inconsistent case\n");
        return 4;
    }
    g_bin = std::fopen(argv[4], "wb");
    if (!g_bin) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 4; }
    return finish(run(cs), argv[3]);
}
