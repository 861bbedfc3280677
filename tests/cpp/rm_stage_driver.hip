// Stage driver of the range-major form of the range-ranked route (kernels/prepare_scan.inc.hip, ranked_route.inc.hip)
// for tests/test_gpu_rm_stages.py: host code only.  It runs the form's launches one stage at a time through the
// launch_* functions of qmcp_kernels.h -- no context, no read threshold --, every device buffer at exactly the size
// api/solve_head.inc.hip / queue_rm_head give its counterpart with a guard band on either side and a canary payload
// where a kernel is to write, and hands every buffer a stage may write back to the host for tests/rm_stage_compare.py
// to hold against the host model (tests/range_major_model.py).
//
//   rm_stage_driver <case.json> <case.bin> <dump.json> <dump.bin>
//
// case.json  {"n", "n_contigs", "ltot", "ell_reg" (0: no filter), "stop_after" ("A".."E"), "n_quota",
//            "tiles_per_block" (0: as the library chooses)} -- flat, integers and one string
// case.bin   little-endian, in this order: starts u32[n], ends u32[n], contig lengths u64[n_contigs], read offsets
//            u64[n_contigs + 1], then n_quota quota vectors, each u32 kind and either (kind 0) u32[ltot], one value per
//            global position, or (kind 1) u32 default, u32 m, u32 position[m], u32 value[m]
// dump files and exit status: stage_driver_common.h.  "derived" holds the geometry the driver took from the library.
// Buffers: table (the solve's hist2), spine2, spine, hist, keys16 (keys[0]), recs (keys[1]), idx (vals[0]), ranges
// (range starts | heaviest load at word 65540 | super_start, tile_base, pass_base from word 65544), stats, boff, selend,
// scalars, mask, scratch (rankamb), exc.
// Stages: A k_prepare (and k_nu_count_groups with a filter); B the scan; C the partition, one or two levels; D bucket
// offsets; E0, E1, ... k_rank_mark, once per quota vector with a zeroed mask and kept_total ("E0o", ...: once more with
// the list kept the other way, where the scratch buffer has room for either); "end": nothing is dumped -- what the
// ranking only reads is held against the host's copy of its last dump, and a buffer that changed is reported among
// "inputs_changed".
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

namespace {
using namespace stage_common;

struct Quota {
    uint32_t kind = 0, dflt = 0;
    std::vector<uint32_t> dense, pos, val;
};
struct Case {
    uint32_t n = 0, n_contigs = 0, ltot = 0, ell_reg = 0, n_quota = 0, tiles_per_block = 0;
    char stop_after = 'E';
    std::vector<uint32_t> starts, ends;
    std::vector<uint64_t> lengths, roff, poff;
    std::vector<Quota> quota;
};

size_t spine_bytes_for(uint32_t n, uint32_t more) { return (size_t)(qmcp::scan_spine_entries(n) + more) * sizeof(uint32_t) + 16; }

// a buffer the later stages only read: still what the host kept of its last dump?
bool unchanged(const std::string& stage, const Buf& b, const std::vector<uint8_t>& kept) {
    std::vector<uint8_t> h(b.bytes);
    if (b.bytes) CHK(hipMemcpy(h.data(), b.base + kGuard, b.bytes, hipMemcpyDeviceToHost));
    if (h.size() != kept.size() || (b.bytes && std::memcmp(h.data(), kept.data(), b.bytes) != 0)) g_inputs_changed.push_back(b.name);
    return true;
}

// -> false after a HIP error or a guard violation: nothing more is launched
bool run(const Case& cs) {
    std::string stage = "setup";
    const uint32_t n = cs.n, ltot = cs.ltot, n_contigs = cs.n_contigs;
    // what enqueue_head and queue_rm_head derive
    const uint32_t shift = qmcp::range_shift_for(ltot);
    if (!qmcp::range_path_supported(ltot)) { g_refused = "range path not supported"; return true; }
    const bool two_level = qmcp::range_path_two_level(ltot);
    const uint32_t pitch = qmcp::part_pass_pitch(n);
    const uint32_t tiles_seg = qmcp::seg_tile_bound(n);
    const size_t spine_bytes = std::max(spine_bytes_for(256u * tiles_seg, 0), spine_bytes_for(ltot + 1, 1));
    const bool filter = cs.ell_reg != 0u;
    const uint32_t exc_cap = std::max(qmcp::pm_exc_slots(n), qmcp::prepare_exc_slots(n));
    const size_t scratch_bytes = qmcp::rank_scratch_bytes(shift, ltot, n);
    const bool by_records = qmcp::rank_scratch_by_records(shift, ltot, n);
    const size_t by_pos_slots = (size_t)((ltot >> shift) + 1) << shift;
    // (the other way of keeping the list, where its slots fit the buffer as well)
    const bool other_fits = (by_records ? by_pos_slots : (size_t)n) * sizeof(uint2) <= scratch_bytes;
    {
        std::ostringstream d;
        d << "\"shift\": " << shift << ", \"two_level\": " << (two_level ? 1 : 0) << ", \"pitch\": " << pitch
          << ", \"sort_tiles\": " << qmcp::sort_tiles(n) << ", \"seg_tile_bound\": " << tiles_seg << ", \"spine_bytes\": " << spine_bytes
          << ", \"exc_cap\": " << (filter ? exc_cap : 0u) << ", \"prepare_exc_slots\": " << qmcp::prepare_exc_slots(n)
          << ", \"scratch_bytes\": " << scratch_bytes << ", \"by_records\": " << (by_records ? 1 : 0)
          << ", \"other_fits\": " << (other_fits ? 1 : 0);
        g_derived = d.str();
    }

    Buf starts, ends, roff, poff, table, spine2, spine, hist, keys16, recs, idx, ranges, stats, boff, selend, scalars, mask, scratch, exc;
    if (!alloc(starts, "starts", (size_t)n * 4, 0, cs.starts.data(), stage)) return false;
    if (!alloc(ends, "ends", (size_t)n * 4, 0, cs.ends.data(), stage)) return false;
    if (!alloc(roff, "roff", (size_t)(n_contigs + 1) * 8, 0, cs.roff.data(), stage)) return false;
    if (!alloc(poff, "poff", (size_t)(n_contigs + 1) * 8, 0, cs.poff.data(), stage)) return false;
    if (!alloc(table, "table", ((size_t)256 * pitch + 4) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(spine2, "spine2", spine_bytes, kCanary, nullptr, stage)) return false;
    if (!alloc(keys16, "keys16", (size_t)n * 8, kCanary, nullptr, stage)) return false;
    if (!alloc(idx, "idx", (size_t)n * 4, kCanary, nullptr, stage)) return false;
    if (two_level) {
        if (!alloc(spine, "spine", spine_bytes, kCanary, nullptr, stage)) return false;
        if (!alloc(hist, "hist", (size_t)256 * tiles_seg * 4, kCanary, nullptr, stage)) return false;
        if (!alloc(recs, "recs", (size_t)n * 8, kCanary, nullptr, stage)) return false;
    }
    if (!alloc(ranges, "ranges", (size_t)qmcp::words::kRangesWords * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(stats, "stats", 12 * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(boff, "boff", ((size_t)ltot + 1) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(selend, "selend", ((size_t)ltot + 8) * 4, kCanary, nullptr, stage)) return false;
    if (!alloc(scalars, "scalars", 64, 0xFF, nullptr, stage)) return false;
    if (!alloc(mask, "mask", (size_t)((n + 63u) / 64u) * 8, 0xFF, nullptr, stage)) return false;
    if (!alloc(scratch, "scratch", scratch_bytes, kCanary, nullptr, stage)) return false;
    if (filter && !alloc(exc, "exc", qmcp::nu_exc_bytes(exc_cap), kCanary, nullptr, stage)) return false;
    uint32_t* const d_exc = filter ? exc.p<uint32_t>() : nullptr;
    uint32_t* const d_exc_cnt = filter ? qmcp::nu_exc_counts(d_exc, exc_cap) : nullptr;
    uint32_t* const d_range_start = ranges.p<uint32_t>();
    uint32_t* const d_max_load = qmcp::words::max_load(d_range_start);
    uint32_t* const d_seg_tables = qmcp::words::seg_tables(d_range_start);

    hipStream_t st;
    CHK(hipStreamCreate(&st));
    auto end_stage = [&]() -> bool {  // guards and read-only inputs, after every stage
        if (!check_guards(stage) || !check_inputs(stage)) return false;
        return g_violations.empty();
    };

    stage = "A";
    {
        const uint32_t init[8] = {0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // the statistics' initial values
        CHK(hipMemcpyAsync(stats.p<uint32_t>(), init, sizeof(init), hipMemcpyHostToDevice, st));
        if (filter) CHK(hipMemsetAsync(d_exc_cnt, 0, ((size_t)exc_cap / 128 + 4) * sizeof(uint32_t), st));
        qmcp::launch_prepare(st, starts.p<uint32_t>(), ends.p<uint32_t>(), n, roff.p<uint64_t>(), poff.p<uint64_t>(), n_contigs, nullptr,
                             nullptr, nullptr, stats.p<uint32_t>(), two_level ? shift + 8 : shift, table.p<uint32_t>(), nullptr, nullptr,
                             mask.p<unsigned long long>(), cs.ell_reg, d_exc, exc_cap, d_exc_cnt, cs.tiles_per_block);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, table, "u32", 4) || !dump(stage, stats, "u32", 4) || !dump(stage, mask, "u64", 8)) return false;
        if (filter && !dump(stage, exc, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'A') return true;

    stage = "B";
    std::vector<uint8_t> h_table;
    {
        qmcp::launch_exclusive_scan(st, table.p<uint32_t>(), 256u * pitch, table.p<uint32_t>(), spine2.p<uint32_t>(), true);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, table, "u32", 4, &h_table) || !dump(stage, spine2, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'B') return true;

    stage = "C";
    std::vector<uint8_t> h_keys16, h_idx, h_ranges;
    {
        if (!two_level) {
            qmcp::launch_range_partition(st, nullptr, starts.p<uint32_t>(), roff.p<uint64_t>(), poff.p<uint64_t>(), n_contigs, n, shift,
                                         table.p<uint32_t>(), keys16.p<uint16_t>(), idx.p<uint32_t>(), d_range_start, d_max_load,
                                         ends.p<uint32_t>(), cs.ell_reg);
        } else {
            qmcp::launch_partition_level1(st, starts.p<uint32_t>(), roff.p<uint64_t>(), poff.p<uint64_t>(), n_contigs, n, shift + 8,
                                          table.p<uint32_t>(), recs.p<void>(), d_seg_tables, d_max_load, ends.p<uint32_t>(), cs.ell_reg);
            CHK(hipGetLastError());
            qmcp::launch_partition_level2(st, recs.p<void>(), n, shift, d_seg_tables, hist.p<uint32_t>(), spine.p<uint32_t>(),
                                          keys16.p<uint16_t>(), idx.p<uint32_t>(), d_range_start, d_max_load);
        }
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, keys16, "u16", 2, &h_keys16) || !dump(stage, idx, "u32", 4, &h_idx) || !dump(stage, ranges, "u32", 4, &h_ranges))
            return false;
        if (two_level && (!dump(stage, recs, "u32", 4) || !dump(stage, hist, "u32", 4))) return false;
        if (!unchanged(stage, table, h_table)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'C') return true;

    stage = "D";
    std::vector<uint8_t> h_boff;
    {
        qmcp::launch_range_offsets(st, keys16.p<uint16_t>(), d_range_start, shift, ltot, boff.p<uint32_t>(), stats.p<uint32_t>() + 3);
        CHK(hipGetLastError());
        CHK(hipStreamSynchronize(st));
        if (!dump(stage, boff, "u32", 4, &h_boff) || !dump(stage, stats, "u32", 4)) return false;
        if (!end_stage()) return false;
    }
    if (cs.stop_after == 'D') {
        stage = "end";
        if (!unchanged(stage, keys16, h_keys16) || !unchanged(stage, idx, h_idx) || !unchanged(stage, ranges, h_ranges) ||
            !unchanged(stage, table, h_table))
            return false;
        return check_inputs(stage);
    }

    const uint32_t* const hb = reinterpret_cast<const uint32_t*>(h_boff.data());
    std::vector<uint8_t> h_selend(((size_t)ltot + 8) * 4, 0);
    uint32_t* const hs = reinterpret_cast<uint32_t*>(h_selend.data());
    for (uint32_t k = 0; k < cs.n_quota; ++k) {
        const Quota& q = cs.quota[k];
        // selend = boff (as the device wrote it) + S_k
        if (q.kind == 0) {
            for (uint32_t p = 0; p < ltot; ++p) hs[p] = hb[p] + q.dense[p];
        } else {
            for (uint32_t p = 0; p < ltot; ++p) hs[p] = hb[p] + q.dflt;
            for (size_t j = 0; j < q.pos.size(); ++j) hs[q.pos[j]] = hb[q.pos[j]] + q.val[j];
        }
        for (int other = 0; other < (other_fits ? 2 : 1); ++other) {
            stage = "E" + std::to_string(k) + (other ? "o" : "");
            CHK(hipMemcpyAsync(selend.p<uint32_t>(), hs, h_selend.size(), hipMemcpyHostToDevice, st));
            CHK(hipMemsetAsync(mask.p<char>(), 0, mask.bytes, st));
            CHK(hipMemsetAsync(scalars.p<char>(), 0, scalars.bytes, st));
            qmcp::launch_rank_mark(st, keys16.p<uint16_t>(), idx.p<uint32_t>(), d_range_start, shift, ltot, boff.p<uint32_t>(),
                                   selend.p<uint32_t>(), mask.p<unsigned long long>(), scalars.p<unsigned long long>(), scratch.p<void>(),
                                   other ? !by_records : by_records);
            CHK(hipGetLastError());
            CHK(hipStreamSynchronize(st));
            if (!dump(stage, mask, "u64", 8) || !dump(stage, scalars, "u32", 4)) return false;
            if (!unchanged(stage, selend, h_selend)) return false;
            if (!end_stage()) return false;
        }
    }
    // what the ranking only reads
    stage = "end";
    if (!unchanged(stage, keys16, h_keys16) || !unchanged(stage, idx, h_idx) || !unchanged(stage, ranges, h_ranges) ||
        !unchanged(stage, boff, h_boff) || !unchanged(stage, table, h_table))
        return false;
    return check_inputs(stage);
}

bool read_quota(std::ifstream& in, Quota& q, uint32_t ltot) {
    std::vector<uint32_t> w;
    if (!read_some(in, w, 1)) return false;
    q.kind = w[0];
    if (q.kind == 0) return read_some(in, q.dense, ltot);
    if (q.kind != 1 || !read_some(in, w, 2)) return false;
    q.dflt = w[0];
    const uint32_t m = w[1];
    if (!read_some(in, q.pos, m) || !read_some(in, q.val, m)) return false;
    for (uint32_t p : q.pos)
        if (p >= ltot) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: %s case.json case.bin dump.json dump.bin\n", argv[0]); return 4; }
    const std::string text = read_text(argv[1]);
    Case cs;
    cs.n = (uint32_t)jint(text, "n");
    cs.n_contigs = (uint32_t)jint(text, "n_contigs");
    cs.ltot = (uint32_t)jint(text, "ltot");
    cs.ell_reg = (uint32_t)jint(text, "ell_reg");
    cs.n_quota = (uint32_t)jint(text, "n_quota");
    cs.tiles_per_block = (uint32_t)jint(text, "tiles_per_block");
    cs.stop_after = jstr(text, "stop_after").c_str()[0];
    if (cs.n == 0 || cs.n_contigs == 0 || cs.ltot == 0 || cs.stop_after < 'A' || cs.stop_after > 'E' || cs.tiles_per_block > 8 ||
        (cs.tiles_per_block & 1u)) {
        std::fprintf(stderr, "bad case\n");
        return 4;
    }
    {
        std::ifstream in(argv[2], std::ios::binary);
        bool ok = in && read_some(in, cs.starts, cs.n) && read_some(in, cs.ends, cs.n) && read_some(in, cs.lengths, cs.n_contigs) &&
                  read_some(in, cs.roff, (size_t)cs.n_contigs + 1);
        cs.quota.resize(cs.n_quota);
        for (uint32_t k = 0; ok && k < cs.n_quota; ++k) ok = read_quota(in, cs.quota[k], cs.ltot);
        if (!ok) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 4; }
    }
    cs.poff.assign((size_t)cs.n_contigs + 1, 0);
    for (uint32_t c = 0; c < cs.n_contigs; ++c) cs.poff[c + 1] = cs.poff[c] + cs.lengths[c];
    if (cs.poff[cs.n_contigs] != cs.ltot || cs.roff[cs.n_contigs] != cs.n || cs.roff[0] != 0) { std::fprintf(stderr, "inconsistent case\n"); return 4; }
    g_bin = std::fopen(argv[4], "wb");
    if (!g_bin) { std::fprintf(stderr, "cannot write %s\n", argv[4]); return 4; }
    return finish(run(cs), argv[3]);
}
