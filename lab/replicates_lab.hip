// lab: the step between two replicates of qmcp_hip_solve_replicates_*, alone.  n candidates in three columns with an
// origin column, a taken mask of the given density (cfg4 at [100] * 4: 5.4 %), and three ways to move the free reads:
//   k_rep_split        (kernels/replicates.inc.hip: whole tiles staged in LDS, streamed out)
//   k_ladder_compact   on the complemented mask (kernels/ladder.inc.hip: a quad per thread, scattered 4-byte stores)
//   hipMemcpyAsync     of the same three columns, device to device: the yardstick
// Both kernels must write the same bytes.  Prints one JSON line; lab/replicates_profile.py runs it and keeps the line.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Igenome-downsampler_amd/csrc lab/replicates_lab.hip \
//         -Lgenome-downsampler_amd/lib -lqmcp_hip -Wl,-rpath,'$ORIGIN/../genome-downsampler_amd/lib' -o lab/replicates_lab
//   lab/replicates_lab [n = 100000000] [taken per mille = 54] [reps = 9]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "qmcp_kernels.h"

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

template <typename F>
static float median_ms(hipStream_t st, int reps, F&& f) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    std::vector<float> ms;
    f();  // warm-up
    for (int r = 0; r < reps; ++r) {
        (void)hipEventRecord(a, st);
        f();
        (void)hipEventRecord(b, st);
        (void)hipEventSynchronize(b);
        float t = 0.f;
        (void)hipEventElapsedTime(&t, a, b);
        ms.push_back(t);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 100000000u;
    const uint32_t per_mille = argc > 2 ? (uint32_t)std::strtoul(argv[2], nullptr, 10) : 54u;
    const int reps = argc > 3 ? std::atoi(argv[3]) : 9;
    if (n == 0 || n > (1u << 30)) return 2;
    const uint32_t words = (n + 63u) / 64u;
    std::mt19937_64 rng(7);
    std::vector<uint64_t> taken(words, 0), rest(words, 0);
    uint32_t n_taken = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (rng() % 1000u < per_mille) {
            taken[i >> 6] |= 1ull << (i & 63u);
            ++n_taken;
        }
    for (uint32_t w = 0; w < words; ++w) rest[w] = ~taken[w];
    if (n & 63u) rest[words - 1] &= (1ull << (n & 63u)) - 1ull;
    const uint32_t n_free = n - n_taken;
    std::vector<uint32_t> col(n);
    for (uint32_t i = 0; i < n; ++i) col[i] = (uint32_t)rng();

    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const size_t cb = (size_t)n * 4;
    uint32_t *d_s, *d_e, *d_o, *d_out[2][3], *d_tw, *d_rw, *d_spine;
    uint64_t *d_taken, *d_rest;
    uint8_t* d_labels;
    CK(hipMalloc(&d_s, cb));
    CK(hipMalloc(&d_e, cb));
    CK(hipMalloc(&d_o, cb));
    for (auto& set : d_out)
        for (auto& p : set) CK(hipMalloc(&p, cb));
    CK(hipMalloc(&d_taken, (size_t)words * 8));
    CK(hipMalloc(&d_rest, (size_t)words * 8));
    CK(hipMalloc(&d_tw, ((size_t)words + 2) * 4));
    CK(hipMalloc(&d_rw, ((size_t)words + 2) * 4));
    CK(hipMalloc(&d_spine, ((size_t)qmcp::scan_spine_entries(words + 1) + 1) * 4 + 16));
    CK(hipMalloc(&d_labels, n));
    CK(hipMemcpy(d_s, col.data(), cb, hipMemcpyHostToDevice));
    std::reverse(col.begin(), col.end());
    CK(hipMemcpy(d_e, col.data(), cb, hipMemcpyHostToDevice));
    for (uint32_t i = 0; i < n; ++i) col[i] = i;  // origin: every candidate its own input index
    CK(hipMemcpy(d_o, col.data(), cb, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_taken, taken.data(), (size_t)words * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_rest, rest.data(), (size_t)words * 8, hipMemcpyHostToDevice));
    CK(hipMemset(d_labels, 0, n));
    qmcp::launch_word_popcounts(st, d_taken, words, d_tw);
    qmcp::launch_exclusive_scan(st, d_tw, words, d_tw, d_spine, true);
    qmcp::launch_word_popcounts(st, d_rest, words, d_rw);
    qmcp::launch_exclusive_scan(st, d_rw, words, d_rw, d_spine, true);
    CK(hipStreamSynchronize(st));

    const float ms_scan = median_ms(st, reps, [&] {
        qmcp::launch_word_popcounts(st, d_taken, words, d_tw);
        qmcp::launch_exclusive_scan(st, d_tw, words, d_tw, d_spine, true);
    });
    const float ms_split = median_ms(st, reps, [&] {
        qmcp::launch_rep_split(st, false, d_s, d_e, d_o, d_taken, d_tw, n, 1, d_labels, d_out[0][0], d_out[0][1], d_out[0][2]);
    });
    const float ms_split_nolabel = median_ms(st, reps, [&] {
        qmcp::launch_rep_split(st, false, d_s, d_e, d_o, d_taken, d_tw, n, 0, d_labels, d_out[0][0], d_out[0][1], d_out[0][2]);
    });
    const float ms_compact = median_ms(st, reps, [&] {
        qmcp::launch_ladder_compact(st, false, d_s, d_e, d_o, d_rest, d_rw, n, d_out[1][0], d_out[1][1], d_out[1][2]);
    });
    const float ms_levels = median_ms(st, reps, [&] { qmcp::launch_ladder_levels(st, false, d_taken, d_o, n, 1, d_labels); });
    const float ms_copy = median_ms(st, reps, [&] {
        (void)hipMemcpyAsync(d_out[1][0], d_s, cb, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(d_out[1][1], d_e, cb, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(d_out[1][2], d_o, cb, hipMemcpyDeviceToDevice, st);
    });
    CK(hipGetLastError());
    // the same bytes either way (the copy above overwrote set 1: compact once more)
    qmcp::launch_ladder_compact(st, false, d_s, d_e, d_o, d_rest, d_rw, n, d_out[1][0], d_out[1][1], d_out[1][2]);
    CK(hipStreamSynchronize(st));
    bool same = true;
    std::vector<uint32_t> a(n_free), b(n_free);
    for (int k = 0; k < 3; ++k) {
        CK(hipMemcpy(a.data(), d_out[0][k], (size_t)n_free * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), d_out[1][k], (size_t)n_free * 4, hipMemcpyDeviceToHost));
        same = same && std::memcmp(a.data(), b.data(), (size_t)n_free * 4) == 0;
    }
    std::vector<uint8_t> lab(n);
    CK(hipMemcpy(lab.data(), d_labels, n, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n && same; ++i) same = lab[i] == ((taken[i >> 6] >> (i & 63u)) & 1ull);
    // bytes the step has to move: three columns in, the free reads' three columns out, the mask and its scan, the labels
    const double moved = 3.0 * cb + 3.0 * 4.0 * n_free + 12.0 * words + (double)n_taken;
    const double copy_gbs = 2.0 * 3.0 * cb / (ms_copy * 1e6);
    std::printf("{\"n\": %u, \"taken\": %u, \"free\": %u, \"same_bytes\": %s, \"ms_popcounts_scan\": %.4f, "
                "\"ms_k_rep_split\": %.4f, \"ms_k_rep_split_without_labels\": %.4f, "
                "\"ms_k_ladder_compact_on_complement\": %.4f, \"ms_k_ladder_levels\": %.4f, \"ms_copy_three_columns\": %.4f, "
                "\"bytes_moved\": %.0f, \"copy_GBps\": %.1f, \"k_rep_split_GBps\": %.1f, \"k_ladder_compact_GBps\": %.1f, "
                "\"k_rep_split_fraction_of_copy_bandwidth\": %.3f, \"k_ladder_compact_plus_levels_fraction_of_copy_bandwidth\": "
                "%.3f}\n",
                n, n_taken, n_free, same ? "true" : "false", ms_scan, ms_split, ms_split_nolabel, ms_compact, ms_levels,
                ms_copy, moved, copy_gbs, moved / (ms_split * 1e6), moved / ((ms_compact + ms_levels) * 1e6),
                moved / (ms_split * 1e6) / copy_gbs, moved / ((ms_compact + ms_levels) * 1e6) / copy_gbs);
    return same ? 0 : 3;
}
