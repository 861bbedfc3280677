// lab: k_pm_prepare_sort ALONE on cfg4's shape (8 contigs of 10^6 positions, 12.5 M reads of 150 each, uniform starts),
// nothing launched behind it -- the way to time the producer's timing-only variants (lab/build_variant.sh with
// -DQMCP_PM_LAB_NO_RANK, -DQMCP_PM_LAB_NO_STORE, -DQMCP_PM_LAB_SLICE_WRITEOUT), whose buffers no consumer may read.
// Buffers at the sizes api/solve_head.inc.hip gives them; 3 launches to warm up, then 20 timed one by one.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Igenome-downsampler_amd/csrc lab/pm_producer_lab.hip \
//         -Lgenome-downsampler_amd/lib -lqmcp_hip -o lab/pm_producer_lab
//   LD_LIBRARY_PATH=lab/variants/<name> lab/pm_producer_lab        (or genome-downsampler_amd/lib for the product)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "qmcp_kernels.h"

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main() {
    const uint32_t n_contigs = 8, per = 12500000u, len = 1000000u, span = 150u, n = n_contigs * per;
    std::vector<uint32_t> starts(n), ends(n);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint32_t i = 0; i < n; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        starts[i] = (uint32_t)((x >> 20) % (len - span + 1u));
        ends[i] = starts[i] + span - 1u;
    }
    std::vector<uint64_t> roff(n_contigs + 1), poff(n_contigs + 1);
    for (uint32_t c = 0; c <= n_contigs; ++c) { roff[c] = (uint64_t)c * per; poff[c] = (uint64_t)c * len; }
    const uint32_t ltot = n_contigs * len, shift = qmcp::range_shift_for(ltot);
    const qmcp::PmGridPlan grid = qmcp::pm_grid_plan(roff.data(), poff.data(), n_contigs, shift, qmcp::pm_pass(), 0);
    const uint32_t pitch = qmcp::pm_pitch(n);
    const size_t slots = qmcp::pm_slots(n, grid.n_ranges);
    std::printf("shift %u  ranges %u  aligned %d  pitch %u  stride %u\n", shift, grid.n_ranges, grid.aligned, pitch, qmcp::pm_stride(grid.n_ranges));

    uint32_t *d_s, *d_e, *d_grid, *d_cnt, *d_lst, *d_stats;
    uint64_t *d_roff, *d_poff;
    uint16_t *d_k, *d_i;
    unsigned long long* d_mask;
    CHK(hipMalloc(&d_s, (size_t)n * 4)); CHK(hipMalloc(&d_e, (size_t)n * 4));
    CHK(hipMalloc(&d_roff, roff.size() * 8)); CHK(hipMalloc(&d_poff, poff.size() * 8));
    CHK(hipMalloc(&d_grid, grid.words.size() * 4));
    CHK(hipMalloc(&d_k, slots * 2)); CHK(hipMalloc(&d_i, slots * 2));
    CHK(hipMalloc(&d_cnt, ((size_t)256 * pitch + 4) * 4)); CHK(hipMalloc(&d_lst, (size_t)256 * pitch * 4));
    CHK(hipMalloc(&d_stats, 64)); CHK(hipMalloc(&d_mask, (size_t)((n + 63u) / 64u) * 8));
    CHK(hipMemcpy(d_s, starts.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_e, ends.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_roff, roff.data(), roff.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_poff, poff.data(), poff.size() * 8, hipMemcpyHostToDevice));
    CHK(hipMemcpy(d_grid, grid.words.data(), grid.words.size() * 4, hipMemcpyHostToDevice));
    const uint32_t init[8] = {0xFFFFFFFFu, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    CHK(hipMemcpy(d_stats, init, sizeof(init), hipMemcpyHostToDevice));

    hipStream_t st;
    CHK(hipStreamCreate(&st));
    hipEvent_t a, b;
    CHK(hipEventCreate(&a)); CHK(hipEventCreate(&b));
    std::vector<float> ms;
    for (int rep = 0; rep < 23; ++rep) {
        CHK(hipEventRecord(a, st));
        qmcp::launch_pm_prepare_sort(st, d_s, d_e, n, d_roff, d_poff, n_contigs, shift, grid.n_ranges, d_grid, d_k, d_i, d_cnt, d_lst,
                                     d_stats, d_mask, 0u, nullptr, 0u, nullptr);
        CHK(hipGetLastError());
        CHK(hipEventRecord(b, st));
        CHK(hipStreamSynchronize(st));
        float t = 0.f;
        CHK(hipEventElapsedTime(&t, a, b));
        if (rep >= 3) ms.push_back(t);
    }
    double sum = 0.0;
    for (float t : ms) sum += t;
    uint32_t stats[8];
    CHK(hipMemcpy(stats, d_stats, sizeof(stats), hipMemcpyDeviceToHost));
    std::printf("k_pm_prepare_sort alone: mean %.4f ms  best %.4f ms  (20 launches; span %u..%u, bad %u)\n", sum / ms.size(),
                *std::min_element(ms.begin(), ms.end()), stats[0], stats[1], stats[2]);
    return 0;
}
