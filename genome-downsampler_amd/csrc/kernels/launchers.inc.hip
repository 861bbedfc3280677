// launchers.inc.hip -- part of qmcp_kernels.hip (one translation unit; included inside namespace qmcp).
// ------------------------------------------------------------------ host-side launchers
static inline uint32_t grid_for(uint64_t n, uint32_t block, uint32_t cap = 256 * 8) {
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

uint32_t sort_tiles(uint32_t n) { return (n + kSortTile - 1) / kSortTile; }
static inline uint32_t tiles_per_block_for(uint32_t n_tiles) {
    // keep >= ~2048 workgroups in flight; up to 8 consecutive tiles per workgroup
    uint32_t g = n_tiles / 2048;
    return g < 1 ? 1 : (g > 8 ? 8 : g);
}

// A run-time integer to a compile-time one: f(std::integral_constant<int, V>{}) for the V among Vs that equals v;
// false when none does (nothing is called).  The launchers pick their template instantiations with it.
template <int... Vs, class F>
static inline bool dispatch_int(int v, F&& f) {
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}
template <class F>
static inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
// ... and the two layouts of sorted reads to the accessor the kernels take: f(SortedK64) or f(SortedRec); with the
// values beside wide keys, f(KeysSplit64) or f(KeysRec)
template <class F>
static inline void dispatch_sorted(bool wide, const void* sorted, F&& f) {
    if (wide) f(SortedK64{(const uint64_t*)sorted});
    else f(SortedRec{(const Rec*)sorted});
}
template <class F>
static inline void dispatch_keys(bool wide, const void* sorted, const uint32_t* svals, F&& f) {
    if (wide) f(KeysSplit64{(const uint64_t*)sorted, svals});
    else f(KeysRec{(const Rec*)sorted});
}

// row pitch, in partition passes (pairs of tiles), of the range partition's [digit][pass] count /
// offset table
uint32_t part_pass_pitch(uint32_t n) { return (((sort_tiles(n) + 1u) >> 1) + 3u) & ~3u; }

void launch_prepare(hipStream_t st, const uint32_t* starts, const uint32_t* ends, uint32_t n,
                    const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs,
                    const uint64_t* keep_mask, uint32_t* gstart, uint32_t* cstart,
                    uint32_t* stats, uint32_t part_shift, uint32_t* part_hist,
                    uint32_t* digit0_hist, uint32_t* global_digit_hist, unsigned long long* zero_mask,
                    uint32_t ell_reg, uint32_t* exc, uint32_t exc_cap, uint32_t* exc_cnt, uint32_t tiles_per_block) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    if (exc == nullptr) ell_reg = 0;
    uint32_t g = tiles_per_block != 0u ? (tiles_per_block > 8u ? 8u : tiles_per_block) : tiles_per_block_for(n_tiles);
    // the partition table has one entry per pass (a pair of tiles) and rows padded to part_pass_pitch(n):
    // a workgroup takes whole passes, and the workgroups cover the padding too (empty tiles: zero counts)
    if (part_hist) g = (g + 1u) & ~1u;
    const uint32_t covered = part_hist ? 2u * part_pass_pitch(n) : n_tiles;
    hipLaunchKernelGGL(k_prepare, dim3((covered + g - 1) / g), dim3(256), 0, st, starts, ends, n,
                       d_roff, d_poff, n_contigs, keep_mask, gstart, cstart, stats, n_tiles, g,
                       part_shift, part_hist, part_pass_pitch(n), digit0_hist, global_digit_hist, zero_mask,
                       ell_reg, exc, exc_cap, exc_cnt);
    if (ell_reg != 0u)  // stats[4] = exceptions listed
        hipLaunchKernelGGL(k_nu_count_groups, dim3(32), dim3(256), 0, st, exc_cnt, n_tiles * 4u, stats);
}
uint32_t prepare_exc_slots(uint32_t n) { return sort_tiles(n) * 4u * 128u + kNuOverflow; }  // the list's slots on this form: 128 per wave and tile, and the overflow region

void launch_general_keys(hipStream_t st, bool wide, const uint32_t* gstart, const uint32_t* starts,
                         const uint32_t* ends, uint32_t n, uint32_t span_bits, uint32_t max_span,
                         const uint64_t* keep_mask, void* keys, uint32_t* ecnt, uint32_t ecnt_len) {
    // small genomes (the end counts fit a workgroup's LDS) with many reads per position: count in LDS
    constexpr uint32_t kLdsBins = 36u * 1024;
    if (ecnt != nullptr && ecnt_len != 0 && ecnt_len <= kLdsBins && n >= 16u * ecnt_len) {
        const size_t lds = (size_t)ecnt_len * sizeof(uint32_t);
        const uint32_t grid = 256;
        if (wide) {
            (void)hipFuncSetAttribute((const void*)k_general_keys_lds<uint64_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_general_keys_lds<uint64_t>, dim3(grid), dim3(1024), lds, st, gstart, starts, ends, n,
                               span_bits, max_span, keep_mask, (uint64_t*)keys, ecnt, ecnt_len);
        } else {
            (void)hipFuncSetAttribute((const void*)k_general_keys_lds<uint32_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(k_general_keys_lds<uint32_t>, dim3(grid), dim3(1024), lds, st, gstart, starts, ends, n,
                               span_bits, max_span, keep_mask, (uint32_t*)keys, ecnt, ecnt_len);
        }
        return;
    }
    if (wide)
        hipLaunchKernelGGL(k_general_keys<uint64_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, gstart,
                           starts, ends, n, span_bits, max_span, keep_mask, (uint64_t*)keys, ecnt);
    else
        hipLaunchKernelGGL(k_general_keys<uint32_t>, dim3(grid_for(n, 256)), dim3(256), 0, st, gstart,
                           starts, ends, n, span_bits, max_span, keep_mask, (uint32_t*)keys, ecnt);
}

uint32_t scan_spine_entries(uint32_t n) { return (n + kScanTile - 1) / kScanTile + 1; }

void launch_exclusive_scan(hipStream_t st, const uint32_t* in, uint32_t n, uint32_t* out,
                           uint32_t* spine, bool write_total) {
    const uint32_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if (n_tiles == 0) return;
    hipLaunchKernelGGL(k_scan_tile_sums, dim3(n_tiles), dim3(kScanThreads), 0, st, in, n, spine);
    hipLaunchKernelGGL(k_scan_spine, dim3(1), dim3(kScanThreads), 0, st, spine, n_tiles);
    hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(kScanThreads), 0, st, in, n, spine, out,
                       write_total ? 1 : 0);
}

void launch_radix_hist(hipStream_t st, bool wide, const void* keys_in, uint32_t n, uint32_t shift,
                       uint32_t* hist) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    if (wide)
        hipLaunchKernelGGL(k_radix_hist<uint64_t>, dim3(n_tiles), dim3(kSortThreads), 0, st,
                           (const uint64_t*)keys_in, n, shift, n_tiles, hist);
    else
        hipLaunchKernelGGL(k_radix_hist<uint32_t>, dim3(n_tiles), dim3(kSortThreads), 0, st,
                           (const uint32_t*)keys_in, n, shift, n_tiles, hist);
}

void launch_radix_scatter(hipStream_t st, bool wide, const void* keys_in, const uint32_t* vals_in,
                          uint32_t n, uint32_t shift, const uint32_t* offs, void* keys_out,
                          uint32_t* vals_out) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    if (wide)
        hipLaunchKernelGGL(k_radix_scatter<uint64_t>, dim3(n_tiles), dim3(kSortThreads), 0, st,
                           (const uint64_t*)keys_in, vals_in, n, shift, n_tiles, offs,
                           (uint64_t*)keys_out, vals_out);
    else
        hipLaunchKernelGGL(k_radix_scatter<uint32_t>, dim3(n_tiles), dim3(kSortThreads), 0, st,
                           (const uint32_t*)keys_in, vals_in, n, shift, n_tiles, offs,
                           (uint32_t*)keys_out, vals_out);
}

// One table of seg_words ([windows' cuts | tier 0 | tier 1 | tier 2], sweep_plan.h) from the windows' cuts: the exact one
// (tier 0, burn 0), or a tier with a boundary `burn` positions of run-in wide every `stride` windows without a cut
static const uint32_t* launch_build_segments(const SweepAxis& ax, uint32_t n_windows, uint32_t* seg_words, uint32_t tier,
                                             uint32_t burn, uint32_t stride, uint32_t* n_speculative) {
    uint32_t* seg = seg_words + sweep_segment_table_offset(ax.n_contigs, n_windows, tier);
    const uint32_t win = (ax.ltot + n_windows - 1) / n_windows;
    hipLaunchKernelGGL(k_build_segments, dim3(1), dim3(kSegThreads), 0, ax.st, seg_words, n_windows, ax.poff, ax.n_contigs,
                       ax.ltot, win, burn, stride, seg, n_speculative);
    return seg;
}
// the axis under the exact table its windows' cuts give
static SweepAxis with_exact_segments(const SweepAxis& ax, uint32_t n_windows, uint32_t* seg_words) {
    SweepAxis cut = ax.with_table(launch_build_segments(ax, n_windows, seg_words, 0, 0u, 1u, nullptr));
    cut.n_seg_max = ax.n_contigs + n_windows;
    return cut;
}
SweepAxis launch_sweep_segments(const SweepAxis& ax, const uint32_t* eoff, uint32_t ell, uint32_t M, uint32_t n_windows,
                                uint32_t* seg_words, const uint32_t* other_cov) {
    const uint32_t win = (ax.ltot + n_windows - 1) / n_windows;
    hipLaunchKernelGGL(k_find_cuts, dim3(n_windows), dim3(256), 0, ax.st, ax.boff, eoff, ax.poff, ax.n_contigs, ax.ltot, ell,
                       M, win, seg_words, other_cov);
    return with_exact_segments(ax, n_windows, seg_words);
}
const uint32_t* launch_sweep_segments_speculative(const SweepAxis& ax, uint32_t n_windows, uint32_t burn,
                                                  uint32_t* seg_words, uint32_t* n_speculative, uint32_t run_ins_apart,
                                                  uint32_t tier) {
    // candidates this many run-ins apart at least (>= 2)
    const uint32_t win = (ax.ltot + n_windows - 1) / n_windows;
    const uint32_t stride = (uint32_t)(((uint64_t)run_ins_apart * burn + win - 1) / win);
    return launch_build_segments(ax, n_windows, seg_words, tier, burn, stride < 1 ? 1u : stride, n_speculative);
}
void launch_spec_verify_merge_mixed(const SweepAxis& ax, uint32_t max_span, uint32_t* out_even, const uint32_t* out_odd,
                                    const uint32_t* snap, uint32_t* mismatches, const uint32_t* redo_in,
                                    uint32_t* redo_out) {
    const uint32_t n_cand = ax.n_seg_max;
    hipLaunchKernelGGL(k_spec_verify_mixed, dim3(n_cand), dim3(256), 0, ax.st, ax.seg, n_cand, max_span, out_even, out_odd,
                       snap, kSpecSnapWords, mismatches, redo_in, redo_out);
    hipLaunchKernelGGL(k_spec_merge_mixed, dim3(n_cand, 32), dim3(256), 0, ax.st, ax.seg, n_cand, max_span, out_even,
                       out_odd, redo_in);
}
void launch_spec_verify(const SweepAxis& ax, uint32_t ell, const uint32_t* owned, const uint32_t* run_in,
                        uint32_t* mismatches, const uint32_t* redo_in, uint32_t* redo_out, const uint32_t* own_marks) {
    hipLaunchKernelGGL(k_spec_verify, dim3(ax.n_seg_max), dim3(256), 0, ax.st, ax.seg, ax.n_seg_max, ell, owned, run_in,
                       mismatches, redo_in, redo_out, own_marks);
}

// the E of the one-span kernels: 64-bit words a span's positions take
static inline int span_words(uint32_t ell) { return (int)((ell + 63) / 64); }

bool launch_sweep_uniform_mw(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats) {
    return dispatch_int<1, 2, 3, 4>(span_words(ell), [&](auto e) {  // (wider spans: the single-wave kernel)
        constexpr int E = decltype(e)::value;
        const size_t lds = MwLayout<E>::kBytes;
        (void)hipFuncSetAttribute((const void*)k_sweep_uniform_mw<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_sweep_uniform_mw<E>, dim3(ax.workgroups()), dim3(448), lds, ax.st, ax.boff, ax.poff, ell, M,
                           ax.ltot, selend, iter_stats, ax.seg);
    });
}

bool launch_sweep_uniform_gen(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats,
                              uint32_t* selend_run_in, const uint32_t* redo_in, const int32_t* nadj,
                              const uint32_t* own_marks) {
    return dispatch_int<1, 2, 3, 4>(span_words(ell), [&](auto e) {
        dispatch_bool(nadj != nullptr, [&](auto adj) {
            constexpr int E = decltype(e)::value;
            auto* kernel = k_sweep_uniform_gen<E, decltype(adj)::value>;
            const size_t lds = MgLayout<E>::kBytes;
            (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kernel, dim3(ax.workgroups()), dim3(448), lds, ax.st, ax.boff, ax.poff, ell, M, ax.ltot,
                               selend, iter_stats, ax.seg, selend_run_in, redo_in, ax.n_seg_max, nadj, own_marks);
        });
    });
}

// the three launches of the event-driven form, separately (the host brackets each with events)
bool launch_sweep_ev_pack(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* pk, const int32_t* nadj,
                          const uint32_t* from) {
    if (!sweep_uniform_ev_supported(ell, M)) return false;
    const uint32_t n_wg = ax.workgroups(), pieces = sweep_ev_pieces(ax.ltot, ell, n_wg);
    return dispatch_int<1, 2, 3, 4>(span_words(ell), [&](auto e) {
        hipLaunchKernelGGL(k_sweep_pack<decltype(e)::value>, dim3((pieces + 3) / 4), dim3(256), 0, ax.st, ax.boff, ax.poff,
                           n_wg, ell, M, ax.ltot, ax.seg, pieces, pk, nadj, from);
    });
}
bool launch_sweep_ev_chain(const SweepAxis& ax, uint32_t ell, uint32_t M, const uint32_t* pk, uint32_t* sev,
                           uint32_t* lastns, uint32_t* iter_stats, const int32_t* nadj, uint32_t* ckpt,
                           const uint32_t* restart) {
    if (!sweep_uniform_ev_supported(ell, M)) return false;
    const size_t lds = (size_t)kEvSlots * 1024;
    return dispatch_int<1, 2, 3, 4>(span_words(ell), [&](auto e) {
        constexpr int E = decltype(e)::value;
        (void)hipFuncSetAttribute((const void*)k_sweep_uniform_ev<E>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_sweep_uniform_ev<E>, dim3(ax.workgroups()), dim3(128), lds, ax.st, ax.boff, ax.poff,
                           ax.n_contigs, ell, M, ax.ltot, pk, sev, lastns, iter_stats, ax.seg, nadj, ckpt, restart);
    });
}
bool launch_sweep_ev_expand(const SweepAxis& ax, uint32_t ell, uint32_t M, const uint32_t* sev, const uint32_t* lastns,
                            uint32_t* selend, const uint32_t* from) {
    if (!sweep_uniform_ev_supported(ell, M)) return false;
    const uint32_t n_wg = ax.workgroups(), pieces = sweep_ev_pieces(ax.ltot, ell, n_wg);
    return dispatch_int<1, 2, 3, 4>(span_words(ell), [&](auto e) {
        hipLaunchKernelGGL(k_sweep_expand<decltype(e)::value>, dim3(pieces), dim3(256), 0, ax.st, ax.boff, ax.poff, n_wg, ell,
                           ax.ltot, ax.seg, pieces, sev, lastns, selend, from);
    });
}

bool launch_sweep_uniform(const SweepAxis& ax, uint32_t ell, uint32_t M, uint32_t* selend, uint32_t* iter_stats) {
    return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(span_words(ell), [&](auto e) {
        hipLaunchKernelGGL(k_sweep_uniform<decltype(e)::value>, dim3(ax.workgroups()), dim3(64), 0, ax.st, ax.boff, ax.poff,
                           ell, M, ax.ltot, selend, iter_stats, ax.seg);
    });
}

void launch_sweep_general(const SweepAxis& ax, const SortedSpans& reads, SweepDemand demand, uint32_t M, uint32_t* selend,
                          uint32_t ring_size, uint32_t* g_rings) {
    // rings in LDS while they fit (two of ring_size words); beyond that in g_rings (2 * ring_size words
    // per workgroup)
    const size_t lds = g_rings ? 0 : 2 * (size_t)ring_size * sizeof(uint32_t);
    if (demand.capped) M = 0;
    auto launch = [&](auto keys, auto gring, auto capped) {
        auto* kernel = k_sweep_general<decltype(keys), decltype(gring)::value, decltype(capped)::value>;
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, dim3(ax.workgroups()), dim3(64), lds, ax.st, ax.boff, demand.per_position, keys, ax.poff,
                           reads.span_bits, reads.max_span, M, selend, ring_size, ax.seg, g_rings);
    };
    dispatch_sorted(reads.wide, reads.sorted, [&](auto keys) {
        dispatch_bool(g_rings != nullptr, [&](auto gring) {
            dispatch_bool(demand.capped, [&](auto capped) { launch(keys, gring, capped); });
        });
    });
}

void launch_group_heads(hipStream_t st, bool wide, const void* sorted, uint32_t n,
                        uint32_t* next_head) {
    dispatch_sorted(wide, sorted, [&](auto keys) {
        hipLaunchKernelGGL(k_group_heads<decltype(keys)>, dim3(grid_for((uint64_t)n + 1, 256)), dim3(256), 0, st, keys, n,
                           next_head);
    });
}

void launch_sweep_general_cached(const SweepAxis& ax, const SortedSpans& reads, const uint32_t* eoff, uint32_t M,
                                 uint32_t* selend, uint32_t ring) {
    const size_t lds = (size_t)GenSlots::kWords * ring * sizeof(uint32_t);
    dispatch_sorted(reads.wide, reads.sorted, [&](auto keys) {
        auto* kernel = k_sweep_general_cached<decltype(keys)>;
        (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, dim3(ax.workgroups()), dim3(64), lds, ax.st, ax.boff, eoff, keys, reads.next_head, ax.poff,
                           reads.span_bits, reads.max_span, M, selend, ring, ax.seg);
    });
}

// register-resident event sweep: buckets per lane B = ceil((max_span + 64) / 64), up to 8
bool launch_sweep_general_reg(const SweepAxis& ax, const SortedSpans& reads, SweepDemand demand, uint32_t M,
                              uint32_t* selend, uint32_t* selend_odd, const uint32_t* redo_in, uint32_t* snap) {
    const uint32_t n_wg = ax.workgroups();
    const uint32_t b = (reads.max_span + 64 + 63) / 64;
    const int buckets = b <= 2 ? 2 : b == 5 ? 6 : b == 7 ? 8 : (int)b;  // instantiated for 2, 3, 4, 6 and 8
    // loader waves per walker: few workgroups (contigs) -> many loaders, so the walker never waits for an
    // entering chunk's three trips to memory; many workgroups (stretches) fill the chip by themselves
    // and extra waves only get in the walkers' way
    const int loaders = n_wg <= 64 ? 4 : 1;  // (769 stretches, cfg3-like mix: 1 loader 2.52 ms, 8 loaders 4.92 ms; one contig: 1.19 vs 1.09 ms)
    if (demand.capped) M = 0;
    auto launch = [&](auto keys, auto bb, auto kk, auto capped, auto... stamps) {
        constexpr int B = decltype(bb)::value, K = decltype(kk)::value;
        hipLaunchKernelGGL((k_sweep_general_reg<decltype(keys), B, K, decltype(capped)::value>), dim3(n_wg),
                           dim3(64 * (1 + K)), 0, ax.st, ax.boff, demand.per_position, keys, reads.next_head, ax.poff,
                           reads.span_bits, reads.max_span, M, selend, ax.seg, selend_odd, redo_in, ax.n_seg_max, snap,
                           stamps...);
    };
    bool taken = false;
    dispatch_sorted(reads.wide, reads.sorted, [&](auto keys) {
        taken = dispatch_int<2, 3, 4, 6, 8>(buckets, [&](auto bb) {
            dispatch_int<1, 4>(loaders, [&](auto kk) {
                dispatch_bool(demand.capped, [&](auto capped) {
#ifdef QMCP_GEN_STAMP
                    launch(keys, bb, kk, capped, (unsigned long long*)nullptr);  // (lab builds: the kernel's stamps)
#else
                    launch(keys, bb, kk, capped);
#endif
                });
            });
        });
    });
    return taken;
}

void launch_mark(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals, uint32_t ltot,
                 const uint32_t* boff, const uint32_t* selend, uint64_t* mask,
                 unsigned long long* n_kept) {
    dispatch_keys(wide, sorted, svals, [&](auto keys) {
        hipLaunchKernelGGL(k_mark<decltype(keys)>, dim3(grid_for(ltot, 256)), dim3(256), 0, st, keys, ltot, boff, selend,
                           (uint32_t*)mask, n_kept);
    });
}

void launch_bucket_heads(hipStream_t st, bool wide, const void* sorted, const uint32_t* svals,
                         uint32_t n, uint32_t span_bits, uint32_t ltot, uint32_t* boff) {
    dispatch_keys(wide, sorted, svals, [&](auto keys) {
        hipLaunchKernelGGL(k_bucket_heads<decltype(keys)>, dim3(grid_for(n, 256)), dim3(256), 0, st, keys, n, span_bits, ltot,
                           boff);
    });
}

void launch_reverse_min_scan(hipStream_t st, uint32_t* data, uint32_t n, uint32_t* spine) {
    const uint32_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if (n_tiles == 0) return;
    hipLaunchKernelGGL(k_rmin_tile_mins, dim3(n_tiles), dim3(kScanThreads), 0, st, data, n, spine);
    hipLaunchKernelGGL(k_rmin_spine, dim3(1), dim3(kScanThreads), 0, st, spine, n_tiles);
    hipLaunchKernelGGL(k_rmin_tiles, dim3(n_tiles), dim3(kScanThreads), 0, st, data, n, spine);
}

void launch_radix_hist_rec(hipStream_t st, bool first, const uint32_t* keys, const void* recs,
                           uint32_t n, uint32_t shift, uint32_t* hist) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    const uint32_t g = tiles_per_block_for(n_tiles);
    const uint32_t grid = (n_tiles + g - 1) / g;
    if (first)
        hipLaunchKernelGGL(k_radix_hist_rec<true>, dim3(grid), dim3(kSortThreads), 0, st, keys,
                           (const Rec*)recs, n, shift, n_tiles, g, hist);
    else
        hipLaunchKernelGGL(k_radix_hist_rec<false>, dim3(grid), dim3(kSortThreads), 0, st, keys,
                           (const Rec*)recs, n, shift, n_tiles, g, hist);
}

void launch_radix_scatter_rec(hipStream_t st, bool first, const uint32_t* keys, const void* recs_in,
                              uint32_t n, uint32_t shift, const uint32_t* offs, void* recs_out) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    const uint32_t g = tiles_per_block_for(n_tiles);
    const uint32_t grid = (n_tiles + g - 1) / g;
    if (first)
        hipLaunchKernelGGL((k_radix_scatter_rec<true, false>), dim3(grid), dim3(kSortThreads), 0, st,
                           keys, (const Rec*)recs_in, n, shift, n_tiles, g, offs, recs_out);
    else
        hipLaunchKernelGGL((k_radix_scatter_rec<false, false>), dim3(grid), dim3(kSortThreads), 0, st,
                           keys, (const Rec*)recs_in, n, shift, n_tiles, g, offs, recs_out);
}


// range-ranked uniform path: geometry, partition table, counts, rank + mark
static constexpr uint32_t kTwoLevelRangeShift = 15;
uint32_t range_shift_for(uint32_t ltot) {
    // smallest shift whose ranges (positions 0..ltot inclusive) fit the 256 digits of one pass; beyond
    // 256 ranges of 32 Ki positions a second partition level supplies eight more digit bits
    uint32_t shift = 0;
    while (shift < kMaxRangeShift && (ltot >> shift) >= 256u) ++shift;
    if ((ltot >> kMaxRangeShift) >= 256u) {
        // two levels: any shift with <= 65 536 ranges (and so <= 256 super-ranges) will do
        uint32_t lowest = 0;
        while ((ltot >> lowest) >= 65536u) ++lowest;
        const uint32_t want = kTwoLevelRangeShift;
        shift = want < lowest ? lowest : (want > kMaxRangeShift ? kMaxRangeShift : want);
    }
    return shift;
}
bool range_path_two_level(uint32_t ltot) { return (ltot >> kMaxRangeShift) >= 256u; }
bool range_path_supported(uint32_t ltot) { return (ltot >> kMaxRangeShift) < 65536u; }  // always, for 32-bit positions < 2^31

template <int MODE, bool OUT_REC>
static void launch_partition_t(hipStream_t st, dim3 grid, const uint32_t* keys, const Rec* recs_in,
                               SegTables seg, const uint64_t* d_roff, const uint64_t* d_poff,
                               uint32_t n_contigs, uint32_t n, uint32_t shift, uint32_t n_tiles,
                               const uint32_t* offs, uint16_t* k16, uint32_t* idx, Rec* out_rec,
                               uint32_t* range_start, uint32_t* max_load, const uint32_t* ends = nullptr,
                               uint32_t ell_reg = 0) {
    (void)hipFuncSetAttribute((const void*)k_range_partition<MODE, OUT_REC>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPartLds);
    hipLaunchKernelGGL((k_range_partition<MODE, OUT_REC>), grid, dim3(kPartThreads), kPartLds, st, keys,
                       recs_in, seg, d_roff, d_poff, n_contigs, n, shift, n_tiles, offs, k16, idx, out_rec,
                       range_start, max_load, ends, ends != nullptr ? ell_reg : 0u);
}

void launch_range_partition(hipStream_t st, const uint32_t* gstart_or_null, const uint32_t* starts,
                            const uint64_t* d_roff, const uint64_t* d_poff, uint32_t n_contigs,
                            uint32_t n, uint32_t shift, const uint32_t* offs, uint16_t* keys16_out,
                            uint32_t* idx_out, uint32_t* range_start, uint32_t* max_load, const uint32_t* ends,
                            uint32_t ell_reg) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    const dim3 grid((n_tiles + kPartTiles - 1) / kPartTiles);
    const SegTables none{nullptr, nullptr, nullptr};
    if (gstart_or_null)
        launch_partition_t<0, false>(st, grid, gstart_or_null, nullptr, none, d_roff, d_poff, n_contigs, n, shift,
                                     part_pass_pitch(n), offs, keys16_out, idx_out, nullptr, range_start, max_load);
    else
        launch_partition_t<1, false>(st, grid, starts, nullptr, none, d_roff, d_poff, n_contigs, n, shift,
                                     part_pass_pitch(n), offs, keys16_out, idx_out, nullptr, range_start, max_load, ends, ell_reg);
}

// Two-level route.  Level 1: stable partition of the reads into <= 256 super-ranges of 2^(shift+8)
// positions, as {global start, index} records; its first workgroup publishes super_start[257].
void launch_partition_level1(hipStream_t st, const uint32_t* starts, const uint64_t* d_roff,
                             const uint64_t* d_poff, uint32_t n_contigs, uint32_t n, uint32_t shift_hi,
                             const uint32_t* offs, void* recs_out, uint32_t* super_start,
                             uint32_t* max_super_load, const uint32_t* ends, uint32_t ell_reg) {
    const uint32_t n_tiles = sort_tiles(n);
    if (n_tiles == 0) return;
    const dim3 grid((n_tiles + kPartTiles - 1) / kPartTiles);
    const SegTables none{nullptr, nullptr, nullptr};
    launch_partition_t<1, true>(st, grid, starts, nullptr, none, d_roff, d_poff, n_contigs, n, shift_hi,
                                part_pass_pitch(n), offs, nullptr, nullptr, (Rec*)recs_out, super_start,
                                max_super_load, ends, ell_reg);
}
// Level 2: every super-range is partitioned on its own into its (<= 256) final ranges.
// tables: [0,257) super_start  [257,514) tile_base  [514,771) pass_base (written here)
uint32_t seg_tile_bound(uint32_t n) { return sort_tiles(n) + 256; }  // upper bound of the tile count
void launch_partition_level2(hipStream_t st, const void* recs_in, uint32_t n, uint32_t shift,
                             uint32_t* tables, uint32_t* hist, uint32_t* spine, uint16_t* keys16_out,
                             uint32_t* idx_out, uint32_t* range_start, uint32_t* max_load) {
    const SegTables seg{tables, tables + 257, tables + 514};
    const uint32_t t_bound = seg_tile_bound(n);
    hipLaunchKernelGGL(k_seg_tables, dim3(1), dim3(256), 0, st, tables, tables + 257, tables + 514, max_load);
    (void)hipMemsetAsync(hist, 0, (size_t)256 * t_bound * sizeof(uint32_t), st);
    hipLaunchKernelGGL(k_seg_hist, dim3(t_bound), dim3(kSortThreads), 0, st, (const Rec*)recs_in, seg, shift, hist);
    launch_exclusive_scan(st, hist, 256u * t_bound, hist, spine, false);
    launch_partition_t<2, false>(st, dim3((t_bound + kPartTiles - 1) / kPartTiles + 256), nullptr,
                                 (const Rec*)recs_in, seg, nullptr, nullptr, 0, n, shift, 0, hist, keys16_out,
                                 idx_out, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(k_seg_range_table, dim3(256), dim3(256), 0, st, hist, seg, n, range_start, max_load);
}

void launch_gstart(hipStream_t st, const uint32_t* starts, uint32_t n, const uint64_t* d_roff,
                   const uint64_t* d_poff, uint32_t n_contigs, uint32_t* gstart) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_gstart, dim3(grid_for(n, 256)), dim3(256), 0, st, starts, n, d_roff, d_poff,
                       n_contigs, gstart);
}
void launch_fill_ends(hipStream_t st, const uint32_t* starts, uint32_t n, uint32_t span_minus_1, uint32_t* ends) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_fill_ends, dim3(grid_for(n, 256 * 4)), dim3(256), 0, st, starts, n, span_minus_1, ends);
}
void launch_range_offsets(hipStream_t st, const uint16_t* keys16, const uint32_t* range_start,
                          uint32_t shift, uint32_t ltot, uint32_t* boff, uint32_t* empty_positions) {
    const uint32_t n_ranges = (ltot >> shift) + 1;  // covers positions 0..ltot
    const size_t lds = (((size_t)1 << shift) + ((size_t)1 << shift) / 32 + 1) * sizeof(uint32_t);
    (void)hipFuncSetAttribute((const void*)k_range_offsets, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(k_range_offsets, dim3(n_ranges), dim3(1024), lds, st, keys16, range_start, shift,
                       ltot, boff, empty_positions);
}
bool rank_scratch_by_records(uint32_t shift, uint32_t ltot, uint32_t n) {
    return (size_t)n < (size_t)((ltot >> shift) + 1) * ((size_t)1 << shift);
}
size_t rank_scratch_bytes(uint32_t shift, uint32_t ltot, uint32_t n) {
    const size_t by_pos = (size_t)((ltot >> shift) + 1) * ((size_t)1 << shift);
    return (by_pos < (size_t)n ? by_pos : (size_t)n) * sizeof(uint2) + 64;
}
void launch_rank_mark(hipStream_t st, const uint16_t* keys16, const uint32_t* idx,
                      const uint32_t* range_start, uint32_t shift, uint32_t ltot, const uint32_t* boff,
                      const uint32_t* selend, unsigned long long* mask, unsigned long long* kept_total,
                      void* scratch, bool scratch_by_records) {
    const uint32_t n_ranges = (ltot >> shift) + 1;
    const size_t lds = (((size_t)1 << shift) + 1) * sizeof(uint32_t);
    (void)hipFuncSetAttribute((const void*)k_rank_mark, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds);
    hipLaunchKernelGGL(k_rank_mark, dim3(n_ranges), dim3(1024), lds, st, keys16, idx, range_start,
                       shift, ltot, boff, selend, mask, kept_total, (uint2*)scratch, scratch_by_records ? 1 : 0);
}

void launch_coverage(hipStream_t st, const uint32_t* boff, const uint32_t* eoff, uint32_t ltot,
                     uint32_t* cov) {
    hipLaunchKernelGGL(k_coverage, dim3(grid_for(ltot, 256)), dim3(256), 0, st, boff, eoff, ltot, cov);
}

void launch_b_and_demand(hipStream_t st, const uint32_t* cov, uint32_t n, uint32_t M, int32_t* b, int32_t* d) {
    const uint32_t grid = (n + 1 + 255) / 256;
    hipLaunchKernelGGL(k_b_and_demand, dim3(grid < 1024 ? grid : 1024), dim3(256), 0, st, cov, n, M, b, d);
}
void launch_complete_pairs(hipStream_t st, uint64_t* mask, uint32_t n_words, uint64_t n_reads) {
    hipLaunchKernelGGL(k_complete_pairs, dim3(grid_for(n_words, 256)), dim3(256), 0, st, mask,
                       n_words, n_reads);
}

void launch_word_popcounts(hipStream_t st, const uint64_t* words, uint32_t n_words, uint32_t* counts) {
    hipLaunchKernelGGL(k_word_popcounts, dim3(grid_for(n_words, 256)), dim3(256), 0, st, words, n_words,
                       counts);
}
void launch_mask_to_indices(hipStream_t st, const uint64_t* mask, uint32_t n_words, const uint32_t* word_base,
                            unsigned long long* out) {
    hipLaunchKernelGGL(k_mask_to_indices, dim3(grid_for(n_words, 256)), dim3(256), 0, st, mask, n_words, word_base, out);
}
void launch_compact_pairs(hipStream_t st, const uint32_t* starts, const uint32_t* ends,
                          const uint64_t* pair_keep, const uint32_t* word_base, uint64_t n_pairs,
                          uint32_t* starts_c, uint32_t* ends_c, uint32_t* orig_pair) {
    hipLaunchKernelGGL(k_compact_pairs, dim3(grid_for(n_pairs, 256)), dim3(256), 0, st, starts, ends,
                       pair_keep, word_base, n_pairs, starts_c, ends_c, orig_pair);
}
void launch_expand_mask(hipStream_t st, const uint64_t* mask_c, const uint32_t* orig_pair,
                        uint32_t n_reads_c, uint64_t* mask) {
    hipLaunchKernelGGL(k_expand_mask, dim3(grid_for(n_reads_c, 256)), dim3(256), 0, st, mask_c,
                       orig_pair, n_reads_c, (uint32_t*)mask);
}

void launch_amplicon_filter(hipStream_t st, const uint32_t* starts, const uint32_t* ends,
                            const uint32_t* seq_lengths, const uint32_t* qualities,
                            uint64_t n_pairs, const uint32_t* amp_starts, const uint32_t* amp_ends,
                            uint32_t n_amp, uint32_t min_length, uint32_t min_mapq,
                            uint64_t* pair_keep) {
    const uint32_t n_cached = n_amp < 4096u ? n_amp : 4096u;
    const uint64_t n_words = (n_pairs + 63) / 64;
    hipLaunchKernelGGL(k_amplicon_filter, dim3(grid_for(n_words * 64, 256)), dim3(256),
                       2 * n_cached * sizeof(uint32_t), st, starts, ends, seq_lengths, qualities,
                       n_pairs, amp_starts, amp_ends, n_amp, min_length, min_mapq, pair_keep);
}
