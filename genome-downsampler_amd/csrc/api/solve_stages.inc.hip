// solve_stages.inc.hip -- part of qmcp_api.hip (one translation unit).
// The stages the sort-based routes share -- the plain solve's (solve_tail.inc.hip) and the capped solve's
// (profile.inc.hip): each takes plain arguments and queues its launches on the context's stream, in the arena the
// caller has sized.  The timing events between them (EV_*) stay with the routes.

// how a call's reads are keyed for the sort and, once queue_sort has run, which buffers hold them sorted
struct SortedReads {
    uint32_t span_bits = 0;  // bits of the span field behind the position (0: one span, the key is the start position)
    bool wide = false;       // position and span need more than 32 bits: u64 keys with a split index column
    uint32_t passes = 0;     // 8-bit digits of the key
    int k = 0, v = 0;        // keys[k]: {key, index} records, or the u64 keys with their indices in vals[v]
};
SortedReads key_layout(uint32_t ltot, uint32_t min_span, uint32_t max_span) {
    SortedReads s;
    const uint32_t pos_bits = bit_width(ltot - 1) == 0 ? 1u : bit_width(ltot - 1);
    s.span_bits = bit_width(max_span - min_span);
    s.wide = pos_bits + s.span_bits > 32;
    s.passes = (pos_bits + s.span_bits + 7) / 8;
    return s;
}

// keys + end counts + scan: the mixed-span keys from gstart (vals[1]) into vals[0] (wide: keys[0]), the reads per end
// position counted into ecnt and scanned into eoff
int queue_mixed_keys(qmcp_hip_ctx* c, const uint32_t* d_starts, const uint32_t* d_ends, uint32_t n, uint32_t ltot,
                     uint32_t max_span, const SortedReads& s) {
    TRY(ensure(c, c->ecnt, ((size_t)ltot + 1) * sizeof(uint32_t)));
    TRY(ensure(c, c->eoff, ((size_t)ltot + 1) * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->ecnt.p, 0, ((size_t)ltot + 1) * sizeof(uint32_t), c->stream));
    {
        KernelSpan sp(c, "k_general_keys");
        qmcp::launch_general_keys(c->stream, s.wide, c->vals[1].u32(), d_starts, d_ends, n, s.span_bits, max_span, nullptr,
                                  s.wide ? c->keys[0].p : c->vals[0].p, c->ecnt.u32(), ltot + 1);
    }
    HIP_TRY(hipGetLastError());
    return scan_counts(c, c->ecnt, c->eoff, ltot);
}

// sort by key (stable LSD, 8-bit digits): {key, read index} records built from the bare keys key32, keys[0] <-> keys[1];
// or, wide, the u64 keys of keys[0] with a split index column.  Fills s.k and s.v.
int queue_sort(qmcp_hip_ctx* c, const uint32_t* key32, uint32_t n, SortedReads& s, const RadixNames& records,
               const RadixNames& wide) {
    if (!s.wide) return radix_sort_records(c, c->stream, key32, n, s.passes, c->hist.u32(), c->spine.u32(), c->keys, records, &s.k);
    WideBufs wb;
    TRY(radix_sort_wide(c, c->stream, n, s.passes, c->hist.u32(), c->spine.u32(), c->keys, c->vals, wide, &wb));
    s.k = wb.k;
    s.v = wb.v;
    return QMCP_OK;
}

// bucket offsets straight from the sorted keys (no atomics): heads, then a reverse min-scan over the empty positions
int queue_bucket_offsets(qmcp_hip_ctx* c, uint32_t n, uint32_t ltot, const SortedReads& s) {
    HIP_TRY(hipMemsetAsync(c->boff.p, 0xFF, ((size_t)ltot + 1) * sizeof(uint32_t), c->stream));
    {
        KernelSpan sp(c, "k_bucket_heads");
        qmcp::launch_bucket_heads(c->stream, s.wide, c->keys[s.k].p, c->vals[s.v].u32(), n, s.span_bits, ltot, c->boff.u32());
    }
    {
        KernelSpan sp(c, "reverse_min_scan(3 kernels)");
        qmcp::launch_reverse_min_scan(c->stream, c->boff.u32(), ltot + 1, c->spine.u32());
    }
    HIP_TRY(hipGetLastError());
    return QMCP_OK;
}

// run lengths of equal (start, end) groups: heads + reverse min-scan -> next_head[]
int queue_run_lengths(qmcp_hip_ctx* c, uint32_t n, const SortedReads& s) {
    TRY(ensure(c, c->next_head, ((size_t)n + 2) * sizeof(uint32_t)));
    TRY(ensure(c, c->spine, scan_spine_bytes(n + 1, 1)));
    {
        KernelSpan sp(c, "k_group_heads");
        qmcp::launch_group_heads(c->stream, s.wide, c->keys[s.k].p, n, c->next_head.u32());
    }
    KernelSpan sp(c, "reverse_min_scan(3 kernels)");
    qmcp::launch_reverse_min_scan(c->stream, c->next_head.u32(), n + 1, c->spine.u32());
    return QMCP_OK;
}

// the plain event sweep's two rings per workgroup: their size, and -- long reads, whose rings no longer fit LDS -- their
// place in global memory (else null)
struct Rings { uint32_t size = 64; uint32_t* global = nullptr; };
int sweep_rings(qmcp_hip_ctx* c, uint32_t max_span, size_t workgroups, Rings& r) {
    while (r.size <= max_span) r.size <<= 1;
    if (max_span > qmcp::kMaxLdsRingSpan) {
        TRY(ensure(c, c->rings, workgroups * 2 * (size_t)r.size * sizeof(uint32_t)));
        r.global = c->rings.u32();
    }
    return QMCP_OK;
}

// keep mask from the sorted records and the sweep's selected prefixes
void queue_mark(qmcp_hip_ctx* c, uint32_t ltot, const SortedReads& s, uint64_t* d_mask) {
    KernelSpan sp(c, "k_mark");
    qmcp::launch_mark(c->stream, s.wide, c->keys[s.k].p, c->vals[s.v].u32(), ltot, c->boff.u32(), c->selend.u32(), d_mask,
                      c->scalars.as<unsigned long long>());
}

// the end of a solve's queue: EV_MARK and the result scalars on their way to h_scalars
int queue_result_scalars(qmcp_hip_ctx* c) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_MARK], c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_scalars, c->scalars.p, qmcp::words::kHostScalarsRead * sizeof(unsigned long long),
                           hipMemcpyDeviceToHost, c->stream));
    return QMCP_OK;
}

// a sweep without a stretch table runs one chain (one wave) per non-empty contig
uint32_t whole_contig_chains(const uint32_t* lengths, uint32_t n_contigs) {
    return (uint32_t)std::count_if(lengths, lengths + n_contigs, [](uint32_t len) { return len != 0; });
}

void phase_times(qmcp_hip_ctx* c, qmcp_hip_stats& st) {
    st.ms_prepare = elapsed(c->ev[EV_BEGIN], c->ev[EV_PREP]);
    st.ms_scan = elapsed(c->ev[EV_PREP], c->ev[EV_SCAN]);
    st.ms_sort = elapsed(c->ev[EV_SCAN], c->ev[EV_SORT]);
    st.ms_sweep = elapsed(c->ev[EV_SORT], c->ev[EV_SWEEP]);
    st.ms_mark = elapsed(c->ev[EV_SWEEP], c->ev[EV_MARK]);
    st.ms_total = elapsed(c->ev[EV_BEGIN], c->ev[EV_MARK]);
}
