// radix_passes.inc.hip -- part of qmcp_api.hip (one translation unit).
// The stable LSD radix sort every sorting entry queues: per 8-bit digit a histogram per tile, its exclusive scan (3
// kernels) and the scatter, ping-ponging two buffers.  Two forms, as the kernels have them: {u32 key, index} records
// built from a bare key column, and u64 keys with a split u32 value column.  Both return WHICH buffers hold the result;
// a caller reads the sorted data through those indices only.
namespace {

// the timing spans of one sort's passes (string literals: they outlive collect_spans).  scan == nullptr: one bracket
// per pass around all three launches, under `hist`
struct RadixNames {
    const char* hist;
    const char* scan = nullptr;
    const char* scatter = nullptr;
};

// records form: pass 0 reads the bare keys key32[n] and writes {key, index} records to rec[0]; later passes ping-pong
// rec[0] <-> rec[1].  *out: the record buffer that holds the sorted records (rec[0] when passes == 0: nothing written)
int radix_sort_records(qmcp_hip_ctx* c, hipStream_t st, const uint32_t* key32, uint32_t n, uint32_t passes, uint32_t* hist,
                       uint32_t* spine, const DevBuf rec[2], const RadixNames& nm, int* out) {
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    const void* recs_in = nullptr;
    int kin = 0;
    for (uint32_t p = 0; p < passes; ++p) {
        const bool first = p == 0;
        const int kout = first ? 0 : (kin ^ 1);
        {
            KernelSpan whole(c, nm.scan ? nullptr : nm.hist);
            {
                KernelSpan sp(c, nm.scan ? nm.hist : nullptr);
                qmcp::launch_radix_hist_rec(st, first, key32, recs_in, n, 8 * p, hist);
            }
            {
                KernelSpan sp(c, nm.scan);
                qmcp::launch_exclusive_scan(st, hist, 256u * n_tiles, hist, spine, false);
            }
            {
                KernelSpan sp(c, nm.scatter);
                qmcp::launch_radix_scatter_rec(st, first, key32, recs_in, n, 8 * p, hist, rec[kout].p);
            }
        }
        HIP_TRY(hipGetLastError());
        kin = kout;
        recs_in = rec[kin].p;
    }
    *out = kin;
    return QMCP_OK;
}

// which buffers hold a wide sort's data: keys[k], and vals[v] (v == -1: no value column yet, a read's value is its index)
struct WideBufs {
    int k = 0;
    int v = -1;
};

// wide form: u64 keys in keys[io.k], sorted by their low 8 * passes bits; the values start as the index (io.v == -1) or
// continue from vals[io.v], what an earlier round of the same sort left.  The key and the value index run independently,
// and the first value column written is vals[0]: vals[1] is gstart in the plain and capped solves, still needed there.
int radix_sort_wide(qmcp_hip_ctx* c, hipStream_t st, uint32_t n, uint32_t passes, uint32_t* hist, uint32_t* spine,
                    const DevBuf keys[2], const DevBuf vals[2], const RadixNames& nm, WideBufs* io) {
    const uint32_t n_tiles = qmcp::sort_tiles(n);
    for (uint32_t p = 0; p < passes; ++p) {
        const int kin = io->k, kout = kin ^ 1, vout = io->v < 0 ? 0 : (io->v ^ 1);
        const uint32_t* vals_in = io->v < 0 ? nullptr : vals[io->v].u32();
        {
            KernelSpan whole(c, nm.scan ? nullptr : nm.hist);
            {
                KernelSpan sp(c, nm.scan ? nm.hist : nullptr);
                qmcp::launch_radix_hist(st, true, keys[kin].p, n, 8 * p, hist);
            }
            {
                KernelSpan sp(c, nm.scan);
                qmcp::launch_exclusive_scan(st, hist, 256u * n_tiles, hist, spine, false);
            }
            {
                KernelSpan sp(c, nm.scatter);
                qmcp::launch_radix_scatter(st, true, keys[kin].p, vals_in, n, 8 * p, hist, keys[kout].p, vals[vout].u32());
            }
        }
        HIP_TRY(hipGetLastError());
        io->k = kout;
        io->v = vout;
    }
    return QMCP_OK;
}

}  // namespace
