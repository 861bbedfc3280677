"""Test helpers for reads of several references (qmcp_hip_solve_by_contig_*, BamApiConfig::per_reference): the
expected keep mask restated on the oracle, and multi-reference BAM files written by the independent writer in
tests/bam_py.py."""
import struct

import numpy as np

import bam_py

NO_CONTIG = 0xFFFFFFFF


def group_stably(contig_ids, n_contigs):
    """-> (order, contig_read_offsets): the placed reads grouped by contig, input order kept inside each contig
    (unplaced reads left out)"""
    ids = np.asarray(contig_ids, dtype=np.uint32)
    placed = ids != NO_CONTIG
    order = np.flatnonzero(placed)
    order = order[np.argsort(ids[order], kind="stable")]
    counts = np.bincount(ids[order].astype(np.int64), minlength=n_contigs)
    return order, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def scatter_back(grouped_mask, order, n_reads):
    """a mask over the grouped reads -> the same kept reads as a mask in input order"""
    bits = np.unpackbits(np.ascontiguousarray(grouped_mask).view(np.uint8), bitorder="little")[:order.size]
    out = np.zeros(((n_reads + 63) // 64) * 64, dtype=np.uint8)
    out[order[bits.astype(bool)]] = 1
    return np.packbits(out, bitorder="little").view(np.uint64)[:(n_reads + 63) // 64].copy()


def oracle_by_contig(oracle, starts, ends, contig_ids, contig_lengths, M):
    """the canonical selection of each contig on its own reads in input order, as one input-order mask"""
    lengths = np.atleast_1d(np.asarray(contig_lengths, dtype=np.uint32))
    order, offs = group_stably(contig_ids, lengths.size)
    s, e = np.asarray(starts, dtype=np.uint32), np.asarray(ends, dtype=np.uint32)
    gmask = oracle.solve(s[order], e[order], lengths, M, contig_read_offsets=offs)
    return scatter_back(gmask, order, s.size)


def random_by_contig(rng, n_contigs, max_reads_per_contig=3000, unplaced=0.03):
    """reads of n_contigs contigs (some empty, mixed spans, depth a few times M for M ~ 20), shuffled, with a few
    unplaced reads between them -> (starts, ends, contig_ids, lengths)"""
    lengths = rng.integers(200, 20_000, size=n_contigs).astype(np.uint32)
    counts = rng.integers(0, max_reads_per_contig + 1, size=n_contigs)
    counts[rng.random(n_contigs) < 0.15] = 0
    ss, ee, ii = [], [], []
    for c in range(n_contigs):
        L = int(lengths[c])
        span = rng.integers(1, min(300, L) + 1, size=counts[c])
        s = (rng.random(counts[c]) * (L - span + 1)).astype(np.int64)
        ss.append(s)
        ee.append(s + span - 1)
        ii.append(np.full(counts[c], c, dtype=np.int64))
    s, e, ids = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (ss, ee, ii))
    n_un = int(unplaced * s.size)
    s = np.concatenate([s, rng.integers(0, 1 << 31, size=n_un)])   # (coordinates of unplaced reads do not matter)
    e = np.concatenate([e, rng.integers(0, 1 << 31, size=n_un)])
    ids = np.concatenate([ids, np.full(n_un, NO_CONTIG, dtype=np.int64)])
    perm = rng.permutation(s.size)
    return (s[perm].astype(np.uint32), e[perm].astype(np.uint32), ids[perm].astype(np.uint32), lengths)


def write_multi_reference_bam(path, rng, references, n_pairs, other_ref=0.05, unmapped=0.03):
    """pairs on `references` ([(name, length)]) in shuffled file order: both mates mostly on one reference, some mates
    on another, some records unmapped (refID -1, pos -1, no CIGAR) -> the parsed records (bam_py.parse) with
    "ref_id" added"""
    recs = []
    for q in range(n_pairs):
        ref = int(rng.integers(0, len(references)))
        for first in (True, False):
            r = ref if rng.random() >= other_ref else int(rng.integers(0, len(references)))
            flag = 0x41 if first else 0x81
            if rng.random() < unmapped:
                recs.append(bam_py.pack_record(f"p{q}", flag | 0x4, -1, 0, [], 100, ref_id=-1))
                continue
            L = references[r][1]
            match = int(rng.integers(60, 151))
            dele = int(rng.integers(1, 10)) if rng.random() < 0.1 else 0
            cigar = [(match, "M")] + ([(dele, "D"), (20, "M")] if dele else [])
            rlen = match + (dele + 20 if dele else 0)
            pos = int(rng.integers(0, L - rlen))
            recs.append(bam_py.pack_record(f"p{q}", flag, pos, int(rng.integers(0, 61)), cigar, match, ref_id=r))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    bam_py.write_bam(path, references, recs)
    header, parsed, ref_lengths = bam_py.parse(path)
    for r in parsed:
        r["ref_id"] = struct.unpack_from("<i", r["raw"], 4)[0]
    return header, parsed, ref_lengths


def expected_per_reference_reads(parsed):
    """read_bam's pairing on the parsed records (bam_py.pair_like_the_reference) -> the reads in pairing order and
    each one's contig id (NO_CONTIG for refID -1)"""
    reads, filtered = bam_py.pair_like_the_reference(parsed)
    ids = [NO_CONTIG if parsed[r["bam_id"]]["ref_id"] < 0 else parsed[r["bam_id"]]["ref_id"] for r in reads]
    return reads, np.array(ids, dtype=np.uint32), filtered
