"""Test helpers for amplicon panels on several references (BamApiConfig::amplicons_by_reference,
qmcp_hip_filter_solve_by_contig_host): the BED / TSV rules restated in Python, panels written as files, read pairs drawn
from them (as columns or as a multi-reference BAM written by the independent writer in tests/bam_py.py), and the
expected keep mask composed from the oracle."""
import struct

import numpy as np

import bam_py
import multi_reference as mr

NO_CONTIG = mr.NO_CONTIG


# ---------------------------------------------------------------- BED / TSV rules
def restate_amplicons(bed_lines, tsv_pairs, ref_names):
    """the rules of build_reference_amplicon_set on parsed lines [(chrom, start, end, name)] and TSV pairs (None: no
    TSV) -> (offsets, starts, ends); ValueError where the library must refuse"""
    primers = {}
    for chrom, s, e, name in bed_lines:
        primers.setdefault(name, [chrom, int(s), int(e)])   # the first line of a name wins
    ref_of = {}
    for k, n in enumerate(ref_names):
        ref_of.setdefault(n, k)
    for chrom, *_ in bed_lines:
        if chrom not in ref_of:
            raise ValueError(chrom)
    per = [[] for _ in ref_names]
    if tsv_pairs is None:
        by_chrom = {}
        for name in sorted(primers):                          # name order within each chrom
            by_chrom.setdefault(primers[name][0], []).append(primers[name])
        for chrom, v in by_chrom.items():
            for i in range(0, len(v) - 1, 2):
                left, right = v[i], v[i + 1]
                if left[1] > right[1]:
                    left, right = right, left
                per[ref_of[chrom]].append((left[1], right[2]))
    else:
        for a, b in tsv_pairs:
            if a not in primers and b not in primers:
                raise ValueError(f"{a} / {b}")
            chrom = primers[a][0] if a in primers else primers[b][0]
            left = primers.setdefault(a, [chrom, 0, 0])
            right = primers.setdefault(b, [chrom, 0, 0])
            if left[0] != right[0]:
                raise ValueError(f"{a} / {b}")
            if left[1] > right[1]:
                left[:], right[:] = right[:], left[:]         # the swap is written back to the map
            per[ref_of[chrom]].append((left[1], right[2]))
    offs = np.concatenate([[0], np.cumsum([len(v) for v in per])]).astype(np.uint32)
    flat = [a for v in per for a in v]
    return (offs, np.array([a[0] for a in flat], dtype=np.uint32), np.array([a[1] for a in flat], dtype=np.uint32))


def in_one_amplicon(offs, a0, a1, c1, s1, e1, c2, s2, e2):
    """the FILTER's amplicon predicate, brute force: both mates on one contig, inside one of its amplicons"""
    if c1 != c2 or c1 == NO_CONTIG:
        return False
    lo, hi = int(offs[c1]), int(offs[c1 + 1])
    return any(a0[k] <= min(s1, s2) and max(e1, e2) <= a1[k] for k in range(lo, hi))


# ---------------------------------------------------------------- panels and reads
def tiled_panel(references, per_ref, size=400, step=300):
    """per reference (name, length): up to per_ref tiled amplicons [start, end] -> {name: [(start, end)]}"""
    panel = {}
    for name, L in references:
        starts = np.arange(0, max(L - size, 1), step)[:per_ref]
        panel[name] = [(int(s), int(s) + size - 1) for s in starts if s + size - 1 < L]
    return panel


def write_panel_files(panel, bed_path, tsv_path):
    """primers are the 25 bp at each end of an amplicon; one TSV line per amplicon"""
    with open(bed_path, "w") as fb, open(tsv_path, "w") as ft:
        for name, amps in panel.items():
            for k, (lo, hi) in enumerate(amps):
                fb.write(f"{name}\t{lo}\t{lo + 24}\t{name}_amp{k}_LEFT\t1\t+\n")
                fb.write(f"{name}\t{hi - 24}\t{hi}\t{name}_amp{k}_RIGHT\t1\t-\n")
                ft.write(f"{name}_amp{k}_LEFT\t{name}_amp{k}_RIGHT\n")


def panel_csr(panel, ref_names):
    offs, a0, a1 = [0], [], []
    for n in ref_names:
        for lo, hi in panel.get(n, []):
            a0.append(lo)
            a1.append(hi)
        offs.append(len(a0))
    return np.array(offs, np.uint32), np.array(a0, np.uint32), np.array(a1, np.uint32)


def panel_pairs(rng, lengths, offs, a0, a1, n_pairs, read_length=150, straddle=0.10, cross=0.01, unplaced=0.0):
    """pairs drawn from the amplicons of each contig (contigs without amplicons get uniform pairs): mate 1 starts
    within 25 bp of the amplicon start, mate 2 ends within 25 bp of its end; a fraction straddles into the next
    amplicon, a fraction puts mate 2 on another contig, a fraction leaves a mate unplaced ->
    (starts, ends, contig_ids), reads 2q, 2q + 1 of pair q"""
    lengths = np.asarray(lengths, dtype=np.int64)
    offs, a0, a1 = (np.asarray(x, dtype=np.int64) for x in (offs, a0, a1))
    C = lengths.size
    c = rng.integers(0, C, size=n_pairs)
    L = lengths[c]
    n_amp = (offs[1:] - offs[:-1])[c]
    has = n_amp > 0
    # uniform pairs (contigs without amplicons)
    rl_u = np.minimum(read_length, L)
    su = (rng.random((n_pairs, 2)) * (L - rl_u + 1)[:, None]).astype(np.int64)
    s, e = su.copy(), su + rl_u[:, None] - 1
    if a0.size:
        j = offs[c] + (rng.random(n_pairs) * np.maximum(n_amp, 1)).astype(np.int64)
        j = np.where(has, j, 0)
        j2 = j + ((rng.random(n_pairs) < straddle) & (j + 1 < offs[c + 1]))
        rl = np.minimum(read_length, a1[j] - a0[j] + 1)
        s1 = a0[j] + rng.integers(0, 26, size=n_pairs)
        e2 = a1[j2] - rng.integers(0, 26, size=n_pairs)
        s[has, 0], e[has, 0] = s1[has], np.minimum(s1 + rl - 1, L - 1)[has]
        s[has, 1], e[has, 1] = np.maximum(e2 - rl + 1, 0)[has], e2[has]
    ids = np.stack([c, c], axis=1)
    s = np.minimum(s, e)
    other = np.flatnonzero(rng.random(n_pairs) < cross)
    k = rng.integers(0, C, size=other.size)
    rl_o = np.minimum(read_length, lengths[k])
    st = (rng.random(other.size) * (lengths[k] - rl_o + 1)).astype(np.int64)
    ids[other, 1], s[other, 1], e[other, 1] = k, st, st + rl_o - 1
    un = rng.random((n_pairs, 2)) < unplaced
    ids[un] = NO_CONTIG
    s[un] = rng.integers(0, 1 << 31, size=int(un.sum()))    # (coordinates of unplaced reads do not matter)
    e[un] = rng.integers(0, 1 << 31, size=int(un.sum()))
    return s.reshape(-1).astype(np.uint32), e.reshape(-1).astype(np.uint32), ids.reshape(-1).astype(np.uint32)


def oracle_filter_by_contig(oracle, pkg, starts, ends, ids, lengths, offs, a0, a1, M, seq_lengths=None,
                            qualities=None, min_length=0, min_mapq=0, complete_pairs=False):
    """the composed oracle of qmcp_hip_filter_solve_by_contig_host -> (input-order mask, pairs dropped):
    oracle.amplicon_filter per contig on its same-contig pairs (offs None: only the length / MAPQ filters, every pair),
    multi_reference.oracle_by_contig on the survivors, oracle.find_pairs, expansion to input order"""
    n = starts.size
    n_pairs = n // 2
    id1, id2 = ids[0::2], ids[1::2]
    keep = np.zeros(n_pairs, bool)
    if offs is None:
        kp = oracle.amplicon_filter(starts, ends, [0], [0xFFFFFFFF], seq_lengths=seq_lengths, qualities=qualities,
                                    min_length=min_length, min_mapq=min_mapq)
        keep[pkg.mask_to_indices(kp, n_pairs).astype(np.int64)] = True
    else:
        same = (id1 == id2) & (id1 != NO_CONTIG)
        for c in range(len(lengths)):
            lo, hi = int(offs[c]), int(offs[c + 1])
            qs = np.flatnonzero(same & (id1 == c))
            if qs.size == 0 or hi == lo:
                continue
            reads = np.stack([2 * qs, 2 * qs + 1], axis=1).reshape(-1)
            sub = lambda x: None if x is None else np.asarray(x)[reads]
            kp = oracle.amplicon_filter(starts[reads], ends[reads], a0[lo:hi], a1[lo:hi], seq_lengths=sub(seq_lengths),
                                        qualities=sub(qualities), min_length=min_length, min_mapq=min_mapq)
            keep[qs[pkg.mask_to_indices(kp, qs.size).astype(np.int64)]] = True
    sel = np.repeat(keep, 2)
    orig = np.flatnonzero(sel)
    m = mr.oracle_by_contig(oracle, starts[sel], ends[sel], ids[sel], lengths, M)
    if complete_pairs:
        m = oracle.find_pairs(m, orig.size)
    kept = orig[pkg.mask_to_indices(m, orig.size).astype(np.int64)]
    return pkg.indices_to_mask(kept, n), int((~keep).sum())


def write_panel_bam(path, rng, references, panel, n_pairs, straddle=0.10, cross=0.02, unmapped=0.02):
    """pairs drawn from the panel's amplicons (panel_pairs' shape) as a multi-reference BAM in shuffled record order
    -> (header, parsed records with "ref_id", reference lengths)"""
    names = [n for n, _ in references]
    lengths = [L for _, L in references]
    offs, a0, a1 = panel_csr(panel, names)
    s, e, ids = panel_pairs(rng, lengths, offs, a0, a1, n_pairs, straddle=straddle, cross=cross)
    recs = []
    for q in range(n_pairs):
        for m, flag in ((0, 0x41), (1, 0x81)):
            i = 2 * q + m
            if rng.random() < unmapped:
                recs.append(bam_py.pack_record(f"p{q}", flag | 0x4, -1, 0, [], 100, ref_id=-1))
                continue
            span = int(e[i]) - int(s[i]) + 1
            recs.append(bam_py.pack_record(f"p{q}", flag, int(s[i]), int(rng.integers(0, 61)), [(span, "M")],
                                           int(rng.integers(span - 40, span + 1)), ref_id=int(ids[i])))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    bam_py.write_bam(path, references, recs)
    header, parsed, ref_lengths = bam_py.parse(path)
    for r in parsed:
        r["ref_id"] = struct.unpack_from("<i", r["raw"], 4)[0]
    return header, parsed, ref_lengths


def inside_by_reference(parsed, offs, a0, a1):
    """bam_py.pair_like_the_reference's `inside` for amplicons matched by reference"""
    def ref(r):
        rid = parsed[r["bam_id"]]["ref_id"]
        return NO_CONTIG if rid < 0 else rid

    def inside(r1, r2):
        return in_one_amplicon(offs, a0, a1, ref(r1), r1["start"], r1["end"], ref(r2), r2["start"], r2["end"])
    return inside


INFLUENZA = [("PB2", 2341), ("PB1", 2341), ("PA", 2233), ("HA", 1778), ("NP", 1565), ("NA", 1413), ("M", 1027),
             ("NS", 890)]   # segment lengths of influenza A (13.6 kb in all)


def segment_panel(references, per_ref=25, size=250):
    """per_ref amplicons of `size` bases tiled evenly over each reference (overlapping where the reference is short)"""
    panel = {}
    for name, L in references:
        step = max((L - size) // (per_ref - 1), 1)
        panel[name] = [(k * step, k * step + size - 1) for k in range(per_ref) if k * step + size - 1 < L]
    return panel
