"""Stratified downsampling (qmcp_hip_solve_stratified_*) restated on the oracle: for every stratum, the per-contig
canonical selection (multi_reference.oracle_by_contig) of that stratum's placed reads alone, at the stratum's cap,
scattered back to input order; the mask is the OR over the strata.  The rows are plain numpy sums."""
import numpy as np

import multi_reference as mr

NO_STRATUM = 0xFFFFFFFF


def unpack(mask, n):
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8), bitorder="little")[:n].astype(bool)


def pack(bits):
    n = bits.size
    out = np.zeros(((n + 63) // 64) * 64, dtype=np.uint8)
    out[:n] = bits
    return np.packbits(out, bitorder="little").view(np.uint64).copy()


def stratified_bits(oracle, starts, ends, contig_ids, strata, contig_lengths, caps):
    """-> bool[n_reads] in input order"""
    s, e = np.asarray(starts, dtype=np.uint32), np.asarray(ends, dtype=np.uint32)
    ids, strata = np.asarray(contig_ids, dtype=np.uint32), np.asarray(strata, dtype=np.uint32)
    keep = np.zeros(s.size, dtype=bool)
    for k, M in enumerate(caps):
        on = np.flatnonzero((strata == k) & (ids != mr.NO_CONTIG))
        if int(M) == 0 or on.size == 0:
            continue
        mask = mr.oracle_by_contig(oracle, s[on], e[on], ids[on], contig_lengths, int(M))
        keep[on[unpack(mask, on.size)]] = True
    return keep


def stratified_mask(oracle, starts, ends, contig_ids, strata, contig_lengths, caps):
    return pack(stratified_bits(oracle, starts, ends, contig_ids, strata, contig_lengths, caps))


def rows(starts, ends, contig_ids, strata, n_strata, keep_bits):
    """-> int array [n_strata, 4]: placed reads, kept reads, bases, kept bases of every stratum"""
    s, e = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    ids, strata = np.asarray(contig_ids, dtype=np.uint32), np.asarray(strata, dtype=np.uint32)
    placed = (ids != mr.NO_CONTIG) & (strata != NO_STRATUM)
    span = np.where(placed, e - s + 1, 0)
    k = np.where(placed, strata, 0).astype(np.int64)
    kept = placed & np.asarray(keep_bits, dtype=bool)
    out = np.zeros((n_strata, 4), dtype=np.int64)
    out[:, 0] = np.bincount(k, weights=placed, minlength=n_strata)[:n_strata]
    out[:, 1] = np.bincount(k, weights=kept, minlength=n_strata)[:n_strata]
    out[:, 2] = np.bincount(k[placed], weights=span[placed].astype(np.float64), minlength=n_strata)[:n_strata]
    out[:, 3] = np.bincount(k[kept], weights=span[kept].astype(np.float64), minlength=n_strata)[:n_strata]
    return out   # (float64 weights are exact here: the sums stay far below 2^53)


def rows_of(stratum_rows):
    """a list of StratumRow -> the same [n_strata, 4] array"""
    return np.array([[r.n_reads, r.n_kept, r.bases_in, r.bases_kept] for r in stratum_rows], dtype=np.int64).reshape(-1, 4)


def random_strata(rng, n, n_strata, none=0.03):
    strata = rng.integers(0, n_strata, size=n).astype(np.uint32)
    strata[rng.random(n) < none] = NO_STRATUM
    return strata


# ---------------------------------------------------------------- a BAM with read groups and both strands (tests only)
READ_GROUPS = ["rgA", "lane.2", "s3"]
REFERENCES = [("chr1", 9_000), ("chr2", 4_000)]


def _aux_before(rng):
    """optional fields of the types A c S i f Z H B, in a random selection and order"""
    import struct
    fields = [b"XA" + b"A" + b"q", b"Xc" + b"c" + struct.pack("<b", -5), b"XS" + b"S" + struct.pack("<H", 60000),
              b"Xi" + b"i" + struct.pack("<i", -123456), b"Xf" + b"f" + struct.pack("<f", 1.5),
              b"XZ" + b"Z" + b"RG:Z:rgA not a tag\0", b"XH" + b"H" + b"1AE301\0",
              b"XB" + b"B" + b"S" + struct.pack("<I", 3) + struct.pack("<3H", 1, 2, 3),
              b"Xb" + b"B" + b"c" + struct.pack("<I", 0), b"Xg" + b"B" + b"f" + struct.pack("<I", 2) + struct.pack("<2f", .5, 2.)]
    pick = [f for f in fields if rng.random() < 0.5]
    return b"".join(pick[i] for i in rng.permutation(len(pick)))


def write_stratified_bam(path, rng, n_pairs=1500):
    """pairs on two references in shuffled file order, both strands, three @RG lines in the header; most records carry an
    RG:Z field between other optional fields of every type, some carry none, one names a read group the header does not
    list -> (header, parsed records with "ref_id", "reverse" and "rg" (None without the field) added, reference
    lengths); the read group is read back from bam_py.to_sam's independent rendering"""
    import struct

    import bam_py
    recs = []
    for q in range(n_pairs):
        ref = int(rng.integers(0, len(REFERENCES)))
        group = READ_GROUPS[int(rng.integers(0, len(READ_GROUPS)))]   # a pair shares its read group, as in real files
        for first in (True, False):
            flag = (0x41 if first else 0x81) | (0x10 if rng.random() < 0.5 else 0)
            roll = rng.random()
            rg = b"" if roll < 0.06 else b"RG" + b"Z" + (b"rgX" if q == 7 and first else group.encode()) + b"\0"
            aux = _aux_before(rng) + rg + _aux_before(rng)
            if rng.random() < 0.03:
                recs.append(bam_py.pack_record(f"p{q}", flag | 0x4, -1, 0, [], 100, ref_id=-1, aux=aux))
                continue
            L = REFERENCES[ref][1]
            match = int(rng.integers(60, 151))
            pos = int(rng.integers(0, L - match))
            recs.append(bam_py.pack_record(f"p{q}", flag, pos, int(rng.integers(0, 61)), [(match, "M")], match, ref_id=ref,
                                           aux=aux))
    recs = [recs[i] for i in rng.permutation(len(recs))]
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join(f"@RG\tSM:sample{k}\tID:{g}\tPL:x\n" for k, g in enumerate(READ_GROUPS)) + \
        "@PG\tID:writer\n"
    bam_py.write_bam(path, REFERENCES, recs, text=text)
    header, parsed, ref_lengths = bam_py.parse(path)
    refs = bam_py.parse_references(header)
    for r in parsed:
        r["ref_id"] = struct.unpack_from("<i", r["raw"], 4)[0]
        r["reverse"] = bool(r["flag"] & 0x10)
        tags = [f for f in bam_py.to_sam(r["raw"], refs).split("\t")[11:] if f.startswith("RG:Z:")]
        r["rg"] = tags[0][5:] if tags else None
    return header, parsed, ref_lengths


def expected_strata(parsed, reads, stratify):
    """the strata and names read_bam(stratify=...) must give for the reads of bam_py.pair_like_the_reference"""
    if stratify == "strand":
        return np.array([1 if parsed[r["bam_id"]]["reverse"] else 0 for r in reads], dtype=np.uint32), ["+", "-"]
    index = {g: k for k, g in enumerate(READ_GROUPS)}
    other = len(READ_GROUPS)
    return (np.array([index.get(parsed[r["bam_id"]]["rg"], other) for r in reads], dtype=np.uint32),
            READ_GROUPS + ["*"])
