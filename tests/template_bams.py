"""BAM files for the tests of the template-aware ingest (read_bam(templates=True), downsample_bam(template_aware=True)),
written by the independent writer in tests/bam_py.py: any name, flag, refID, position, MAPQ, CIGAR and raw optional
fields per record.  expected_segments restates the ingest on the packed records with struct alone -- nothing shared with
genome-downsampler_amd/host/src/bam_io.cpp.
  record              one packed record from (name, flag, ref_id, pos, mapq, cigar as [(len, op)], aux bytes)
  cg_record           a record whose real CIGAR sits in a CG:B,I field behind the placeholder <l_seq>S<rlen>N
  single_end_records  a single-end library: one record per name
  mixed_records       pairs (some with an unmapped mate), spliced reads alone and in pairs, split reads with supplementary
                      alignments on other references, secondary alignments, one CG-field record; shuffled
  expected_segments   -> dict(starts, ends, contig_ids, template_ids, qualities, seq_lengths, segment_records,
                      n_templates, filtered_out)"""
import struct

import numpy as np

import bam_py

NO_CONTIG = 0xFFFFFFFF
REF_OPS = "MDN=X"
QUERY_OPS = "MIS=X"


def record(name, flag, ref_id, pos, mapq, cigar, aux=b"", l_seq=None):
    if l_seq is None:
        l_seq = sum(n for n, op in cigar if op in QUERY_OPS) or 50
    return bam_py.pack_record(name, flag, pos, mapq, cigar, l_seq, ref_id=ref_id, aux=aux)


def cg_field(cigar):
    vals = [(n << 4) | bam_py.CIGAR_OPS.index(op) for n, op in cigar]
    return b"CGBI" + struct.pack(f"<I{len(vals)}I", len(vals), *vals)


def cg_record(name, flag, ref_id, pos, mapq, cigar, before=b"", after=b""):
    """the long-CIGAR convention: the in-place CIGAR is <l_seq>S<rlen>N, the real one the CG:B,I field; `before` and
    `after` are further optional fields around it"""
    l_seq = sum(n for n, op in cigar if op in QUERY_OPS)
    rlen = sum(n for n, op in cigar if op in REF_OPS)
    return record(name, flag, ref_id, pos, mapq, [(l_seq, "S"), (rlen, "N")], aux=before + cg_field(cigar) + after,
                  l_seq=l_seq)


def _simple_cigar(rng, lo=60, hi=150):
    match = int(rng.integers(lo, hi + 1))
    if rng.random() < 0.15:
        return [(match, "M"), (int(rng.integers(1, 10)), "D"), (20, "M")]
    if rng.random() < 0.15:
        return [(int(rng.integers(1, 30)), "S"), (match, "M")]
    return [(match, "M")]


def _spliced_cigar(rng, L):
    blocks = int(rng.integers(2, 4))
    cigar = []
    for b in range(blocks):
        if b:
            cigar.append((int(rng.integers(50, max(51, min(1000, L // 6)))), "N"))
        cigar.append((int(rng.integers(30, 80)), "M"))
    return cigar


def _rlen(cigar):
    return sum(n for n, op in cigar if op in REF_OPS)


def _place(rng, refs, cigar, ref=None):
    ref = int(rng.integers(0, len(refs))) if ref is None else ref
    return ref, int(rng.integers(0, refs[ref][1] - _rlen(cigar)))


def single_end_records(rng, refs, n):
    out = []
    for i in range(n):
        cigar = _simple_cigar(rng)
        ref, pos = _place(rng, refs, cigar)
        out.append(record(f"r{i}", 16 if rng.random() < 0.5 else 0, ref, pos, int(rng.integers(0, 61)), cigar))
    return out


def mixed_records(rng, refs, n_templates):
    out = []
    for i in range(n_templates):
        name, kind, mapq = f"t{i}", rng.random(), int(rng.integers(0, 61))
        if kind < 0.45:                                                  # a pair; some mates unmapped
            ref = int(rng.integers(0, len(refs)))
            for flag in (0x41, 0x81):
                cigar = _simple_cigar(rng)
                r, pos = _place(rng, refs, cigar, ref if rng.random() < 0.9 else None)
                u = rng.random()
                if u < 0.04:
                    out.append(record(name, flag | 0x4, -1, -1, 0, [], l_seq=100))
                elif u < 0.06:                                           # unmapped, placed at its mate's position
                    out.append(record(name, flag | 0x4, r, pos, 0, [], l_seq=100))
                else:
                    out.append(record(name, flag, r, pos, mapq, cigar))
        elif kind < 0.6:                                                 # a single-end read
            cigar = _simple_cigar(rng)
            r, pos = _place(rng, refs, cigar)
            out.append(record(name, 0, r, pos, mapq, cigar))
        elif kind < 0.8:                                                 # a spliced read, alone or with a mate
            paired = rng.random() < 0.5
            r = int(rng.integers(0, len(refs)))
            cigar = _spliced_cigar(rng, refs[r][1])
            _, pos = _place(rng, refs, cigar, r)
            out.append(record(name, 0x41 if paired else 0, r, pos, mapq, cigar))
            if paired:
                cigar = _spliced_cigar(rng, refs[r][1]) if rng.random() < 0.5 else _simple_cigar(rng)
                _, pos = _place(rng, refs, cigar, r)
                out.append(record(name, 0x81, r, pos, mapq, cigar))
        else:                                                            # a split read: a primary and supplementaries
            cigar = [(int(rng.integers(40, 90)), "M"), (60, "S")]
            r, pos = _place(rng, refs, cigar)
            out.append(record(name, 0, r, pos, mapq, cigar))
            for _ in range(int(rng.integers(1, 3))):
                cigar = [(40, "H"), (int(rng.integers(30, 60)), "M")]
                r, pos = _place(rng, refs, cigar)
                out.append(record(name, 0x800, r, pos, mapq, cigar))
        if rng.random() < 0.1:                                           # a secondary alignment of the same read
            cigar = _simple_cigar(rng)
            r, pos = _place(rng, refs, cigar)
            out.append(record(name, 0x100, r, pos, 0, cigar))
    # one split, spliced read with three supplementaries, and one record under the long-CIGAR convention
    out.append(record("big", 0, 0, 100, 60, [(50, "M"), (300, "N"), (40, "M"), (200, "N"), (30, "M")]))
    for k in range(3):
        out.append(record("big", 0x800, k % len(refs), 50 + 10 * k, 60, [(80, "H"), (45, "M")]))
    out.append(cg_record("long", 0, 0, 700, 50, [(40, "M"), (150, "N"), (35, "M"), (2, "D"), (25, "M")],
                         before=b"NMC\x03" + b"RGZgroup1\0", after=b"XSi" + struct.pack("<i", -7)))
    return [out[i] for i in rng.permutation(len(out))]


def expected_segments(records, split_spliced=True, include_secondary=False, min_mapq=0, min_length=0):
    cols = {k: [] for k in ("starts", "ends", "contig_ids", "template_ids", "qualities", "seq_lengths", "segment_records")}
    names, failed, accepted = {}, set(), []
    for rec_id, raw in enumerate(records):
        ref_id, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHI", raw, 4)
        qname = raw[36:36 + l_name - 1]
        o = 36 + l_name
        cigar = [(v >> 4, bam_py.CIGAR_OPS[v & 0xF]) for v in struct.unpack_from(f"<{n_cigar}I", raw, o)]
        accepted.append(not (flag & 0x100) or include_secondary)
        if not accepted[-1]:
            continue
        if len(cigar) == 2 and cigar[0] == (l_seq, "S") and cigar[1][1] == "N":
            aux = raw[o + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:]
            at = aux.find(b"CGBI")               # (good enough for the records this module writes)
            if at >= 0:
                count, = struct.unpack_from("<I", aux, at + 4)
                cigar = [(v >> 4, bam_py.CIGAR_OPS[v & 0xF]) for v in struct.unpack_from(f"<{count}I", aux, at + 8)]
        tpl = names.setdefault(qname, len(names))
        blocks = []
        if flag & 0x4 or ref_id < 0:
            blocks, contig = [(0, 0)], NO_CONTIG
        else:
            contig = ref_id
            if mapq < min_mapq or l_seq < min_length:
                failed.add(tpl)
            at, length = pos, 0
            for n, op in cigar:
                if op in "MD=X" or (op == "N" and not split_spliced):
                    length += n
                elif op == "N":
                    if length:
                        blocks.append((at, at + length - 1))
                    at, length = at + length + n, 0
            if length:
                blocks.append((at, at + length - 1))
            if not blocks:
                blocks = [(pos, pos + max(_rlen(cigar), 1) - 1)]
        for s, e in blocks:
            for k, v in zip(cols, (s, e, contig, tpl, mapq, l_seq, rec_id)):
                cols[k].append(v)
    keep = [t not in failed for t in cols["template_ids"]]
    renumber = {}
    for t in range(len(names)):
        if t not in failed:
            renumber[t] = len(renumber)
    for rec_id, t in zip(cols["segment_records"], cols["template_ids"]):
        if t in failed:
            accepted[rec_id] = False
    out = {k: np.array([x for x, ok in zip(v, keep) if ok], np.int64) for k, v in cols.items()}
    out["template_ids"] = np.array([renumber[t] for t in out["template_ids"].tolist()], np.int64)
    for k in ("starts", "ends", "contig_ids", "template_ids", "qualities", "seq_lengths"):
        out[k] = out[k].astype(np.uint32)
    out["n_templates"] = len(renumber)
    out["filtered_out"] = np.flatnonzero(~np.array(accepted, bool)) if accepted else np.zeros(0, np.int64)
    return out
