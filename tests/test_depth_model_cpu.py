"""tests/depth_model.py against a literal per-position loop on tiny seeded instances, and against the oracle's own solve:
a valid answer has no deficit anywhere, and clearing one needed kept bit shows up inside that read only."""
import numpy as np

import depth_model as dm
import multi_reference as mr
import quality_model as qm

NO_CONTIG = 0xFFFFFFFF


def _literal(s, e, ids, lengths, M, mask, regions, padding, n_bins):
    n = len(s)
    kept = [True] * n if mask is None else [bool((int(mask[i >> 6]) >> (i & 63)) & 1) for i in range(n)]
    cov = [[0] * L for L in lengths]
    kc = [[0] * L for L in lengths]
    for i in range(n):
        if ids[i] == NO_CONTIG:
            continue
        for p in range(s[i], e[i] + 1):
            cov[ids[i]][p] += 1
            kc[ids[i]][p] += int(kept[i])

    def row(c, a, b):
        if b < a:
            return (c,) + (0,) * 13
        ci, ck = cov[c][a:b + 1], kc[c][a:b + 1]
        short = [max(0, min(x, M) - y) for x, y in zip(ci, ck)]
        return (c, a, b, min(ci), max(ci), min(ck), max(ck), 0, b - a + 1, sum(ci), sum(ck), sum(x > M for x in ci),
                sum(x > 0 for x in short), sum(short))

    contig_rows = [row(c, 0, L - 1) for c, L in enumerate(lengths)]
    region_rows, scope = [], []
    if regions is not None:
        offs, t0, t1 = regions
        for c, L in enumerate(lengths):
            inside = [False] * L
            for k in range(offs[c], offs[c + 1]):
                for p in range(max(t0[k] - padding, 0), min(t1[k] + padding, L - 1) + 1):
                    inside[p] = True
            p = 0
            while p < L:
                if inside[p]:
                    a = p
                    while p + 1 < L and inside[p + 1]:
                        p += 1
                    region_rows.append(row(c, a, p))
                p += 1
            scope += [(c, p) for p in range(L) if inside[p]]
    else:
        scope = [(c, p) for c, L in enumerate(lengths) for p in range(L)]
    hist_in, hist_kept = [0] * n_bins, [0] * n_bins
    if n_bins:
        for c, p in scope:
            hist_in[min(cov[c][p], n_bins - 1)] += 1
            hist_kept[min(kc[c][p], n_bins - 1)] += 1
    return contig_rows, region_rows, hist_in, hist_kept, len(scope)


def _tiny(rng):
    n_contigs = int(rng.integers(1, 5))
    lengths = [int(rng.integers(1, 40)) if rng.random() > 0.2 else 0 for _ in range(n_contigs)]
    live = [c for c, L in enumerate(lengths) if L]
    s, e, ids = [], [], []
    for _ in range(int(rng.integers(0, 60))):
        if not live or rng.random() < 0.1:
            s.append(int(rng.integers(0, 1000))); e.append(int(rng.integers(0, 1000))); ids.append(NO_CONTIG)
            continue
        c = live[int(rng.integers(0, len(live)))]
        a = int(rng.integers(0, lengths[c]))
        s.append(a); e.append(int(rng.integers(a, lengths[c]))); ids.append(c)
    return s, e, ids, lengths


def test_model_equals_a_per_position_loop():
    with_regions = unplaced_bits = 0
    for seed in range(300):
        rng = np.random.default_rng(seed)
        s, e, ids, lengths = _tiny(rng)
        n = len(s)
        M = int(rng.integers(1, 5))
        mask = None
        if seed % 3:
            mask = rng.integers(0, 1 << 63, size=max((n + 63) // 64, 1), dtype=np.uint64) * np.uint64(2) + \
                rng.integers(0, 2, size=max((n + 63) // 64, 1), dtype=np.uint64)     # bits of unplaced reads and beyond n too
            unplaced_bits += int(any(i == NO_CONTIG for i in ids))
        regions = None
        padding = int(rng.choice([0, 2]))
        if seed % 2:
            offs, t0, t1 = [0], [], []
            for L in lengths:
                for _ in range(int(rng.integers(0, 4))):
                    a = int(rng.integers(0, L + 5))                      # some beyond the contig
                    t0.append(a); t1.append(a + int(rng.integers(0, 12)))
                    if rng.random() < 0.4:                               # nested, overlapping
                        t0.append(a + 1); t1.append(a + 3)
                offs.append(len(t0))
            regions = (offs, t0, t1)
            with_regions += 1
        depth_max = 60
        n_bins = int(rng.choice([0, 1, 2, depth_max + 5]))
        want = _literal(s, e, ids, lengths, M, mask, regions, padding, n_bins)
        got = dm.report(s, e, ids, lengths, M, keep_mask=mask, n_bins=n_bins, padding=padding,
                        **({} if regions is None else dict(target_offsets=regions[0], target_starts=regions[1],
                                                           target_ends=regions[2])))
        assert got["contig_rows"] == want[0], seed
        assert got["region_rows"] == want[1], seed
        assert got["hist_in"].tolist() == want[2] and got["hist_kept"].tolist() == want[3], seed
        assert got["stats"]["scope_positions"] == want[4], seed
        if regions is not None:
            assert got["stats"]["regions_merged"] == len(want[1]) <= len(regions[1]) == got["stats"]["regions_in"], seed
        placed = [i for i in range(n) if ids[i] != NO_CONTIG]
        assert got["stats"]["reads_placed"] == len(placed)
        if mask is None:
            assert got["stats"]["reads_kept"] == len(placed)
    assert with_regions > 100 and unplaced_bits > 50


def test_the_oracles_answer_has_no_deficit_and_a_missing_read_shows_inside_that_read_only(oracle):
    hit = 0
    for seed in range(12):
        rng = np.random.default_rng(500 + seed)
        s, e, ids, lengths = mr.random_by_contig(rng, int(rng.integers(1, 5)), max_reads_per_contig=600)
        M = int(rng.choice([2, 5, 20]))
        mask = mr.oracle_by_contig(oracle, s, e, ids, lengths, M)
        rep = dm.report(s, e, ids, lengths, M, keep_mask=mask)
        assert all(r[12] == 0 and r[13] == 0 for r in rep["contig_rows"]) and rep["stats"]["deficit_positions"] == 0
        covs = dm.coverages(s, e, ids, lengths, mask)
        bits = qm.bits_of(mask, s.size)
        # a kept read that covers a position where kept == min(cov, M): without it that position is short
        for i in np.flatnonzero(bits).tolist():
            c = int(ids[i])
            ci, ck = covs[c][0][s[i]:e[i] + 1], covs[c][1][s[i]:e[i] + 1]
            tight = ck == np.minimum(ci, M)
            if not tight.any():
                continue
            less = bits.copy()
            less[i] = False
            rep2 = dm.report(s, e, ids, lengths, M, keep_mask=qm.mask_of(less))
            assert rep2["contig_rows"][c][12] == int(tight.sum()) == rep2["contig_rows"][c][13]
            assert all(r[12] == 0 for k, r in enumerate(rep2["contig_rows"]) if k != c)
            # ... and nowhere outside the read: regions = the read's interval and its complement
            offs = np.zeros(len(lengths) + 1, np.uint32)
            offs[c + 1:] = 1
            inside = dm.report(s, e, ids, lengths, M, keep_mask=qm.mask_of(less), target_offsets=offs,
                               target_starts=[s[i]], target_ends=[e[i]])
            assert inside["stats"]["deficit_positions"] == int(tight.sum())
            hit += 1
            break
    assert hit >= 8
