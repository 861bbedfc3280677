"""qmcp_hip_solve_pairs_*: the staged, pair-aware solve on the device.  Every mask is compared bit for bit with
tests/pair_model.py (the stages restated on the coverage profile's model and the oracle's find_pairs), through both the
host and the device entry, and the per-stage counts of qmcp_hip_pair_stats with the model's."""
import functools

import numpy as np
import pytest
import torch

import bam_py
import multi_reference as mr
import pair_model as pairs
import profile_model as pm

pytestmark = pytest.mark.gpu

NO_CONTIG = 0xFFFFFFFF
QMCP_EINVAL, QMCP_ERANGE = -1, -3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def solve_device(pkg, solver, s, e, ids, lengths, M, stages):
    n = s.size
    cols = [_dev(x) for x in (s, e, ids)]
    d_mask = torch.full((pkg.mask_words(n) + 1,), -1, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    st, ps = solver.solve_pairs_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, lengths, M,
                                       d_mask.data_ptr(), stages, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_mask.cpu().numpy().view(np.uint64)
    assert out[pkg.mask_words(n)] == np.uint64(0xFFFFFFFFFFFFFFFF)      # nothing written past the mask
    return out[:pkg.mask_words(n)].copy(), st, ps


def check_both_entries(pkg, solver, oracle, inst, M, stages, model_inst=None):
    """host and device entry against the model (on model_inst, a translated copy of the instance, when given);
    -> the host call's (stats, pair_stats) and the model's (selected, kept)"""
    s, e, ids, lengths = inst
    want, selected, kept, _ = pairs.staged(oracle, *(model_inst or inst), M, stages, fast=True)
    out = None
    for entry in ("host", "device"):
        if entry == "host":
            got, st, ps = solver.solve_pairs(s, e, ids, lengths, M, stages)
        else:
            got, st, ps = solve_device(pkg, solver, s, e, ids, lengths, M, stages)
        diff = int(np.count_nonzero(pm.unpack(got ^ want, s.size))) if s.size else 0
        assert np.array_equal(got, want), (entry, M, stages, diff)
        k = len(selected)
        assert ps.n_stages == k and list(ps.target)[:k] == (pairs.default_stages(M) if stages is None else list(stages))
        assert list(ps.n_selected)[:k] == selected and list(ps.n_kept)[:k] == kept, (entry, M, stages)
        assert st.n_kept == selected[0] and ps.sweeps[0] == 0
        out = out or (st, ps)
    return out, (selected, kept)


# ------------------------------------------------------------------------------------------ random calls
def random_pair_call(seed, n_contigs, max_reads=3000):
    """multi_reference.random_by_contig (some contigs empty, 3 % unplaced reads, shuffled: mates on other contigs and
    unplaced mates of placed reads) cut to an even count, with one more contig that has no read"""
    rng = np.random.default_rng(seed)
    s, e, ids, lengths = mr.random_by_contig(rng, n_contigs, max_reads_per_contig=max_reads)
    n = s.size - (s.size & 1)
    return s[:n], e[:n], ids[:n], np.concatenate([lengths, [777]]).astype(np.uint32)


RANDOM_CASES = [(M, kind) for M in (1, 2, 3, 7, 20) for kind in ("default", "one", "from 1") if not (M == 1 and kind == "from 1")]
RANDOM_CASES.append((16, "1..16"))


@pytest.mark.parametrize("case", range(len(RANDOM_CASES)))
def test_random_calls_equal_the_model(pkg, solver, oracle, case):
    M, kind = RANDOM_CASES[case]
    stages = {"default": None, "one": [M], "from 1": [1, M], "1..16": list(range(1, 17))}[kind]
    inst = random_pair_call(1000 + case, 1 + case % 6)
    s, e, ids, lengths = inst
    (st, ps), (selected, kept) = check_both_entries(pkg, solver, oracle, inst, M, stages)
    placed = ids != NO_CONTIG
    assert st.n_reads == int(placed.sum())
    # the instance has what the test is for: unplaced reads, unplaced mates of placed reads, an empty contig, and --
    # with reads on more than one contig -- mates on different contigs
    both = placed[0::2] & placed[1::2]
    assert (~placed).any() and (placed[0::2] != placed[1::2]).any() and not (ids == lengths.size - 1).any()
    assert np.unique(ids[placed]).size == 1 or (ids[0::2][both] != ids[1::2][both]).any()
    if ps.n_stages > 1:
        assert sum(ps.sweeps[1:ps.n_stages]) >= 1


@pytest.mark.parametrize("M", [1, 5, 40])
def test_one_stage_is_the_by_contig_solve_and_the_pair_completion(pkg, solver, oracle, M):
    s, e, ids, lengths = random_pair_call(50 + M, 4)
    n = s.size
    cols = [_dev(x) for x in (s, e, ids)]
    d_plain = torch.zeros(pkg.mask_words(n), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    solver.solve_by_contig_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, lengths, M,
                                  d_plain.data_ptr(), stream=stream)
    plain_kept = solver.last_stats.n_kept
    solver.complete_pairs_device(d_plain.data_ptr(), n, stream=stream)
    torch.cuda.synchronize()
    want = d_plain.cpu().numpy().view(np.uint64)
    got_d, st, ps = solve_device(pkg, solver, s, e, ids, lengths, M, [M])
    got_h, _, _ = solver.solve_pairs(s, e, ids, lengths, M, [M])
    assert np.array_equal(got_d, want) and np.array_equal(got_h, want)
    assert np.array_equal(want, pairs.plain(oracle, s, e, ids, lengths, M))
    assert ps.n_stages == 1 and ps.n_selected[0] == plain_kept == st.n_kept
    assert ps.n_kept[0] == int(pm.unpack(want, n).sum()) and ps.sweeps[0] == 0


# ------------------------------------------------------------------------------------------ need tails, credit edges
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
def test_need_tails_and_a_contig_of_one_position(pkg, solver, oracle, tail):
    """total axis lengths with ltot % 4 = tail; contig 1 has one position (and reads on it), the last positions of the
    axis are covered: the groups of four that k_pair_need takes whole end before them"""
    rng = np.random.default_rng(70 + tail)
    lengths = np.array([403, 1, 400 + tail], np.uint32)
    assert int(lengths.sum()) % 4 == tail
    ids = rng.integers(0, 3, size=600).astype(np.uint32)
    ids[:40] = 1
    L = lengths[ids].astype(np.int64)
    span = np.minimum(rng.integers(1, 60, size=ids.size), L)
    s = (rng.random(ids.size) * (L - span + 1)).astype(np.int64)
    s[40:60] = L[40:60] - span[40:60]                                   # reads that end on their contig's last position
    e = s + span - 1
    inst = (s.astype(np.uint32), e.astype(np.uint32), ids, lengths)
    for M, stages in ((4, None), (7, [2, 3, 7])):
        (_, ps), _ = check_both_entries(pkg, solver, oracle, inst, M, stages)
        assert sum(ps.sweeps[1:ps.n_stages]) >= 1


def test_credit_events_that_meet_in_one_cell(pkg, solver, oracle):
    """a kept read ends at a contig's last position and a kept read starts at position 0 of the next contig: the -1 and the
    +1 land on the same cell of the batch's axis"""
    lengths = np.array([100, 100, 50], np.uint32)
    rows = [  # (start, end, contig), pairs in file order
        (60, 99, 0), (0, 39, 1),        # the two reads of the doc string, one pair
        (60, 99, 0), (0, 39, 1),
        (50, 99, 0), (0, 45, 1), (70, 99, 0), (0, 20, 1), (80, 99, 0), (0, 10, 1), (90, 99, 0), (0, 5, 1),
        (95, 99, 0), (0, 2, 1), (99, 99, 0), (0, 0, 1), (0, 49, 2), (0, 49, 2), (10, 99, 0), (20, 99, 1),
    ]
    s, e, ids = (np.array(x, np.uint32) for x in zip(*rows))
    inst = (s, e, ids, lengths)
    for M, stages in ((4, None), (6, [1, 3, 6]), (3, [1, 2, 3])):
        (_, ps), (selected, kept) = check_both_entries(pkg, solver, oracle, inst, M, stages)
        assert kept[0] >= 2


@pytest.mark.parametrize("M", [2])
def test_saturated_credit_queues_no_sweep(pkg, solver, oracle, M):
    """mates with identical intervals at M = 2: stage 1 at 1 keeps one read per demand, its mate doubles the depth, so
    wherever a read is left the credit has reached M -- stage 2 finds candidates, asks for nothing and queues no sweep"""
    rng = np.random.default_rng(5)
    lengths = np.array([3000, 2000], np.uint32)
    n_pairs = 1500
    ids = np.repeat(rng.integers(0, 2, size=n_pairs), 2).astype(np.uint32)
    span = np.repeat(rng.integers(1, 120, size=n_pairs), 2)
    s = np.repeat(rng.random(n_pairs), 2)
    s = (s * (lengths[ids].astype(np.int64) - span + 1)).astype(np.int64)
    inst = (s.astype(np.uint32), (s + span - 1).astype(np.uint32), ids, lengths)
    (st, ps), (selected, kept) = check_both_entries(pkg, solver, oracle, inst, M, None)
    assert ps.n_stages == 2 and list(ps.target)[:2] == [1, 2]
    assert kept[0] < s.size                                              # candidates are left ...
    assert ps.n_selected[1] == 0 and ps.n_kept[1] == ps.n_kept[0] == 2 * ps.n_selected[0]
    assert ps.demand[1] == 0 and ps.sweeps[1] == 0                       # ... and nothing is asked of them


# ------------------------------------------------------------------------------------------ word edges
def every_fourth_pair_instance(n_reads):
    """groups of four pairs on one contig: pair 4g is two identical reads over the whole group's stretch, the other three
    pairs are short reads inside it.  Stage 1 at T = 1 keeps read 8g alone (leftmost deficit, furthest end, lowest index)
    and the completion its mate: exactly every fourth pair is in S, and the candidates are the other three of each four"""
    n_pairs = n_reads // 2
    rng = np.random.default_rng(n_reads)
    s, e = np.zeros(n_reads, np.int64), np.zeros(n_reads, np.int64)
    for q in range(n_pairs):
        base = 40 * (q // 4)
        if q % 4 == 0:
            s[2 * q:2 * q + 2], e[2 * q:2 * q + 2] = base, base + 37
        else:
            a = base + rng.integers(1, 30, size=2)
            s[2 * q:2 * q + 2], e[2 * q:2 * q + 2] = a, np.minimum(a + rng.integers(0, 8, size=2), base + 37)
    L = 40 * ((n_pairs + 3) // 4) + 3
    return s.astype(np.uint32), e.astype(np.uint32), np.zeros(n_reads, np.uint32), np.array([L], np.uint32)


@pytest.mark.parametrize("n_reads", [0, 2, 62, 64, 66, 126, 128, 130, 8190, 8194])
def test_word_edges_of_the_gathered_mask_and_the_compaction(pkg, solver, oracle, n_reads):
    inst = every_fourth_pair_instance(n_reads)
    (st, ps), (selected, kept) = check_both_entries(pkg, solver, oracle, inst, 3, [1, 3])
    n_pairs = n_reads // 2
    assert selected[0] == (n_pairs + 3) // 4 and kept[0] == 2 * selected[0]     # every fourth pair, and only those
    _, _, _, sets = pairs.staged(oracle, *inst, 3, [1, 3], fast=True)
    assert np.array_equal(np.flatnonzero(sets[0]) // 2 % 4, np.zeros(kept[0], np.int64))
    assert ps.sweeps[1] == (1 if n_pairs >= 2 else 0)


# ------------------------------------------------------------------------------------------ 64-bit keys, two batches
def island_pairs(seed, lengths, max_span, per_island=30):
    """reads of spans 1..max_span (both present) in islands at both ends of every contig and around a multiple of 64
    inside it, shuffled over the contigs: mates mostly lie on different contigs"""
    rng = np.random.default_rng(seed)
    ss, ee, ii = [], [], []
    for c, L in enumerate(lengths):
        for a in (0, 64 * int(rng.integers(L // 256, L // 128)), L - 1):
            span = np.minimum(rng.integers(1, max_span + 1, size=per_island), L)
            span[0], span[1] = min(max_span, L), 1
            s = np.clip(a - rng.integers(0, span) + rng.integers(-2, 3, size=per_island), 0, L - span)
            ss.append(s); ee.append(s + span - 1); ii.append(np.full(per_island, c))
    s, e, ids = (np.concatenate(x) for x in (ss, ee, ii))
    perm = rng.permutation(s.size)
    u = lambda x: np.asarray(x, np.uint32)
    return u(s[perm]), u(e[perm]), u(ids[perm]), u(lengths)


def test_capped_route_with_64_bit_keys(pkg, solver, oracle):
    """2^18 + 5 positions (19 bits) and spans 1..20 000 (15 bits): 34 key bits, the smallest wide shape
    test_gpu_profile_forms.py documents.  The model runs on profile_model.compact's copy; the stage-2 candidates still
    hold a 1-base read and a 20 000-base read, so their keys are wide too"""
    inst = island_pairs(31, [100_000, 100_000, (1 << 18) + 5 - 200_000], 20_000)
    s, e, ids, lengths = inst
    model_inst = pm.compact(s, e, ids, lengths)[:4]
    M, stages = 6, [2, 6]
    _, _, _, sets = pairs.staged(oracle, *model_inst, M, stages, fast=True)
    rest_span = (e.astype(np.int64) - s + 1)[~sets[0]]
    assert int(rest_span.max() - rest_span.min()).bit_length() + int(int(lengths.sum()) - 1).bit_length() > 32
    for cut_points in (-1, 1):
        with solver.options(cut_points=cut_points):
            (st, ps), _ = check_both_entries(pkg, solver, oracle, inst, M, stages, model_inst)
        assert ps.sweeps[1] == 1 and ps.n_selected[1] > 0


TWO_BATCH_LENGTHS = [1_200_000_000, 1_150_000_123, 5_000]


@functools.lru_cache(maxsize=None)
def two_batch_instance():
    inst = island_pairs(83, TWO_BATCH_LENGTHS, 300, per_island=40)
    return inst, pm.compact(*inst)[:4]


def test_two_position_batches_with_mates_across_them(pkg, solver, oracle):
    """two contigs of about 1.2e9 positions (one call takes 2^31 - 2) and a short third: contig 0 is a batch of its own,
    and most pairs have their mates in different batches, so stage 2 of the first batch needs the second batch's stage 1.
    Under cut_points = 1 (stretches): one chain per contig would walk 1.2e9 positions"""
    inst, model_inst = two_batch_instance()
    s, e, ids, lengths = inst
    L = lengths.astype(np.int64)
    assert int(L[:2].sum()) > (1 << 31) - 2 >= int(L[1:].sum())
    batch_of = (ids != 0).astype(np.int64)
    assert int(np.count_nonzero(batch_of[0::2] != batch_of[1::2])) > 50
    with solver.options(cut_points=1):
        (st, ps), (selected, kept) = check_both_entries(pkg, solver, oracle, inst, 5, None, model_inst)
    assert st.total_length == int(L.sum()) and st.n_contigs == 3
    assert ps.sweeps[1] == 2 and ps.n_selected[1] > 0


# ------------------------------------------------------------------------------------------ errors
def test_errors_come_back_before_anything_is_launched(pkg, solver, oracle):
    s = np.arange(10, dtype=np.uint32)
    e = s + 5
    ids = np.zeros(10, np.uint32)
    lengths = np.array([100], np.uint32)
    cases = [
        (s[:9], 5, None, QMCP_EINVAL, "odd"),
        (s, 5, [3, 2, 5], QMCP_EINVAL, "stages[1]"),
        (s, 5, [5, 3], QMCP_EINVAL, "stages[1]"),
        (s, 5, [2, 4], QMCP_EINVAL, "max_coverage"),
        (s, 17, list(range(1, 18)), QMCP_EINVAL, "n_stages 17"),
        (s, 2**31, [2**31], QMCP_ERANGE, "2^31"),
        (s, 2**31 - 1, [5, 2**31, 2**31 - 1], QMCP_ERANGE, "stages[1]"),
        (s, 2**31, None, QMCP_ERANGE, "2^31"),
        (s, 0, None, QMCP_EINVAL, "max_coverage"),
        (s, 5, [0, 5], QMCP_EINVAL, "stages[0]"),
    ]
    d_mask = torch.full((2,), -1, dtype=torch.int64, device="cuda:0")
    cols = [_dev(x) for x in (s, e, ids)]
    torch.cuda.synchronize()
    for starts, M, stages, code, word in cases:
        n = starts.size
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_pairs(starts, e[:n], ids[:n], lengths, M, stages)
        assert err.value.code == code and word in str(err.value), (M, stages, str(err.value))
        with pytest.raises(pkg.QmcpError) as err:
            solver.solve_pairs_device(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, lengths, M,
                                      d_mask.data_ptr(), stages)
        assert err.value.code == code and word in str(err.value)
    torch.cuda.synchronize()
    assert (d_mask.cpu().numpy() == -1).all()                           # the device mask was never touched
    # the context is still good
    got, _, ps = solver.solve_pairs(s, e, ids, lengths, 5)
    assert ps.n_stages == 2 and np.array_equal(got, pairs.staged(oracle, s, e, ids, lengths, 5)[0])


# ------------------------------------------------------------------------------------------ the file flow
def test_downsample_bam_pair_aware_writes_the_reads_of_the_final_mask(pkg, solver, oracle, tmp_path):
    """a multi-reference BAM (mates on other references, unmapped mates) through downsample_bam(pair_aware=True): the
    records written are those of the model's final mask -- whole pairs, with no further find_pairs -- under the default
    stages and under a list; every refused combination raises ValueError"""
    path = tmp_path / "in.bam"
    refs = [("chrA", 5000), ("chrB", 3000), ("chrC", 1200)]
    header, parsed, _ = mr.write_multi_reference_bam(path, np.random.default_rng(17), refs, 1500)
    cols = pkg.read_bam(path, per_reference=True)
    n = cols["starts"].size
    assert n % 2 == 0 and n > 2000
    M = 6
    plain_written = pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "plain.bam", M, per_reference=True)
    for stages in (None, [1, 2, 6]):
        want, _, kept, sets = pairs.staged(oracle, cols["starts"], cols["ends"], cols["contig_ids"], cols["contig_lengths"],
                                           M, stages, fast=True)
        assert pairs.whole_pairs(sets[-1]) and np.array_equal(oracle.find_pairs(want, n), want)
        kept_ids = np.sort(np.asarray(cols["bam_ids"], np.int64)[pkg.mask_to_indices(want, n).astype(np.int64)])
        out = tmp_path / "out.bam"
        written = pkg.downsample_bam("quasi-mcp-hip", path, out, M, per_reference=True, pair_aware=True, pair_stages=stages)
        oh, orecs, _ = bam_py.parse(out)
        assert oh == header and written == kept_ids.size == len(orecs) == kept[-1]
        assert [r["raw"] for r in orecs] == [parsed[i]["raw"] for i in kept_ids.tolist()]
        assert written < plain_written                                  # fewer records than solve + find_pairs writes
    bed = tmp_path / "t.bed"
    bed.write_text("chrA\t10\t500\n")
    graph = tmp_path / "caps.bedgraph"
    graph.write_text("chrA\t10\t500\t3\n")
    go = functools.partial(pkg.downsample_bam, "quasi-mcp-hip", path, tmp_path / "no.bam", M, pair_aware=True)
    refused = [dict(per_reference=False), dict(targets=bed), dict(profile=graph), dict(ladder=[3], ladder_out=tmp_path / "l{M}.bam"),
               dict(stratify="strand"), dict(dedup=True), dict(bed=bed, amplicons_by_reference=True), dict(tsv=bed),
               dict(report=tmp_path / "r.tsv"), dict(track=tmp_path / "t.bedgraph"),
               dict(pair_stages=[3, 5]), dict(pair_stages=[4, 2, 6]), dict(pair_stages=[])]
    for kw in refused:
        with pytest.raises(ValueError):
            go(**{"per_reference": True, **kw})
    with pytest.raises(ValueError):
        pkg.downsample_bam("quasi-mcp-hip-quality", path, tmp_path / "no.bam", M, per_reference=True, pair_aware=True)
    with pytest.raises(ValueError):
        pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "no.bam", M, per_reference=True, pair_stages=[3, 6])
    assert not (tmp_path / "no.bam").exists()
