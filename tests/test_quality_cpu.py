"""quasi-mcp-hip-quality without a device: the contract's model against a literal greedy with the four-key order, the
C ABI surface of the quality entries, and the host's solver lookup (no solve: without a device the adapter ends in
std::terminate, as the reference's GPU solver does)."""
import ctypes as C
import os
import re

import numpy as np

import quality_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qmcp_hip_solve_quality_host", "qmcp_hip_solve_quality_device", "qmcp_hip_solve_quality_by_contig_host")


def _instance(rng):
    n_contigs = int(rng.integers(1, 4))
    lengths = rng.integers(5, 40, size=n_contigs)
    ss, ee, counts = [], [], []
    mixed = rng.random() < 0.6
    for L in lengths.tolist():
        k = int(rng.integers(0, 60))
        span = rng.integers(1, min(8, L) + 1, size=k) if mixed else np.full(k, min(int(rng.integers(1, 6)), L))
        s = (rng.random(k) * (L - span + 1)).astype(np.int64)
        ss.append(s)
        ee.append(s + span - 1)
        counts.append(k)
    s = np.concatenate(ss).astype(np.uint32)
    e = np.concatenate(ee).astype(np.uint32)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    kind = rng.random()
    if kind < 0.15:
        q = np.full(s.size, int(rng.integers(0, 61)), np.uint32)          # all equal
    elif kind < 0.5:
        q = rng.integers(0, 3, size=s.size).astype(np.uint32)              # many ties
    else:
        q = rng.integers(0, 61, size=s.size).astype(np.uint32)
    return s, e, q, lengths.astype(np.uint32), offs, int(rng.integers(1, 9))


def test_greedy_with_quality_equals_the_model_of_the_plain_selection(oracle):
    rng = np.random.default_rng(2024)
    changed = 0
    for trial in range(300):
        s, e, q, lengths, offs, M = _instance(rng)
        plain = oracle.solve(s, e, lengths, M, contig_read_offsets=offs)
        model = qm.quality_choice(plain, s, e, qm.contig_of(offs, s.size), q)
        greedy = qm.greedy_quality_multi(s, e, lengths, offs, M, q)
        assert np.array_equal(model, greedy), f"trial {trial}"
        # same coverage and count as the plain mask; all-equal qualities change nothing
        n = s.size
        kp, kq = qm.bits_of(plain, n), qm.bits_of(model, n)
        assert kp.sum() == kq.sum()
        for k in range(lengths.size):
            a, b = int(offs[k]), int(offs[k + 1])
            L = int(lengths[k])
            assert np.array_equal(oracle.cover(s[a:b], e[a:b], L, keep_mask=qm.mask_of(kp[a:b])),
                                  oracle.cover(s[a:b], e[a:b], L, keep_mask=qm.mask_of(kq[a:b])))
        if np.unique(q).size <= 1:
            assert np.array_equal(model, plain)
        changed += int(not np.array_equal(model, plain))
    assert changed > 50


def test_model_keeps_the_best_reads_of_every_cell():
    # one cell of five reads, two kept: the two best qualities, the earlier index on a tie
    s = np.zeros(5, np.uint32)
    e = np.full(5, 9, np.uint32)
    q = np.array([3, 60, 7, 60, 59], np.uint32)
    plain = qm.mask_of(np.array([1, 1, 0, 0, 0], bool))
    assert qm.bits_of(qm.quality_choice(plain, s, e, None, q), 5).tolist() == [False, True, False, True, False]


def test_header_declares_the_quality_entries_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "qmcp_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg.ABI_SYMBOLS
        assert name in pkg.exported_symbols()
    body = re.search(r"typedef struct qmcp_hip_quality_stats \{(.*?)\} qmcp_hip_quality_stats;", header, re.S).group(1)
    fields = re.findall(r"\b(uint32_t|uint64_t|float)\s+([a-z_, ]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [f for f, _ in pkg.QualityStats._fields_]
    assert C.sizeof(pkg.QualityStats) == 40
    assert "#define QMCP_HIP_ABI_VERSION 5" in header


def test_solver_lookup_on_the_host(pkg):
    assert pkg.solver_uses_quality("quasi-mcp-hip-quality") is True
    assert pkg.solver_uses_quality("quasi-mcp-hip") is False
    assert pkg.solver_uses_quality("qmcp-cpu") is None
    assert pkg.solver_names() == ["quasi-mcp-hip"]


def test_quality_entries_check_qualities_first(pkg):
    # NULL qualities are refused before the context is looked at (so before any device call): the message names the
    # qualities even with a null context; with qualities given, the null context is what is refused
    q = np.zeros(4, np.uint32)
    for call in (lambda qp: pkg._hip.qmcp_hip_solve_quality_host(None, None, None, qp, 0, None, None, 0, 0, None, None,
                                                                 None),
                 lambda qp: pkg._hip.qmcp_hip_solve_quality_device(None, None, None, qp, 0, None, None, 0, 0, None,
                                                                   None, None, None),
                 lambda qp: pkg._hip.qmcp_hip_solve_quality_by_contig_host(None, None, None, None, qp, 0, None, 0, 0,
                                                                           None, None, None)):
        assert call(None) == pkg.QMCP_EINVAL
        assert "qualities" in pkg._hip.qmcp_hip_last_error().decode()
        assert call(pkg._p32(q)) == pkg.QMCP_EINVAL
        assert "null context" in pkg._hip.qmcp_hip_last_error().decode()
