"""The depth report without a device: the C ABI (header, exports, struct layout in C99), the refusals the host makes before
it looks at the context, window_regions, write_depth_report, and the position-batch plan (g++ only)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qmcp_hip_depth_report_host", "qmcp_hip_depth_report_device")


def _header():
    with open(os.path.join(ROOT, "include", "qmcp_hip.h")) as f:
        return f.read()


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint32_t|uint64_t|float)\s+([a-z_, ]+);", body)
    return [(n.strip(), t) for t, group in fields for n in group.split(",")]


def test_header_declares_the_entries_and_the_library_exports_them(pkg):
    header = _header()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg.ABI_SYMBOLS
        assert name in pkg.exported_symbols()
    ctype = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float}
    for struct, mirror in (("qmcp_hip_depth_row", pkg.DepthRow), ("qmcp_hip_depth_stats", pkg.DepthStats)):
        fields = _struct_fields(header, struct)
        assert [n for n, _ in fields] == [f for f, _ in mirror._fields_], struct
        assert [ctype[t] for _, t in fields] == [t for _, t in mirror._fields_], struct
    assert pkg.DEPTH_ROW_DTYPE.names == tuple(f for f, _ in pkg.DepthRow._fields_)
    assert [pkg.DEPTH_ROW_DTYPE.fields[f][1] for f, _ in pkg.DepthRow._fields_] == \
        [getattr(pkg.DepthRow, f).offset for f, _ in pkg.DepthRow._fields_]
    assert pkg.abi_version() == 5


def test_header_is_c99_and_the_struct_layouts_match(pkg, tmp_path):
    row = [f for f, _ in pkg.DepthRow._fields_]
    stats = [f for f, _ in pkg.DepthStats._fields_]
    prints = "".join('printf("%%zu\\n", offsetof(qmcp_hip_depth_row, %s));\n' % f for f in row) + \
        "".join('printf("%%zu\\n", offsetof(qmcp_hip_depth_stats, %s));\n' % f for f in stats)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\nint main(void){\n'
           'int (*h)(qmcp_hip_ctx*, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t, const uint32_t*, uint32_t, '
           'const uint64_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, '
           'qmcp_hip_depth_row*, qmcp_hip_depth_row*, uint64_t, uint64_t*, uint64_t*, uint64_t*, qmcp_hip_depth_stats*) = '
           'qmcp_hip_depth_report_host; (void)h;\n'
           'int (*d)(qmcp_hip_ctx*, const uint32_t*, const uint32_t*, const uint32_t*, uint64_t, const uint32_t*, uint32_t, '
           'const uint64_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, '
           'qmcp_hip_depth_row*, qmcp_hip_depth_row*, uint64_t, uint64_t*, uint64_t*, uint64_t*, void*, '
           'qmcp_hip_depth_stats*) = qmcp_hip_depth_report_device; (void)d;\n'
           'printf("%zu %zu\\n", sizeof(qmcp_hip_depth_row), sizeof(qmcp_hip_depth_stats));\n' + prints + 'return 0; }\n')
    exe = tmp_path / "depth_abi"
    lib = os.path.join(ROOT, "genome-downsampler_amd", "lib")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                          "-L", lib, "-lqmcp_hip", "-Wl,-rpath," + lib, "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True).stdout.split("\n")
    assert lines[0].split() == ["80", str(C.sizeof(pkg.DepthStats))] and C.sizeof(pkg.DepthRow) == 80
    offsets = [int(x) for x in lines[1:1 + len(row) + len(stats)]]
    assert offsets[:len(row)] == [getattr(pkg.DepthRow, f).offset for f in row]
    assert offsets[len(row):] == [getattr(pkg.DepthStats, f).offset for f in stats]
    # 7 x uint32 + a reserved one, then 6 x uint64: no implicit padding
    assert sum(C.sizeof(t) for _, t in pkg.DepthRow._fields_) == 80


PATTERN = 0xA5


def _call(pkg, ctx=None, n_bins=0, offs=None, t0=None, t1=None, capacity=8, with_region_rows=True, lengths=(50, 70)):
    """qmcp_hip_depth_report_host on three reads, every output pre-filled with a pattern -> (rc, message, untouched)"""
    u32 = lambda a: np.ascontiguousarray(a, np.uint32)
    s, e, ids, lengths = u32([1, 2, 3]), u32([9, 9, 9]), u32([0, 1, 0]), u32(lengths)
    contig_rows = np.full(lengths.size * 80, PATTERN, np.uint8)
    region_rows = np.full(8 * 80, PATTERN, np.uint8)
    hist_in, hist_kept = np.full(4096 * 8, PATTERN, np.uint8), np.full(4096 * 8, PATTERN, np.uint8)
    n_rows = np.full(8, PATTERN, np.uint8)
    stats = np.full(C.sizeof(pkg.DepthStats), PATTERN, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    p64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    p = pkg._p32
    rc = pkg._hip.qmcp_hip_depth_report_host(
        ctx, p(s), p(e), p(ids), 3, p(lengths), lengths.size, None, 5, None if offs is None else p(u32(offs)),
        None if t0 is None else p(u32(t0)), None if t1 is None else p(u32(t1)), 0, n_bins, vp(contig_rows),
        vp(region_rows) if with_region_rows else None, capacity, p64(n_rows), p64(hist_in), p64(hist_kept),
        C.cast(vp(stats), C.POINTER(pkg.DepthStats)))
    untouched = all(np.all(a == PATTERN) for a in (contig_rows, region_rows, hist_in, hist_kept, n_rows, stats))
    return rc, pkg._hip.qmcp_hip_last_error().decode(), untouched


def test_refusals_made_on_the_host_need_no_device_and_write_nothing(pkg):
    rc, msg, untouched = _call(pkg)                                               # everything fine but the context
    assert rc == pkg.QMCP_EINVAL and "null context" in msg and untouched
    rc, msg, untouched = _call(pkg, n_bins=4097)
    assert rc == pkg.QMCP_EINVAL and "n_bins 4097" in msg and untouched
    rc, msg, untouched = _call(pkg, n_bins=4096)                                  # the largest allowed: only the context is wrong
    assert rc == pkg.QMCP_EINVAL and "null context" in msg and untouched
    for offs in ([1, 1, 2], [0, 2, 1]):                                           # not from 0; decreasing
        rc, msg, untouched = _call(pkg, offs=offs, t0=[1, 2], t1=[3, 4])
        assert rc == pkg.QMCP_EINVAL and "target_offsets" in msg and untouched
    rc, msg, untouched = _call(pkg, offs=[0, 1, 2], t0=[5, 9], t1=[7, 8])         # start > end
    assert rc == pkg.QMCP_EINVAL and "start > end" in msg and untouched
    rc, msg, untouched = _call(pkg, offs=[0, 1, 2], t0=None, t1=None)
    assert rc == pkg.QMCP_EINVAL and "null target table" in msg and untouched
    # three regions of contig 0 merge into two; a capacity of one names the count needed
    regions = dict(offs=[0, 3, 3], t0=[1, 3, 20], t1=[4, 8, 22])
    rc, msg, untouched = _call(pkg, capacity=1, **regions)
    assert rc == pkg.QMCP_EINVAL and "2 merged regions" in msg and untouched
    rc, msg, untouched = _call(pkg, capacity=2, **regions)                        # enough: on to the context
    assert "null context" in msg and untouched
    rc, msg, untouched = _call(pkg, capacity=0, with_region_rows=False, **regions)  # no region rows asked for
    assert "null context" in msg and untouched
    rc, msg, untouched = _call(pkg, lengths=(50, 0xFFFFFFFF))                     # one contig beyond a position batch
    assert rc == pkg.QMCP_ERANGE and "contig 1" in msg and untouched


def test_window_regions_against_a_loop(pkg):
    rng = np.random.default_rng(2)
    for _ in range(60):
        lengths = [int(rng.integers(0, 90)) for _ in range(int(rng.integers(1, 6)))]
        size = int(rng.integers(1, 40))
        offs, t0, t1 = [0], [], []
        for L in lengths:
            for a in range(0, L, size):
                t0.append(a)
                t1.append(min(a + size, L) - 1)
            offs.append(len(t0))
        got = pkg.window_regions(lengths, size)
        assert all(g.dtype == np.uint32 for g in got)
        assert got[0].tolist() == offs and got[1].tolist() == t0 and got[2].tolist() == t1
    with pytest.raises(ValueError):
        pkg.window_regions([10], 0)


def test_write_depth_report_round_trips(pkg, tmp_path):
    rng = np.random.default_rng(9)
    names = ["chr1", "chr2", "chrM"]
    contig_rows = np.zeros(3, pkg.DEPTH_ROW_DTYPE)
    region_rows = np.zeros(4, pkg.DEPTH_ROW_DTYPE)
    for rows in (contig_rows, region_rows):
        for k in range(rows.size):
            a = int(rng.integers(0, 1000))
            b = a + int(rng.integers(0, 1000))
            rows[k] = (k % 3, a, b, 1, 900, 0, 40, 0, b - a + 1, int(rng.integers(0, 1 << 40)), int(rng.integers(0, 1 << 40)),
                       int(rng.integers(0, 99)), int(rng.integers(0, 99)), int(rng.integers(0, 1 << 33)))
    contig_rows[1] = (1,) + (0,) * 13                                              # a contig of length 0
    report = pkg.DepthReport(contig_rows, region_rows, np.array([5, 0, 7], np.uint64), np.array([9, 3, 0], np.uint64),
                             pkg.DepthStats())
    path = tmp_path / "depth.tsv"
    pkg.write_depth_report(path, report, names)
    lines = path.read_text().split("\n")
    assert lines[-1] == "" and lines[0] == "#" + "\t".join(pkg.DEPTH_REPORT_COLUMNS)
    assert lines[0].split("\t")[:7] == ["#kind", "reference", "start", "end", "positions", "mean_in", "mean_kept"]
    body = [ln.split("\t") for ln in lines[1:-1] if not ln.startswith("#")]
    assert len(body) == 7 and [b[0] for b in body] == ["contig"] * 3 + ["region"] * 4
    for b, r in zip(body, list(contig_rows) + list(region_rows)):
        pos = int(r["positions"])
        assert b[1] == names[int(r["contig"])] and int(b[2]) == int(r["start"]) and int(b[4]) == pos
        assert int(b[3]) - int(b[2]) == pos                                        # end exclusive
        for text, total in ((b[5], int(r["sum_in"])), (b[6], int(r["sum_kept"]))):
            assert re.fullmatch(r"\d+\.\d{6}", text)
            assert abs(float(text) - (total / pos if pos else 0.0)) <= 5e-7 * max(1.0, total / max(pos, 1))
        assert [int(x) for x in b[7:]] == [int(r[f]) for f in ("min_in", "max_in", "min_kept", "max_kept",
                                                              "capped_positions", "deficit_positions", "deficit_sum")]
    hist = [ln.split("\t") for ln in lines[1:-1] if ln.startswith("#hist")]
    assert [[int(x) for x in h[1:]] for h in hist] == [[0, 5, 9], [1, 0, 3], [2, 7, 0]]


@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("depth_plan") / "depth_plan_driver"
    out = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I",
                          os.path.join(ROOT, "genome-downsampler_amd", "csrc"),
                          os.path.join(ROOT, "tests", "cpp", "depth_plan_driver.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def _plan(exe, budget, lengths):
    out = subprocess.run([exe], input=f"{budget} {len(lengths)} " + " ".join(map(str, lengths)), capture_output=True,
                         text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().split("\n")
    rc, bad = map(int, lines[0].split())
    return rc, bad, [tuple(map(int, ln.split())) for ln in lines[1:]]


def test_position_batches(plan_driver):
    rng = np.random.default_rng(3)
    several = 0
    for _ in range(200):
        lengths = [int(rng.integers(0, 1000)) if rng.random() > 0.15 else 0 for _ in range(int(rng.integers(1, 40)))]
        budget = int(rng.integers(max(lengths + [1]), 4000))
        rc, _, batches = _plan(plan_driver, budget, lengths)
        assert rc == 0
        nxt = 0
        for first, count, positions in batches:                                    # every contig in exactly one batch
            assert first == nxt and count >= 1
            assert positions == sum(lengths[first:first + count]) <= budget
            nxt = first + count
        assert nxt == len(lengths)
        for (f0, c0, p0), (f1, _, _) in zip(batches, batches[1:]):                 # greedy: the next contig did not fit
            assert p0 + lengths[f1] > budget
        several += len(batches) > 1
    assert several > 100
    rc, bad, batches = _plan(plan_driver, 500, [100, 501, 3])                      # one contig over the budget
    assert rc == -3 and bad == 1 and batches == []
    # GRCh38's primary assembly under the default budget of 2^31 - 2 positions: two batches
    grch38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717,
              133797422, 135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616,
              64444167, 46709983, 50818468, 156040895, 57227415, 16569]
    rc, _, batches = _plan(plan_driver, 0, grch38)
    assert rc == 0 and len(batches) == 2 and sum(b[2] for b in batches) == sum(grch38) > 3_000_000_000


def test_a_report_of_the_file_flow_needs_per_reference(pkg, tmp_path):
    import bam_py
    path = tmp_path / "refs.bam"
    bam_py.write_bam(path, [("chr1", 5000), ("chr2", 3000)],
                     [bam_py.pack_record("p0", 0x41, 10, 30, [(50, "M")], 50, ref_id=0),
                      bam_py.pack_record("p0", 0x81, 100, 30, [(50, "M")], 50, ref_id=1)])
    with pytest.raises(ValueError, match="per_reference"):
        pkg.downsample_bam("quasi-mcp-hip", path, tmp_path / "out.bam", 10, report=tmp_path / "depth.tsv")
    assert not (tmp_path / "out.bam").exists() and not (tmp_path / "depth.tsv").exists()
    assert pkg.solver_names() == ["quasi-mcp-hip"]
    # the C++ mirror refuses the same configuration (BamApiConfig::depth_report_filepath without per_reference)
    import ctypes as C
    err = C.create_string_buffer(1024)
    request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path=path, out_path=tmp_path / "o.bam", max_coverage=10,
                                      amplicon_mode=-1, per_reference=0, amplicons_by_reference=0, target_padding=0,
                                      keep_off_target=0, report=tmp_path / "d.tsv", report_bins=0)
    n = pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 1024)
    assert n == -4 and "per_reference" in err.value.decode()
