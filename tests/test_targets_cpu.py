"""On-target downsampling without a device: BED targets (parsing, half-open -> inclusive, name matching, errors), the
BamApiConfig rule that targets need per_reference, and the C ABI (header, C99, exports, struct layout)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bam_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("qmcp_hip_solve_targets_host", "qmcp_hip_solve_targets_device")
REFS = [("chr1", 5000), ("chr2", 3000), ("chrM", 800)]


def _bed(tmp_path, text, name="targets.bed"):
    path = tmp_path / name
    path.write_text(text)
    return path


def test_targets_from_bed(pkg, tmp_path):
    bed = _bed(tmp_path, "track name=panel\nbrowser position chr1:1-100\n# a comment\n\n"
                         "chr2\t100\t200\tprobe7\t0\t+\n"
                         "chr1\t0\t1\n"
                         "chr1 4000 5000 spaces-work-too\n"
                         "chr2\t150\t151\n")
    offs, t0, t1 = pkg.targets_from_bed(bed, [n for n, _ in REFS])
    assert offs.dtype == t0.dtype == t1.dtype == np.uint32
    assert offs.tolist() == [0, 2, 4, 4]                                  # chrM has none
    assert list(zip(t0.tolist(), t1.tolist())) == [(0, 0), (4000, 4999), (100, 199), (150, 150)]
    empty = pkg.targets_from_bed(_bed(tmp_path, "# nothing\n", "empty.bed"), ["a", "b"])
    assert empty[0].tolist() == [0, 0, 0] and empty[1].size == 0 and empty[2].size == 0


@pytest.mark.parametrize("text,needle", [
    ("chr3\t1\t2\n", "chr3"),                    # names no reference
    ("Chr1\t1\t2\n", "Chr1"),                    # names match exactly
    ("chr1\t5\n", "chrom, start and end"),
    ("chr1\tx\t9\n", "integers"),
    ("chr1\t9\t9\n", "empty"),                   # half-open [9, 9) holds nothing
    ("chr1\t9\t3\n", "empty"),
])
def test_targets_from_bed_errors(pkg, tmp_path, text, needle):
    with pytest.raises(ValueError) as ex:
        pkg.targets_from_bed(_bed(tmp_path, "chr1\t1\t5\n" + text), [n for n, _ in REFS])
    assert needle in str(ex.value) and ":2:" in str(ex.value)


def _bam(tmp_path):
    path = tmp_path / "refs.bam"
    recs = [bam_py.pack_record("p0", 0x41, 10, 30, [(50, "M")], 50, ref_id=0),
            bam_py.pack_record("p0", 0x81, 100, 30, [(50, "M")], 50, ref_id=1)]
    bam_py.write_bam(path, REFS, recs)
    return path


def test_bam_api_config_targets_need_per_reference(pkg, tmp_path):
    bam = _bam(tmp_path)
    bed = _bed(tmp_path, "track x\nchr2\t100\t200\nchr1\t0\t10\tname\n")
    assert pkg.check_targets_config(bam, bed, per_reference=True, target_padding=5) == 2
    assert pkg.check_targets_config(bam, None, per_reference=False) == 0
    with pytest.raises(ValueError, match="per_reference"):
        pkg.check_targets_config(bam, bed, per_reference=False)
    with pytest.raises(ValueError, match="chrX"):
        pkg.check_targets_config(bam, _bed(tmp_path, "chrX\t1\t2\n", "x.bed"), per_reference=True)
    with pytest.raises(ValueError, match="integers"):
        pkg.check_targets_config(bam, _bed(tmp_path, "chr1\t1\tq\n", "q.bed"), per_reference=True)
    with pytest.raises(ValueError, match="could not open"):
        pkg.check_targets_config(bam, tmp_path / "missing.bed", per_reference=True)
    # downsample_bam refuses the same configuration before it touches a solver
    with pytest.raises(ValueError, match="per_reference"):
        pkg.downsample_bam("quasi-mcp-hip", bam, tmp_path / "out.bam", 10, targets=bed)


def test_header_declares_the_target_entries_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "qmcp_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in pkg.ABI_SYMBOLS
        assert name in pkg.exported_symbols()
    assert re.search(r"#define\s+QMCP_TARGETS_KEEP_OFF_TARGET\s+1u", header)
    assert pkg.TARGETS_KEEP_OFF_TARGET == 1
    body = re.search(r"typedef struct qmcp_hip_target_stats \{(.*?)\} qmcp_hip_target_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(uint32_t|uint64_t|float)\s+([a-z_, ]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [f for f, _ in pkg.TargetStats._fields_]
    assert pkg.abi_version() == 5


def test_header_with_the_target_entries_is_c99_and_the_struct_layout_matches(pkg, tmp_path):
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_hip.h"\n'
           'int main(void){ int (*h)(qmcp_hip_ctx*, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, '
           'uint64_t, const uint32_t*, uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t, uint32_t, '
           'uint32_t, uint64_t*, qmcp_hip_stats*, qmcp_hip_target_stats*) = qmcp_hip_solve_targets_host; (void)h;\n'
           'printf("%zu %zu %zu %u\\n", sizeof(qmcp_hip_target_stats), offsetof(qmcp_hip_target_stats, regions_in), '
           'offsetof(qmcp_hip_target_stats, ms_targets), QMCP_TARGETS_KEEP_OFF_TARGET); return 0; }\n')
    exe = tmp_path / "target_abi"
    lib = os.path.join(ROOT, "genome-downsampler_amd", "lib")
    out = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-",
                          "-L", lib, "-lqmcp_hip", "-Wl,-rpath," + lib, "-o", str(exe)],
                         input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    size, off_regions, off_ms, flag = map(int, subprocess.run([str(exe)], capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(pkg.TargetStats) == 40
    assert off_regions == pkg.TargetStats.regions_in.offset and off_ms == pkg.TargetStats.ms_targets.offset
    assert flag == 1
