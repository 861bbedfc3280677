"""downsample_bam's characterisation grid (tests/downsample_grid.py), the cases that end in an exception: each raises the
type and the message recorded in tests/golden/downsample_grid.json and writes nothing.  None of them gets as far as a
solve, so no GPU is needed.  Also: the request struct of the host bridge has the layout its C99 header gives it."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import downsample_grid as grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = json.load(open(os.path.join(ROOT, "tests", "golden", "downsample_grid.json")))
REFUSED = [combo for combo in grid.CASES if "error" in RECORD[grid.key_of(combo)]]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return grid.make_inputs(str(tmp_path_factory.mktemp("grid_inputs")))


def test_the_record_covers_the_grid():
    assert sorted(RECORD) == sorted(grid.key_of(combo) for combo in grid.CASES) and len(grid.CASES) == 178
    assert 100 < len(REFUSED) < len(grid.CASES)


@pytest.mark.parametrize("combo", REFUSED, ids=grid.key_of)
def test_a_refused_case_raises_what_it_raised_before(pkg, inputs, tmp_path, combo):
    assert grid.outcome(pkg, combo, inputs, str(tmp_path)) == RECORD[grid.key_of(combo)]


def test_request_layout_matches_the_header_which_is_c99(pkg, tmp_path):
    header = os.path.join(ROOT, "genome-downsampler_amd", "host", "include", "qmcp_host_request.h")
    body = re.search(r"typedef struct qmcp_host_downsample_request \{(.*?)\} qmcp_host_downsample_request;",
                     open(header).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    fields = [name for name, _ in pkg.DownsampleRequest._fields_]
    assert declared == fields and fields[0] == "struct_size"
    args = ", ".join(f"offsetof(qmcp_host_downsample_request, {f})" for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "qmcp_host_request.h"\nint main(void){ '
           f'size_t v[] = {{sizeof(qmcp_host_downsample_request), {args}}}; '
           'for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%zu ", v[i]); return 0; }\n')
    exe = tmp_path / "layout"
    out = subprocess.run(["gcc", "-std=c99", "-pedantic-errors", "-Wall", "-I", os.path.join(ROOT, "include"), "-I",
                          os.path.dirname(header), "-x", "c", "-", "-o", str(exe)], input=src, text=True, capture_output=True)
    assert out.returncode == 0, out.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = pkg.DownsampleRequest
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    # the one file-to-file entry of the host library
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.HOST_LIB_PATH], capture_output=True, text=True).stdout
    assert re.findall(r" T (qmcp_host_downsample_bam\w*)", nm) == ["qmcp_host_downsample_bam"]


def test_a_request_of_another_size_or_with_an_unknown_field_is_refused(pkg):
    with pytest.raises(KeyError):
        pkg._downsample_request(no_such_field=1)
    request = pkg._downsample_request(solver_name="quasi-mcp-hip", in_path="in.bam", out_path="out.bam", max_coverage=3)
    request.struct_size -= 4
    err = C.create_string_buffer(256)
    assert pkg._host.qmcp_host_downsample_bam(C.byref(request), None, 0, None, None, None, None, None, err, 256) == -4
    assert "struct_size" in err.value.decode()
    assert pkg._host.qmcp_host_downsample_bam(None, None, 0, None, None, None, None, None, err, 256) == -4
