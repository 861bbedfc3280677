"""The word layouts of genome-downsampler_amd/csrc/solve_words.h, compiled with g++ alone: the range-major host model
(tests/range_major_model.py) states the layout of `ranges` a second time on purpose, and the two must agree."""
import os
import subprocess

import range_major_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = r"""
#include <cstdio>
#include "solve_words.h"
int main() {
    using namespace qmcp::words;
    uint32_t ranges[1];
    std::printf("%u %u %u %td %td\n", (unsigned)kRangesWords, (unsigned)kMaxLoad, (unsigned)kSegTables,
                max_load(ranges) - ranges, seg_tables(ranges) - ranges);
    return 0;
}
"""


def test_the_model_and_the_header_agree_on_ranges(tmp_path):
    src = tmp_path / "words.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "words"
    out = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "genome-downsampler_amd", "csrc"), str(src),
                          "-o", str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    words = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert words == [model.RANGES_WORDS, model.MAX_LOAD_AT, model.SEG_TABLES_AT, model.MAX_LOAD_AT, model.SEG_TABLES_AT]
