"""csrc/pm_div.h -- the walk's division by the sweep's span as a multiply and a shift -- against the `/` operator, as a
stand-alone host program (tests/cpp/pm_div_check.cpp): every divisor 1 ... 512 at the multiples around 2^16, 2^24 and
2^31 - 1 and their neighbours, and 10^6 random dividends; once plain, once under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pm_div_check.cpp")
INC = os.path.join(ROOT, "genome-downsampler_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_quotients_equal_the_divide(flags, tmp_path):
    exe = str(tmp_path / "pm_div_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + INC, *flags, SRC, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    # 512 divisors x (2 bounds + three windows of multiples, three dividends each) and the random ones
    assert int(out.stdout.split()[-1]) > 1_000_000 + 512 * 2
