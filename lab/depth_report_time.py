"""The depth report's time on cfg4's reads (10^8 shuffled over 8 contigs, mask from the plain by-contig solve,
n_bins = 256, without regions and with 776 of them) against the grouping stages of the plain by-contig solve:
runs tests/test_gpu_depth_report.py's timing test and keeps its figures in profiles/depth_report_time.json.
    python lab/depth_report_time.py [out.json]"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_report_time.json")
env = dict(os.environ, QMCP_DEPTH_TIME_OUT=out)
test = "tests/test_gpu_depth_report.py::test_a_report_costs_no_more_than_the_grouping_stages_of_the_plain_solve"
rc = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-s", test], cwd=ROOT, env=env).returncode
print(f"figures in {out}" if os.path.exists(out) else "no figures were written")
sys.exit(rc)
