"""Recorded side-by-side runs of the REAL reference (this container only): re-runs the reference's side of
tests/test_mirror_vs_live_reference.py, test_oracle.py::test_oracle_vs_live_reference and
test_sophia.py::test_sophiag_side_by_side_with_live_reference live (through ``ref_shim``)
and stores every result those tests compare against.

    python tests/golden/make_golden_live.py       # writes tests/golden/live_{mirror,oracle,sophia}.npz   (data only)
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    env = dict(os.environ, USFLOWS_RECORD_LIVE="1")
    cmd = [sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", "tests/test_mirror_vs_live_reference.py",
           "tests/test_oracle.py::test_oracle_vs_live_reference", "tests/test_sophia.py::test_sophiag_side_by_side_with_live_reference"]
    sys.exit(subprocess.run(cmd, cwd=ROOT, env=env).returncode)


if __name__ == "__main__":
    main()
