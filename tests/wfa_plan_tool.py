"""tests/tools/wfa_plan_check.cpp -- the launch plan of the alignment kernels (trgt_amd/csrc/wfa_plan.hpp) on the host compiler --
built into a directory of the caller and run; tests/test_wfa_plan.py requires it to pass, tests/test_wfa_launch_errors_gpu.py reads
the plans of its workspace-limit rows.  No GPU."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path):
    """(exit status, output) of the checker"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "wfa_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "wfa_plan_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def rows(output):
    """the "plan <row> key=value ..." lines: row -> dict of its integer fields (and `why`, the message of a refused plan)"""
    out = {}
    for line in output.splitlines():
        m = re.match(r"plan (\S+) (.*)$", line)
        if m:
            head, _, why = m.group(2).partition(" why=")
            out[m.group(1)] = dict({k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)(?= |$)", head)}, why=why)
    return out
