"""tests/tools/ingest_plan_check.cpp -- the plan of the device-side read ingestion (trgt_amd/csrc/ingest_plan.hpp) on the host compiler --
built into a directory of the caller and run; tests/test_ingest_plan.py requires it to pass.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path):
    """(exit status, output) of the checker"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "ingest_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "tools", "ingest_plan_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout
