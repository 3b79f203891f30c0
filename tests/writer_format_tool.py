"""tests/tools/writer_format_check.cpp -- the writer's per-locus formatting (trgt_amd/csrc/writer_format.hpp) on the host compiler --
built into a directory of the caller and run; tests/test_writer_format.py requires it to pass.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path):
    """(exit status, output) of the checker"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "writer_format_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "writer_format_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout
