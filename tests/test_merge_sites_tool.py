"""tests/tools/merge_sites_check.cpp -- the checks and the host twin of trgt_merge_sites_batch (trgt_amd/csrc/merge_sites_host.hpp) on three
literal inputs -- built stand-alone by the host compiler with the address and undefined-behaviour sanitizers and run as it is.  No GPU,
and nothing loaded into Python."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_twin_runs_clean_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "merge_sites_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "tools", "merge_sites_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.rstrip().splitlines()[-1] == "merge_sites_check: all held"


def test_the_host_header_includes_nothing_from_hip():
    csrc = os.path.join(ROOT, "trgt_amd", "csrc")
    for name, own in (("merge_sites_host.hpp", ["merge_host.hpp"]), ("merge_host.hpp", ["../../include/trgt_hip.h"])):
        with open(os.path.join(csrc, name)) as f:
            includes = re.findall(r'#include\s+([<"][^>"]+)[>"]', f.read())
        assert [i[1:] for i in includes if i[0] == '"'] == own, (name, includes)
        assert not [i for i in includes if "hip/" in i or i[1:] == "common.hpp"], (name, includes)
