"""hmm_trace_ppl_lds (trgt_amd/csrc/hmm_trace_ppl_lds.hpp) is the one constexpr function from which hmm_trace_ppl_kernel<G> carves a job's
LDS and its launcher sizes the launch.  It compiles without HIP, so its checker (tests/tools/hmm_trace_lds_check.cpp: pieces on 16-byte
boundaries, no overlap, each as large as its use, a job's carve-up inside its class's slot, the 64 / G jobs of a wave inside 64 KB) runs
here, on the host compiler.  No GPU needed."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_layout_builds_without_hip_and_the_checker_passes(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = os.path.join(str(tmp_path), "hmm_trace_lds_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "trgt_amd", "csrc"),
                        os.path.join(ROOT, "tests", "tools", "hmm_trace_lds_check.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.rstrip().endswith("hmm_trace_lds_check: all held")
    rows = {int(g): (int(a), int(b)) for g, a, b in re.findall(r"lds G=(\d+) largest_job=(\d+) wave=(\d+)", r.stdout)}
    # at most 2 KB per job of eight lanes -- ten one-wave workgroups per CU (160 KB) -- and fifteen workgroups of four jobs of sixteen
    assert rows[8][0] <= 2048 and 10 * rows[8][1] <= 160 * 1024 and 15 * rows[16][1] <= 160 * 1024


def test_lds_layout_header_includes_nothing():
    text = open(os.path.join(ROOT, "trgt_amd", "csrc", "hmm_trace_ppl_lds.hpp")).read()
    assert not re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
