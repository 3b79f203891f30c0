"""Timing of hmm_viterbi_big_kernel ("Large motif sets"): 512 alleles of one large motif set per trgt_hmm_batch call, kernel
time by the library's HIP events, the CPU oracle on the same jobs at 16 threads and (32 jobs, scaled) at one.  PERF_QUICK=1: GPU only
(for a run under rocprofv3 --kernel-trace --stats, or with a `make HMMPROF=1` library through TRGT_HIP_LIB).  Usage: hmm_big_perf.py [out.json]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import rand_dna, repeat_allele  # noqa: E402
from oracle import binding as orc  # noqa: E402
from trgt_amd import _lib, hmm as H  # noqa: E402

QUICK = os.environ.get("PERF_QUICK") == "1"
rng = np.random.default_rng(1)
res = {}
for name, motifs, alen in (("S2108_one_700b_motif", [rand_dna(rng, 700)], 2100), ("S1517_ten_50b_motifs", [rand_dna(rng, 50) for _ in range(10)], 1500)):
    sets = [motifs]
    jobs = [(0, repeat_allele(rng, motifs, alen, err=0.02)) for _ in range(512)]
    batch = H.pack_hmm_batch(sets, jobs)
    ctx = _lib.Context(0)
    L = _lib.lib()
    L.trgt_hip_timing_enable(ctx.handle, 1)
    H.hmm_batch(batch, ctx=ctx, want_path=False)  # warm-up
    ms_k, wall = [], []
    for _ in range(3):
        L.trgt_hip_timing_reset(ctx.handle)
        t0 = time.perf_counter(); got = H.hmm_batch(batch, ctx=ctx, want_path=False); wall.append((time.perf_counter() - t0) * 1e3)
        ms = C.c_double(); a = C.c_int64(); b = C.c_int64()
        L.trgt_hip_timing_get(ctx.handle, 2, C.byref(ms), C.byref(a), C.byref(b)); ms_k.append(ms.value)
    cols = float(np.mean(batch["seq_len"])) + 2
    if QUICK:
        print(name, "kernel ms", ms_k, "wall", wall, "cols", cols, flush=True); ctx.close(); continue
    t0 = time.perf_counter(); ref = orc.hmm_batch(batch, n_threads=16, want_path=False); o16 = (time.perf_counter() - t0) * 1e3
    sub = H.pack_hmm_batch(sets, jobs[:32])
    t0 = time.perf_counter(); orc.hmm_batch(sub, n_threads=1, want_path=False); o1 = (time.perf_counter() - t0) * 1e3 * 16
    assert np.array_equal(got["purity"].view(np.uint64), ref["purity"].view(np.uint64)) and np.array_equal(got["counts"], ref["counts"])
    res[name] = dict(jobs=512, states=H.num_states(motifs), mean_columns=cols, hmm_kernels_ms=ms_k, call_wall_ms=wall, oracle_16_threads_ms=o16,
                     oracle_1_thread_ms_scaled_from_32_jobs=o1, us_per_column_two_jobs_per_cu=min(ms_k) * 1e3 / 2 / cols)
    ctx.close()
    print(name, json.dumps(res[name]), flush=True)
if not QUICK:
    json.dump(res, open(sys.argv[1] if len(sys.argv) > 1 else "hmm_big_perf.json", "w"), indent=1)
