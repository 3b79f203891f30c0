"""Call time of trgt_plot_align_batch next to what a caller could do before it existed.

The batch: PANELS panels of 30 reads, flanks of 50 bases, alleles of about 600 bases over one or two motifs of a pathogenic catalog, reads
with 1 % substitutions and 0.5 % indels, a beta on every CpG-like tenth base.  Both modes on the same loci: mode 0 (allele plot) labels the
PANELS consensus sequences and aligns every read against its consensus; mode 1 (waterfall) labels the repeat part of every read and aligns
its two flanks.

Arms, alternating call by call on one context, blocking calls, host clock around each (every call ends in a synchronise inside the library):
  plot        trgt_plot_align_batch, host blobs, host outputs; its two kernels from trgt_plot_kernel_ms (HIP events inside the library)
  primitives  trgt_hmm_batch with state paths + trgt_wfa_batch with expanded operations, both read back to the host, on the SAME jobs: what
              a caller could run before, MINUS the conversion to segments and the projection of the betas, which it would still have to do
              on the host
Reported: median (min .. max) of REPEATS calls after WARMUP calls, per mode and arm, and the bytes each arm brings back.  No ratio is
claimed where the ranges overlap.  The lines are also written to the file named by the first argument (default:
profiles/plot_align_timing.txt).  PLOT_ALIGN_TIMING_PANELS=<n>: panels (default 200); PLOT_ALIGN_TIMING_REPEATS=<n>: calls per arm (default 15)."""
import ctypes as C
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from trgt_amd import _lib, hmm, plot  # noqa: E402

WARMUP = 3
MOTIF_SETS = [["CAG"], ["CAG", "CCG"], ["GGCCCC"], ["AAGGG", "AAAAG"], ["GAA"], ["CTG"], ["CCTG"], ["ATTCT"], ["GCN"], ["CGG"]]


def med(t):
    return "median %8.3f ms  (min %.3f .. max %.3f of %d)" % (statistics.median(t), min(t), max(t), len(t))


def edit(rng, seq, sub_rate=0.01, indel_rate=0.005):
    s = list(seq)
    for _ in range(int(len(s) * sub_rate + rng.random())):
        s[rng.randrange(len(s))] = rng.choice("ACGT")
    for _ in range(int(len(s) * indel_rate + rng.random())):
        i = rng.randrange(len(s))
        if rng.random() < 0.5:
            del s[i]
        else:
            s.insert(i, rng.choice("ACGT"))
    return "".join(s)


def make_panels(n_panels, mode, seed=20251021):
    rng = random.Random(seed)
    panels = []
    for p in range(n_panels):
        motifs = MOTIF_SETS[p % len(MOTIF_SETS)]
        lf, rf = "".join(rng.choice("ACGT") for _ in range(50)), "".join(rng.choice("ACGT") for _ in range(50))
        allele = ""
        while len(allele) < rng.randint(540, 660):
            allele += rng.choice(motifs).replace("N", rng.choice("ACGT")) * rng.randint(3, 40)
        allele = edit(rng, allele, 0.01, 0.003)
        reads = []
        for _ in range(30):
            seq = edit(rng, lf + allele + rf) if mode == 0 else lf + edit(rng, allele) + rf
            if mode == 1 and rng.random() < 0.3:
                seq = edit(rng, lf, 0.04, 0.0)[:50] + seq[50:]
            reads.append(dict(seq=seq, betas=[(q, 0.5) for q in range(3, len(seq), 10)]))
        panels.append(dict(motifs=motifs, lf=lf, rf=rf, ref=lf + allele + rf if mode == 0 else lf + rf, reads=reads))
    return panels


def primitives_jobs(mode, panels):
    """the HMM batch and the alignment batch of the same call, in the ABI layouts of trgt_hmm_batch / trgt_wfa_batch"""
    sets = [p["motifs"] for p in panels]
    hjobs, pats, txts = [], [], []
    for i, p in enumerate(panels):
        lf, rf = len(p["lf"]), len(p["rf"])
        if mode == 0:
            hjobs.append((i, p["ref"][lf:len(p["ref"]) - rf]))
        for r in p["reads"]:
            s = r["seq"]
            if mode == 0:
                pats.append(p["ref"]); txts.append(s)
            else:
                hjobs.append((i, s[lf:len(s) - rf]))
                pats += [p["lf"], p["rf"]]; txts += [s[:lf], s[len(s) - rf:]]
    hb = hmm.pack_hmm_batch(sets, [j for j in hjobs if j[1]])
    pats, txts = [x.encode() for x in pats], [x.encode() for x in txts]
    plen, tlen = np.array([len(x) for x in pats], np.uint32), np.array([len(x) for x in txts], np.uint32)
    blob = np.frombuffer(b"".join(pats) + b"".join(txts), np.uint8).copy()
    pat_off = np.zeros(len(pats), np.uint64)
    pat_off[1:] = np.cumsum(plen[:-1], dtype=np.uint64)
    txt_off = np.zeros(len(txts), np.uint64)
    txt_off[1:] = np.cumsum(tlen[:-1], dtype=np.uint64)
    txt_off += np.uint64(int(plen.sum()))
    ops_off = np.zeros(len(pats) + 1, np.uint64)
    ops_off[1:] = np.cumsum(plen.astype(np.uint64) + tlen, dtype=np.uint64)
    return hb, dict(seqs=blob, pat_off=pat_off, pat_len=plen, txt_off=txt_off, txt_len=tlen, ops_off=ops_off)


def main():
    import torch
    n_panels = int(os.environ.get("PLOT_ALIGN_TIMING_PANELS", "200"))
    repeats = max(5, int(os.environ.get("PLOT_ALIGN_TIMING_REPEATS", "15")))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "plot_align_timing.txt")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("python tools/plot_align_timing.py -- device: %s; %d calls per arm after %d warm-up calls, arms alternating" % (torch.cuda.get_device_name(0), repeats, WARMUP))
    L, p = _lib.lib(), _lib.ptr
    ctx = _lib.Context(0)
    ctx.timing_enable(True)
    for mode in (0, 1):
        panels = make_panels(n_panels, mode)
        b = plot.pack(mode, panels)
        outs = plot.alloc_outputs(b)
        hb, wb = primitives_jobs(mode, panels)
        nh, nw = len(hb["job_set"]), len(wb["pat_len"])
        say("mode %d (%s): %d panels x 30 reads, %.2f MB of read bases, reads of %d..%d bases; %d HMM jobs (%.2f M bases), %d alignments (%.2f M bases of pattern + text), %d betas" % (
            mode, "allele plot" if mode == 0 else "waterfall", n_panels, float(b["read_len"].sum()) / 1e6, int(b["read_len"].min()), int(b["read_len"].max()),
            nh, float(hb["seq_len"].sum()) / 1e6, nw, float(wb["pat_len"].sum() + wb["txt_len"].sum()) / 1e6, int(b["beta_begin"][-1])))
        # the primitives' outputs, allocated once
        h_path, h_plen = np.zeros(int(hb["path_off"][-1]), np.uint16), np.zeros(nh, np.uint32)
        h_nsp, h_cnt, h_pur = np.zeros(nh, np.uint32), np.zeros(int(hb["count_off"][-1]) + 1, np.uint32), np.zeros(nh, np.float64)
        w_status, w_score, w_ops, w_olen = np.zeros(nw, np.int32), np.zeros(nw, np.int32), np.zeros(int(wb["ops_off"][-1]) + 1, np.uint8), np.zeros(nw, np.uint32)
        wp = _lib.WfaParams()
        L.trgt_wfa_default_params(C.byref(wp))
        wp.metric, wp.mismatch, wp.gap_open1, wp.gap_ext1, wp.span, wp.scope, wp.memory_mode = 3, 2, 5, 1, 0, 1, 0

        def run_plot():
            plot.call(b, outs, ctx)

        def run_primitives():
            ctx.check(L.trgt_hmm_batch(ctx.handle, len(hb["set_motif_begin"]) - 1, p(hb["motif_blob"]), p(hb["motif_off"]), p(hb["set_motif_begin"]), nh, p(hb["job_set"]),
                                       p(hb["seq_blob"]), p(hb["seq_off"]), p(hb["seq_len"]), p(h_path), p(hb["path_off"]), p(h_plen), None, None, p(h_nsp), p(h_cnt),
                                       p(hb["count_off"]), p(h_pur), None, None))
            ctx.check(L.trgt_wfa_batch(ctx.handle, C.byref(wp), nw, p(wb["seqs"]), p(wb["pat_off"]), p(wb["pat_len"]), p(wb["txt_off"]), p(wb["txt_len"]), p(w_status), p(w_score),
                                       None, None, None, None, None, p(w_ops), p(wb["ops_off"]), p(w_olen)))

        arms = {"plot": run_plot, "primitives": run_primitives}
        times = {k: [] for k in arms}
        k0, k1 = [], []
        for i in range(WARMUP + repeats):
            for name, f in arms.items():
                t0 = time.perf_counter()
                f()
                t = (time.perf_counter() - t0) * 1e3
                if i >= WARMUP:
                    times[name].append(t)
                    if name == "plot":
                        ms = plot.kernel_ms(ctx)
                        k0.append(ms[0]); k1.append(ms[1])
        assert (w_status == 0).all()
        n_seg = int(outs["n_rseg"].sum()) + (int(outs["n_pseg"].sum()) if mode == 0 else 0)
        say("  trgt_plot_align_batch            %s   %d segments out; copied back: %.1f MB of segments (the used part of every slot), %.1f MB of projected betas" % (
            med(times["plot"]), n_seg, 8 * n_seg / 1e6, outs["beta_proj"].nbytes / 1e6))
        say("    plot_motif_segs_kernel         %s" % med(k0))
        say("    plot_read_segs_kernel          %s" % med(k1))
        say("  trgt_hmm_batch + trgt_wfa_batch  %s   copied back: %.1f MB of path slots, %.1f MB of operation slots; segments and betas still to do on the host" % (
            med(times["primitives"]), h_path.nbytes / 1e6, w_ops.nbytes / 1e6))
        a, c = times["plot"], times["primitives"]
        say("  the two ranges %s" % ("do not overlap" if max(a) < min(c) or max(c) < min(a) else "overlap: no difference is claimed"))
    ctx.close()
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
