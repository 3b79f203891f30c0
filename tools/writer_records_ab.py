"""A/B of the writer's records_device mode (trgt_writer_set_records_device, trgt_amd/csrc/bam_records_dev.hip) on the e2e workload of
bench.py: 4 000 loci, 30 reads of 6 kb, chunks of 1 000 loci, device ingestion, deflate_device, write-behind off and on.  Mode off (the
host formats the records: the baseline) and mode on alternate within one process, `--walks` walks each after a warm-up walk; a walk is
`--passes` passes over the chunks.  Printed: medians and the spread (min .. max) of
  (a) the writer alone (chunks ingested and genotyped beforehand): time of trgt_writer_write + close per chunk; from the writer's trace lines
      (synchronous writer only: the host path prints none with write-behind) its formatting and deflate + write parts,
  (b) the pipeline ingest | GPU | write: loci/s and the time the writing stage worked per chunk,
  (c) bytes the writer moved to and from the device per chunk.
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats (--only-writer keeps that run short).
Usage: python tools/writer_records_ab.py [--loci 4000] [--read-len 6000] [--walks 5] [--passes 3] [--only-writer]"""
import argparse
import collections
import itertools
import json
import os
import queue
import re
import statistics
import sys
import tempfile
import threading
import time
from concurrent.futures import ThreadPoolExecutor

os.environ["TRGT_WRITER_TRACE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trgt_amd import _lib, ingest, locus, synth_bam, writers  # noqa: E402

TRACE = re.compile(r"\[writer\] (\d+) loci.*?formatting ([\d.]+) ms \((.*?)\), deflate \+ write ([\d.]+) ms, link (\d+) B up / (\d+) B down")
ON_DEV = re.compile(r"on the device: ([\d.]+) ms")


class Stderr:
    """fd 2 into a file while a walk runs (the trace lines come from the library)"""
    def __init__(self, path):
        self.path = path

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        self.f = open(self.path, "w+")
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read()
        self.f.close()


def ordered(fn, callers, firsts):
    with ThreadPoolExecutor(callers) as ex:
        it, pend = iter(firsts), collections.deque()
        for a in itertools.islice(it, callers + 2):
            pend.append(ex.submit(fn, a))
        while pend:
            r = pend.popleft().result()
            nxt = next(it, None)
            if nxt is not None:
                pend.append(ex.submit(fn, nxt))
            yield r


def summary(v):
    return dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3), n=len(v))


def trace_figures(text, n_chunks):
    rows = [m for m in map(TRACE.search, text.splitlines()) if m]
    out = {}
    if rows:
        out["formatting_ms"] = sum(float(m.group(2)) for m in rows) / len(rows)
        out["deflate_write_ms"] = sum(float(m.group(4)) for m in rows) / len(rows)
        dev = [float(x) for x in ON_DEV.findall(text)]
        if dev:
            out["records_on_device_ms"] = sum(dev) / len(dev)
        out["h2d_bytes_per_chunk"] = int(rows[-1].group(5)) / n_chunks   # ("so far": the last line of a writer holds its totals)
        out["d2h_bytes_per_chunk"] = int(rows[-1].group(6)) / n_chunks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=4000)
    ap.add_argument("--read-len", type=int, default=6000)
    ap.add_argument("--walks", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--only-writer", action="store_true")
    args = ap.parse_args()
    chunk, dev = 1000, 0
    d = tempfile.mkdtemp(prefix="trgt_wab_")
    ds = synth_bam.write_dataset(d, n_loci=args.loci, read_len=args.read_len)
    rd = ingest.Reader(ds["bam"], ds["fasta"])
    ctx = _lib.Context(dev)
    params = locus.Params()
    firsts = list(range(0, args.loci, chunk))
    ing = lambda a: rd.batch(ds["bed"], first_locus=a, max_loci=chunk, keep_native=True, copy=False, read_names=False, threads=8, ingest_device=dev)
    gpu = lambda b: locus.run_batch(b, params, ctx, reads_dev=ingest.device_reads(b))
    batches = [ing(a) for a in firsts]
    outs = [gpu(b) for b in batches]
    n_chunks = len(firsts) * args.passes
    files = {}

    def writer(tag, mode, wb):
        return writers.Writer(rd, os.path.join(d, tag + ".vcf"), os.path.join(d, tag + ".bam"), deflate_device=dev, write_behind=wb, records_device=dev if mode else -1)

    def digest(tag):
        import hashlib
        return [hashlib.sha256(open(os.path.join(d, tag + e), "rb").read()).hexdigest() for e in (".vcf", ".bam")]

    def writer_walk(mode, wb):
        tag = "w%d%d" % (mode, wb)
        with Stderr(os.path.join(d, "trace.txt")) as cap:
            w = writer(tag, mode, wb)
            t0 = time.perf_counter()
            for _ in range(args.passes):
                for b, o in zip(batches, outs):
                    w.write(b, o)
            st = w.records_stats()
            w.close()
            dt = time.perf_counter() - t0
        files.setdefault((mode, wb), digest(tag))
        assert st["device_batches"] == (n_chunks if mode else 0) and st["host_batches"] == 0, st
        return dict(ms_per_chunk=1e3 * dt / n_chunks, **trace_figures(cap.text, n_chunks))

    def pipeline_walk(mode, wb):
        tag = "p%d%d" % (mode, wb)
        q1, q2, err = queue.Queue(3), queue.Queue(2), []
        busy = 0.0

        def stage_ingest():
            try:
                for b in ordered(ing, 3, firsts * args.passes):
                    q1.put(b)
            except BaseException as e:  # noqa: BLE001
                err.append(e)
            q1.put(None)

        def stage_gpu():
            try:
                while True:
                    b = q1.get()
                    if b is None:
                        break
                    q2.put((b, gpu(b)))
            except BaseException as e:  # noqa: BLE001
                err.append(e)
            q2.put(None)
        with Stderr(os.path.join(d, "trace.txt")) as cap:
            w = writer(tag, mode, wb)
            t0 = time.perf_counter()
            th = [threading.Thread(target=stage_ingest, daemon=True), threading.Thread(target=stage_gpu, daemon=True)]
            for t in th:
                t.start()
            while True:
                item = q2.get()
                if item is None:
                    break
                tb = time.perf_counter()
                w.write(*item)
                busy += time.perf_counter() - tb
            w.close()
            dt = time.perf_counter() - t0
            for t in th:
                t.join()
        if err:
            raise err[0]
        return dict(loci_per_s=args.loci * args.passes / dt, write_stage_ms_per_chunk=1e3 * busy / n_chunks, **trace_figures(cap.text, n_chunks))

    result = dict(workload="%d loci, 30 reads of %d bases, chunks of %d, device ingestion, deflate_device, %d walks of %d passes per setting" % (args.loci, args.read_len, chunk, args.walks, args.passes))
    for name, walk in (("writer_alone", writer_walk),) + (() if args.only_writer else (("pipeline", pipeline_walk),)):
        for wb in (0, 1):
            runs = {0: [], 1: []}
            for k in range(args.walks + 1):  # (walk 0 warms up: buffers, slabs, the page cache)
                for mode in (0, 1):
                    r = walk(mode, wb)
                    if k:
                        runs[mode].append(r)
            for mode in (0, 1):
                keys = sorted(set().union(*[r.keys() for r in runs[mode]]))
                result["%s write_behind=%d records_device=%s" % (name, wb, "on" if mode else "off")] = {k: summary([r[k] for r in runs[mode] if k in r]) for k in keys}
    same = all(files[(0, wb)] == files[(1, wb)] for wb in (0, 1))
    result["same_files"] = same
    for k, v in result.items():
        print("%s: %s" % (k, json.dumps(v)))
    if not same:
        raise SystemExit("writer_records_ab: the files differ between the modes")


if __name__ == "__main__":
    main()
