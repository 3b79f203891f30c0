"""Host-side mirror of what `trgt merge` computes per site between reading N records and writing one, over the batch ABI
trgt_merge_exact_batch / trgt_merge_exact_host (include/trgt_hip_merge.h).

Reference (PacificBiosciences/trgt v3.0.0):
  merge_exact   src/merge/strategy/exact.rs:6-88   -> merge_exact(vcf_gts, sample_alleles)   one site, the reference's signature
                                                      exact_batch(sites)                      many sites in one call
The de-duplication, the (length, bytes) order and the rewriting of the GT indices run in trgt_merge_exact_batch
(trgt_amd/csrc/merge_exact.hip) when a context is given and in its host twin trgt_merge_exact_host otherwise; this module only packs
batches and unpacks results.

  merge_variants / merge_variant   src/merge/vcf_processor.rs:237-299, 350-415, 452-532, 570-656
                                                   -> sites_batch(files)    the sites of one contig, the padding of pre-1.0 files, the
                                                                            entries with their dense FORMAT rows, the template records
                                                      merge_contig(files)   ... chained into merge_exact: what merge_variant writes per site
over trgt_merge_sites_batch / trgt_merge_sites_host (include/trgt_hip_merge_sites.h, trgt_amd/csrc/merge_sites.hip).  Reading the VCFs,
header merging, the FORMAT strings themselves, skip_n / process_n and writing stay with the caller.

Genotype values.  exact_batch takes and returns them in BCF encoding (ints): (i + 1) << 1 Unphased(i), ((i + 1) << 1) | 1 Phased(i), 0
UnphasedMissing, 1 PhasedMissing, VECTOR_END passed through.  merge_exact takes GenotypeAllele as tuples: ("U", i) Unphased(i), ("P", i)
Phased(i), ("U", None) UnphasedMissing, ("P", None) PhasedMissing.
"""
import ctypes as C

import numpy as np

from . import _lib

VECTOR_END = -2147483647   # TRGT_MERGE_GT_VECTOR_END, bcf_int32_vector_end
REF_MISMATCH, NO_REF, GT_OUT_OF_RANGE = 1, 2, 3   # site_status
_VP = C.c_void_p
_NEGATIVE = (1 << 29)      # merge_exact: the index a negative GenotypeAllele index is sent as (beyond every entry, so the site gets status 3)


class MergeIn(C.Structure):  # trgt_merge_in, include/trgt_hip_merge.h
    _fields_ = [("n_sites", C.c_int64), ("site_entry_begin", _VP), ("entry_allele_begin", _VP), ("allele_off", _VP), ("allele_len", _VP),
                ("allele_blob", _VP), ("blob_len", C.c_uint64), ("entry_gt_begin", _VP), ("gt", _VP)]


class MergeOut(C.Structure):  # trgt_merge_out
    _fields_ = [(n, _VP) for n in ("site_status", "out_n_alleles", "out_allele_src", "out_allele_begin", "allele_map", "gt_out")]


def _b(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def site_alleles_limit():
    """trgt_merge_site_alleles_limit: the largest site (input alleles) the device takes; larger ones go to the host twin (no GPU needed)"""
    return int(_lib.lib().trgt_merge_site_alleles_limit())


def kernel_ms(ctx=None):
    """trgt_merge_kernel_ms: (merge_hash_kernel, merge_site_kernel) of the context's last timed call, in ms"""
    ctx = ctx or _lib.context()
    out = (C.c_double * 2)()
    ctx.check(_lib.lib().trgt_merge_kernel_ms(ctx.handle, out))
    return float(out[0]), float(out[1])


def gt_encode(g):
    """("U" | "P", index or None) -> the BCF value"""
    kind, i = g
    phased = 1 if kind == "P" else 0
    if i is None:
        return phased
    return ((min(int(i), _NEGATIVE) if i >= 0 else _NEGATIVE) + 1) << 1 | phased


def gt_decode(v):
    v = int(v)
    return ("P" if v & 1 else "U", None if v < 2 else (v >> 1) - 1)


def pack(sites, pad=(0,)):
    """sites: [(entries_alleles, entries_gts)] -- per entry the list of its alleles (bytes or str, REF first; [] for a file without a record
    there) and the flat list of its genotype values (ints) -> the ABI arrays (host).  The alleles lie in the blob in input order; allele k
    is preceded by pad[k % len(pad)] filler bytes (tests move sequences across dword boundaries with it).  Every site gets the slot it
    needs: 1 + its ALT alleles, at least 2."""
    seb, eab, egb, slot = [0], [0], [0], [0]
    seqs, gts = [], []
    for alleles, egts in sites:
        assert len(alleles) == len(egts), "one list of genotype values per entry"
        n_alt = 0
        for al, g in zip(alleles, egts):
            seqs.extend(_b(a) for a in al)
            gts.extend(int(v) for v in g)
            eab.append(len(seqs))
            egb.append(len(gts))
            n_alt += max(len(al) - 1, 0)
        seb.append(len(eab) - 1)
        slot.append(slot[-1] + max(1 + n_alt, 2))
    off, pieces, at = [], [], 0
    for k, s in enumerate(seqs):
        p = int(pad[k % len(pad)])
        pieces.append(b"N" * p)
        at += p
        off.append(at)
        pieces.append(s)
        at += len(s)
    blob = b"".join(pieces)
    u64 = lambda v: np.array(v, np.uint64)  # noqa: E731
    return dict(n_sites=len(sites), site_entry_begin=u64(seb), entry_allele_begin=u64(eab), entry_gt_begin=u64(egb), out_allele_begin=u64(slot),
                allele_off=u64(off + [0])[:max(len(off), 1)], allele_len=np.array([len(s) for s in seqs] + [0], np.uint32)[:max(len(seqs), 1)],
                allele_blob=np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(1, np.uint8), blob_len=len(blob),
                gt=np.array(gts + [0], np.int32)[:max(len(gts), 1)], n_alleles=len(seqs), n_gt=len(gts), seqs=seqs)


OUT_NAMES = ("site_status", "out_n_alleles", "out_allele_src", "allele_map", "gt_out")


def alloc_outputs(b, fill=0):
    """host output arrays of a packed batch, pre-filled with `fill` (a byte)"""
    def arr(n):
        a = np.empty(max(int(n), 1), np.int32)
        a.view(np.uint8)[:] = fill
        return a
    return dict(site_status=arr(b["n_sites"]), out_n_alleles=arr(b["n_sites"]), out_allele_src=arr(b["out_allele_begin"][-1]),
                allele_map=arr(b["n_alleles"]), gt_out=arr(b["n_gt"]))


def call(b, outs, ctx=None, blob=None, check=True):
    """trgt_merge_exact_batch (ctx given) or trgt_merge_exact_host (ctx None) on a packed batch.  blob: a torch uint8 tensor already in
    HBM, instead of the host blob; outs: host arrays or HBM tensors per output name.  Returns the return code (raises unless check=False)."""
    p = _lib.ptr
    cin = MergeIn(b["n_sites"], p(b["site_entry_begin"]), p(b["entry_allele_begin"]), p(b["allele_off"]), p(b["allele_len"]),
                  p(blob if blob is not None else b["allele_blob"]), b["blob_len"], p(b["entry_gt_begin"]), p(b["gt"]))
    cout = MergeOut(p(outs.get("site_status")), p(outs.get("out_n_alleles")), p(outs.get("out_allele_src")), p(b["out_allele_begin"]),
                    p(outs.get("allele_map")), p(outs.get("gt_out")))
    L = _lib.lib()
    if ctx is None:
        rc = L.trgt_merge_exact_host(C.byref(cin), C.byref(cout))
        if rc != 0 and check:
            raise _lib.TrgtHipError("libtrgt_hip error %d: %s" % (rc, L.trgt_hip_last_error(None).decode()))
        return rc
    rc = L.trgt_merge_exact_batch(ctx.handle, C.byref(cin), C.byref(cout))
    if check:
        ctx.check(rc)
    return rc


def unpack(b, outs):
    """-> per site (status, alleles, gts): the merged alleles as bytes in output order (status 1: the two REFs that differ; 2, 3: []) and per
    entry the rewritten genotype values (None for a site with a status)"""
    res = []
    seb, eab, egb, slot = b["site_entry_begin"], b["entry_allele_begin"], b["entry_gt_begin"], b["out_allele_begin"]
    for s in range(b["n_sites"]):
        status = int(outs["site_status"][s])
        n = 2 if status == REF_MISMATCH else int(outs["out_n_alleles"][s])
        alleles = [b["seqs"][int(a)] for a in outs["out_allele_src"][int(slot[s]):int(slot[s]) + n]]
        gts = None
        if status == 0:
            gts = [[int(v) for v in outs["gt_out"][int(egb[e]):int(egb[e + 1])]] for e in range(int(seb[s]), int(seb[s + 1]))]
        res.append((status, alleles, gts))
    return res


def exact_batch(sites, ctx=None):
    """merge_exact for every site of `sites` (see pack) in one call: on the device of `ctx`, or by the host twin when ctx is None.
    Returns per site (status, alleles, gts) (see unpack); a site's status never fails the call."""
    if not sites:
        return []
    b = pack(sites)
    outs = alloc_outputs(b)
    call(b, outs, ctx)
    return unpack(b, outs)


def merge_exact(vcf_gts, sample_alleles, ctx=None):
    """merge_exact, exact.rs:6-88, for one site.  vcf_gts[i][sample] is the list of GenotypeAllele tuples of one sample of input i,
    sample_alleles[i] the alleles of input i (REF first, [] when the file has no record).  Returns (out_gts, sorted_alleles); raises
    ValueError with the reference's message where the reference returns Err."""
    flat = [[gt_encode(g) for sample in entry for g in sample] for entry in vcf_gts]
    status, alleles, gts = exact_batch([(list(sample_alleles), flat)], ctx)[0]
    if status == REF_MISMATCH:
        raise ValueError("Reference alleles do not match: '%s' and '%s'" % tuple(a.decode("utf-8", "replace") for a in alleles))
    if status == NO_REF:
        raise ValueError("No reference allele found")
    if status == GT_OUT_OF_RANGE:
        for entry, al in zip(vcf_gts, sample_alleles):
            for sample in entry:
                for _, i in sample:
                    if i is not None and i < 0:
                        raise ValueError("Index out of range: %d" % i)
                    if i is not None and i >= len(al):
                        raise ValueError("Index out of bounds or allele not found in index: None")
    out, k = [], 0
    for entry, vals in zip(vcf_gts, gts):
        k = 0
        samples = []
        for sample in entry:
            samples.append([gt_decode(v) for v in vals[k:k + len(sample)]])
            k += len(sample)
        out.append(samples)
    return out, alleles


# ---- sites, padding and FORMAT rows of one contig: trgt_merge_sites_batch / trgt_merge_sites_host (include/trgt_hip_merge_sites.h) ----

SITE_RAGGED = 4                                   # TRGT_MERGE_SITE_RAGGED
ERR_INVALID, ERR_UNSUPPORTED, ERR_NOMEM = -1, -3, -5   # TRGT_ERR_*: what the sizing protocol and the call errors return
MISSING_INTEGER = -2147483648                     # vcf_processor.rs:24-27
MISSING_FLOAT, VECTOR_END_FLOAT = 0x7F800001, 0x7F800002
FIELDS = ("gt", "AL", "SD", "AP", "AM")           # the five numeric fields of a record, in the order of trgt_merge_sites_in


class MergeField(C.Structure):  # trgt_merge_field
    _fields_ = [("width", _VP), ("begin", _VP), ("values", _VP)]


class MergeSitesIn(C.Structure):  # trgt_merge_sites_in
    _fields_ = [("n_files", C.c_int32), ("n_samples", _VP), ("pre_v1", _VP), ("am_is_int", _VP), ("file_record_begin", _VP), ("pos", _VP), ("pad_base", _VP),
                ("record_allele_begin", _VP), ("allele_off", _VP), ("allele_len", _VP), ("allele_blob", _VP), ("blob_len", C.c_uint64)] + [(n, MergeField) for n in ("gt", "al", "sd", "ap", "am")]


class MergeSitesOut(C.Structure):  # trgt_merge_sites_out
    _fields_ = [("cap_sites", C.c_int64), ("n_sites", C.c_int64)] + \
        [(n, _VP) for n in ("record_site", "site_pos", "site_template", "site_stage_status", "entry_record", "site_entry_begin", "entry_allele_begin", "allele_off", "allele_len",
                            "allele_src", "entry_gt_begin", "gt", "allele_blob")] + [("blob_cap", C.c_uint64), ("blob_written", C.c_uint64)] + [(n, _VP) for n in ("al", "sd", "ap", "am", "sample_src")]


def f32_bits(x):
    """the value of a float field as the 32-bit pattern the ABI moves: a float is rounded to float32, an int IS the pattern (NaN payloads)"""
    if isinstance(x, (int, np.integer)):
        return int(x) & 0xFFFFFFFF
    return int(np.array([x], np.float32).view(np.uint32)[0])


def sites_kernel_ms(ctx=None):
    """trgt_merge_sites_kernel_ms: (grouping, fill, blob copy) of the context's last timed trgt_merge_sites_batch, in ms"""
    ctx = ctx or _lib.context()
    out = (C.c_double * 3)()
    ctx.check(_lib.lib().trgt_merge_sites_kernel_ms(ctx.handle, out))
    return tuple(float(v) for v in out)


def pack_sites(files, pad=(0,)):
    """files: one dict per input VCF -- n_samples, pre_v1, am_is_int, records -- with the records of one contig in file order; a record is a
    dict of pos, alleles (bytes or str, REF first), pad_base (a byte: int, bytes or str; read for pre_v1 files) and the per-sample lists gt
    (BCF-encoded ints), AL, SD (ints), AP (floats, or ints as bit patterns) and AM (the same; ints as VALUES in a file with am_is_int).
    A field's width in a record is its longest sample list (at least 1); shorter lists are filled up with vector end, as BCF does, and
    a list may spell vector end itself.  -> the ABI arrays (host).  pad: filler bytes in front of allele k in the blob, as in pack."""
    nf = len(files)
    frb, rab, pos, pad_base, seqs = [0], [0], [], [], []
    fld = {k: ([], [0], []) for k in FIELDS}
    for f in files:
        for r in f["records"]:
            pos.append(int(r["pos"]))
            pb = r.get("pad_base", 0)
            pad_base.append(pb if isinstance(pb, int) else _b(pb)[0])
            seqs.extend(_b(a) for a in r["alleles"])
            rab.append(len(seqs))
            for k in FIELDS:
                width, begin, values = fld[k]
                samples = r[k]
                assert len(samples) == f["n_samples"], "one list per sample in %s" % k
                is_int = k in ("gt", "AL", "SD") or (k == "AM" and f["am_is_int"])
                end = (VECTOR_END & 0xFFFFFFFF) if is_int else VECTOR_END_FLOAT
                w = r.get("width", {}).get(k, max([1] + [len(s) for s in samples]))
                for s in samples:
                    values.extend([(int(v) & 0xFFFFFFFF) if is_int else f32_bits(v) for v in s] + [end] * (w - len(s)))
                width.append(w)
                begin.append(len(values))
        frb.append(len(pos))
    off, pieces, at = [], [], 0
    for k, s in enumerate(seqs):
        p = int(pad[k % len(pad)])
        pieces.append(b"N" * p)
        at += p
        off.append(at)
        pieces.append(s)
        at += len(s)
    blob = b"".join(pieces)
    one = lambda v, t: np.array(list(v) + [0], t)[:max(len(v), 1)]  # noqa: E731  (never an empty array: its pointer is read)
    b = dict(n_files=nf, n_samples=one([f["n_samples"] for f in files], np.int32), pre_v1=one([int(bool(f["pre_v1"])) for f in files], np.uint8),
             am_is_int=one([int(bool(f["am_is_int"])) for f in files], np.uint8), file_record_begin=np.array(frb, np.uint64), pos=one(pos, np.int64),
             pad_base=one(pad_base, np.uint8), record_allele_begin=np.array(rab, np.uint64), allele_off=one(off, np.uint64), allele_len=one([len(s) for s in seqs], np.uint32),
             allele_blob=np.frombuffer(blob, np.uint8).copy() if blob else np.zeros(1, np.uint8), blob_len=len(blob), n_records=len(pos), n_alleles=len(seqs),
             S=sum(f["n_samples"] for f in files), seqs=seqs, any_pre_v1=any(f["pre_v1"] for f in files))
    for k in FIELDS:
        width, begin, values = fld[k]
        b[k] = dict(width=one(width, np.uint8), begin=np.array(begin, np.uint64), values=one(values, np.uint32))
    b["blob_need"] = sum(len(s) for s in seqs) + len(seqs)   # (sum of lengths + one per allele always suffices)
    return b


SITES_OUT = (("record_site", np.int32), ("site_pos", np.int64), ("site_template", np.int32), ("site_stage_status", np.int32), ("entry_record", np.int32),
             ("site_entry_begin", np.uint64), ("entry_allele_begin", np.uint64), ("allele_off", np.uint64), ("allele_len", np.uint32), ("allele_src", np.int32),
             ("entry_gt_begin", np.uint64), ("gt", np.int32), ("allele_blob", np.uint8), ("al", np.int32), ("sd", np.int32), ("ap", np.uint32), ("am", np.uint32), ("sample_src", np.int32))


def sites_sizes(b, cap_sites):
    """elements of every output array of trgt_merge_sites_out for a packed input and cap_sites"""
    nf, S, na = b["n_files"], b["S"], b["n_alleles"]
    return dict(record_site=b["n_records"], site_pos=cap_sites, site_template=cap_sites, site_stage_status=cap_sites, entry_record=cap_sites * nf,
                site_entry_begin=cap_sites + 1, entry_allele_begin=cap_sites * nf + 1, allele_off=na, allele_len=na, allele_src=na, entry_gt_begin=cap_sites * nf + 1,
                gt=cap_sites * S * 2, allele_blob=b["blob_need"] if b["any_pre_v1"] else 0, al=cap_sites * S * 2, sd=cap_sites * S * 2, ap=cap_sites * S * 2, am=cap_sites * S * 2,
                sample_src=cap_sites * S)


def alloc_sites_outputs(b, cap_sites, fill=0):
    """host output arrays of a packed input for cap_sites sites, pre-filled with `fill` (a byte)"""
    sizes = sites_sizes(b, cap_sites)
    outs = {}
    for name, t in SITES_OUT:
        a = np.empty(max(int(sizes[name]), 1), t)
        a.view(np.uint8)[:] = fill
        outs[name] = a
    return outs


def call_sites(b, outs, cap_sites, ctx=None, blob=None, check=True, blob_cap=None):
    """trgt_merge_sites_batch (ctx given) or trgt_merge_sites_host (ctx None) on a packed input.  blob: a torch uint8 tensor with the input
    blob already in HBM; outs: host arrays, or HBM tensors for allele_blob and the rows (None: NULL).  Returns the return code (raises
    unless check=False) and leaves n_sites and blob_written in outs."""
    p = _lib.ptr
    fl = [MergeField(p(b[k]["width"]), p(b[k]["begin"]), p(b[k]["values"])) for k in FIELDS]
    cin = MergeSitesIn(b["n_files"], p(b["n_samples"]), p(b["pre_v1"]), p(b["am_is_int"]), p(b["file_record_begin"]), p(b["pos"]), p(b["pad_base"]), p(b["record_allele_begin"]),
                       p(b["allele_off"]), p(b["allele_len"]), p(blob if blob is not None else b["allele_blob"]), b["blob_len"], *fl)
    g = lambda n: p(outs.get(n))  # noqa: E731
    if blob_cap is None:
        blob_cap = 0 if outs.get("allele_blob") is None else (outs["allele_blob"].numel() if hasattr(outs["allele_blob"], "numel") else outs["allele_blob"].size)
    cout = MergeSitesOut(int(cap_sites), -1, g("record_site"), g("site_pos"), g("site_template"), g("site_stage_status"), g("entry_record"), g("site_entry_begin"), g("entry_allele_begin"),
                         g("allele_off"), g("allele_len"), g("allele_src"), g("entry_gt_begin"), g("gt"), g("allele_blob"), int(blob_cap), 0, g("al"), g("sd"), g("ap"), g("am"), g("sample_src"))
    L = _lib.lib()
    if ctx is None:
        rc = L.trgt_merge_sites_host(C.byref(cin), C.byref(cout))
    else:
        rc = L.trgt_merge_sites_batch(ctx.handle, C.byref(cin), C.byref(cout))
    outs["n_sites"], outs["blob_written"] = int(cout.n_sites), int(cout.blob_written)
    if rc != 0 and check:
        raise _lib.TrgtHipError("libtrgt_hip error %d: %s" % (rc, L.trgt_hip_last_error(ctx.handle if ctx is not None else None).decode()))
    return rc


def _host(outs, name):
    """an output array on the host, in the element type of the ABI (an HBM tensor is fetched)"""
    a = outs[name]
    return (a.cpu().numpy() if hasattr(a, "cpu") else a).view(dict(SITES_OUT)[name])


def out_allele_bytes(b, outs):
    """the bytes of every output allele, from the input sequences and the padding the lengths show (no blob is read)"""
    rab = b["record_allele_begin"]
    res = []
    for x in range(b["n_alleles"]):
        src = int(outs["allele_src"][x])
        s = b["seqs"][src]
        if int(outs["allele_len"][x]) != len(s):
            rec = int(np.searchsorted(rab, src, "right")) - 1
            s = bytes([int(b["pad_base"][rec])]) + s
        res.append(s)
    return res


def unpack_sites(b, outs):
    """-> per site a dict: pos, template (record index), status, records (per file its record index or -1), alleles (per file the list of
    its alleles as bytes, padded where the call padded), and the rows gt, AL, SD (ints), AP, AM (32-bit patterns) with two values per
    sample column, and sample_src per column.  A site with a status has None for its rows."""
    nf, S = b["n_files"], b["S"]
    seqs = out_allele_bytes(b, outs)
    rows = {k: _host(outs, n) for k, n in zip(FIELDS, ("gt", "al", "sd", "ap", "am"))}
    ssrc = _host(outs, "sample_src")
    res = []
    for t in range(outs["n_sites"]):
        eab = outs["entry_allele_begin"][t * nf:(t + 1) * nf + 1]
        status = int(outs["site_stage_status"][t])
        d = dict(pos=int(outs["site_pos"][t]), template=int(outs["site_template"][t]), status=status, records=[int(r) for r in outs["entry_record"][t * nf:(t + 1) * nf]],
                 alleles=[seqs[int(eab[f]):int(eab[f + 1])] for f in range(nf)])
        for k in FIELDS:
            d[k] = None if status else [int(v) for v in rows[k][t * S * 2:(t + 1) * S * 2]]
        d["sample_src"] = None if status else [int(v) for v in ssrc[t * S:(t + 1) * S]]
        res.append(d)
    return res


def run_sites(b, ctx=None, blob=None, device_outputs=False):
    """the sizing call and the call itself on a packed input -> outs.  device_outputs (ctx given): the output blob and the four FORMAT rows
    stay in HBM (torch tensors)."""
    probe = dict(record_site=np.empty(max(b["n_records"], 1), np.int32))
    rc = call_sites(b, probe, 0, ctx, blob, check=False)
    if rc not in (0, ERR_NOMEM):
        call_sites(b, probe, 0, ctx, blob)   # (raises with the message)
    n = probe["n_sites"]
    outs = alloc_sites_outputs(b, n)
    if n == 0:
        outs["n_sites"], outs["blob_written"] = 0, 0
        return outs
    if device_outputs and ctx is not None:
        import torch
        dev = "cuda:%d" % ctx.device
        sizes = sites_sizes(b, n)
        outs["allele_blob"] = torch.empty(max(sizes["allele_blob"], 1), dtype=torch.uint8, device=dev)
        for name in ("al", "sd", "ap", "am", "sample_src"):
            outs[name] = torch.empty(max(sizes[name], 1), dtype=torch.int32, device=dev)
    call_sites(b, outs, n, ctx, blob, blob_cap=sites_sizes(b, n)["allele_blob"])
    return outs


def sites_batch(files, ctx=None, blob=None):
    """The sites of one contig (see pack_sites for `files`), with padding, entries, FORMAT rows and template records: on the device of `ctx`,
    or by the host twin when ctx is None.  blob: the input allele blob already in HBM.  Returns unpack_sites' list."""
    b = pack_sites(files)
    return unpack_sites(b, run_sites(b, ctx, blob))


def merge_in_of_sites(b, outs, blob=None):
    """the packed batch of exact's call() for the sites of a finished sites call: the arrays are the sites call's own, the blob is its
    output blob when it wrote one (host array or HBM tensor) and the input blob otherwise.  -> (batch, blob tensor or None)"""
    n, nf = outs["n_sites"], b["n_files"]
    eab = outs["entry_allele_begin"][:n * nf + 1].astype(np.int64)
    per_entry = np.diff(eab).reshape(n, nf) if n * nf else np.zeros((n, 0), np.int64)
    alts = per_entry.sum(axis=1) - (per_entry > 0).sum(axis=1)
    slot = np.concatenate([[0], np.cumsum(np.maximum(1 + alts, 2))]).astype(np.uint64)
    wrote = b["any_pre_v1"]
    ob = outs["allele_blob"] if wrote else (blob if blob is not None else b["allele_blob"])
    on_dev = hasattr(ob, "data_ptr")
    b2 = dict(n_sites=n, site_entry_begin=outs["site_entry_begin"], entry_allele_begin=outs["entry_allele_begin"], allele_off=outs["allele_off"], allele_len=outs["allele_len"],
              allele_blob=None if on_dev else ob, blob_len=outs["blob_written"] if wrote else b["blob_len"], entry_gt_begin=outs["entry_gt_begin"], gt=outs["gt"], out_allele_begin=slot,
              n_alleles=b["n_alleles"], n_gt=n * b["S"] * 2)
    return b2, (ob if on_dev else None)


def merge_contig(files, ctx=None):
    """merge_variants for one contig: the sites call chained into merge_exact.  With a context the output blob and the FORMAT rows stay in
    HBM between the two calls (the blob is handed to trgt_merge_exact_batch where it lies); gt is a host array in both ABIs.  Returns per
    site what merge_variant would write: a dict of pos, template (record index), status (the stage status, else merge_exact's), alleles
    (merged, bytes), gt (flatten_genotypes: two values per sample), AL, SD, AP, AM (two values per sample; AP, AM as 32-bit patterns) and
    sample_src (the input record-sample whose ALLR / MC / MS strings belong to the column, -1 for ".").  A site with a status has None
    for alleles and rows."""
    b = pack_sites(files)
    outs = run_sites(b, ctx, device_outputs=ctx is not None)
    n, S = outs["n_sites"], b["S"]
    if n == 0:
        return []
    b2, dev_blob = merge_in_of_sites(b, outs)
    outs2 = alloc_outputs(b2)
    call(b2, outs2, ctx, blob=dev_blob)
    seqs = out_allele_bytes(b, outs)
    rows = {k: _host(outs, nm) for k, nm in zip(FIELDS[1:], ("al", "sd", "ap", "am"))}
    ssrc = _host(outs, "sample_src")
    res = []
    for t in range(n):
        status = int(outs["site_stage_status"][t]) or int(outs2["site_status"][t])
        d = dict(pos=int(outs["site_pos"][t]), template=int(outs["site_template"][t]), status=status, alleles=None, gt=None, AL=None, SD=None, AP=None, AM=None, sample_src=None)
        if status == 0:
            s0 = int(b2["out_allele_begin"][t])
            d["alleles"] = [seqs[int(a)] for a in outs2["out_allele_src"][s0:s0 + int(outs2["out_n_alleles"][t])]]
            d["gt"] = [int(v) for v in outs2["gt_out"][t * S * 2:(t + 1) * S * 2]]
            for k in FIELDS[1:]:
                d[k] = [int(v) for v in rows[k][t * S * 2:(t + 1) * S * 2]]
            d["sample_src"] = [int(v) for v in ssrc[t * S:(t + 1) * S]]
        res.append(d)
    return res
