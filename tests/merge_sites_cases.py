"""Inputs of the tests of trgt_merge_sites_batch / trgt_merge_sites_host -- designed contigs (each with a self-check of the condition it is
there for) and seeded random ones -- and check_outputs, which holds every output array of a call to tests/pymergesites.py."""
import random

import numpy as np

import pymergesites as ps
from trgt_amd import merge

VE = ps.VECTOR_END_INTEGER
BASES = "ACGT"
NANS = [0x7FC00001, 0x7F800003, 0xFFFFFFFF, 0x7FA00000, 0xFF800001, 0x7FFFFFFF]   # payloads other than the two constants


def ref_at(pos, n=None):
    """the full (post-1.0) REF of a position, and its ALT pool: every file agrees on them, so sites merge cleanly"""
    r = random.Random(pos * 7919 + 13)
    n = n if n is not None else r.randint(2, 12)
    first = r.choice(BASES)
    ref = first + "".join(r.choice(BASES) for _ in range(n - 1))
    alts = [first + "".join(r.choice(BASES) for _ in range(r.randint(0, 14))) for _ in range(3)]
    return ref, [a for a in alts if a != ref]


def record(rng, pos, n_samples, pre_v1=False, am_is_int=False, ref_len=None, widths=None, al_zero=False):
    """a record of a file at pos: pre-1.0 files store the alleles without their first base, which is then the padding base"""
    ref, pool = ref_at(pos, ref_len)
    alts = rng.sample(pool, rng.randint(0, len(pool)))
    full = [ref] + alts
    alleles = [a[1:] for a in full] if pre_v1 else full
    widths = widths or {}

    def samples(make, key):
        w = widths.get(key)
        return [[make() for _ in range(w if w else rng.randint(1, 2))] for _ in range(n_samples)]
    rec = dict(pos=pos, alleles=alleles, pad_base=full[0][0],
               gt=samples(lambda: rng.choice([0, 1] + [(i + 1) << 1 | rng.randint(0, 1) for i in range(len(full))] * 3), "gt"),
               AL=samples(lambda: 0 if al_zero else rng.randint(1, 900), "AL"), SD=samples(lambda: rng.choice([ps.MISSING_INTEGER, rng.randint(0, 90)]), "SD"),
               AP=samples(lambda: rng.choice([rng.random(), 1.0, ps.MISSING_FLOAT]), "AP"))
    if am_is_int:
        rec["AM"] = samples(lambda: rng.choice([ps.MISSING_INTEGER, rng.randint(0, 255)]), "AM")
    else:
        rec["AM"] = samples(lambda: rng.choice([rng.random(), ps.MISSING_FLOAT]), "AM")
    return rec


def make_file(rng, positions, n_samples=1, pre_v1=False, am_is_int=False, **kw):
    return dict(n_samples=n_samples, pre_v1=pre_v1, am_is_int=am_is_int, records=[record(rng, p, n_samples, pre_v1, am_is_int, **kw) for p in positions])


def contig(rng, n_files, positions, present=0.7, samples=(1,), pre=0.0, legacy=0.0, **kw):
    files = []
    for i in range(n_files):
        here = sorted(p for p in positions if rng.random() < present)
        files.append(make_file(rng, here, samples[i % len(samples)], rng.random() < pre, rng.random() < legacy, **kw))
    return files


def n_sites(files):
    return len(ps.key_sites(files))


def designed():
    """[(name, files, pad)]"""
    rng = random.Random(20261021)
    cases = []

    def add(name, files, ok, pad=(0, 1, 2, 3, 1)):
        assert ok, name
        cases.append((name, files, pad))

    for nf in (1, 2, 63, 64, 65, 257):   # the wave and workgroup boundaries of the fill
        f = contig(rng, nf, [10, 11, 500], present=1.1 if nf < 3 else 0.8, pre=0.3, legacy=0.3)
        add("files_%d" % nf, f, len(f) == nf and n_sites(f) == 3)
    f = contig(rng, 7, [3, 9, 27, 81], samples=(1, 2, 3), pre=0.4, legacy=0.4)
    add("samples_1_2_3", f, sum(x["n_samples"] for x in f) % 64 != 0 and {1, 2, 3} == {x["n_samples"] for x in f})
    f = [make_file(rng, [5, 6], 3), make_file(rng, [5, 7], 70, am_is_int=True), make_file(rng, [6, 7], 2, pre_v1=True)]
    add("samples_cross_64_in_one_file", f, f[1]["n_samples"] > 64 and f[0]["n_samples"] < 64)
    f = contig(rng, 5, [100, 200, 300, 400], present=1.1)
    add("every_file_at_every_site", f, all(len(x["records"]) == 4 for x in f))
    f = [make_file(rng, [10 * i + 1, 10 * i + 2]) for i in range(5)]
    add("one_file_per_site", f, n_sites(f) == 10)
    f = [make_file(rng, [4, 8]), make_file(rng, []), make_file(rng, [8])]
    add("a_file_without_records", f, not f[1]["records"])
    add("no_records_at_all", [make_file(rng, []), make_file(rng, [])], True)
    for name, a, b in (("bit_0", 4, 5), ("bit_8", 0x1200, 0x1300), ("bit_33", 1 << 33, 0), ("zero_and_top", 0, (1 << 40) - 1), ("bit_23_and_24", 1 << 23, 1 << 24)):
        lo, hi = min(a, b), max(a, b)
        f = [make_file(rng, [hi]), make_file(rng, [lo]), make_file(rng, [lo, hi]), make_file(rng, [hi])]
        add("positions_" + name, f, n_sites(f) == 2)
    f = [make_file(rng, [7, 7, 7, 9]), make_file(rng, [7]), make_file(rng, [7, 7, 7, 7], 2), make_file(rng, [7, 9])]
    add("three_and_four_records_at_one_position", f, n_sites(f) == 5)
    f = [make_file(rng, [50], 2, widths={k: 1 + ((i >> j) & 1) for j, k in enumerate(("gt", "AL", "SD", "AP", "AM"))}, am_is_int=i % 3 == 0) for i in range(32)]
    add("widths_mixed_per_field", f, n_sites(f) == 1)
    for k in ("gt", "AL", "SD", "AP", "AM"):
        f = [make_file(rng, [1, 2, 3], 2), make_file(rng, [1, 2, 3], 3, am_is_int=(k == "AM")), make_file(rng, [2], 1)]
        f[1]["records"][1][k][2] = []                      # width 1 or 2 with nothing in front of vector end
        f[1]["records"][2][k][0] = [VE if k in ("gt", "AL", "SD") or k == "AM" else ps.VECTOR_END_FLOAT, 5]
        exp = ps.merge_variants(f)
        add("ragged_" + k, f, [e["status"] == ps.RAGGED for e in exp] == [False, True, True])
    f = [make_file(rng, [1, 2], 2, pre_v1=True), make_file(rng, [1, 2], 1)]
    f[0]["records"][1]["AL"][0] = []
    add("ragged_first_al_of_a_pre_v1_file", f, [e["status"] for e in ps.merge_variants(f)] == [0, ps.RAGGED])
    # padded and unpadded files meet; AL 0 is not padded; the documented haploid zero in a width-2 record is not padded
    f = [make_file(rng, [30, 40, 50], 2, pre_v1=True), make_file(rng, [30, 40, 50], 1), make_file(rng, [30, 40], 1, pre_v1=True)]
    f[0]["records"][1]["AL"] = [[0, 7], [3, 3]]
    f[0]["records"][2]["AL"] = [[0], [5, 6]]
    f[2]["records"][0]["AL"] = [[-5]]
    exp = ps.merge_variants(f)
    add("padding_rules", f, [e["padded"] for e in exp] == [[0, 2], [2], []] and exp[0]["status"] == 0 and f[0]["records"][2]["AL"][0] == [0])
    lens = (0, 1, 3, 4, 5, 255, 256, 257, 1000)
    for name, pre in (("all", (True, True)), ("some", (True, False)), ("none", (False, False))):
        f = [dict(n_samples=1, pre_v1=p, am_is_int=False, records=[]) for p in pre]
        pad, at, want = [], 0, 0
        for i, n in enumerate(lens):
            for rep in range(4):
                pos = 1000 * i + rep
                for fi, x in enumerate(f):
                    r = record(rng, pos, 1, x["pre_v1"], ref_len=n + 1)
                    r["alleles"] = r["alleles"][:1] + [r["alleles"][0] + "T"]    # REF of n (pre-1.0) or n + 1 bytes and an ALT one longer
                    r["gt"] = [[2, 4]]
                    x["records"].append(r)
        for x in f:                                                              # the pads that put the alleles of every length at all four offsets
            for r in x["records"]:
                for a in r["alleles"]:
                    p = (want - at) % 4
                    pad.append(p)
                    at += p + len(a)
                    want += 1
                want += 1
        b = merge.pack_sites(f, pad=pad)
        seen = {(int(n), int(o) % 4) for n, o in zip(b["allele_len"], b["allele_off"])}
        need = [n for n in lens if pre[0]] + [n + 1 for n in lens]
        add("allele_lengths_pre_v1_" + name, f, all((n, o) in seen for n in need for o in range(4)), pad=tuple(pad))
    f = [make_file(rng, [5, 6], 1, pre_v1=True), make_file(rng, [5, 6], 1, pre_v1=True)]
    for x in f:
        x["records"][0]["pad_base"] = 0
        x["records"][1]["pad_base"] = b"*"
    add("pad_base_not_a_letter", f, ps.merge_variants(f)[0]["alleles"][0][0] == 0)
    f = [make_file(rng, [5, 6], 3), make_file(rng, [5], 2)]
    f[0]["records"][0]["AP"] = [[NANS[0], NANS[1]], [NANS[2]], [0.5, NANS[3]]]
    f[0]["records"][0]["AM"] = [[NANS[4]], [NANS[5], 0.25], [NANS[1], NANS[0]]]
    f[1]["records"][0]["AM"] = [[ps.MISSING_FLOAT, NANS[3]], [NANS[2]]]
    add("nan_payloads", f, ps.merge_variants(f)[0]["AM"][:2] == [NANS[4], ps.VECTOR_END_FLOAT])
    values = list(range(256)) + [ps.MISSING_INTEGER, 2 ** 31 - 1, 16777217, -1, 16777216, -16777217, 1 << 30]
    f = [make_file(rng, [77], len(values), am_is_int=True), make_file(rng, [77, 78], 1, am_is_int=True)]
    f[0]["records"][0]["AM"] = [[v] if i % 3 else [v, values[-1 - i]] for i, v in enumerate(values)]
    add("legacy_am_values", f, len(values) > 256 + 4)
    return cases


def random_contigs(n=300, seed=7):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        nf = min(40, 1 + int(rng.expovariate(1 / 8.0)))
        positions = sorted(rng.sample(range(0, 5000), rng.randint(1, 14)))
        dup = [p for p in positions for _ in range(1 + (rng.random() < 0.08) * rng.randint(1, 3))]
        files = []
        for i in range(nf):
            here = [p for p in dup if rng.random() < rng.choice((0.3, 0.9))][:60]
            ns = rng.choice((1, 1, 1, 2, 3))
            f = make_file(rng, here, ns, rng.random() < 0.3, rng.random() < 0.3, al_zero=False)
            for r in f["records"]:
                if rng.random() < 0.05:
                    r["AL"][0] = [0] + r["AL"][0][1:]
                if rng.random() < 0.02:
                    r[rng.choice(("gt", "AL", "SD", "AP", "AM"))][rng.randrange(ns)] = []
            files.append(f)
        out.append(files)
    return out


def global_tables(files):
    """(first global record index per file, first record-sample index per global record)"""
    frb, rs, k, s = [], [], 0, 0
    for f in files:
        frb.append(k)
        for _ in f["records"]:
            rs.append(s)
            s += f["n_samples"]
        k += len(f["records"])
    return frb, rs


def check_outputs(files, b, outs, exp, name, in_blob=None):
    """every output array of a finished sites call (merge.call_sites) against the restatement's sites `exp`, with no tolerance.  The allele
    bytes are read from the blob the call names: its output blob with a pre-1.0 file, the input blob otherwise."""
    nf, S = b["n_files"], b["S"]
    frb, rs = global_tables(files)
    assert outs["n_sites"] == len(exp), name
    n = len(exp)
    wrote = b["any_pre_v1"]
    if wrote:
        blob = merge._host(outs, "allele_blob")
        lens = outs["allele_len"][:b["n_alleles"]].astype(np.int64)
        assert outs["blob_written"] == int(lens.sum()), name
        assert list(outs["allele_off"][:b["n_alleles"]]) == list(np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else []), (name, "tightly packed, entry order")
    else:
        blob = b["allele_blob"] if in_blob is None else in_blob
        assert outs["blob_written"] == 0, name
    rows = {k: merge._host(outs, nm) for k, nm in zip(merge.FIELDS, ("gt", "al", "sd", "ap", "am"))}
    ssrc = merge._host(outs, "sample_src")
    seen = np.full(max(b["n_records"], 1), -1, np.int64)
    gt_begin, x = 0, 0
    for t, e in enumerate(exp):
        where = (name, "site", t)
        assert int(outs["site_pos"][t]) == e["pos"], where
        assert int(outs["site_template"][t]) == frb[e["template"][0]] + e["template"][1], where
        assert int(outs["site_entry_begin"][t]) == t * nf, where
        ragged = e["status"] == ps.RAGGED
        assert int(outs["site_stage_status"][t]) == (ps.RAGGED if ragged else 0), where
    recs_of = ps.heap_sites(files)
    for t, (pos, recs) in enumerate(recs_of):
        e = exp[t]
        ragged = e["status"] == ps.RAGGED
        for i, r in enumerate(recs):
            ent = t * nf + i
            assert int(outs["entry_record"][ent]) == (-1 if r is None else frb[i] + r), (name, t, i)
            assert int(outs["entry_gt_begin"][ent]) == gt_begin, (name, t, i)
            assert int(outs["entry_allele_begin"][ent]) == x, (name, t, i)
            gt_begin += 2 * files[i]["n_samples"]
            if r is None:
                continue
            g = frb[i] + r
            seen[g] = t
            rec = files[i]["records"][r]
            for j, a in enumerate(rec["alleles"]):
                src = int(outs["allele_src"][x])
                assert src == int(b["record_allele_begin"][g]) + j, (name, t, i, j)
                if not ragged:
                    off, ln = int(outs["allele_off"][x]), int(outs["allele_len"][x])
                    assert bytes(blob[off:off + ln]) == e["entry_alleles"][i][j], (name, t, i, j)
                    if not wrote:
                        assert off == int(b["allele_off"][src]), (name, t, i, j)
                x += 1
        if not ragged:
            lo, hi = t * S * 2, (t + 1) * S * 2
            assert [int(v) for v in rows["gt"][lo:hi]] == [v for eg in e["entry_gt"] for v in eg], (name, t, "gt")
            for k in ("AL", "SD"):
                assert [int(v) for v in rows[k][lo:hi]] == e[k], (name, t, k)
            for k in ("AP", "AM"):
                assert [int(v) for v in rows[k][lo:hi]] == e[k], (name, t, k, [hex(int(v)) for v in rows[k][lo:hi]], [hex(v) for v in e[k]])
            want = [-1 if s is None else rs[frb[s[0]] + s[1]] + s[2] for s in e["strings"]]
            assert [int(v) for v in ssrc[t * S:(t + 1) * S]] == want, (name, t, "sample_src")
    if n:
        assert int(outs["site_entry_begin"][n]) == n * nf and int(outs["entry_gt_begin"][n * nf]) == gt_begin and int(outs["entry_allele_begin"][n * nf]) == x, name
    assert x == b["n_alleles"], name
    assert [int(v) for v in outs["record_site"][:b["n_records"]]] == [int(v) for v in seen[:b["n_records"]]], (name, "record_site")


def check_contig(files, got, exp, name):
    """merge.merge_contig's list against the restatement's merge_variant list"""
    frb, rs = global_tables(files)
    assert len(got) == len(exp), name
    for t, (g, e) in enumerate(zip(got, exp)):
        assert g["pos"] == e["pos"] and g["template"] == frb[e["template"][0]] + e["template"][1] and g["status"] == e["status"], (name, t, g["status"], e["status"])
        if e["status"]:
            assert g["alleles"] is None and g["gt"] is None, (name, t)
            continue
        for k in ("alleles", "gt", "AL", "SD", "AP", "AM"):
            assert g[k] == e[k], (name, t, k)
        assert g["sample_src"] == [-1 if s is None else rs[frb[s[0]] + s[1]] + s[2] for s in e["strings"]], (name, t)
